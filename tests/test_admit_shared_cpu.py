"""One admission filter shared by the ranks of a group, the part that needs no GPU: the slot
partition (xf_admit_range against tests/_admit_shared_checker.py), the worker's admit_shared
parameter and its refusals, and the restatement alone on the cases of
tests/test_gpu_admit_shared.py — that they contain what they are there to show."""
import ctypes as C
import time

import numpy as np
import pytest

from xflow_amd import capi

from . import _admit_checker as A
from . import _admit_shared_checker as S

LS, WORLDS = (2, 3, 10, 26, 32), (1, 2, 3, 7, 8, 255)


# ------------------------------------------------------------------ the slot partition
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("world", WORLDS)
def test_ranges_partition_the_slots(L, world):
    slots = 1 << L
    got = [capi.admit_range(L, world, r) for r in range(world)]
    assert got == [S.admit_range(L, world, r) for r in range(world)]
    at, seen_empty = 0, False
    for first, n in got:
        assert first % 4 == 0 and n % 4 == 0                     # whole counter words
        assert first == at                                       # ordered, disjoint, no gap
        assert not (seen_empty and n)                            # empty ranges only at the end
        seen_empty = seen_empty or n == 0
        at += n
    assert at == slots                                           # they cover [0, 2^L)
    per = S.per(L, world)
    assert per * world >= slots and (slots - 1) - (world - 1) * per < 2 ** 32   # local slots: 32 bits
    for r, (first, n) in enumerate(got):
        for s in (first - 1, first, first + 1, first + n - 2, first + n - 1, first + n):
            if n and 0 <= s < slots:
                o = S.owner(s, L, world)
                assert got[o][0] <= s < got[o][0] + got[o][1]
                assert (o == r) == (first <= s < first + n)
                assert 0 <= s - o * per < 2 ** 32


def test_the_example_of_two_ranks_that_own_nothing():
    assert [capi.admit_range(2, 3, r) for r in range(3)] == [(0, 4), (4, 0), (4, 0)]


@pytest.mark.parametrize("args", [(1, 1, 0), (33, 1, 0), (10, 0, 0), (10, 2, 2), (10, 2, -1)])
def test_range_refuses_what_is_no_rank_of_a_filter(args):
    with pytest.raises(capi.XFError, match="xf_admit_range"):
        capi.admit_range(*args)


# ------------------------------------------------------------------ the worker's parameter
def _start(**params):
    """XFStartTrain through the C ABI itself (capi.XFlow.train asks for a GPU first)"""
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode(), x


def test_admit_shared_takes_zero_or_one():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test")
    x.set("admit_shared", 1)
    x.set("admit_shared", 0)
    for bad in (2, -1, "yes"):
        with pytest.raises(capi.XFError, match="admit_shared must be 0 or 1"):
            x.set("admit_shared", bad)


REFUSALS = [
    (dict(admit_count=2, world=2, admit_shared=0), ["admit_count", "world", "one worker only"]),
    (dict(admit_count=2, world=2, admit_shared=1, core_num=2), ["admit_count", "core_num"]),
    (dict(admit_count=2, world=2, admit_shared=1, key_build="host"), ["admit_count", "key_build"]),
    (dict(admit_count=2, world=2, admit_shared=1, parity="reference_order"),
     ["admit_count", "parity"]),
    (dict(admit_count=2, world=2, admit_shared=1, admit_log2_slots=33), ["admit_log2_slots", "33"]),
    (dict(admit_count=2, world=2, admit_shared=1, schedule="owner"), ["admit_shared", "schedule=owner"]),
    (dict(admit_count=2, world=2, admit_shared=1, model=1, fm_mode="canonical"),
     ["fm_mode=canonical", "one worker"]),
    (dict(admit_count=2, world=2, admit_shared=1, feature_values="on"),
     ["feature_values=on", "one worker"]),
]


@pytest.mark.parametrize("params,words", REFUSALS, ids=[",".join("%s=%s" % kv for kv in p.items())
                                                        for p, _ in REFUSALS])
def test_refusals_fire_before_any_rendezvous(params, words):
    """world=2 and no second process anywhere: a refusal that came after the rendezvous would wait
    for it"""
    t0 = time.time()
    rc, msg, _ = _start(**params)
    assert rc == 1, (rc, msg)                    # XF_EINVAL
    assert msg.startswith("XFStartTrain:")
    for w in words:
        assert w in msg, msg
    assert time.time() - t0 < 10


# ------------------------------------------------------------------ the GPU test's cases
GRID = [(world, N, h, L) for world in (1, 2, 3) for N in (1, 2, 255) for h in (1, 3) for L in (2, 10)]


@pytest.mark.parametrize("world,N,h,L", [g for g in GRID if g[3] == 10],
                         ids=["w%d-N%d-h%d-L%d" % g for g in GRID if g[3] == 10])
def test_the_cases_contain_what_they_are_there_to_show(world, N, h, L):
    """(a) a nonzero kept on a rank whose own occurrences of the key number fewer than N, (b) a
    dropped nonzero, (c) a nonzero admitted although its key occurred fewer than N times on all
    ranks together, (d) nonzeros on the first and the last slot of every non-empty range.  N = 1
    keeps everything it counts by contract — (a), (b), (c) are asked of N > 1 — and one rank has
    no other rank's occurrences to be admitted by: (a) needs world > 1."""
    seq = S.sequence(world, N, h, L)
    exp = S.expected(seq, N, h, L)
    assert 10 <= len(seq) <= 20
    own = [dict() for _ in range(world)]         # key -> occurrences counted so far, per rank
    kinds, on_slots = set(), set()
    for (name, update, parts), (_, ranks) in zip(seq, exp):
        if update:
            for r, (_, ks) in enumerate(parts):
                for k, c in zip(*np.unique(ks, return_counts=True)):
                    own[r][int(k)] = own[r].get(int(k), 0) + int(c)
        for r, ((_, ks), out) in enumerate(zip(parts, ranks)):
            keep = out[4]
            if not keep.all():
                kinds.add("b")
            for k in np.unique(ks[keep]).tolist():
                everywhere = sum(o.get(k, 0) for o in own)
                if own[r].get(k, 0) < N <= everywhere:           # (admitted by the other ranks')
                    kinds.add("a")
                if everywhere < N:
                    kinds.add("c")
            on_slots.update(A.slots(ks, S.SEED, L, h).astype(np.int64).ravel().tolist())
    want = {"b", "c"} | ({"a"} if world > 1 else set()) if N > 1 else set()
    assert want <= kinds, (want, kinds)
    assert set(S.boundary_slots(L, world)) <= on_slots
    # every rank sees R = 0 or NNZ = 0 at some apply, and the 2048-nonzero tile from both sides
    sizes = {(len(rp) - 1 == 0, len(ks) == 0) for _, _, parts in seq for rp, ks in parts}
    assert (True, True) in sizes and (False, True) in sizes
    assert {2047, 2048, 2049} <= {len(ks) for _, _, parts in seq for _, ks in parts}
    assert any(not update for _, update, _ in seq)
