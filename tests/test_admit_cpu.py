"""Feature admission without a GPU: the slot function of the library against the numpy
restatement (tests/_admit_checker.py), the restatement against a loop in plain Python, and the
worker's three parameters with every refusal of XFStartTrain."""
import ctypes as C
import time

import numpy as np
import pytest

from xflow_amd import capi

from . import _admit_checker as A

MASK = (1 << 64) - 1
SEEDS = (0, 12345, 0xfedcba9876543210)


# ------------------------------------------------------------------ the slot function
@pytest.mark.parametrize("L", [2, 10, 26, 32])
def test_slot_function_equals_the_restatement(L):
    rng = np.random.RandomState(100 + L)
    keys = rng.randint(0, 1 << 62, size=10000).astype(np.uint64) * np.uint64(4) + \
        rng.randint(0, 4, size=10000).astype(np.uint64)
    keys[:4] = [0, 1, MASK, 1 << 63]
    f = capi.lib().xf_admit_slot
    for seed in SEEDS:
        want = A.slots(keys, seed, L, 8)
        assert int(want.max()) < 1 << L
        for j in range(8):
            got = np.array([f(int(k), seed, L, j) for k in keys], np.uint64)
            assert np.array_equal(got, want[j]), (L, seed, j)


def test_slot_function_out_of_range_is_zero():
    for L, j in ((1, 0), (33, 0), (10, -1)):
        assert capi.admit_slot(123, 0, L, j) == 0


# ------------------------------------------------------------------ the restatement itself
def _py_mix64(x):
    x = (x + 0x9e3779b97f4a7c15) & MASK
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def _py_slot(key, seed, L, j):
    return _py_mix64(key ^ _py_mix64((seed + j) & MASK)) >> (64 - L)


def _brute(counters, N, L, h, seed, rowptr, keys, update):
    """the semantics as a loop: -> (rowptr, keys) kept"""
    if update:
        for k in keys:
            for j in range(h):
                s = _py_slot(int(k), seed, L, j)
                counters[s] = min(N, counters[s] + 1)
    out_rp, out_keys = [0], []
    for r in range(len(rowptr) - 1):
        for i in range(rowptr[r], rowptr[r + 1]):
            if all(counters[_py_slot(int(keys[i]), seed, L, j)] == N for j in range(h)):
                out_keys.append(int(keys[i]))
        out_rp.append(len(out_keys))
    return out_rp, out_keys


def test_restatement_against_a_plain_loop():
    L, h, N, seed = 6, 3, 3, 7
    twin = next(k for k in range(1, 100000)
                if len({_py_slot(k, seed, L, j) for j in range(h)}) == 2)  # two j on one slot
    rng = np.random.RandomState(5)
    keys = rng.randint(1000, 1012, size=50).astype(np.uint64)
    keys[[3, 17, 40]] = twin
    cuts = np.sort(rng.randint(0, 51, size=11))
    rowptr = np.concatenate([[0], cuts, [50]]).astype(np.uint64)        # 12 rows, some empty
    flt, ctr = A.Filter(L, N, h, seed), [0] * (1 << L)
    for update in (True, True, False, True):
        rp, ks, _, _ = flt.filter(rowptr, keys, update=update)
        brp, bks = _brute(ctr, N, L, h, seed, [int(x) for x in rowptr], keys, update)
        assert rp.tolist() == brp and ks.tolist() == bks
        assert flt.c.tolist() == ctr
    # the twin's shared slot counted twice per occurrence: three occurrences saturate N = 3 at once
    one = A.Filter(L, N, h, seed)
    one.count(np.array([twin], np.uint64))
    assert sorted(one.c[one.c > 0].tolist()) == [1, 2]
    assert flt.seen == 150 and 0 < flt.kept < 150


def test_count_one_keeps_everything_in_the_restatement():
    rng = np.random.RandomState(6)
    keys = rng.randint(0, 1 << 40, size=300).astype(np.uint64)
    rowptr = np.arange(0, 301, 3, dtype=np.uint64)
    rp, ks, _, _ = A.Filter(4, 1, 3, 0).filter(rowptr, keys)
    assert np.array_equal(rp, rowptr.astype(np.uint32)) and np.array_equal(ks, keys)


# ------------------------------------------------------------------ the worker's parameters
def _start(**params):
    """XFStartTrain through the C ABI itself (capi.XFlow.train asks for a GPU first)"""
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode(), x


def test_the_three_parameters_are_accepted():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test")
    for name, value in (("admit_count", 2), ("admit_log2_slots", 12), ("admit_hashes", 4),
                        ("admit_count", 0), ("admit_count", 255)):
        x.set(name, value)
    assert x.metric("admit_seen") == 0 and x.metric("admit_kept") == 0


REFUSALS = [
    (dict(admit_count=2, world=2), ["admit_count", "world"]),
    (dict(admit_count=2, core_num=2), ["admit_count", "core_num"]),
    (dict(admit_count=2, key_build="host"), ["admit_count", "key_build"]),
    (dict(admit_count=2, parity="reference_order"), ["admit_count", "parity"]),
    (dict(admit_count=256), ["admit_count", "256"]),
    (dict(admit_count=-1), ["admit_count"]),
    (dict(admit_count=2, admit_log2_slots=1), ["admit_log2_slots"]),
    (dict(admit_count=2, admit_log2_slots=33), ["admit_log2_slots", "33"]),
    (dict(admit_count=2, admit_hashes=0), ["admit_hashes"]),
    (dict(admit_count=2, admit_hashes=9), ["admit_hashes", "9"]),
]


@pytest.mark.parametrize("params,words", REFUSALS, ids=[",".join("%s=%s" % kv for kv in p.items())
                                                        for p, _ in REFUSALS])
def test_refusals_name_their_parameter(params, words):
    t0 = time.time()
    rc, msg, _ = _start(**params)
    assert rc == 1, (rc, msg)                    # XF_EINVAL
    assert msg.startswith("XFStartTrain:")
    for w in words:
        assert w in msg, msg
    assert time.time() - t0 < 10


def test_count_zero_creates_nothing():
    """admit_count=0: the other two parameters are not even looked at — the start gets past the
    admission checks (and fails on the missing GPU or the missing file), no filter exists"""
    rc, msg, x = _start(admit_count=0, admit_log2_slots=99, admit_hashes=77, world=1)
    assert rc != 0
    assert "admit" not in msg, msg
    assert x.metric("admit_seen") == 0 and x.metric("admit_kept") == 0
