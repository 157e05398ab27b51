"""Table eviction, what needs no GPU: the numpy restatement (tests/_evict_checker.py) on
hand-written rows, the crafted tables' patterns, the share of zero weights the training stream's
lambda1 leaves (the oracle's CPU run), the worker's parameters and refusals, and the ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _evict_checker as E
from xflow_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build(verbose=False)


def _state(rows):
    k, w, n, z = zip(*rows)
    return (np.array(k, np.uint64), np.array(w, np.float32), np.array(n, np.float32),
            np.array(z, np.float32))


def test_checker_on_hand_written_rows():
    sub = np.float32(1e-45)                          # the smallest subnormal: not zero
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    rows = [(1, 0.0, 0.5, 0.1),                      # dropped
            (2, -0.0, 0.5, -0.1),                    # dropped: either sign of zero
            (3, 0.0, 1.0, 0.2),                      # n == x: kept
            (4, 0.0, below, 0.2),                    # n just below x: dropped
            (5, sub, 0.0, 0.3),                      # a subnormal weight: kept
            (6, 0.0, float("nan"), 0.4),             # NaN n: kept
            (7, 0.25, 0.0, 0.5),                     # a weight: kept
            (8, 0.0, 0.0, 0.0),                      # a first touch never stepped: dropped
            (2**64 - 1, 0.0, 0.5, 0.0)]              # the reserved key: like any other
    st = _state(rows)
    got, seen, dropped = E.evict(st, 1.0)
    assert list(got[0]) == [3, 5, 6, 7] and (seen, dropped) == (9, 5)
    E.same_state(got, tuple(a[[2, 4, 5, 6]] for a in st))
    got, seen, dropped = E.evict(st, INF)            # every zero-weight row but the NaN one
    assert list(got[0]) == [5, 6, 7] and (seen, dropped) == (9, 6)
    got, seen, dropped = E.evict(st, 0.0)            # off: nothing is judged
    assert (seen, dropped) == (0, 0)
    E.same_state(got, st)
    got, _, dropped = E.evict(st, 1e-30)             # only the rows whose n is 0
    assert dropped == 1 and 8 not in list(got[0])
    assert list(E.keep_mask([0.0, -0.0, 0.0], [-1.0, -0.0, 1e-30], 1e-30)) == [False, False, True]


def test_patterns_hit_the_edges_they_name():
    B, S = 4096, 64
    assert E.sizes(B, S)[-1] == 257 * B + 1 and len(E.sizes(B, S)) == 10
    n = 5 * B + 37
    for name in E.PATTERNS:
        d = E.drop_pattern(name, n, B, S)
        assert d.shape == (n,) and d.dtype == bool
        keys, w, nn, z = E.crafted(n, d)
        assert np.all(np.diff(keys.astype(np.float64)) >= 0) and len(np.unique(keys)) == n
        assert np.array_equal(E.keep_mask(w, nn, E.X), ~d), name
    keep = ~E.drop_pattern("one_per_wave", n, B, S)
    assert np.all(np.add.reduceat(keep, np.arange(0, n, S))[:-1] == 1)
    assert len(set(np.flatnonzero(keep)[:S] % S)) > S // 2       # the lane moves
    keep = ~E.drop_pattern("one_per_block_last", n, B, S)
    assert list(np.flatnonzero(keep)) == [B - 1 + i * B for i in range(5)]
    d = E.drop_pattern("blocks", n, B, S)
    assert not d[:B].any() and d[B:2 * B].all() and not d[2 * B:3 * B].any()
    assert np.signbit(E.crafted(n, np.ones(n, bool))[1]).any()   # -0.0 among the dropped


def test_lambda1_of_the_training_stream_leaves_a_share_of_zero_weights():
    """the oracle's CPU run of T1 steps: between 10 % and 90 % of the keys at w == 0, and the
    finite threshold splits them"""
    keys, w, n, z = E.oracle_after_t1()
    zero = w == 0
    share = float(zero.mean())
    print("lambda1 = %g: %d of %d keys at w == 0 (%.1f %%), their n in [%g, %g]" % (
        E.L1, zero.sum(), len(keys), 100 * share, n[zero].min(), n[zero].max()))
    assert 0.1 <= share <= 0.9
    below = zero & (n < np.float32(E.X_TRAIN))
    assert 0 < below.sum() < zero.sum()


def _worker(**params):
    h = capi.vp()
    L = capi.lib()
    assert L.XFCreate(C.byref(h), b"/nonexistent/train", b"/nonexistent/test") == 0
    for k, v in params.items():
        assert L.XFSetParam(h, k.encode(), str(v).encode()) == 0, (k, v, L.xf_last_error())
    return h


def test_worker_parameters_parse_and_refuse_without_a_gpu():
    L = capi.lib()
    h = _worker()
    try:
        for n, v in [("evict_n", "inf"), ("evict_n", "0"), ("evict_n", "1e-9"), ("evict_n", "0.5"),
                     ("evict_every", "1"), ("evict_every", "7")]:
            assert L.XFSetParam(h, n.encode(), v.encode()) == 0, (n, v, L.xf_last_error())
        for n, v, why in [("evict_n", "-1", "evict_n must be 0 (off), a positive number or inf"),
                          ("evict_n", "nan", "evict_n must be"), ("evict_n", "lots", "evict_n must be"),
                          ("evict_n", "", "evict_n must be"), ("evict_n", "1x", "evict_n must be"),
                          ("evict_every", "0", "evict_every must be >= 1"),
                          ("evict_every", "-2", "evict_every must be >= 1")]:
            assert L.XFSetParam(h, n.encode(), v.encode()) != 0, (n, v)
            assert why in L.xf_last_error().decode(), L.xf_last_error()
    finally:
        L.XFDestroy(C.byref(h))


@pytest.mark.parametrize("params,why", [
    (dict(model=1, evict_n="inf"), r"evict_n=inf with model 1 \(FM\)"),
    (dict(optimizer="sgd", evict_n=1e-9), r"evict_n=1e-09 together with optimizer=sgd"),
    (dict(world=2, rank=0, schedule="owner", evict_n="inf"), r"evict_n=inf together with schedule=owner"),
])
def test_start_refuses_what_eviction_does_not_cover_before_anything_else(params, why):
    """at XFStartTrain, by name, before a table, a file or a rendezvous is touched"""
    L = capi.lib()
    h = _worker(**params)
    try:
        assert L.XFStartTrain(C.byref(h)) != 0
        assert re.search(why, L.xf_last_error().decode()), L.xf_last_error()
    finally:
        L.XFDestroy(C.byref(h))


def test_abi_symbols_in_the_header_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "xflow_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = set(ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip())
    for name in ("xf_table_evict", "xf_evict_shape", "xf_sharded_evict"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported and name in capi.SIGNATURES, name
    assert capi.SIGNATURES["xf_table_evict"][1][1] is C.c_float
    for cls, meth in ((capi.Table, "evict"), (capi.Sharded, "evict")):
        assert callable(getattr(cls, meth))
    assert callable(capi.evict_shape)
