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


# ------------------------------------------------------------------ replay across evictions
# what gives tests/test_gpu_evict_replay.py its power: the evicting oracle alone, on the CPU
HYPERS = {"HYPER": E.HYPER, "ALL_ZERO": E.HYPER_ALL_ZERO}
REPLAY = [("HYPER", INF, 1), ("HYPER", INF, 2), ("HYPER", E.X_TRAIN, 1), ("HYPER", E.X_TRAIN, 2),
          ("ALL_ZERO", INF, 1), ("ALL_ZERO", INF, 2)]
_runs = {}


def _replay(hname, x, every):
    key = (hname, x, every)
    if key not in _runs:
        _runs[key] = E.replay_run(HYPERS[hname], x, every)[0]
    return _runs[key]


def _differ(a, b):
    return any(x.shape != y.shape or not np.array_equal(E.bits(x), E.bits(y)) for x, y in zip(a, b))


def test_replay_stream_carries_the_reserved_key_and_key_zero():
    for rowptr, keys, labels in E.replay_stream():
        assert len(labels) == 600 and len(np.unique(keys)) > 500
        first = rowptr[:-1].astype(np.int64)[np.diff(rowptr.astype(np.int64)) > 0]
        has = keys[first] == E.SPARE
        assert 0.4 < has.mean() < 0.6 and (keys == E.SPARE).sum() == has.sum()
        assert 1 <= (keys == 0).sum() <= 5
        lab = labels[np.diff(rowptr.astype(np.int64)) > 0]
        assert (lab[has] == 1).mean() > 0.8 and (lab[~has] == 1).mean() < 0.2


@pytest.mark.parametrize("hname,x,every", REPLAY)
def test_replayed_epochs_meet_evictions_that_bite(hname, x, every):
    out = _replay(hname, x, every)
    epoch_keys = np.unique(np.concatenate([r[1] for r in E.replay_stream()]))
    evictions = [i for i, o in enumerate(out) if o[0] == "evict"]
    assert [out[i][1] for i in evictions] == E.boundaries(E.EPOCHS, every) and evictions
    assert len(E.boundaries(E.EPOCHS, every)) == {1: 3, 2: 1}[every]
    for i in evictions:
        (_, e, pre, _), (_, _, post, (seen, dropped)) = out[i - 1], out[i]
        assert out[i - 1][0] == "epoch" and seen == len(pre[0]) == len(epoch_keys)
        share = dropped / seen
        print("%s x = %g every %d, after epoch %d: %d of %d dropped (%.1f %%)" % (
            hname, x, every, e + 1, dropped, seen, 100 * share))
        if hname == "ALL_ZERO":
            assert share == 1.0 and len(post[0]) == 0
        else:
            assert 0.1 <= share <= 0.9
        gone = np.setdiff1d(pre[0], post[0])
        assert len(gone) == dropped and e + 1 < E.EPOCHS
        assert np.isin(gone, epoch_keys).all()          # the next epoch touches every one again
        # the reserved key meets both fates
        assert (E.SPARE in post[0]) == (hname == "HYPER") and E.SPARE in pre[0]
        if hname == "HYPER":
            assert post[1][-1] != 0
    if hname == "ALL_ZERO":
        for o in out:
            assert not E.bits(o[2][1]).any(), o[:2]     # every weight is +0
    # a run that ignored re-entry would end elsewhere: the state without any eviction, as it is
    # and filtered, is another one
    final = out[-1][2]
    plain = _replay(hname, 0.0, 0)[-1][2]
    assert out[-1][0] == "epoch" and np.array_equal(final[0], plain[0])
    assert _differ(final, plain)
    if hname == "HYPER":
        assert _differ(E.evict(final, x)[0], E.evict(plain, x)[0])
    for o in out:
        if o[0] == "epoch":
            assert _differ(o[2], _replay(hname, 0.0, 0)[o[1]][2]) == (
                o[1] > E.boundaries(E.EPOCHS, every)[0])


def test_the_schedules_and_the_values_of_the_replay_bite_too():
    """the one-rank exchange rules and the valued steps, x = inf at every boundary"""
    for kw in (dict(schedule="sequential"), dict(schedule="stale1"), dict(valued=True)):
        out = E.replay_run(E.HYPER, INF, 1, **kw)[0]
        plain = E.replay_run(E.HYPER, 0.0, 0, **kw)[0]
        counts = [o[3] for o in out if o[0] == "evict"]
        assert len(counts) == 3 and all(0.1 <= d / s <= 0.9 for s, d in counts), (kw, counts)
        assert _differ(out[-1][2], plain[-1][2]), kw
    seq = E.replay_run(E.HYPER, INF, 1, schedule="sequential")[0]
    one = _replay("HYPER", INF, 1)
    for a, b in zip(seq, one):        # one rank, sequential: the plain step after step
        E.same_state(a[2], b[2])
    assert _differ(E.replay_run(E.HYPER, INF, 1, schedule="stale1")[0][-1][2], one[-1][2])


def test_a_threshold_that_drops_nothing():
    """x = X_NONE takes only rows whose n is 0: some after one epoch, none after two"""
    assert E.replay_run(E.HYPER, E.X_NONE, 1)[0][1][3][1] > 0
    out = E.replay_run(E.HYPER, E.X_NONE, 0, at=E.AT_NONE)[0]
    plain = _replay("HYPER", 0.0, 0)
    counts = [o[3] for o in out if o[0] == "evict"]
    assert counts == [(len(plain[0][2][0]), 0)] * 2
    E.same_state(out[-1][2], plain[-1][2])


# ---- the worker tests' text
WORKER = [(4, 1), (4, 2), (3, 2)]


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    return E.worker_text(tmp_path_factory.mktemp("evict_text"), two=True)


@pytest.mark.parametrize("x", [INF, E.X_WORKER])
@pytest.mark.parametrize("epochs,every", WORKER)
def test_lambda1_of_the_worker_text_keeps_the_band(text, epochs, every, x):
    r = E.worker_reference(text, epochs, every, x)
    assert r["blocks"] == [3]
    want = [e + 1 for e in range(epochs) if (e + 1) % every == 0 or e + 1 == epochs]
    assert [e for e, _, _ in r["log"]] == want
    for e, seen, dropped in r["log"]:
        print("lambda1 = %g x = %g epochs %d every %d, epoch %d: %d of %d dropped (%.1f %%)" % (
            E.L1_WORKER, x, epochs, every, e, dropped, seen, 100.0 * dropped / seen))
        assert 0.1 <= dropped / seen <= 0.9
    assert E.evict(r["model"], x)[2] == 0
    plain = E.worker_reference(text, epochs, 0, 0.0)
    assert plain["log"] == [] and plain["rows"] == r["rows"]
    assert _differ(r["model"], E.evict(plain["model"], x)[0])
    if x != INF:      # the finite threshold leaves zero rows the infinite one takes
        inf = E.worker_reference(text, epochs, every, INF)
        assert all(a[2] < b[2] for a, b in zip(r["log"], inf["log"]))


def test_worker_text_with_values_and_on_two_ranks_keeps_the_band(text):
    runs = [E.worker_reference(text, 4, 1, INF, valued=True)]
    runs += [E.worker_reference(text, 3, 1, INF, schedule=s, ranks=2)
             for s in ("sequential", "stale1")]
    assert runs[1]["blocks"] == [3, 2]
    for r in runs:
        assert all(0.1 <= d / s <= 0.9 for _, s, d in r["log"]), r["log"]
    plain = E.worker_reference(text, 3, 0, 0.0, schedule="stale1", ranks=2)
    assert _differ(runs[2]["model"], E.evict(plain["model"], INF)[0])
    # the schedules part ways in the epochs that replay (the first one flushes after every turn)
    assert _differ(runs[1]["model"], runs[2]["model"])
    assert not _differ(runs[1]["states"][0], runs[2]["states"][0])


@pytest.mark.parametrize("epochs", [3, 4])
def test_epoch_by_epoch_without_eviction_is_the_oracle_train_call(text, epochs):
    """the worker reference steps the blocks epoch by epoch; without eviction that is one
    O.train(..., epochs=N) call"""
    from oracle import pyoracle as O
    r = E.worker_reference(text, epochs, 0, 0.0)
    s = O.Store(O.OPT_FTRL, 1)
    s.set_ftrl(E.HYPER["alpha"], E.HYPER["beta"], E.L1_WORKER, E.HYPER["lambda2"])
    with O.sum_mode(1):
        rows = O.train(0, s, None, os.path.join(text, "train-00000"), epochs, 1 << 20)
        lab, p = O.predict(0, s, None, os.path.join(text, "test-00000"))
    assert rows == r["rows"]
    assert np.array_equal(lab, r["labels"]) and p.tobytes() == r["pctr"].tobytes()
    E.same_state(s.export(), r["store"].export())
