"""Table eviction on real hardware (xf_table_evict / xf_sharded_evict / evict_n=): every result is
held against the numpy restatement (tests/_evict_checker.py: keep = ~((w == 0) & (n < x)) in
float32, applied to an export) with == on bits."""
import ctypes as C
import os
import shutil
import traceback

import numpy as np
import pytest

from tests import _evict_checker as E
from xflow_amd import capi

from . import test_gpu_sharded_modes as SM     # _spawn (the module, not its tests)
from .conftest import GOLDEN
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
INF = float("inf")
SIZE_IDS = ["1", "S-1", "S", "S+1", "B-1", "B", "B+1", "2B+1", "5B+37", "257B+1"]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def _shape():
    s = capi.evict_shape()
    assert s["wave"] == 64 and s["rows"] % s["wave"] == 0 and s["rows"] >= 4 * s["wave"]
    return s["rows"], s["wave"]


def _capacity(n):
    cap = 64
    while cap < 2 * n + 16:
        cap *= 2
    return cap


def _table(state, settle=True, **hyper):
    """a table holding `state` (keys ascending, w, n, z), settled: key r owns row r"""
    t = capi.Table(capi.OPT_FTRL, 1, capacity=_capacity(len(state[0])), **hyper)
    t.import_(*state)
    if settle:
        t.defrag()
    return t


def _evict_and_check(t, x, what=""):
    """t.evict(x) against the checker's verdict on the export before it -> the survivors"""
    before = t.export()
    want, seen, dropped = E.evict(before, x)
    assert t.evict(x) == (seen, dropped), what
    E.same_state(t.export(), want, what)
    assert len(t) == len(want[0]), what
    # the survivors are the settled tier, but for the reserved key (its row follows the tier)
    assert t.settled == len(want[0]) - int(len(want[0]) > 0 and want[0][-1] == E.SPARE), what
    return want


# ------------------------------------------------------------------ 1. compaction at its edges
@pytest.mark.parametrize("pattern", E.PATTERNS)
@pytest.mark.parametrize("si", range(10), ids=SIZE_IDS)
def test_compaction_at_its_edges(si, pattern):
    B, S = _shape()
    n = E.sizes(B, S)[si]
    drop = E.drop_pattern(pattern, n, B, S)
    state = E.crafted(n, drop)
    t = _table(state)
    E.same_state(t.export(), state)
    assert t.settled == n
    want = _evict_and_check(t, E.X, (n, pattern))
    assert len(want[0]) == n - int(drop.sum())
    assert np.all(want[0][1:] > want[0][:-1])


def _edge_rows(spare_w):
    sub = np.float32(1e-45)
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    rows = [(11, 0.0, 0.5, 0.1), (12, -0.0, 0.5, -0.1), (13, 0.0, 1.0, 0.2), (14, 0.0, below, 0.2),
            (15, sub, 0.0, 0.3), (16, 0.0, float("nan"), 0.4), (17, 0.25, 0.0, 0.5),
            (18, 0.0, 0.0, 0.0), (19, -0.0, 1.5, 0.0), (2**64 - 1, spare_w, 0.5, 0.75)]
    k, w, n, z = zip(*rows)
    return (np.array(k, np.uint64), np.array(w, np.float32), np.array(n, np.float32),
            np.array(z, np.float32))


@pytest.mark.parametrize("spare", ["dropped", "kept"])
@pytest.mark.parametrize("x", [1.0, INF, 0.0, 1e-30])
def test_predicate_edges_and_the_reserved_key(x, spare):
    """n == x, n just below x, w = -0.0, w the smallest subnormal, n = NaN, x = inf, x = 0, and
    the key 2^64-1 once with a zero weight (it goes when x > 0.5) and once with a weight"""
    state = _edge_rows(0.0 if spare == "dropped" else 0.5)
    t = _table(state)
    E.same_state(t.export(), state)
    want = _evict_and_check(t, x, (x, spare))
    gone = spare == "dropped" and x > 0.5
    assert (E.SPARE in want[0]) == (not gone)
    if x == 1.0:
        assert list(want[0][:4]) == [13, 15, 16, 17]
    # the reserved key comes (back) as any key does: found with its state, or a first touch
    assert t.pull(np.array([E.SPARE], np.uint64))[0] == np.float32(0.0 if spare == "dropped" else 0.5)
    after = t.export()
    assert after[0][-1] == E.SPARE
    if gone:
        assert (after[1][-1], after[2][-1], after[3][-1]) == (0.0, 0.0, 0.0)
    else:
        assert after[3][-1] == np.float32(0.75)
    E.same_state(tuple(a[:-1] for a in after), tuple(a[want[0] != E.SPARE] for a in want))


def test_only_the_reserved_key_and_an_empty_table():
    t = capi.Table(capi.OPT_FTRL, 1, capacity=64)
    assert t.evict(INF) == (0, 0)
    one = tuple(a[-1:] for a in _edge_rows(0.0))
    t.import_(*one)
    assert t.evict(0.25) == (1, 0) and len(t) == 1      # n = 0.5: kept
    assert t.evict(INF) == (1, 1) and len(t) == 0 and t.settled == 0
    assert len(t.export()[0]) == 0


def test_refusals_of_the_table_layer():
    with pytest.raises(capi.XFError, match="only FTRL tables"):
        capi.Table(capi.OPT_SGD, 1, capacity=64).evict(1.0)
    with pytest.raises(capi.XFError, match="only tables of dim 1"):
        capi.Table(capi.OPT_FTRL, 4, capacity=64).evict(1.0)
    t = _table(_edge_rows(0.0))
    for bad in (-1.0, float("nan"), -INF):
        with pytest.raises(capi.XFError, match="n_below must be >= 0"):
            t.evict(bad)
    E.same_state(t.export(), _edge_rows(0.0))


# ------------------------------------------------------------------ 2. an unsettled arrival tier
def test_eviction_with_an_unsettled_arrival_tier():
    """some keys settled, some arrived since (pulled: zero rows; imported: with state): the result
    is that of defrag-then-filter"""
    B, S = _shape()
    n = B + 700
    state = E.crafted(n, E.drop_pattern("random_half", n, B, S))
    t = _table(state)
    rng = np.random.default_rng(7)
    fresh = np.unique(rng.integers(2**63, 2**64 - 2, size=900, dtype=np.uint64))
    pulled, imported = fresh[::2], fresh[1::2]
    assert not t.pull(pulled).any()
    d = rng.random(len(imported)) < 0.5
    _, w, nn, z = E.crafted(len(imported), d, seed=3)
    t.import_(imported, w, nn, z)
    assert t.settled == n and len(t) == n + len(fresh)
    before = t.export()
    want = _evict_and_check(t, E.X)
    assert not np.isin(pulled, want[0]).any()                      # first touches: (0, 0, 0) go
    assert np.array_equal(np.isin(imported, want[0]), ~d)
    assert len(before[0]) - len(want[0]) > n // 4


# ------------------------------------------------------------------ 3. the zero tail
def test_zero_tail_invariant_in_both_buffers():
    """rows between the new count and the old one are zero in BOTH state buffers: after a shrink,
    more new keys than were dropped are first touches (0, 0, 0) — straight away and after the
    defrag that moves them into the other buffer.  The second round's eviction settles arrivals
    first, so its target is the other of the two buffers."""
    B, S = _shape()
    n = 2 * B + 100
    t = _table(E.crafted(n, E.drop_pattern("random_half", n, B, S)))
    rng = np.random.default_rng(11)
    hi = 2**63
    for rnd in range(2):
        if rnd == 1:      # arrivals, and every row evictable or not anew, all with nonzero n and z
            t.pull(np.unique(rng.integers(hi, hi + 2**40, size=33, dtype=np.uint64)))
            hi += 2**41
            k = t.export()[0]
            _, w, nn, z = E.crafted(len(k), rng.random(len(k)) < 0.5, seed=5)
            t.import_(k, w, nn, z)
            assert t.settled < len(t)
        before = t.export()
        assert np.all(before[2] != 0) and np.count_nonzero(before[3]) > len(before[0]) // 2
        want = _evict_and_check(t, E.X, rnd)
        dropped = len(before[0]) - len(want[0])
        assert dropped > B // 2
        fresh = np.unique(rng.integers(hi, hi + 2**40, size=dropped + 77, dtype=np.uint64))
        hi += 2**41
        assert len(fresh) > dropped
        assert not E.bits(t.pull(fresh)).any()
        for settle in (False, True):
            if settle:
                t.defrag()
            after = t.export()
            at = np.isin(after[0], fresh)
            assert at.sum() == len(fresh)
            for a in after[1:]:
                assert not E.bits(a[at]).any(), (rnd, settle)
            E.same_state(tuple(a[~at] for a in after), want, (rnd, settle))


# ------------------------------------------------------------------ 4. the numbering
def test_nothing_dropped_leaves_the_numbering_alone():
    raw = E.stream()[0]
    keys = np.unique(raw[1])
    one = np.ones(len(keys), np.float32)
    t = _table((keys, one, one, -one))          # |z| = 1 >> lambda1: every step leaves a weight
    ws = capi.Workspace()
    b = capi.LocalBatch(t, *raw, retain_keys=False)
    capi.lr_step(t, b, ws)
    t.check()
    assert t.evict(INF) == (len(keys), 0)
    capi.lr_step(t, b, ws)                      # the rows it was compiled against are still those
    t.check()
    t.import_(keys[5:6], np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32))
    assert t.evict(INF) == (len(keys), 1)
    with pytest.raises(capi.XFError, match="compile it again"):
        capi.lr_step(t, b, ws)


# ------------------------------------------------------------------ 5. everything dropped
def test_everything_dropped_is_a_created_table_again():
    B, S = _shape()
    n = B + 5
    raw = E.stream()[1]
    ws = capi.Workspace()
    a = capi.Table(capi.OPT_FTRL, 1, capacity=_capacity(n), **E.HYPER)
    a.import_(*E.crafted(n, np.ones(n, bool)))
    a.pull(np.unique(raw[1])[:100])                   # (some of the minibatch's keys among them)
    assert a.evict(INF) == (n + 100, n + 100)
    assert len(a) == 0 and a.settled == 0 and a.capacity == _capacity(n)
    fresh = capi.Table(capi.OPT_FTRL, 1, capacity=_capacity(n), **E.HYPER)
    infos = []
    for t in (a, fresh):
        b = capi.LocalBatch(t, *raw)
        infos.append(b.cells_info())
        capi.lr_step(t, b, ws)
        t.check()
    assert infos[0] == infos[1]
    assert a.settled == fresh.settled == len(np.unique(raw[1]))   # the first-minibatch path
    assert not a.w_derived() and fresh.w_derived()    # (the import's verdict on `a` is sticky)
    E.same_state(a.export(), fresh.export())
    assert len(a) == len(np.unique(raw[1]))


# ------------------------------------------------------------------ 6. predictions, training
def _values(raw):
    rng = np.random.default_rng(len(raw[1]))
    return rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=len(raw[1]))


def _step(path, t, ws, raw):
    if path == "update_dev":
        b = capi.LocalBatch.update(t, ws, *raw)
    else:
        b = capi.LocalBatch(t, *raw, values=_values(raw) if path == "valued" else None)
        capi.lr_step(t, b, ws)
    t.check()
    return b


def _held(path, t, raw):
    return capi.LocalBatch(t, *raw, values=_values(raw) if path == "valued" else None)


@pytest.mark.parametrize("path,x", [("cells", E.X_TRAIN), ("cells", INF), ("update_dev", INF),
                                    ("valued", INF)])
def test_predictions_unchanged_and_training_goes_on(path, x):
    """lambda1 = 1.6e-3 (tests/_evict_checker.py): the oracle's CPU run of the T1 = 3 steps leaves
    59.5 % of the 4783 keys at w == 0, their n in [0, 2.4e-5] (tests/test_evict_cpu.py asserts
    10 % .. 90 %); x = 5e-6 splits them, inf takes them all.  Table A trains T1 minibatches,
    predicts, evicts, predicts again (==) and trains T2 more; table B starts from the filtered
    export of A and trains the same T2: the exports are =="""
    raw = E.stream()
    held = raw[-1]
    ws = capi.Workspace()
    a = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 15, **E.HYPER)
    for i in range(E.T1):
        _step(path, a, ws, raw[i])
    if path != "valued":
        for got, ref in zip(a.export(), E.oracle_after_t1()):
            assert got.dtype == ref.dtype and np.array_equal(got, ref)
    p0 = capi.lr_predict(a, _held(path, a, held), ws)
    before = a.export()
    zero = before[1] == 0
    assert 0.1 <= zero.mean() <= 0.9
    derived = a.w_derived()
    want, seen, dropped = E.evict(before, x)
    assert 0 < dropped <= zero.sum() and (dropped == zero.sum()) == (x == INF)
    assert a.evict(x) == (seen, dropped)
    assert a.w_derived() == derived
    E.same_state(a.export(), want)
    hb = _held(path, a, held)
    p1 = capi.lr_predict(a, hb, ws)
    assert p0.tobytes() == p1.tobytes()
    b = _table(want, **E.HYPER)
    if b.capacity != a.capacity:
        b.reserve(a.capacity)
    assert capi.lr_predict(b, _held(path, b, held), ws).tobytes() == p0.tobytes()
    for t in (a, b):
        for i in range(E.T1, E.T1 + E.T2):
            _step(path, t, ws, raw[i])
    E.same_state(a.export(), b.export())
    assert capi.lr_predict(a, hb, ws).tobytes() == \
        capi.lr_predict(b, _held(path, b, held), ws).tobytes()


# ------------------------------------------------------------------ 7. two ranks
def _rank_stream(rank):
    from tests._hyper_cases import synth
    rng = np.random.RandomState(60 + rank)
    return [synth(rng, 300, 10, 4000, 1.2 if i % 2 else None, True) for i in range(E.T1 + 2)]


def _two_rank(rank, world, port, schedule, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ["XF_COLLECTIVE_TIMEOUT_S"] = "60"
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 14, schedule=schedule,
                          seed=7, **E.HYPER)
        raw = _rank_stream(rank)
        out = {}

        def stage(name):
            for nm, a in zip("kwnz", st.w.export()):
                out[name + "_" + nm] = a
        alive = []
        for i in range(E.T1):
            alive.append(st.compile(*raw[i]))
            st.step(alive[-1])
        st.check()
        hb = st.compile(*raw[E.T1])
        out["p0"] = st.predict(hb)
        g.barrier()                       # (every rank's Pulls of the predict have been served)
        for nm, a in zip("kwnz", st.w.export()):
            out["before_" + nm] = a
        out["counts"] = np.array(st.evict(float("inf")), np.uint64)
        for nm, a in zip("kwnz", st.w.export()):
            out["after_" + nm] = a
        g.barrier()
        out["p1"] = st.predict(hb)
        last = st.compile(*raw[E.T1 + 1])
        st.step(last)
        st.step(alive[0])                 # a minibatch compiled before the eviction, replayed
        st.check()
        out["end_k"] = st.w.export()[0]
        stage("end")
        # all the held minibatches replayed as a second epoch, a second eviction, a third epoch
        for b in alive:
            st.step(b)
        st.check()
        stage("epoch2")
        out["counts2"] = np.array(st.evict(float("inf")), np.uint64)
        stage("evicted2")
        for b in alive:
            st.step(b)
        st.check()
        stage("epoch3")
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


def _two_rank_oracle(schedule):
    """what _two_rank does, on the evicting oracle under the schedule's pull / push rule: a step is
    one minibatch of either rank; a predict flushes and pulls (inserts) its keys
    -> {stage: state}, the two evictions' (seen, dropped)"""
    raws = [_rank_stream(r) for r in range(2)]
    rk = E.Ranks(E.EvictingStore(E.HYPER), schedule)
    stages = {}

    def turn(i):
        rk.step([raws[0][i], raws[1][i]])

    def predict():
        rk.flush()
        for r in range(2):
            rk.store.s.pull(np.unique(raws[r][E.T1][1]))
    for i in range(E.T1):
        turn(i)
    predict()
    stages["before"] = rk.export()
    c1 = rk.evict(INF)
    stages["after"] = rk.export()
    predict()
    turn(E.T1 + 1)
    turn(0)
    stages["end"] = rk.export()
    for i in range(E.T1):
        turn(i)
    stages["epoch2"] = rk.export()
    c2 = rk.evict(INF)
    stages["evicted2"] = rk.export()
    for i in range(E.T1):
        turn(i)
    stages["epoch3"] = rk.export()
    return stages, c1, c2


@pytest.mark.parametrize("schedule", ["sequential", "stale1"])
def test_two_ranks_evict_their_shards(tmp_path, schedule):
    port = free_port()
    SM._spawn(_two_rank, [(r, 2, port, schedule, str(tmp_path)) for r in range(2)])
    parts = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(2)]

    def cat(prefix):
        k = np.concatenate([p[prefix + "_k"] for p in parts])
        order = np.argsort(k)
        return tuple(np.concatenate([p[prefix + "_" + nm] for p in parts])[order] for nm in "kwnz")
    before, after = cat("before"), cat("after")
    want, seen, dropped = E.evict(before, INF)
    assert 0 < dropped < seen
    E.same_state(after, want)
    assert sum(int(p["counts"][0]) for p in parts) == seen
    assert sum(int(p["counts"][1]) for p in parts) == dropped
    for r, p in enumerate(parts):
        one, s1, d1 = E.evict(tuple(p["before_" + nm] for nm in "kwnz"), INF)
        assert (int(p["counts"][0]), int(p["counts"][1])) == (s1, d1) and d1 > 0, r
        assert len(p["p0"]) == 300 and p["p0"].tobytes() == p["p1"].tobytes(), r
        assert len(p["end_k"]) > len(p["after_k"])
    # every stage against the evicting oracle under the schedule's rule: the held minibatches
    # replayed as a second epoch, a second eviction, a third epoch
    stages, c1, c2 = _two_rank_oracle(schedule)
    assert c1 == (seen, dropped)
    for name in ("before", "after", "end", "epoch2", "evicted2", "epoch3"):
        E.same_state(cat(name), stages[name], (schedule, name))
    assert tuple(sum(int(p["counts2"][i]) for p in parts) for i in range(2)) == c2
    assert 0 < c2[1] < c2[0]
    # every dropped key of the replayed minibatches came back with the third epoch
    gone = np.setdiff1d(stages["epoch2"][0], stages["evicted2"][0])
    held = np.unique(np.concatenate([raw[1] for r in range(2) for raw in _rank_stream(r)[:E.T1]]))
    back = gone[np.isin(gone, held)]
    assert len(back) > 100 and np.isin(back, stages["epoch3"][0]).all()


def _owner_refused(port, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        msgs = []
        for sched in ("owner", "owner_stale1"):
            st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule=sched)
            try:
                st.evict(1.0)
                msgs.append(None)
            except capi.XFError as e:
                msgs.append(str(e))
            st.close()
        g.close()
        q.put((0, ("ok", msgs)))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_owner_schedules_and_other_trainers_are_refused():
    res = SM._spawn(_owner_refused, [(free_port(),)])
    assert res[0][1][0] == "ok", res
    for sched, msg in zip(("owner", "owner_stale1"), res[0][1][1]):
        assert msg and "schedule %s is not built" % sched in msg and "sequential" in msg, msg
    fm = capi.Sharded(model="fm", optimizer="ftrl", k=4, capacity=1 << 12)
    with pytest.raises(capi.XFError, match=r"only LR \(model 0\)"):
        fm.evict(1.0)
    fm.close()
    sgd = capi.Sharded(model="lr", optimizer="sgd", capacity=1 << 12)
    with pytest.raises(capi.XFError, match="only optimizer=ftrl"):
        sgd.evict(1.0)
    sgd.close()


# ------------------------------------------------------------------ 8. the worker
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("evict")
    shutil.copy(os.path.join(GOLDEN, "small_train-00000"), str(d / "train-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "test-00000"))
    return d


def _worker(data, tag, **extra):
    pred, mdl = str(data / ("pred_%s.txt" % tag)), str(data / ("model_%s.bin" % tag))
    x = capi.XFlow(str(data / "train"), str(data / "test"), model=0, capacity=1 << 14,
                   lambda1=E.L1, pred_path=pred, model_out=mdl, **extra)
    x.train()
    return x, pred, mdl


def _export(x):
    wh, _ = x.tables()
    return capi.Table.from_handle(wh, 1).export()


def _model(data, mdl):
    """the (keys, w, n, z) a model file holds: loaded into a worker that trains nothing"""
    y = capi.XFlow(str(data / "train"), str(data / "test"), model=0, capacity=1 << 14,
                   lambda1=E.L1)
    y.load(mdl)
    return y, _export(y)


def _test_keys(data):
    return np.unique(np.concatenate([b[1] for b in capi.read_blocks(str(data / "test-00000"),
                                                                     4 << 20)]))


def test_worker_end_to_end(data, capfd):
    """epochs=1 evict_n=inf against the same run without it.  The eviction runs after the last
    step, ahead of save_model and predict: the SAVED model is the plain one's filtered by the
    checker; the tables after predict hold, beside that, the test file's keys the predict pulled
    (first touches: (0, 0, 0)), as the plain run's do."""
    plain, pred0, mdl0 = _worker(data, "plain", epochs=1)
    capfd.readouterr()
    ev, pred1, mdl1 = _worker(data, "evict", epochs=1, evict_n="inf")
    lines = [ln for ln in capfd.readouterr().out.split("\n") if ln.startswith("evict epoch ")]
    for n in ("logloss_ref", "auc", "tp", "fp", "rows_trained"):
        assert ev.metric(n) == plain.metric(n), n
    assert open(pred0, "rb").read() == open(pred1, "rb").read()
    (_, m0), (_, m1) = _model(data, mdl0), _model(data, mdl1)
    # (200 rows a minibatch: one occurrence moves z by 2.5e-3 > lambda1, so only the keys whose
    # losses cancel stay at 0 — 6.7 % of the sample's keys after one epoch)
    want, seen, dropped = E.evict(m0, INF)
    E.same_state(m1, want)
    assert (ev.metric("evict_seen"), ev.metric("evict_dropped")) == (seen, dropped)
    assert ev.metric("evict_dropped") == len(m0[0]) - len(m1[0]) > 0
    assert lines == ["evict epoch 1: rows = %d dropped = %d" % (seen, dropped)]
    assert plain.metric("evict_seen") == plain.metric("evict_dropped") == 0
    # tables(): the filtered plain export + the test keys predict inserted again
    full = _export(plain)
    kept, _, _ = E.evict(full, INF)
    got = _export(ev)
    tk = _test_keys(data)
    extra = np.isin(got[0], tk) & ~np.isin(got[0], kept[0])
    assert extra.any() and np.all(np.isin(got[0][extra], full[0]))
    for a in got[1:]:
        assert not E.bits(a[extra]).any()
    E.same_state(tuple(a[~extra] for a in got), kept)
    assert ev.metric("keys") == len(got[0])
    # a saved and reloaded model predicts the same
    y, _ = _model(data, mdl1)
    y.set("pred_path", str(data / "pred_reload.txt"))
    y.predict()
    for n in ("logloss_ref", "auc", "tp", "fp"):
        assert y.metric(n) == ev.metric(n), n
    assert open(str(data / "pred_reload.txt"), "rb").read() == open(pred1, "rb").read()


def test_worker_evict_every_and_the_final_eviction(data, capfd):
    capfd.readouterr()
    ev, _, mdl = _worker(data, "every2", epochs=3, evict_every=2, evict_n="inf")
    lines = [ln for ln in capfd.readouterr().out.split("\n") if ln.startswith("evict epoch ")]
    assert [ln.split(":")[0] for ln in lines] == ["evict epoch 2", "evict epoch 3"], lines
    _, m = _model(data, mdl)
    assert len(m[0]) and E.evict(m, INF)[2] == 0            # no evictable row is saved
    assert ev.metric("evict_dropped") > 0
    # the epochs replay minibatches compiled before an eviction: the same model as the run that
    # evicts at every boundary but the first, whose dropped keys come back as first touches too
    every, _, mdl_b = _worker(data, "every1", epochs=3, evict_every=1, evict_n="inf")
    assert every.metric("rows_trained") == ev.metric("rows_trained")
    m_b = _model(data, mdl_b)[1]
    assert E.evict(m_b, INF)[2] == 0
    # both runs against the evicting oracle stepping the sample's one block epoch by epoch
    lines_b = [ln for ln in capfd.readouterr().out.split("\n") if ln.startswith("evict epoch ")]
    for x, saved, got_lines, k in ((ev, m, lines, 2), (every, m_b, lines_b, 1)):
        ref = E.worker_reference(str(data), 3, k, INF, lambda1=E.L1)
        assert ref["blocks"] == [1]
        E.same_state(saved, ref["model"], k)
        ll, auc, tp, fp = ref["metrics"]
        assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
            (np.float32(ll), np.float32(auc))
        assert (x.metric("tp"), x.metric("fp"), x.metric("rows_trained")) == (tp, fp, ref["rows"])
        assert x.metric("evict_seen") == sum(s for _, s, _ in ref["log"])
        assert x.metric("evict_dropped") == sum(d for _, _, d in ref["log"])
        assert got_lines == ["evict epoch %d: rows = %d dropped = %d" % l for l in ref["log"]]


def test_worker_refusals(data):
    for extra, why in ((dict(model=1, evict_n="inf"), r"model 1 \(FM\)"),
                       (dict(optimizer="sgd", evict_n=1.0), "optimizer=sgd")):
        x = capi.XFlow(str(data / "train"), str(data / "test"), **extra)
        with pytest.raises(capi.XFError, match=why):
            x.train()
    x = capi.XFlow(str(data / "train"), str(data / "test"))
    with pytest.raises(capi.XFError, match="evict_n must be"):
        x.set("evict_n", -1)
    x.set("evict_n", float("inf"))          # XFlow(..., evict_n=inf) goes through set()
    x.set("evict_every", 2)
