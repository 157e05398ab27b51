"""Minibatches compiled BEFORE a table eviction and stepped AFTER it, on real hardware.

An eviction compacts the state rows, so every row number handed out before it is stale; every
cache of row numbers hangs on the table's (uid, epoch) and is rebuilt from retained keys, a dropped
key re-entering as a first touch (0, 0, 0).  Here the held minibatches of an epoch are replayed
epoch after epoch across evictions — what the worker does with epochs > 1 and evict_n > 0 — and
every state is held to the evicting oracle (tests/_evict_checker.py: the CPU oracle's steps in
sum_mode(1) around the numpy eviction; tests/test_evict_cpu.py shows that the evictions bite and
that a run which ignored re-entry would end elsewhere) with == on bits: the table layer on every
batch kind and key build, one rank of capi.Sharded on the fused and the exchange path, and the
worker on a three-block text.  (Two ranks: tests/test_gpu_evict.py.)"""
import os
import subprocess
import traceback

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import _evict_checker as E
from xflow_amd import build, capi

from . import test_gpu_evict as TE             # _model (the module, not its tests)
from . import test_gpu_sharded_modes as SM     # _spawn
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(build.LIBDIR, "xflow_lr")
HYPERS = {"HYPER": E.HYPER, "ALL_ZERO": E.HYPER_ALL_ZERO}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------ 1. the table layer
def _held(kind, t, raws, retain=True):
    if kind == "local":
        return [capi.LocalBatch(t, *r, retain_keys=retain) for r in raws]
    if kind == "valued":
        return [capi.LocalBatch(t, *r, values=E.replay_values(r)) for r in raws]
    return [capi.Batch(*r) for r in raws]              # a key list: resolved at the step


def _table_replay(kind, hname, x, every, at=None, retain=True, settle_first=False):
    """table A compiles its T1 minibatches once and holds them; E.EPOCHS epochs of lr_step over
    them with t.evict(x) at the boundaries; every export and every (seen, dropped) against the
    evicting oracle; at the end lr_predict on the first held minibatch -> the exports"""
    valued = kind == "valued"
    raws = E.replay_stream()
    ref, store = E.replay_run(HYPERS[hname], x, every, valued=valued, at=at)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 15, **HYPERS[hname])
    ws = capi.Workspace()
    if settle_first:      # every key settled before the minibatches are compiled (first touches)
        keys = np.unique(np.concatenate([r[1] for r in raws]))
        assert not t.pull(keys).any()
        t.defrag()
        assert t.settled == len(t) - 1                 # (the reserved key's row follows the tier)
    held = _held(kind, t, raws, retain)
    got, i = [], 0
    for e in range(E.EPOCHS):
        for b in held:
            capi.lr_step(t, b, ws)
        t.check()
        assert ref[i][:2] == ("epoch", e)
        got.append(t.export())
        E.same_state(got[-1], ref[i][2], (kind, hname, x, "epoch", e))
        i += 1
        if i < len(ref) and ref[i][0] == "evict":
            assert t.evict(x) == ref[i][3], (kind, hname, x, "eviction after epoch", e)
            got.append(t.export())
            E.same_state(got[-1], ref[i][2], (kind, hname, x, "evicted after epoch", e))
            assert len(t) == len(ref[i][2][0])
            i += 1
    assert i == len(ref) and any(o[0] == "evict" for o in ref)
    want = store.predict(raws[0], E.replay_values(raws[0]) if valued else None)
    assert _bits(capi.lr_predict(t, held[0], ws)) == _bits(want)
    t.check()
    return got


SCHEDULES = [("HYPER", INF, 1), ("HYPER", INF, 2), ("HYPER", E.X_TRAIN, 1), ("HYPER", E.X_TRAIN, 2),
             ("ALL_ZERO", INF, 1)]
SIDS = ["inf-every", "inf-every2", "x-every", "x-every2", "all_zero-inf-every"]


@pytest.mark.parametrize("hname,x,every", SCHEDULES, ids=SIDS)
@pytest.mark.parametrize("kind", ["local", "valued", "keylist"])
def test_held_minibatches_step_on_across_evictions(kind, hname, x, every):
    """ALL_ZERO: every eviction empties the table, so the first replayed minibatch meets a created
    table again (the first-minibatch path) on a (uid, epoch) it does not know; four epochs, so
    both state buffers and both tiers have been the live one twice"""
    _table_replay(kind, hname, x, every)


@pytest.mark.parametrize("x", [INF, E.X_TRAIN], ids=["inf", "x"])
@pytest.mark.parametrize("kind", ["local", "valued", "keylist"])
def test_a_settled_table_that_loses_rows_under_held_minibatches(kind, x):
    """what guards xf_table_evict's OWN epoch bump.  The eviction settles the table first, and
    that defrag bumps the epoch itself whenever keys have arrived since the last one — as they
    have at every boundary of the schedules above (the first epoch's first touches, then the
    dropped keys coming back).  Here every key is settled before the minibatches are compiled
    and the first epoch brings none: the first eviction's defrag returns at once, rows are
    dropped, and nothing but the eviction's epoch tells the held minibatches (keys kept, valued,
    key list) that their row numbers are stale.  Without it they would step the rows of other
    keys: the export after the second epoch would differ from the oracle's."""
    _table_replay(kind, "HYPER", x, 1, settle_first=True)


@pytest.mark.parametrize("kind", ["local", "valued", "keylist"])
def test_an_eviction_that_drops_nothing_leaves_held_minibatches_alone(kind):
    ref = E.replay_run(E.HYPER, E.X_NONE, 0, at=E.AT_NONE, valued=kind == "valued")[0]
    counts = [o[3] for o in ref if o[0] == "evict"]
    assert len(counts) == 2 and all(d == 0 and s > 4000 for s, d in counts)
    _table_replay(kind, "HYPER", E.X_NONE, 0, at=E.AT_NONE)


@pytest.mark.parametrize("hname,x,every", [("HYPER", INF, 1), ("HYPER", E.X_TRAIN, 2),
                                           ("ALL_ZERO", INF, 1)],
                         ids=["inf-every", "x-every2", "all_zero-inf-every"])
def test_every_key_build_rebuilds_the_same_rows(hname, x, every):
    """key_build 0 .. 3 (xf_tune): each against the oracle, so all against each other"""
    runs = []
    try:
        for mode in range(4):
            capi.tune("key_build", mode)
            runs.append(_table_replay("local", hname, x, every))
    finally:
        capi.tune("key_build", 0)
    for mode, run in enumerate(runs[1:], 1):
        assert len(run) == len(runs[0])
        for a, b in zip(run, runs[0]):
            E.same_state(a, b, ("key_build", mode))


def test_a_minibatch_without_its_keys_is_refused_after_rows_were_dropped():
    raws = E.replay_stream()
    st = E.EvictingStore(E.HYPER)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 15, **E.HYPER)
    ws = capi.Workspace()
    assert not t.pull(np.unique(np.concatenate([r[1] for r in raws]))).any()
    t.defrag()            # (settled: compiling the later minibatches renumbers nothing)
    held = _held("local", t, raws, retain=False)
    for b, raw in zip(held, raws):
        capi.lr_step(t, b, ws)
        st.step(raw)
    t.check()
    counts = st.evict(INF)
    assert counts[1] > 0 and t.evict(INF) == counts
    before = t.export()
    E.same_state(before, st.export())
    for b in held:
        with pytest.raises(capi.XFError, match="did not keep its keys"):
            capi.lr_step(t, b, ws)
    t.check()
    E.same_state(t.export(), before)


def test_a_minibatch_without_its_keys_steps_on_when_nothing_was_dropped():
    """on an already settled table the eviction that drops nothing renumbers nothing"""
    _table_replay("local", "HYPER", E.X_NONE, 0, at=E.AT_NONE, retain=False, settle_first=True)


# ------------------------------------------------------------------ 2. one rank of capi.Sharded
def _sharded_replay(g, schedule, valued, x, every, settle=False):
    """-> [("epoch" | "evict", export, counts)], the predictions of the first held minibatch, the
    export after a freshly compiled minibatch's step.  settle: every key is pulled (a first touch)
    and the table settled before the minibatches are compiled, so that the first eviction's own
    defrag renumbers nothing and only the eviction's epoch marks the held rows stale"""
    raws = E.replay_stream()
    vals = [E.replay_values(r) if valued else None for r in raws]
    st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 15, schedule=schedule, seed=7,
                      **E.HYPER)
    if settle:
        keys = np.unique(np.concatenate([r[1] for r in raws]))
        assert not st.w.pull(keys).any()
        st.defrag()
        assert st.w.settled == len(st.w) - 1           # (the reserved key's row follows the tier)
    held = [st.compile(*r, keep=True, values=v) for r, v in zip(raws, vals)]
    out = []
    at = E.boundaries(E.EPOCHS, every)
    for e in range(E.EPOCHS):
        for b in held:
            st.step(b)
        st.check()
        out.append(("epoch", st.w.export(), None))
        if e in at:
            counts = st.evict(x)
            out.append(("evict", st.w.export(), counts))
    pctr = st.predict(held[0])
    fresh = st.compile(*raws[1], keep=True, values=vals[1])    # the count went down and up again
    st.step(fresh)
    st.check()
    after = st.w.export()
    del held, fresh
    st.close()
    return out, pctr, after


def _check_sharded(res, rule, valued, x, every):
    out, pctr, after = res
    raws = E.replay_stream()
    ref, store = E.replay_run(E.HYPER, x, every, valued=valued, schedule=rule)
    assert len(out) == len(ref) and any(o[0] == "evict" for o in ref)
    for got, want in zip(out, ref):
        assert got[0] == want[0]
        E.same_state(got[1], want[2], (rule, valued) + want[:2])
        assert got[2] == want[3], (rule, valued) + want[:2]
    v0, v1 = (E.replay_values(raws[i]) if valued else None for i in (0, 1))
    assert _bits(pctr) == _bits(store.predict(raws[0], v0))
    rk = E.Ranks(store, rule)
    rk.step([raws[1]], [v1])
    E.same_state(after, rk.export(), (rule, valued, "a fresh minibatch after the run"))


ONE_RANK = [("sequential", False, INF, 1), ("stale1", False, E.X_TRAIN, 2),
            ("sequential", True, INF, 1), ("stale1", False, INF, 1)]
OIDS = ["sequential-inf-every", "stale1-x-every2", "sequential-values-inf-every",
        "stale1-inf-every"]


@pytest.mark.parametrize("schedule,valued,x,every", ONE_RANK, ids=OIDS)
def test_one_rank_fused_replays_across_evictions(schedule, valued, x, every):
    """the object the worker drives; the fused step of one rank is one step after the other under
    either schedule"""
    _check_sharded(_sharded_replay(None, schedule, valued, x, every), "sequential", valued, x, every)


def _general_rank(port, schedule, valued, x, every, q, settle=False):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"         # a group of one on the exchange path
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ["XF_COLLECTIVE_TIMEOUT_S"] = "60"
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        res = _sharded_replay(g, schedule, valued, x, every, settle)
        g.close()
        q.put((0, ("ok", res)))
    except Exception:
        q.put((0, traceback.format_exc()))


@pytest.mark.parametrize("schedule,valued,x,every", ONE_RANK, ids=OIDS)
def test_one_rank_on_the_exchange_path_replays_across_evictions(schedule, valued, x, every):
    """XF_SHARDED_GENERAL=1 in a spawned child: front_pull's rows_uid / rows_epoch check; under
    stale1 the previous step's Push lands after this step's Pull, and an eviction flushes"""
    res = SM._spawn(_general_rank, [(free_port(), schedule, valued, x, every)])
    assert res[0][1][0] == "ok", res
    _check_sharded(res[0][1][1], schedule, valued, x, every)


def _settled_rank(port, schedule, valued, x, every, q):
    _general_rank(port, schedule, valued, x, every, q, settle=True)


SETTLED = [("sequential", False), ("stale1", False), ("sequential", True)]


@pytest.mark.parametrize("schedule,valued", SETTLED,
                         ids=["sequential", "stale1", "sequential-values"])
@pytest.mark.parametrize("path", ["fused", "exchange"])
def test_one_rank_on_a_settled_table_that_loses_rows(path, schedule, valued):
    """guards xf_table_evict's own epoch bump on the trainer's two caches of row numbers (the
    fused step's cells, front_pull's rows_uid / rows_epoch): every key settled before the
    minibatches are compiled, so the first eviction's defrag has nothing to renumber"""
    if path == "fused":
        res, rule = _sharded_replay(None, schedule, valued, INF, 1, settle=True), "sequential"
    else:
        got = SM._spawn(_settled_rank, [(free_port(), schedule, valued, INF, 1)])
        assert got[0][1][0] == "ok", got
        res, rule = got[0][1][1], schedule
    _check_sharded(res, rule, valued, INF, 1)


# ------------------------------------------------------------------ 3. the worker
@pytest.fixture(scope="module")
def text(tmp_path_factory):
    import pathlib
    return pathlib.Path(E.worker_text(tmp_path_factory.mktemp("evict_replay"), two=True))


_refs = {}


def _reference(text, epochs, every, x, **kw):
    key = (epochs, every, x) + tuple(sorted(kw.items()))
    if key not in _refs:
        _refs[key] = E.worker_reference(str(text), epochs, every, x, **kw)
    return _refs[key]


def _pred_lines(ref):
    return ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(ref["pctr"], ref["labels"])]


def check_worker(x, ref, pred, saved, lines):
    E.same_state(saved, ref["model"])
    assert len(saved[0]) > 100 and E.evict(saved, INF)[2] < len(saved[0])
    assert open(pred).read().split("\n")[:-1] == _pred_lines(ref)
    ll, auc, tp, fp = ref["metrics"]
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    assert x.metric("rows_trained") == ref["rows"]
    assert x.metric("evict_seen") == sum(s for _, s, _ in ref["log"])
    assert x.metric("evict_dropped") == sum(d for _, _, d in ref["log"]) > 0
    assert lines == ["evict epoch %d: rows = %d dropped = %d" % l for l in ref["log"]]


WORKER = [(4, 1, INF, "host", 1), (4, 1, INF, "gpu", 1), (4, 1, INF, "host", 0),
          (4, 1, INF, "gpu", 0), (4, 2, INF, "gpu", 1), (3, 2, INF, "host", 0),
          (4, 1, E.X_WORKER, "gpu", 0), (4, 2, E.X_WORKER, "host", 1),
          (3, 2, E.X_WORKER, "gpu", 1)]


@pytest.mark.parametrize("epochs,every,x,ingest,cache", WORKER,
                         ids=["%d-every%d-%g-%s-cache%d" % c for c in WORKER])
def test_worker_replays_its_cache_across_evictions(text, capfd, epochs, every, x, ingest, cache):
    """the worker replays cache_ after each evict_epoch (cache_batches=0: compiles the blocks
    again): the saved model, the predictions, the metrics, the counts and the printed lines
    against the evicting oracle stepping the 1 MiB blocks epoch by epoch"""
    ref = _reference(text, epochs, every, x)
    assert ref["blocks"] == [3]
    tag = "%d_%d_%g_%s_%d" % (epochs, every, x, ingest, cache)
    pred, mdl = str(text / ("pred_%s.txt" % tag)), str(text / ("model_%s.bin" % tag))
    capfd.readouterr()
    w = capi.XFlow(str(text / "train"), str(text / "test"), model=0, capacity=1 << 14,
                   block_size_mb=1, lambda1=E.L1_WORKER, epochs=epochs, evict_every=every,
                   evict_n=x, ingest=ingest, cache_batches=cache, pred_path=pred, model_out=mdl)
    w.train()
    lines = [ln for ln in capfd.readouterr().out.split("\n") if ln.startswith("evict epoch ")]
    assert (w.metric("blocks_gpu") > 0) == (ingest == "gpu")
    check_worker(w, ref, pred, TE._model(text, mdl)[1], lines)


def test_worker_with_feature_values_replays_across_evictions(text, capfd):
    ref = _reference(text, 4, 1, INF, valued=True)
    pred, mdl = str(text / "pred_values.txt"), str(text / "model_values.bin")
    capfd.readouterr()
    w = capi.XFlow(str(text / "train"), str(text / "test"), model=0, capacity=1 << 14,
                   block_size_mb=1, lambda1=E.L1_WORKER, epochs=4, evict_every=1, evict_n="inf",
                   feature_values="on", ingest="host", pred_path=pred, model_out=mdl)
    w.train()
    lines = [ln for ln in capfd.readouterr().out.split("\n") if ln.startswith("evict epoch ")]
    check_worker(w, ref, pred, TE._model(text, mdl)[1], lines)
    assert _reference(text, 4, 1, INF)["log"] != ref["log"]      # (the values change the run)


@pytest.mark.parametrize("schedule", ["sequential", "stale1"])
def test_local_sh_two_workers_replay_across_evictions(text, tmp_path, schedule):
    """scripts/local.sh 2 2 xflow_lr ... epochs 3, evict_every=1: a turn is one block of every rank
    that still has one (rank 1's last turn is empty) under the schedule's pull / push rule, the
    epoch's end flushes, every rank evicts its shard; the two saved shard files in one table"""
    ref = _reference(text, 3, 1, INF, schedule=schedule, ranks=2)
    assert ref["blocks"] == [3, 2]
    ckpt, pred = str(tmp_path / "model"), str(tmp_path / "pred.txt")
    env = dict(os.environ, DMLC_PS_ROOT_PORT=str(free_port()))
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI,
                          str(text / "train"), str(text / "test"), "0", "3", "transport=host",
                          "block_size_mb=1", "capacity=16384", "model_out=" + ckpt,
                          "pred_path=" + pred, "lambda1=%r" % E.L1_WORKER, "evict_n=inf",
                          "evict_every=1", "schedule=" + schedule],
                         capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert O.format_auc_line(*ref["metrics"]) in lines, lines
    assert open(pred).read().split("\n")[:-1] == _pred_lines(ref)
    # (the CLI run leaves no handle to ask for evict_seen / evict_dropped: the printed lines carry
    # every eviction's counts summed over the ranks, whose totals those two metrics are)
    assert [ln for ln in lines if ln.startswith("evict epoch ")] == \
        ["evict epoch %d: rows = %d dropped = %d" % l for l in ref["log"]]
    one = capi.Sharded(None, model="lr", optimizer="ftrl", capacity=1 << 15)
    one.load(ckpt)                                               # two shard files -> one table
    E.same_state(one.w.export(), ref["model"])
    one.close()
