"""Progressive validation on real hardware: the accumulate kernel's counts against the restatement
(tests/_progress_checker.py) with ==, the tap of every training step path (counts == the
restatement of the step's own losses; tables bit for bit those of the step without a progress),
the weight of negative subsampling beside it, two ranks on one GPU, and the worker end to end."""
import math
import os
import re
import shutil
import subprocess
import traceback

import numpy as np
import pytest

from xflow_amd import build, capi

from . import _ffm_checker as FF
from . import _progress_checker as P
from . import _sharded_modes_checker as M
from . import _valued_cases as Cs
from . import test_gpu_fm_canonical as TC      # synth, _tables (the module, not its tests)
from . import test_gpu_sharded_modes as SM     # _spawn, _trainer, _import_old, _compile
from .conftest import GOLDEN
from .test_gpu_parity import synth
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(build.LIBDIR, "xflow_lr")
W4 = 4.0
W03 = float(np.float32(1) / np.float32(0.3))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def eq(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), what


def same_counts(got, want, what=""):
    (gc, go), (wc, wo) = got, want
    bad = np.argwhere(gc != wc)
    assert len(bad) == 0, (what, bad[:5], gc[gc != wc][:5], wc[gc != wc][:5])
    assert list(go) == list(wo), (what, go, wo)


# ------------------------------------------------------------------ the kernel
def _accumulate(p, loss, labels):
    import torch
    loss = np.ascontiguousarray(loss, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    if len(loss) == 0:
        p.accumulate(None, None, 0)
        return
    d_loss, d_lab = torch.from_numpy(loss).cuda(), torch.from_numpy(labels).cuda()
    p.accumulate(d_loss.data_ptr(), d_lab.data_ptr(), len(loss))
    torch.cuda.synchronize()


def _random_losses(rng, R):
    """logistic rows: p from spread logits, loss = p - label in fp32"""
    p = (1.0 / (1.0 + np.exp(-rng.normal(0, 4, size=R)))).astype(np.float32)
    y = (rng.random(R) < 0.3).astype(np.int32)
    return (p - y.astype(np.float32)).astype(np.float32), y


@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_counts_of_random_rows(R):
    rng = np.random.default_rng(100 + R)
    loss, y = _random_losses(rng, R)
    p = capi.Progress()
    before = capi.progress_launches()
    _accumulate(p, loss, y)
    assert capi.progress_launches() - before == (1 if R else 0)
    same_counts(p.read(), P.counts_of(loss, y))


@pytest.mark.parametrize("case", ["one_rank", "rank_C", "both_classes_rank_C"])
def test_every_row_on_one_rank(case):
    R = 4097
    q = np.float32(0.5) if case != "one_rank" else np.float32(0.03125)
    y = np.zeros(R, np.int32)
    if case == "both_classes_rank_C":
        y[::3] = 1
    loss = np.where(y != 0, -q, q).astype(np.float32)
    p = capi.Progress()
    _accumulate(p, loss, y)
    counts, other = p.read()
    same_counts((counts, other), P.counts_of(loss, y))
    r = P.C if case != "one_rank" else capi.progress_rank(0.03125)
    assert counts[0, r] == (y == 0).sum() and counts[1, r] == (y != 0).sum()
    assert counts.sum() == R


def test_more_distinct_ranks_than_the_lds_table_holds():
    """one workgroup's rows on more distinct (class, rank) pairs than its table has slots: rows
    that find no slot within the probes add straight to global memory"""
    shape = capi.progress_shape()
    rows, slots = shape["rows"], shape["slots"]
    assert rows > slots                      # a full workgroup of distinct pairs must overflow
    R = 2 * rows + 17                        # two full workgroups and a ragged third
    ranks = (np.arange(R, dtype=np.int64) * 37) % (P.C - 2048) + 1024   # distinct inside a workgroup
    assert len(np.unique(ranks[:rows])) == rows > slots
    q = (ranks.astype(np.uint32) << np.uint32(P.SH)).view(np.float32)   # the buckets' lower edges
    y = (np.arange(R) % 2).astype(np.int32)
    loss = np.where(y != 0, -q, q).astype(np.float32)
    assert np.array_equal(P.ranks(loss), ranks)
    p = capi.Progress()
    _accumulate(p, loss, y)
    same_counts(p.read(), P.counts_of(loss, y))


def test_edges_nan_and_labels_outside_01():
    qs = [e[0] for e in P.EDGES]
    loss = np.array(qs + [-x for x in qs] + [-0.0, float("nan"), 1.5, -1.5, float("inf"), 0.3, 0.3,
                                             -0.7, -0.7], np.float32)
    y = np.array([0] * len(qs) + [1] * len(qs) + [0, 0, 1, 0, 1, -1, 2, -1, 2], np.int32)
    p = capi.Progress()
    _accumulate(p, loss, y)
    counts, other = p.read()
    same_counts((counts, other), P.counts_of(loss, y))
    assert list(other) == [2, 2]             # NaN and -1.5 with label 0; 1.5 and inf with label 1
    for q, r in P.EDGES:
        assert counts[0, r] >= 1 and counts[1, r] >= 1
    # labels -1 and 2 are positives (label != 0), as for the negatives' weight
    assert counts[1, capi.progress_rank(0.3)] == 2 and counts[1, capi.progress_rank(0.7)] == 2


def test_two_accumulates_one_read_and_reset():
    rng = np.random.default_rng(5)
    a, b = _random_losses(rng, 700), _random_losses(rng, 1300)
    p = capi.Progress()
    _accumulate(p, *a)
    _accumulate(p, *b)
    ca, cb = P.counts_of(*a), P.counts_of(*b)
    same_counts(p.read(reset=True), (ca[0] + cb[0], ca[1] + cb[1]))
    counts, other = p.read()
    assert counts.sum() == 0 and other.sum() == 0
    _accumulate(p, *a)
    same_counts(p.read(), ca)


# ------------------------------------------------------------------ the step paths
def _table_bits(tables):
    return [np.ascontiguousarray(a).tobytes() for t in tables for a in t.export()[:4]]


def _lr_raws():
    rng = np.random.RandomState(3040)
    return [synth(rng, 3000, 40, 30000, 1.15 if i == 2 else None, i > 0) for i in range(3)]


def _run_lr_cells(ws):
    """the local build's cells (steps 0, 2) and the generic build's (step 1)"""
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 17)
    out = []
    for i, raw in enumerate(_lr_raws()):
        b = capi.Batch(*raw) if i == 1 else capi.LocalBatch(t, *raw)
        capi.lr_step(t, b, ws)
        out.append((ws.fetch_loss(b.R), raw[2]))
    return [t], out


def _run_lr_update(ws):
    """xf_lr_update_dev: steps 2 and 3 bring new keys — a second forward segment"""
    R, nnz, nkeys = 3000, 40, 30000
    rng = np.random.RandomState(17)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 17)
    out, segs = [], []
    for step in range(4):
        hi = nkeys // 2 if step < 2 else nkeys
        raw = synth(rng, R, nnz, hi, 1.15 if step % 2 else None, True)
        b = capi.LocalBatch.update(t, ws, *raw)
        out.append((ws.fetch_loss(R), raw[2]))
        segs.append(b.cells_info()["segments"])
        if step == 0:
            t.pull(capi.hash_decimal_range(0, nkeys // 2))
            t.defrag()
    assert segs[1:] == [1, 2, 2], segs
    return [t], out


def _run_valued(ws, path):
    mbs = Cs.stream("ragged")
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 16)
    t.import_(*Cs.old_state(Cs.stream_keys(mbs), "ftrl", 1, "w"))
    out = []
    for rp, ks, vs, lb in mbs:
        b = capi.LocalBatch(t, rp, ks, lb, values=vs) if path == "local" else \
            capi.Batch(rp, ks, lb, on_gpu=True, values=vs)
        capi.lr_step(t, b, ws)
        out.append((ws.fetch_loss(b.R), lb))
    return [t], out


def _run_reference_fm(ws, k):
    """k = 4: the forward over the table-resident records; k = 10: the row-gather forward"""
    opt = capi.OPT_SGD if k == 4 else capi.OPT_FTRL
    init = (capi.INIT_CONST, 0.001) if k == 4 else (capi.INIT_HASHNORM, 0.0)
    rng = np.random.RandomState(k)
    tw = capi.Table(opt, 1, capacity=1 << 16)
    tv = capi.Table(opt, k, init[0], init[1], seed=99, capacity=1 << 16)
    out = []
    for i in range(3):
        raw = synth(rng, 500, 30, 4000, 1.3 if i == 2 else None, True)
        capi.fm_step(tw, tv, capi.Batch(*raw), ws)
        out.append((ws.fetch_loss(500), raw[2]))
    return [tw, tv], out


def _run_canonical(ws):
    rng = np.random.RandomState(16)
    tw, tv, _ = TC._tables("ftrl", 16)
    ws.fm_mode("canonical")
    out = []
    for z in (None, 1.3, None):
        raw = TC.synth(rng, 400, 25, 3000, z)
        b = capi.Batch(*raw, on_gpu=True)
        capi.fm_step(tw, tv, b, ws)
        out.append((ws.fetch_loss(b.R), raw[2]))
    return [tw, tv], out


def _run_ffm(ws):
    Fd, k = 18, 4
    mbs = FF.stream("ragged", Fd)
    tw = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 16)
    tv = capi.Table(capi.OPT_FTRL, Fd * k, capi.INIT_HASHNORM, 0.0, seed=7, capacity=1 << 16)
    tw.import_(*Cs.old_state(FF.stream_keys(mbs), "ftrl", 1, "w"))
    tv.import_(*Cs.old_state(FF.stream_keys(mbs), "ftrl", Fd * k))
    ws.fm_fields(Fd)
    ws.fm_mode("field_aware")
    out = []
    for rp, ks, fg, vs, lb in mbs:
        b = capi.Batch(rp, ks, lb, on_gpu=True, values=vs, fields=Fd, fgid=fg)
        capi.fm_step(tw, tv, b, ws)
        out.append((ws.fetch_loss(b.R), lb))
    return [tw, tv], out


PATHS = {
    "lr_cells": _run_lr_cells,
    "lr_update_dev": _run_lr_update,
    "valued_lr_generic": lambda ws: _run_valued(ws, "generic"),
    "valued_lr_local": lambda ws: _run_valued(ws, "local"),
    "reference_fm_records": lambda ws: _run_reference_fm(ws, 4),
    "reference_fm": lambda ws: _run_reference_fm(ws, 10),
    "canonical_fm": _run_canonical,
    "field_aware_fm_values": _run_ffm,
}


def _run(path, progress, w=1.0):
    ws = capi.Workspace()
    if w != 1.0:
        ws.neg_weight(w)
    p = capi.Progress() if progress else None
    if p is not None:
        ws.progress(p)
    tables, steps = PATHS[path](ws)
    bits = _table_bits(tables)
    counts = p.read() if p is not None else None
    ws.progress(None)
    return bits, steps, counts


@pytest.mark.parametrize("path", list(PATHS))
def test_every_step_path_at_weight_one(path):
    launches, weighs = capi.progress_launches(), capi.lib().xf_weigh_negatives_launches()
    off_bits, off_steps, _ = _run(path, False)
    assert capi.progress_launches() == launches          # off is off
    on_bits, on_steps, counts = _run(path, True)
    assert capi.progress_launches() - launches == len(on_steps)      # one launch a step
    assert capi.lib().xf_weigh_negatives_launches() == weighs        # no weight kernel at w = 1
    assert on_bits == off_bits, "tables with a progress attached"
    want_c = np.zeros((2, P.RANKS), np.uint64)
    want_o = np.zeros(2, np.uint64)
    for (loss_on, labels), (loss_off, _) in zip(on_steps, off_steps):
        eq(loss_on, loss_off, "the step's losses")
        c, o = P.counts_of(loss_on, labels)
        want_c += c
        want_o += o
    same_counts(counts, (want_c, want_o))
    assert counts[0].sum() == sum(len(s[1]) for s in on_steps) and counts[1].sum() == 0


@pytest.mark.parametrize("w", [W4, W03], ids=["w4", "w1/0.3"])
@pytest.mark.parametrize("path", ["lr_cells", "lr_update_dev", "valued_lr_local", "canonical_fm"])
def test_weighted_steps(path, w):
    L = capi.lib()
    w0 = L.xf_weigh_negatives_launches()
    off_bits, off_steps, _ = _run(path, False, w)
    w1 = L.xf_weigh_negatives_launches()
    on_bits, on_steps, counts = _run(path, True, w)
    w2 = L.xf_weigh_negatives_launches()
    assert on_bits == off_bits, "tables with a progress attached"
    for (a, _), (b, _) in zip(on_steps, off_steps):
        eq(a, b, "the weighted losses")
    n = len(on_steps)
    if path == "canonical_fm":
        assert (w1 - w0, w2 - w1) == (n, n)
    else:                     # the cells steps launch the weight kernel only beside a progress
        assert (w1 - w0, w2 - w1) == (0, n)
    # the counts are those of the unweighted losses: undo the weight where that is exact (w = 4);
    # fp32(1/0.3) is covered by the next test, against the same minibatch at w = 1
    if w == W4:
        want_c = np.zeros((2, P.RANKS), np.uint64)
        want_o = np.zeros(2, np.uint64)
        for loss, labels in on_steps:
            plain = np.where(np.asarray(labels) == 0, loss / np.float32(4), loss).astype(np.float32)
            c, o = P.counts_of(plain, labels)
            want_c += c
            want_o += o
        same_counts(counts, (want_c, want_o))


@pytest.mark.parametrize("w", [W4, W03], ids=["w4", "w1/0.3"])
@pytest.mark.parametrize("model", ["lr_cells", "canonical_fm"])
def test_weighted_counts_are_those_of_weight_one(model, w):
    """one minibatch on a fresh table: the counts do not see the weight"""
    got = []
    for weight in (1.0, w):
        ws = capi.Workspace()
        ws.neg_weight(weight)
        p = capi.Progress()
        ws.progress(p)
        if model == "lr_cells":
            first, raw = _lr_raws()[:2]
            t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 17)
            capi.lr_step(t, capi.LocalBatch(t, *first), capi.Workspace())   # (not every row at C)
            capi.lr_step(t, capi.LocalBatch(t, *raw), ws)
        else:
            tw, tv, _ = TC._tables("ftrl", 16)
            ws.fm_mode("canonical")
            raw = TC.synth(np.random.RandomState(16), 400, 25, 3000, None)
            capi.fm_step(tw, tv, capi.Batch(*raw, on_gpu=True), ws)
        got.append(p.read())
    same_counts(got[1], got[0])
    assert got[0][0].sum() == len(raw[2])


def test_known_answer_on_a_fresh_table():
    """a fresh LR table's weights are zero: every row's p is 0.5"""
    rng = np.random.RandomState(1)
    raw = synth(rng, 256, 20, 5000, None, True)
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 15)
    ws, p = capi.Workspace(), capi.Progress()
    ws.progress(p)
    capi.lr_step(t, capi.LocalBatch(t, *raw), ws)
    counts, other = p.read()
    assert counts[:, P.C].sum() == 256 and counts.sum() == 256 and other.sum() == 0
    m = capi.progress_summary(counts, other)
    assert P.same(m, P.summary(counts, other))
    assert m["logloss"] == math.log(2.0) and m["auc"] == 0.5 and m["pctr"] == 0.5
    assert m["ctr"] == (raw[2] != 0).mean()
    # predict never accumulates
    capi.lr_predict(t, capi.Batch(*raw), ws)
    same_counts(p.read(), (counts, other))


# ------------------------------------------------------------------ two ranks on one GPU
TWO = (("lr", 2, 0, 0, "ftrl", "sequential", "ragged", False),
       ("lr", 2, 0, 0, "ftrl", "stale1", "ragged", False),
       ("canonical", 2, 0, 4, "ftrl", "sequential", "ragged", False),
       ("canonical", 2, 0, 4, "ftrl", "stale1", "ragged", False))


def _progress_rank(rank, world, port, spec, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        mode, _, F, k, opt, schedule, case, valued = spec
        strs = M.streams(mode, case, world, F)
        st = SM._trainer(g, spec)
        st.set_progress(True)
        SM._import_old(st, spec, strs, rank, world)
        train, _ = strs[rank]
        alive, losses, labels = [], [], []
        for mb in train:
            b = st.compile(mb[0], mb[1], mb[4])
            alive.append(b)
            st.step(b)
            losses.append(st.last_loss(b))
            labels.append(np.asarray(mb[4], np.int32))
        own_c, own_o = st.progress_read()
        mer_c, mer_o = st.progress_read(reset=True, merged=True)
        zero_c, zero_o = st.progress_read()
        st.check()
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), own_c=own_c, own_o=own_o, mer_c=mer_c,
                 mer_o=mer_o, left=np.array([zero_c.sum() + zero_o.sum()]),
                 loss=np.concatenate(losses), labels=np.concatenate(labels))
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("spec", TWO, ids=["%s-%s" % (s[0], s[5]) for s in TWO])
def test_two_ranks(tmp_path, spec):
    world = 2
    port = free_port()
    SM._spawn(_progress_rank, [(r, world, port, spec, str(tmp_path)) for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    sum_c = parts[0]["own_c"] + parts[1]["own_c"]
    sum_o = parts[0]["own_o"] + parts[1]["own_o"]
    for r in range(world):
        same_counts((parts[r]["mer_c"], parts[r]["mer_o"]), (sum_c, sum_o), "merged, rank %d" % r)
        same_counts((parts[r]["own_c"], parts[r]["own_o"]),
                    P.counts_of(parts[r]["loss"], parts[r]["labels"]), "rank %d's own" % r)
        assert parts[r]["left"][0] == 0
        assert parts[r]["own_c"].sum() == len(parts[r]["labels"]) > 0


def _owner_refusal(port, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"       # a group of one on the exchange path
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        seen = []
        for sched in ("owner", "owner_stale1"):
            st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule=sched)
            st.set_progress(False)                   # (off is the default: accepted)
            try:
                st.set_progress(True)
            except capi.XFError as e:
                assert re.search(r"xf_sharded_progress.*schedule %s\b" % sched, str(e)) \
                    and "sequential" in str(e), str(e)
                seen.append(sched)
            st.close()
        st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule="stale1")
        st.set_progress(True)
        try:
            st.set_schedule("owner")
        except capi.XFError as e:
            assert "xf_sharded_set_schedule" in str(e), str(e)
            seen.append("then owner")
        st.set_schedule("sequential")
        try:
            capi.Sharded(g, model="lr", capacity=1 << 12).progress_read()
        except capi.XFError as e:
            assert "progressive validation is off" in str(e), str(e)
            seen.append("read while off")
        st.close()
        g.close()
        q.put((0, ("ok", seen)))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_owner_schedules_refuse_progress():
    res = SM._spawn(_owner_refusal, [(free_port(),)])
    assert res[0][1] == ("ok", ["owner", "owner_stale1", "then owner", "read while off"]), res


# ------------------------------------------------------------------ the worker end to end
EPOCHS = 3
NAMES = ("logloss", "auc", "auc_slack", "ctr", "pctr")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("progress")
    shutil.copy(os.path.join(GOLDEN, "small_train-00000"), str(d / "train-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "test-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "train-00001"))   # (two workers)
    return d


_refs = {}


def reference(data, model):
    """the same blocks through capi.Sharded with progress on: per epoch, the summary of its counts"""
    if model not in _refs:
        st = capi.Sharded(model="lr" if model == 0 else "fm", capacity=1 << 14)
        st.set_progress(True)
        blocks = [st.compile(rp, keys, labels) for rp, keys, fg, labels, vals in
                  capi.read_blocks(str(data / "train-00000"), 2 << 20, values=True)]
        assert len(blocks) == 1
        out = []
        for epoch in range(EPOCHS):
            for b in blocks:
                st.step(b)
            counts, other = st.progress_read(reset=True)
            assert counts.sum() == sum(b.R for b in blocks)
            out.append(capi.progress_summary(counts, other))
            assert P.same(out[-1], P.summary(counts, other))
        st.close()
        _refs[model] = out
    return _refs[model]


def run_worker(data, model, ingest, tag, **extra):
    pred = str(data / ("pred_%s.txt" % tag))
    mdl = str(data / ("model_%s.bin" % tag))
    x = capi.XFlow(str(data / "train"), str(data / "test"), model=model, capacity=1 << 14,
                   ingest=ingest, epochs=EPOCHS, pred_path=pred, model_out=mdl, **extra)
    x.train()
    return x, pred, mdl


@pytest.mark.parametrize("ingest", ["host", "gpu"])
@pytest.mark.parametrize("model", [0, 1], ids=["lr", "fm"])
def test_worker_end_to_end(data, model, ingest):
    ref = reference(data, model)
    tag = "%d%s" % (model, ingest)
    x, pred, mdl = run_worker(data, model, ingest, tag + "on", progress=1)
    for n in NAMES:
        assert x.metric("progress_" + n) == ref[-1][n], n
    assert x.metric("progress_rows") == ref[-1]["rows_pos"] + ref[-1]["rows_neg"]
    assert x.metric("progress_logloss_first") == ref[0]["logloss"]
    assert x.metric("progress_auc_first") == ref[0]["auc"]
    if model == 0:      # a fresh LR table: epoch 0 is ln 2 (200 rows: not a power of two, 1 ulp)
        assert abs(ref[0]["logloss"] - math.log(2.0)) < 1e-15 and ref[0]["auc"] == 0.5
    assert ref[-1]["logloss"] < ref[0]["logloss"]
    y, pred_off, mdl_off = run_worker(data, model, ingest, tag + "off")
    assert open(pred, "rb").read() == open(pred_off, "rb").read()
    assert open(mdl, "rb").read() == open(mdl_off, "rb").read()
    for n in ("logloss_ref", "auc", "tp", "fp", "keys", "rows_trained"):
        assert x.metric(n) == y.metric(n), n
    with pytest.raises(capi.XFError):
        y.metric("progress_logloss")


def _cli(args, cwd, prefix=()):
    out = subprocess.run(list(prefix) + [CLI] + args, capture_output=True, text=True, timeout=300,
                         cwd=str(cwd))
    assert out.returncode == 0, out.stderr
    return out.stdout.split("\n")


def test_cli_prints_one_line_per_epoch(data, tmp_path):
    ref = reference(data, 0)
    base = [str(data / "train"), str(data / "test"), "0", str(EPOCHS), "capacity=16384"]
    on = _cli(base + ["pred_path=on.txt", "progress=1"], tmp_path)
    off = _cli(base + ["pred_path=off.txt"], tmp_path)
    lines = [ln for ln in on if ln.startswith("progress epoch ")]
    assert len(lines) == EPOCHS and not any(ln.startswith("progress") for ln in off)
    for e, ln in enumerate(lines):
        assert ln.startswith("progress epoch %d: rows = 200 logloss = %.6f (+- 4.9e-04) auc = %.6f "
                             % (e, ref[e]["logloss"], ref[e]["auc"])), ln
        assert "ctr = %.6f pctr = %.6f" % (ref[e]["ctr"], ref[e]["pctr"]) in ln, ln
    # the other lines and their order do not change (the throughput line is a measurement)
    rest = [ln for ln in on if not ln.startswith("progress epoch ")]
    strip = lambda ls: [ln for ln in ls if not ln.startswith("examples/sec")]  # noqa: E731
    assert strip(rest) == strip(off)
    assert any("logloss" in ln and "auc" in ln for ln in strip(off))


def test_local_sh_two_workers_print_the_merged_figures(data, tmp_path):
    env_port = str(free_port())
    args = [str(data / "train"), str(data / "test"), "0", "2", "transport=host", "capacity=16384",
            "pred_path=two.txt", "progress=1"]   # (host transport: both ranks share one GPU)
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI] + args,
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path),
                         env=dict(os.environ, DMLC_PS_ROOT_PORT=env_port))
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.split("\n") if ln.startswith("progress epoch ")]
    assert len(lines) == 2, out.stdout                      # rank 0 alone prints
    rows = sum(len(open(str(data / f)).read().strip().split("\n"))
               for f in ("train-00000", "train-00001"))
    for e, ln in enumerate(lines):
        assert ln.startswith("progress epoch %d: rows = %d logloss = " % (e, rows)), ln
    assert float(lines[1].split("logloss = ")[1].split(" ")[0]) < \
        float(lines[0].split("logloss = ")[1].split(" ")[0])
