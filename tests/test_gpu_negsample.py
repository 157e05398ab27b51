"""Negative subsampling (xf_negsample.hip, the trainers' weight, the worker's neg_keep=) on a real
MI355X.  The only reference of the sampler is the numpy restatement tests/_negsample_checker.py
(pinned to a plain loop by tests/test_negsample_cpu.py); the weighted steps are each mode's
existing checker, cut between its forward and its gradient with the loss scaled in between.
Every comparison is exact — integer arrays, float arrays as their bits.

* the sampler: the compacted arrays and the statistics over keep x companions, on minibatches
  chosen where the passes can go wrong — R = 0, NNZ = 0, all rows positive, all rows negative,
  empty rows first, last and in runs, first and last row dropped, a run of dropped rows longer than
  a tile, R around the row tile, one row of 5 000 nonzeros kept and (another seed) dropped, 300
  short rows, ordinals across 2^32 — one after the other on ONE sampler with running ordinals;
* keep = 1 is the identity, down to the table a trainer steps on the sampled minibatch;
* the weight on one GPU in every step path, on two ranks on both exchange schedules;
* the worker end to end against the restatement feeding the weighted checkers."""
import os
import re
import subprocess
import traceback

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import build, capi

from . import _admit_checker as A
from . import _ffm_checker as FF
from . import _fmc_checker as FC
from . import _negsample_checker as N
from . import _sharded_modes_checker as M
from . import _valued_cases as Cs
from . import _valued_checker as V
from . import test_gpu_fm_canonical as TC      # synth, _tables (the module, not its tests)
from . import test_gpu_sharded_modes as SM     # _spawn, _check_tables, _import_old, ...
from .test_gpu_parity import synth
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W4 = np.float32(4.0)
W03 = np.float32(1.0) / np.float32(0.3)
WEIGHTS = [W4, W03]
WIDS = ["w4", "w1/0.3"]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(a, b):
        i = np.flatnonzero((a != b).ravel())
        raise AssertionError("%s: %d of %d differ; first (at, got, want): %s" % (
            what, i.size, a.size, [(j, a.ravel()[j], b.ravel()[j]) for j in i[:6]]))


def same_table(t, s, what="table"):
    """keys and weights, and FTRL's (n, z)"""
    m = 4 if t.opt == capi.OPT_FTRL else 2
    for a, e in zip(t.export()[:m], s.export()[:m]):
        same(a, e, what)


def tile_size():
    """the row tile of the flag and the place pass, read from the source"""
    src = open(os.path.join(os.path.dirname(HERE), "xflow_amd", "csrc", "xf_negsample.hip")).read()
    return int(re.search(r"constexpr uint32_t kNsTile = (\d+);", src).group(1))


# ------------------------------------------------------------------ the sampler's minibatches
STREAM = (5 << 32) | 2
POOL = None      # (filled on first use: needs the library)


def pool():
    global POOL
    if POOL is None:
        POOL = capi.hash_decimal_range(0, 3000)
    return POOL


def _mb(rng, lens, labels):
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    P = pool()
    keys = P[rng.randint(0, len(P), size=int(rowptr[-1]))]
    labels = np.asarray(labels, np.int32)
    assert len(labels) == len(lens)
    return rowptr, keys, labels


def long_row_seeds():
    """two seeds under which the negative row of 5000 nonzeros (row 2 of `long_row`, whose first
    ordinal the sequence fixes) is kept, respectively dropped, at keep = 0.25 — found with the
    restatement"""
    at = np.array([LONG_ROW_AT + 2], np.uint64)
    kept = next(s for s in range(1, 100) if N.keep_negative(s, STREAM, at, 0.25)[0])
    dropped = next(s for s in range(1, 100) if not N.keep_negative(s, STREAM, at, 0.25)[0])
    return kept, dropped


LONG_ROW_AT = 1 << 20          # the first ordinal of the `long_row` minibatch
EDGE_AT = 1 << 21              # ... and where `ends_dropped` is searched from


def sequence(seed):
    """[(name, first_ordinal, rowptr, keys, labels)] in the order they are applied to one sampler:
    ordinals run on from minibatch to minibatch, with jumps forward to the places some cases need"""
    rng = np.random.RandomState(23)
    T = tile_size()
    out, at = [], [7]       # (the file's first rows are not ordinal 0 here: a running count)

    def add(name, mb, first=None):
        if first is not None:
            assert first >= at[0]
            at[0] = first
        out.append((name, at[0]) + mb)
        at[0] += len(mb[2])

    few = lambda n, p=0.05: (rng.rand(n) < p).astype(np.int32)  # noqa: E731
    add("no_rows", (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32)))
    add("no_nonzeros", (np.zeros(8, np.uint64), np.zeros(0, np.uint64),
                        np.array([0, 1, 0, 0, 0, 1, 0], np.int32)))
    add("all_positive", _mb(rng, rng.randint(0, 9, size=300), np.ones(300, np.int32)))
    add("all_negative", _mb(rng, rng.randint(0, 9, size=600), np.zeros(600, np.int32)))
    # ragged: empty rows first, last and in runs
    lens = rng.randint(0, 40, size=700)
    lens[:3] = 0
    lens[-2:] = 0
    lens[300:340] = 0
    lens[rng.rand(700) < 0.05] = 0
    add("ragged", _mb(rng, lens, few(700)))
    # a run of negatives longer than a tile between two positives (keep = 2^-32: all dropped)
    lab = np.zeros(T + 40, np.int32)
    lab[[0, 1, T + 38, T + 39]] = 1
    add("long_run", _mb(rng, rng.randint(1, 6, size=T + 40), lab))
    for R in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
        add("rows%d" % R, _mb(rng, rng.randint(0, 5, size=R), few(R, 0.1)))
    add("long_row", _mb(rng, [3, 0, 5000, 0, 7], np.zeros(5, np.int32)), first=LONG_ROW_AT)
    add("short_rows", _mb(rng, rng.randint(1, 4, size=300), few(300)))
    # first and last row negative and dropped at keep = 0.25 under this seed: the place is searched
    R = 90
    first = next(f for f in range(EDGE_AT, EDGE_AT + 1000)
                 if not N.keep_negative(seed, STREAM, np.array([f, f + R - 1], np.uint64), 0.25).any())
    add("ends_dropped", _mb(rng, rng.randint(1, 6, size=R), np.zeros(R, np.int32)), first=first)
    add("across_2^32", _mb(rng, rng.randint(0, 6, size=50), few(50, 0.1)), first=(1 << 32) - 3)
    return out


def companions(keys):
    """an fgid and a value per nonzero that say where the nonzero came from"""
    n = len(keys)
    return (np.arange(n, dtype=np.int32) % 977,
            (np.arange(n, dtype=np.float32) * np.float32(0.25) - np.float32(3)).astype(np.float32))


KEEPS = [2.0 ** -32, 0.25, 0.999, 1.0]
COMP = [(False, False), (True, False), (False, True), (True, True)]
GRID = [(k, c, which) for k in KEEPS for c in COMP for which in (0, 1)]


@pytest.mark.parametrize("keep,comp,which", GRID, ids=[
    "keep%g-%s-seed%s" % (k, {(False, False): "none", (True, False): "fgid", (False, True): "vals",
                              (True, True): "both"}[c], "AB"[w]) for k, c, w in GRID])
def test_sampled_arrays_and_stats(keep, comp, which):
    seed = long_row_seeds()[which]
    mbs = sequence(seed)
    with_fg, with_vs = comp
    # the restatement first: the expected arrays of every call, and that the case is worth
    # running — before the GPU is asked anything
    ref, expect = N.Sampler(keep, seed), []
    pos_held = 0
    for name, first, rowptr, keys, labels in mbs:
        fg, vs = companions(keys)
        e = ref.apply(STREAM, first, rowptr, keys, labels, fg, vs)
        expect.append(e + (ref.stats(),))
        pos_held += int((e[2] != 0).sum())
        assert int((e[2] != 0).sum()) == int((labels != 0).sum()), name   # positives are held
        kept_neg = int((e[2] == 0).sum())
        if name == "all_negative" and keep == 2.0 ** -32:
            assert len(e[2]) == 0 and len(e[1]) == 0                      # R_out = 0
        if name == "long_run" and keep == 2.0 ** -32:
            assert kept_neg == 0 and len(e[2]) == 4
        if name == "long_row" and keep == 0.25:
            assert (len(e[1]) >= 5000) == (which == 0)                    # kept under A, dropped under B
        if name == "ends_dropped" and keep == 0.25:
            m = ref.mask(STREAM, first, labels)
            assert not m[0] and not m[-1] and m.any()
        if keep == 1.0:
            assert e[0].tobytes() == rowptr.astype(np.uint32).tobytes() and \
                e[1].tobytes() == keys.tobytes() and e[2].tobytes() == labels.tobytes()
    _, rows_kept, neg_seen, neg_kept = ref.stats()
    if keep == 0.25:
        assert 0 < neg_kept < neg_seen and pos_held > 0, ref.stats()
    smp = capi.NegSample(keep, seed=seed)
    for (name, first, rowptr, keys, labels), (rp, ks, lb, efg, evs, stats) in zip(mbs, expect):
        fg, vs = companions(keys)
        got = smp.apply(STREAM, first, rowptr, keys, labels, fgid=fg if with_fg else None,
                        values=vs if with_vs else None)
        same(got[0], rp, name + " rowptr")
        same(got[1], ks, name + " keys")
        same(got[2], lb, name + " labels")
        at = 3
        if with_fg:
            same(got[at], efg, name + " fgid")
            at += 1
        if with_vs:
            same(got[at], evs, name + " values")
            at += 1
        assert len(got) == at and smp.stats() == stats, name


def test_row_slice_of_a_block():
    """host arrays whose first offset is not 0: rows [100, 300) of a block"""
    name, first, rowptr, keys, labels = sequence(1)[4]
    smp, ref = capi.NegSample(0.25, seed=9), N.Sampler(0.25, 9)
    got = smp.apply(STREAM, 1000, rowptr[100:301], keys, labels[100:300])
    e = ref.apply(STREAM, 1000, rowptr[100:301], keys, labels[100:300])
    for a, b in zip(got, e[:3]):
        same(a, b)
    assert 0 < len(got[2]) < 200
    with pytest.raises(capi.XFError, match="descend"):
        smp.apply(STREAM, 0, np.array([0, 3, 2], np.uint64), np.zeros(3, np.uint64),
                  np.zeros(2, np.int32))


def test_keep_one_is_the_identity():
    rng = np.random.RandomState(5)
    smp = capi.NegSample(1.0, seed=3)
    for name, first, rowptr, keys, labels in sequence(1):
        fg, vs = companions(keys)
        got = smp.apply(STREAM, first, rowptr, keys, labels, fg, vs)
        for g, want in zip(got, (rowptr.astype(np.uint32), keys, labels, fg, vs)):
            assert g.dtype == want.dtype and g.tobytes() == want.tobytes(), name
    assert smp.weight == np.float32(1.0)
    # binary LR: a table stepped on the sampled device arrays is the table stepped on the minibatch
    name, first, rowptr, keys, _ = sequence(1)[4]
    labels = rng.randint(0, 2, size=len(rowptr) - 1).astype(np.int32)
    a = capi.Sharded(model="lr", capacity=1 << 14)
    b = capi.Sharded(model="lr", capacity=1 << 14)
    a.set_neg_weight(smp.weight)
    for _ in range(3):
        d = smp.apply_dev(STREAM, first, rowptr, keys, labels)
        assert (d.R, d.NNZ) == (len(labels), len(keys))
        a.step(a.compile_dev(*d[:5]))
        a.check()
        b.step(b.compile(rowptr, keys, labels))
        b.check()
    for x, y in zip(a.w.export(), b.w.export()):
        same(x, y)
    assert len(a.w) > 100


# ------------------------------------------------------------------ the weight, one GPU
def _go(opt):
    return capi.OPT_FTRL if opt == "ftrl" else capi.OPT_SGD


def _oo(opt):
    return O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD


_LR = {}


def lr_raws():
    """three training minibatches and a held-out one, made once (test_gpu_keybuild's first shape)"""
    if not _LR:
        rng = np.random.RandomState(3040)
        _LR["train"] = [synth(rng, 3000, 40, 30000, 1.15 if i == 2 else None, i > 0)
                        for i in range(3)]
        _LR["held"] = synth(rng, 1000, 40, 30000, None, True)
    return _LR["train"], _LR["held"]


def _plain_lr_step(s, raw):
    ob = O.Batch(*raw)
    with O.sum_mode(1):
        loss, _ = ob.lr_loss(s.pull(ob.ukeys))
        O.lr_update(s, ob)
    return loss


@pytest.mark.parametrize("w", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_weighted_lr_on_cells(opt, w):
    """the local build's cells and the generic build's (step 1), both optimizers"""
    train, held = lr_raws()
    t, s = capi.Table(_go(opt), 1, capacity=1 << 17), O.Store(_oo(opt), 1)
    ws = capi.Workspace()
    ws.neg_weight(w)
    for i, raw in enumerate(train):
        b = capi.Batch(*raw) if i == 1 else capi.LocalBatch(t, *raw)
        capi.lr_step(t, b, ws)
        loss = N.lr_step(s, *raw, w)
        assert (raw[2] == 0).any() and (raw[2] != 0).any()
        same(ws.fetch_loss(b.R), loss, "step %d: the weighted loss" % i)
    same_table(t, s)
    # predict never weights
    ob = O.Batch(*held)
    with O.sum_mode(1):
        pctr = ob.lr_loss(s.pull(ob.ukeys))[1]
    same(capi.lr_predict(t, capi.Batch(*held), ws), pctr, "held-out pctr")
    # w = 1 after w != 1 is the plain step again
    ws.neg_weight(1.0)
    b = capi.LocalBatch(t, *train[0])
    capi.lr_step(t, b, ws)
    same(ws.fetch_loss(b.R), _plain_lr_step(s, train[0]), "the plain loss")
    same_table(t, s, "table after the plain step")


@pytest.mark.parametrize("w", WEIGHTS, ids=WIDS)
def test_weighted_update_in_one_call(w):
    """xf_lr_update_dev: the weight after its LAST forward segment — a minibatch that brings new
    keys runs the forward again over a second segment of cells"""
    R, nnz, nkeys = 3000, 40, 30000
    rng = np.random.RandomState(17)
    t, s = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 17), O.Store(O.OPT_FTRL, 1)
    ws = capi.Workspace()
    ws.neg_weight(w)
    segs = []
    for step in range(4):
        hi = nkeys // 2 if step < 2 else nkeys       # steps 2, 3: half the keys are new
        raw = synth(rng, R, nnz, hi, 1.15 if step % 2 else None, True)
        loss = N.lr_step(s, *raw, w)
        b = capi.LocalBatch.update(t, ws, *raw)
        same(ws.fetch_loss(R), loss, "step %d" % step)
        segs.append(b.cells_info()["segments"])
        if step == 0:                                # every key of the first half, then settle
            allk = capi.hash_decimal_range(0, nkeys // 2)
            t.pull(allk)
            s.pull(allk)
            t.defrag()
    assert segs[1:] == [1, 2, 2], segs
    t.check()
    same_table(t, s)


_VAL = {}


def valued_checker(opt, w):
    """the valued LR checker over Cs.stream('ragged') from aged tables, weighted: computed once
    per (opt, w) and left unchanged -> losses, the store's export, held-out pctr, the plain replay"""
    key = (opt, float(w))
    if key not in _VAL:
        mbs = Cs.stream("ragged")
        audit = []
        sw, _ = Cs.stores("lr", opt, 1, mbs)
        losses = [N.valued_lr_step(sw, rp, ks, vs, lb, w, audit)[2] for rp, ks, vs, lb in mbs]
        after = sw.export()
        # (a held-out key that is not aged is pulled — inserted — with weight 0: its products
        # are zeros, the sums stay exact)
        held = Cs.stream("ragged", seed=50)[0]
        pctr = V.lr_predict(sw, *held, audit)
        rp, ks, vs, lb = mbs[-1]
        plain = V.lr_step(sw, rp, ks, vs, lb, audit)[2]
        V.assert_exact(audit)
        _VAL[key] = (mbs, losses, after, held, pctr, plain, sw.export())
    return _VAL[key]


@pytest.mark.parametrize("w", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("path", ["generic", "local"])
def test_weighted_valued_lr(path, w):
    opt = "ftrl"
    mbs, losses, after, held, pctr, plain, final = valued_checker(opt, w)
    t = capi.Table(_go(opt), 1, capacity=1 << 16)
    t.import_(*Cs.old_state(Cs.stream_keys(mbs), opt, 1, "w"))
    ws = capi.Workspace()
    ws.neg_weight(w)

    def batch(mb):
        rp, ks, vs, lb = mb
        if path == "local":
            return capi.LocalBatch(t, rp, ks, lb, values=vs)
        return capi.Batch(rp, ks, lb, on_gpu=True, values=vs)
    b = None
    for i, (mb, loss) in enumerate(zip(mbs, losses)):
        b = batch(mb)
        capi.lr_step(t, b, ws)
        same(ws.fetch_loss(b.R), loss, "step %d: the weighted loss" % i)
    m = 4
    for a, e in zip(t.export()[:m], after[:m]):
        same(a, e, "table")
    same(capi.lr_predict(t, batch(held), ws), pctr, "held-out pctr")
    ws.neg_weight(1.0)
    capi.lr_step(t, b, ws)
    same(ws.fetch_loss(b.R), plain, "the plain loss")
    for a, e in zip(t.export()[:m], final[:m]):
        same(a, e, "table after the plain step")


@pytest.mark.parametrize("w", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("opt,k", [("sgd", 4), ("ftrl", 10)], ids=["k4-records", "k10"])
def test_weighted_reference_fm(opt, k, w):
    """k = 4: the forward over the table-resident records; k = 10: the row-gather forward"""
    rng = np.random.RandomState(k)
    go, oo = _go(opt), _oo(opt)
    init = (capi.INIT_CONST, 0.001) if opt == "sgd" else (capi.INIT_HASHNORM, 0.0)
    tw = capi.Table(go, 1, capacity=1 << 16)
    tv = capi.Table(go, k, init[0], init[1], seed=99, capacity=1 << 16)
    sw, sv = O.Store(oo, 1), O.Store(oo, k, init[0], init[1], 99)
    ws = capi.Workspace()
    ws.neg_weight(w)
    raws = [synth(rng, 500, 30, 4000, 1.3 if i == 2 else None, True) for i in range(3)]
    for i, raw in enumerate(raws):
        capi.fm_step(tw, tv, capi.Batch(*raw), ws)
        same(ws.fetch_loss(500), N.fm_step(sw, sv, *raw, w), "step %d: the weighted loss" % i)
    same_table(tw, sw, "w")
    same_table(tv, sv, "v")
    held = synth(rng, 300, 30, 4000, None, True)
    ob = O.Batch(*held)
    with O.sum_mode(1):
        pctr = ob.fm_loss(k, sw.pull(ob.ukeys), sv.pull(ob.ukeys))[1]
    same(capi.fm_predict(tw, tv, capi.Batch(*held), ws), pctr, "held-out pctr")
    ws.neg_weight(1.0)
    capi.fm_step(tw, tv, capi.Batch(*raws[0]), ws)
    with O.sum_mode(1):
        O.fm_update(sw, sv, O.Batch(*raws[0]))
    same_table(tw, sw, "w after the plain step")
    same_table(tv, sv, "v after the plain step")


@pytest.mark.parametrize("w", WEIGHTS, ids=WIDS)
def test_weighted_canonical_fm(w):
    opt, k = "ftrl", 16
    rng = np.random.RandomState(k)
    tw, tv, (sw, sv) = TC._tables(opt, k)
    ws = capi.Workspace(capture=True)
    ws.fm_mode("canonical")
    ws.neg_weight(w)
    raws = [TC.synth(rng, 400, 25, 3000, z) for z in (None, 1.3, None)]
    for raw in raws:
        b = capi.Batch(*raw, on_gpu=True)
        capi.fm_step(tw, tv, b, ws)
        ukeys, wu, loss, gw = N.fmc_step(sw, sv, *raw, w)
        g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
        same(g_wu, wu)
        same(g_loss, loss, "the weighted loss")
        same(g_gw, gw)
    TC.same_tables(tw, tv, sw, sv)
    held = TC.synth(rng, 300, 20, 6000, None)
    same(capi.fm_predict(tw, tv, capi.Batch(*held), ws), FC.predict(sw, sv, *held))
    ws.neg_weight(1.0)
    capi.fm_step(tw, tv, capi.Batch(*raws[0]), ws)
    FC.step(sw, sv, *raws[0])
    TC.same_tables(tw, tv, sw, sv)


_FFM = {}


def ffm_checker(w):
    """field-aware FM with values over FF.stream('ragged', 18) from aged tables, weighted"""
    key = float(w)
    if key not in _FFM:
        Fd, k, opt = 18, 4, "ftrl"
        mbs = FF.stream("ragged", Fd)
        audit = []
        sw, sv = FF.aged_stores(opt, Fd, k, mbs)
        steps = [N.ffm_step(sw, sv, Fd, rp, ks, fg, vs, lb, w, audit) for rp, ks, fg, vs, lb in mbs]
        after = (sw.export(), sv.export())
        rp, ks, fg, vs, lb = mbs[-1]
        pctr = FF.predict(sw, sv, Fd, rp, ks, fg, vs, lb, audit)
        plain = FF.step(sw, sv, Fd, rp, ks, fg, vs, lb, audit)
        FF.assert_exact(audit)
        _FFM[key] = (Fd, k, opt, mbs, steps, after, pctr, plain, (sw.export(), sv.export()))
    return _FFM[key]


@pytest.mark.parametrize("w", WEIGHTS, ids=WIDS)
def test_weighted_field_aware_fm_with_values(w):
    Fd, k, opt, mbs, steps, after, pctr, plain, final = ffm_checker(w)
    tw = capi.Table(_go(opt), 1, capacity=1 << 16)
    tv = capi.Table(_go(opt), Fd * k, capi.INIT_HASHNORM, 0.0, seed=7, capacity=1 << 16)
    tw.import_(*Cs.old_state(FF.stream_keys(mbs), opt, 1, "w"))
    tv.import_(*Cs.old_state(FF.stream_keys(mbs), opt, Fd * k))
    ws = capi.Workspace()
    ws.fm_fields(Fd)
    ws.fm_mode("field_aware")
    ws.neg_weight(w)
    b = None
    for (rp, ks, fg, vs, lb), (ukeys, wu, loss, gw) in zip(mbs, steps):
        b = capi.Batch(rp, ks, lb, on_gpu=True, values=vs, fields=Fd, fgid=fg)
        capi.fm_step(tw, tv, b, ws)
        g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
        same(g_wu, wu)
        same(g_loss, loss, "the weighted loss")
        same(g_gw, gw)
    for t, ex in zip((tw, tv), after):
        for x, e in zip(t.export()[:4], ex[:4]):
            same(x, e, "table")
    # (the held-out minibatch is the last one, as in the mode's own test: its keys are aged)
    same(capi.fm_predict(tw, tv, b, ws), pctr, "pctr")
    ws.neg_weight(1.0)
    capi.fm_step(tw, tv, b, ws)
    for a, e in zip(ws.fetch(b.U, b.R), plain[1:4]):
        same(a, e, "the plain step")
    for t, ex in zip((tw, tv), final):
        for x, e in zip(t.export()[:4], ex[:4]):
            same(x, e, "table after the plain step")


def test_setters_refuse_on_the_device_too():
    st = capi.Sharded(model="lr", capacity=1 << 12)
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(capi.XFError, match="xf_sharded_set_neg_weight"):
            st.set_neg_weight(bad)
    st.set_neg_weight(4.0)
    st.set_neg_weight(1.0)


# ------------------------------------------------------------------ the weight, two ranks
# (mode, world, fields, k, optimizer, schedule, stream, valued) as tests/_sharded_modes_checker.py
TWO_RANKS = (("canonical", 2, 0, 4, "ftrl", "sequential", "ragged", False),
             ("canonical", 2, 0, 4, "ftrl", "stale1", "ragged", False))
LR_TWO = (("ftrl", "sequential"), ("sgd", "stale1"))


def _weighted_rank(rank, world, port, spec, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        mode, _, F, k, opt, schedule, case, valued = spec
        strs = M.streams(mode, case, world, F)
        st = SM._trainer(g, spec)
        st.set_neg_weight(W4)
        SM._import_old(st, spec, strs, rank, world)
        out = SM._steps(st, spec, strs, rank, defrag=schedule == "sequential")
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("spec", TWO_RANKS, ids=M.case_id)
def test_weighted_canonical_fm_on_two_ranks(tmp_path, spec):
    mode, world, F, k, opt, schedule, case, valued = spec
    strs = M.streams(mode, case, world, F)
    audit = []
    ws, vs, pctr = N.sharded_run(mode, opt, k, F, valued, schedule, strs, W4, audit)
    V.assert_exact(audit)
    port = free_port()
    SM._spawn(_weighted_rank, [(r, world, port, spec, str(tmp_path)) for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    SM._check_tables(parts, world, ws, vs, opt)
    for r in range(world):
        same(parts[r]["pctr"], np.asarray(pctr[r], np.float32), "rank %d pctr" % r)


def lr_rank_streams(world):
    """per rank: three binary minibatches and a held-out one (the valued streams' rows and keys)"""
    out = []
    for r in range(world):
        train, held = (Cs.stream("ragged", seed=s) for s in (M.rank_seed(r), M.rank_seed(r) + 5))
        three = lambda m: (m[0], m[1], m[3])  # noqa: E731
        out.append(([three(m) for m in train], three(held[0])))
    return out


def _weighted_lr_rank(rank, world, port, opt, schedule, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        st = capi.Sharded(g, model="lr", optimizer=opt, capacity=1 << 15, schedule=schedule,
                          seed=7)
        st.set_neg_weight(W4)
        train, held = lr_rank_streams(world)[rank]
        alive = []
        for mb in train:
            b = st.compile(*mb)
            alive.append(b)
            st.step(b)
        st.check()
        out = {"pctr": st.predict(st.compile(*held))}
        st.check()
        SM._export(st, out)
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("opt,schedule", LR_TWO, ids=["%s-%s" % c for c in LR_TWO])
def test_weighted_lr_on_two_ranks(tmp_path, opt, schedule):
    world = 2
    store, pctr = N.sharded_lr_run(opt, schedule, lr_rank_streams(world), W4)
    port = free_port()
    SM._spawn(_weighted_lr_rank, [(r, world, port, opt, schedule, str(tmp_path))
                                  for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    SM._check_tables(parts, world, store, None, opt)
    for r in range(world):
        same(parts[r]["pctr"], np.asarray(pctr[r], np.float32), "rank %d pctr" % r)


def _owner_refusal(port, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"       # a group of one on the exchange path
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        seen = []
        for sched in ("owner", "owner_stale1"):
            st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule=sched)
            st.set_neg_weight(1.0)                   # (the default is no weight: accepted)
            try:
                st.set_neg_weight(4.0)
            except capi.XFError as e:
                assert re.search(r"xf_sharded_set_neg_weight.*schedule %s\b" % sched, str(e)) \
                    and "sequential" in str(e), str(e)
                seen.append(sched)
            st.close()
        # the other order is shut as well: a trainer on the exchange schedules never becomes an
        # owner-compute one
        st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule="stale1")
        st.set_neg_weight(4.0)
        try:
            st.set_schedule("owner")
        except capi.XFError as e:
            assert "xf_sharded_set_schedule" in str(e), str(e)
            seen.append("then owner")
        st.set_schedule("sequential")
        st.close()
        g.close()
        q.put((0, ("ok", seen)))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_owner_schedules_refuse_the_weight():
    res = SM._spawn(_owner_refusal, [(free_port(),)])
    assert res[0][1] == ("ok", ["owner", "owner_stale1", "then owner"]), res


# ------------------------------------------------------------------ the worker end to end
from . import test_gpu_admit as TA             # noqa: E402  (MODELS, Model, FIELDS, K: the module)

KEEP = 0.25
W = N.weight(KEEP)
ROOT = os.path.dirname(HERE)
CLI = os.path.join(build.LIBDIR, "xflow_lr")


from ._zipf_text import zipf_text      # noqa: E402,F401  (moved: the CPU tests form it too)


# (the seed: the field-aware checker's sums are not exact in fp64; the interval rule of
# tests/_interval.py must pin every one of them to a single fp32 value.  With seeds 23 .. 39 it
# does in the replaying, the admitting and the resampling run — except seed 25, whose resampling
# run leaves one of 139 000 gv sums open between two adjacent fp32 values: found with the checker
# alone)
TRAIN_SEED = 27


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("negsample")
    train = zipf_text(TRAIN_SEED, (2 << 20) + (200 << 10))
    assert 2 << 20 < len(train) < 3 << 20                        # three 1 MiB blocks
    (d / "train-00000").write_bytes(train)
    (d / "test-00000").write_bytes(zipf_text(22, 60 << 10, 0.3))
    return d


class WeightedModel(TA.Model):
    """tests/test_gpu_admit.py's Model with the loss of every step weighted between the mode's
    forward and its gradient"""

    def __init__(self, name, w):
        TA.Model.__init__(self, name)
        self.w = w

    def step(self, mb):
        rp, keys, fg, vals, labels = mb
        if self.name == "lr":
            N.lr_step(self.ws, rp, keys, labels, self.w)
        elif self.name == "canonical":
            N.fmc_step(self.ws, self.vs, rp, keys, labels, self.w)
        elif len(keys):
            _, _, loss = self.run.begin((rp, keys, fg, vals, labels))
            self.run.finish(N.weigh(loss[:, 0], labels, self.w))


_refs = {}


def reference(data, name, admit=False, resample=False, keep=KEEP, blocks_want=3):
    """the restatement does what the worker does: every training block sampled in file order (the
    ordinal a running row count, the stream (epoch << 32) | rank 0), then filtered by admission when
    on, then stepped with the weight; the second epoch replays the first epoch's minibatches
    (resample: samples again, under the next epoch's stream); the test blocks are never sampled.  A
    block whose rows are all dropped is no minibatch (one worker)"""
    key = (str(data), name, admit, resample, keep)
    if key in _refs:
        return _refs[key]
    smp, m = N.Sampler(keep, 0), WeightedModel(name, N.weight(keep))   # the worker's seed: 0
    flt = A.Filter(12, 2, 3, 0) if admit else None
    blocks = list(capi.read_blocks(str(data / "train-00000"), 1 << 20, values=True))
    assert len(blocks) == blocks_want

    def sampled(epoch):
        out, ordinal = [], 0
        for rp, keys, fg, labels, vals in blocks:
            srp, sk, sl, sfg, sv = smp.apply(epoch << 32, ordinal, rp, keys, labels, fg, vals)
            ordinal += len(labels)
            assert len(sl) < len(labels) and (sl != 0).sum() == (labels != 0).sum()
            assert len(sl) > 0 or keep != KEEP
            if len(sl) == 0:
                out.append(None)
                continue
            if flt is not None:
                srp, sk, sfg, sv = flt.filter(srp.astype(np.uint64), sk, sfg, sv, update=True)
            out.append((srp.astype(np.uint64), sk, sfg, sv, sl))
        return out

    first = None
    for epoch in range(2):
        mbs = sampled(epoch) if epoch == 0 or resample else first
        if epoch == 1 and resample:                              # other negatives this time
            assert any(len(a[4]) != len(b[4]) or not np.array_equal(a[1], b[1])
                       for a, b in zip(mbs, first))
        first = first or mbs
        for mb in mbs:
            if mb is not None:
                m.step(mb)
    cap = (4 << 20) if name == "lr" else (2 << 20)
    labs, ps = [], []
    for rp, keys, fg, labels, vals in capi.read_blocks(str(data / "test-00000"), cap, values=True):
        if flt is not None:
            frp, keys, fg, vals = flt.filter(rp, keys, fg, vals, update=False)
            rp = frp.astype(np.uint64)
        ps.append(m.predict((rp, keys, fg, vals, labels)))
        labs.append(labels)
    if m.judge is not None:
        assert m.judge.open_count() == 0, m.judge.format(name)
    lab, p = np.concatenate(labs), np.concatenate(ps)
    _refs[key] = (m, lab, p, O.auc_logloss(lab, p), smp.stats(),
                  (flt.seen, flt.kept) if flt is not None else (0, 0))
    return _refs[key]


def unsampled_keys(data):
    """the keys an LR run WITHOUT sampling holds at the end: key 0, every key of the training
    file, every key of the test file (a test-time Pull inserts)"""
    ks = [np.zeros(1, np.uint64)]
    for path, cap in (("train-00000", 1 << 20), ("test-00000", 4 << 20)):
        ks += [b[1] for b in capi.read_blocks(str(data / path), cap)]
    return len(np.unique(np.concatenate(ks)))


def check_worker(x, pred, ref, name, some_negatives=True):
    m, lab, p, (ll, auc, tp, fp), stats, admitted = ref
    opt = capi.OPT_SGD if name.startswith("field_aware") else capi.OPT_FTRL
    wh, vh = x.tables()
    tabs = [(capi.Table.from_handle(wh, 1, opt), m.ws)]
    if m.vs is not None:
        tabs.append((capi.Table.from_handle(vh, m.vs.dim, opt), m.vs))
    for t, s in tabs:
        for a, e in zip(t.export()[:4 if opt == capi.OPT_FTRL else 2], s.export()):
            same(a, e, name)
    assert open(pred).read().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    assert x.metric("keys") == len(m.ws)
    rows_seen, rows_kept, neg_seen, neg_kept = stats
    assert (x.metric("neg_seen"), x.metric("neg_kept"), x.metric("rows_kept")) == \
        (neg_seen, neg_kept, rows_kept)
    assert neg_kept < neg_seen and (neg_kept > 0) == some_negatives
    assert (x.metric("admit_seen"), x.metric("admit_kept")) == admitted


def run_worker(data, name, ingest, tag, **extra):
    pred = str(data / ("pred_%s_%s.txt" % (name, tag)))
    p = dict(TA.MODELS[name][0], neg_keep=KEEP)
    p.update(extra)
    x = capi.XFlow(str(data / "train"), str(data / "test"), block_size_mb=1, capacity=1 << 14,
                   ingest=ingest, pred_path=pred, **p)
    x.train()
    return x, pred


@pytest.mark.parametrize("admit", [False, True], ids=["plain", "admission"])
@pytest.mark.parametrize("name", list(TA.MODELS))
@pytest.mark.parametrize("ingest", ["host", "gpu"])
def test_worker_end_to_end(data, name, ingest, admit):
    ingest = TA.MODELS[name][1] if ingest == "gpu" else "host"
    ref = reference(data, name, admit)
    extra = dict(TA.ADMIT) if admit else {}
    x, pred = run_worker(data, name, ingest, "%s%d" % (ingest, admit), epochs=2, **extra)
    assert x.metric("blocks_gpu") == (0 if ingest == "host" else 3)
    check_worker(x, pred, ref, name)
    # rows_trained counts the kept rows: the first epoch's, replayed once
    assert x.metric("rows_trained") == 2 * ref[4][1]


@pytest.mark.parametrize("name", list(TA.MODELS))
@pytest.mark.parametrize("ingest", ["host", "gpu"])
def test_worker_samples_again_without_the_batch_cache(data, name, ingest):
    """cache_batches=0: the second epoch reads the file again — the ordinal starts from 0 again, the
    stream id carries the epoch — on the host parser's path and on the tokeniser's"""
    ingest = TA.MODELS[name][1] if ingest == "gpu" else "host"
    ref = reference(data, name, resample=True)
    assert ref[4][0] == 2 * reference(data, name)[4][0]          # (twice the rows were seen)
    x, pred = run_worker(data, name, ingest, "resample_" + ingest, epochs=2, cache_batches=0)
    check_worker(x, pred, ref, name)
    assert x.metric("rows_trained") == ref[4][1]


# ---- a block whose rows are all dropped
TINY = 2.0 ** -32


@pytest.fixture(scope="module")
def data_dropped(tmp_path_factory):
    """a training file whose first 1 MiB block holds negatives only, the rest 5 % positives: at
    neg_keep = 2^-32 the first block loses every row, the others keep their positives"""
    d = tmp_path_factory.mktemp("negsample_dropped")
    train = zipf_text(31, (1 << 20) + (40 << 10), 0.0) + zipf_text(32, 300 << 10, 0.05)
    assert 1 << 20 < len(train) < 2 << 20                        # two 1 MiB blocks
    (d / "train-00000").write_bytes(train)
    (d / "test-00000").write_bytes(zipf_text(22, 60 << 10, 0.3))
    return d


@pytest.mark.parametrize("ingest", ["host", "gpu"])
def test_a_block_whose_rows_are_all_dropped_is_no_minibatch(data_dropped, ingest):
    """one worker: the first block yields no minibatch (nothing is stepped, nothing is cached), the
    ordinal runs on over its rows, the second block's positives train; rows_trained counts them"""
    ref = reference(data_dropped, "lr", keep=TINY, blocks_want=2)
    rows_seen, rows_kept, neg_seen, neg_kept = ref[4]
    blocks = list(capi.read_blocks(str(data_dropped / "train-00000"), 1 << 20))
    assert not blocks[0][3].any() and blocks[1][3].any()         # negatives only; some positives
    assert neg_kept == 0 and 0 < rows_kept == int(blocks[1][3].sum())
    x, pred = run_worker(data_dropped, "lr", ingest, "dropped_" + ingest, epochs=2, neg_keep=TINY)
    assert x.metric("blocks_gpu") == (0 if ingest == "host" else 2)
    check_worker(x, pred, ref, "lr", some_negatives=False)
    assert x.metric("rows_trained") == 2 * rows_kept


def test_a_file_whose_rows_are_all_dropped_trains_nothing(tmp_path):
    """negatives only: no minibatch at all — the table holds key 0 and what the test file's Pulls
    insert, every prediction is sigmoid(0)"""
    (tmp_path / "train-00000").write_bytes(zipf_text(33, 200 << 10, 0.0))
    (tmp_path / "test-00000").write_bytes(zipf_text(22, 60 << 10, 0.3))
    ref = reference(tmp_path, "lr", keep=TINY, blocks_want=1)
    assert ref[4][1] == 0 and ref[4][3] == 0 and ref[4][2] == ref[4][0] > 1000
    assert set(ref[2].tolist()) == {0.5}
    for ingest in ("host", "gpu"):
        x, pred = run_worker(tmp_path, "lr", ingest, "none_" + ingest, epochs=2, neg_keep=TINY)
        check_worker(x, pred, ref, "lr", some_negatives=False)
        assert x.metric("rows_trained") == 0


def test_a_bad_neg_keep_is_refused_by_name_outside_training_too(tmp_path):
    """XFLoadModel builds the tables (and warms the kernels up) without XFStartTrain's checks in
    front: the refusal still names the parameter, not the weight derived from it"""
    for bad in (1.5, 0, -0.25):
        x = capi.XFlow(str(tmp_path / "train"), str(tmp_path / "test"), neg_keep=bad)
        with pytest.raises(capi.XFError, match=r"neg_keep must be in \(0, 1\]"):
            x.load(str(tmp_path / "no_model"))


def test_fewer_keys_enter_the_table(data):
    """... than without sampling on the same file; the restatement says how many"""
    ref = reference(data, "lr")
    pred = str(data / "pred_unsampled.txt")
    x = capi.XFlow(str(data / "train"), str(data / "test"), block_size_mb=1, epochs=1,
                   capacity=1 << 14, pred_path=pred)
    x.train()
    assert x.metric("keys") == unsampled_keys(data)
    assert (x.metric("neg_seen"), x.metric("neg_kept"), x.metric("rows_kept")) == (0, 0, 0)
    assert len(ref[0].ws) < unsampled_keys(data)
    y, _ = run_worker(data, "lr", "host", "fewer", epochs=2)
    assert y.metric("keys") == len(ref[0].ws) < x.metric("keys")


def test_block_cache_gives_the_same_run(data, tmp_path):
    ref = reference(data, "lr")
    for tag in ("write", "read"):                                # the cache is written, then read
        x, pred = run_worker(data, "lr", "host", "cache_" + tag, epochs=2, block_cache=1,
                             block_cache_dir=str(tmp_path))
        check_worker(x, pred, ref, "lr")


def test_cli_prints_the_same_metric_line(data, tmp_path):
    _, lab, p, (ll, auc, tp, fp), stats, _ = reference(data, "lr")
    out = subprocess.run([CLI, str(data / "train"), str(data / "test"), "0", "2",
                          "block_size_mb=1", "capacity=16384", "pred_path=cli.txt", "neg_keep=0.25"],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert O.format_auc_line(ll, auc, tp, fp) in lines, out.stdout
    assert "rank 0 neg_seen = %d neg_kept = %d rows_kept = %d" % (stats[2], stats[3], stats[1]) \
        in lines, out.stdout
    assert open(str(tmp_path / "cli.txt")).read().split("\n")[:-1] == \
        ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]


# ---- two workers: scripts/local.sh 2 2 xflow_lr ... neg_keep=0.25 [admit_shared=1 ...]
@pytest.fixture(scope="module")
def data2(tmp_path_factory):
    d = tmp_path_factory.mktemp("negsample_two")
    for r, (seed, nbytes) in enumerate(((25, (2 << 20) + (200 << 10)), (26, (1 << 20) + (200 << 10)))):
        (d / ("train-%05d" % r)).write_bytes(zipf_text(seed, nbytes))
    (d / "test-00000").write_bytes(zipf_text(22, 60 << 10, 0.3))
    return d


def reference_two(data2, shared, keep=KEEP, blocks_want=(3, 2)):
    """the restatement feeding the oracle's rank-ordered schedule: a turn is one block of every
    rank that still has one, each sampled by its own rank (stream (epoch << 32) | rank, the
    ordinal the rank's running row count); with a shared admission filter the sampled blocks of a
    turn are counted together and filtered rank by rank; both ranks pull, then push in rank order;
    the second epoch replays"""
    blocks = [list(capi.read_blocks(str(data2 / ("train-%05d" % r)), 1 << 20)) for r in range(2)]
    assert [len(b) for b in blocks] == list(blocks_want)         # (3, 2): rank 1's last turn is empty
    smp = [N.Sampler(keep, 0), N.Sampler(keep, 0)]
    w = N.weight(keep)
    flt = A.Filter(12, 2, 3, 0) if shared else None
    ordinal, astats = [0, 0], [[0, 0], [0, 0]]

    def turn(t):
        out = []
        for r in range(2):
            if t >= len(blocks[r]):
                out.append(None)
                continue
            rp, keys, _, labels = blocks[r][t]
            srp, sk, sl, _, _ = smp[r].apply(r, ordinal[r], rp, keys, labels)   # (epoch 0)
            ordinal[r] += len(labels)
            out.append((srp.astype(np.uint64), sk, sl))
        if flt is not None:
            flt.count(np.concatenate([mb[1] for mb in out if mb is not None]))
            for r, mb in enumerate(out):
                if mb is None:
                    continue
                rp, keys, labels = mb
                keep = flt.keep_mask(keys)
                before = np.concatenate([[0], np.cumsum(keep)])
                astats[r][0] += len(keys)
                astats[r][1] += int(keep.sum())
                out[r] = (before[rp.astype(np.int64)].astype(np.uint64), keys[keep], labels)
        return out

    with O.sum_mode(1):
        s = O.Store(O.OPT_FTRL, 1)
        s.push(np.array([0], np.uint64), np.zeros(1, np.float32))
        turns = [turn(t) for t in range(max(blocks_want))]
        for epoch in range(2):
            for tn in turns:
                obs = [O.Batch(*mb) for mb in tn if mb is not None and len(mb[1])]
                pulled = [s.pull(ob.ukeys) for ob in obs]
                grads = [ob.lr_grad(N.weigh(ob.lr_loss(pw)[0], ob.labels, w))
                         for ob, pw in zip(obs, pulled)]
                for ob, g in zip(obs, grads):
                    s.push(ob.ukeys, g)
        trained = s.export()                 # (the model file is written before the test file's
        labs, ps = [], []                    # Pulls insert its unseen keys)
        for blk in capi.read_blocks(str(data2 / "test-00000"), 4 << 20):
            rp, keys, labels = blk[0], blk[1], blk[3]
            if flt is not None:
                keep = flt.keep_mask(keys)
                before = np.concatenate([[0], np.cumsum(keep)])
                rp, keys = before[rp.astype(np.int64)].astype(np.uint64), keys[keep]
            b = O.Batch(rp, keys, labels)
            ps.append(b.lr_loss(s.pull(b.ukeys))[1])
            labs.append(labels)
    lab, p = np.concatenate(labs), np.concatenate(ps)
    return trained, lab, p, O.auc_logloss(lab, p), [x.stats() for x in smp], astats


def local_sh_against(ref, data, tmp_path, *args):
    trained, lab, p, (ll, auc, tp, fp), stats, astats = ref
    ckpt, pred = str(tmp_path / "model"), str(tmp_path / "pred.txt")
    env = dict(os.environ, DMLC_PS_ROOT_PORT=str(free_port()))
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI,
                          str(data / "train"), str(data / "test"), "0", "2", "transport=host",
                          "block_size_mb=1", "capacity=16384", "model_out=" + ckpt,
                          "pred_path=" + pred, *args],
                         capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert O.format_auc_line(ll, auc, tp, fp) in lines, lines
    assert open(pred).read().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    want = sorted("rank %d neg_seen = %d neg_kept = %d rows_kept = %d" % (r, st[2], st[3], st[1])
                  for r, st in enumerate(stats))
    assert sorted(ln for ln in lines if "neg_seen" in ln) == want
    if "admit_shared=1" in args:
        want = sorted("rank %d admit_seen = %d admit_kept = %d" % (r, *astats[r]) for r in range(2))
        assert sorted(ln for ln in lines if "admit_seen" in ln) == want
    one = capi.Sharded(None, model="lr", optimizer="ftrl", capacity=1 << 15)
    one.load(ckpt)                                               # two shard files -> one table
    for a, e in zip(one.w.export(), trained):
        same(a, e)
    assert len(trained[0]) > 100


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "admit_shared"])
def test_local_sh_two_workers(data2, tmp_path, shared):
    extra = ["admit_count=2", "admit_shared=1", "admit_log2_slots=12"] if shared else []
    local_sh_against(reference_two(data2, shared), data2, tmp_path, "neg_keep=0.25", *extra)


@pytest.mark.parametrize("ingest", ["host", "gpu"])
def test_local_sh_a_rank_whose_rows_are_all_dropped(tmp_path, ingest):
    """rank 1's file holds negatives only and neg_keep = 2^-32 drops them all: in every turn rank 1
    steps the empty minibatch beside rank 0's positives, on the host parser's path and on the
    tokeniser's"""
    d = tmp_path / "data"
    d.mkdir()
    (d / "train-00000").write_bytes(zipf_text(25, (1 << 20) + (200 << 10), 0.05))
    (d / "train-00001").write_bytes(zipf_text(26, (1 << 20) + (200 << 10), 0.0))
    (d / "test-00000").write_bytes(zipf_text(22, 60 << 10, 0.3))
    ref = reference_two(d, False, keep=TINY, blocks_want=(2, 2))
    (_, kept0, _, neg0), (seen1, kept1, neg1, nk1) = ref[4]
    assert kept0 > 0 and neg0 == 0 and (kept1, nk1) == (0, 0) and neg1 == seen1 > 1000
    local_sh_against(ref, d, tmp_path, "neg_keep=%r" % TINY, "ingest=" + ingest)
