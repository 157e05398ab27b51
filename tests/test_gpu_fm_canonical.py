"""Canonical FM (fm_mode=canonical) on a real MI355X against the numpy checker of
tests/_fmc_checker.py and the oracle's optimizer steps and inits — bit for bit."""
import os
import subprocess
import time

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import build, capi

from . import _fmc_checker as F
from . import _hyper_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(a, b):
        i = np.flatnonzero((a != b).ravel())
        raise AssertionError("%d of %d differ; first (got, want): %s" % (
            i.size, a.size, [(float(a.ravel()[j]), float(b.ravel()[j])) for j in i[:6]]))


def same_tables(tw, tv, sw, sv):
    """keys and weights, and FTRL's (n, z)"""
    m = 4 if tw.opt == capi.OPT_FTRL else 2
    for a, e in zip(tw.export()[:m], sw.export()[:m]):
        same(a, e)
    for a, e in zip(tv.export()[:m], sv.export()[:m]):
        same(a, e)


_KEYS = {}


def synth(rng, R, nnz_per_row, nkeys, zipf=None):
    """ragged rows (empty ones among them), keys repeated inside rows"""
    if nkeys not in _KEYS:
        _KEYS[nkeys] = capi.hash_decimal_range(0, nkeys)
    lens = rng.randint(0, 2 * nnz_per_row + 1, size=R)
    lens[:3] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(lens.sum())
    fid = (np.minimum(rng.zipf(zipf, size=n), nkeys) - 1) if zipf else rng.randint(0, nkeys, n)
    for r in range(3, R, 7):                     # a key twice in a row
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        if e - b >= 2:
            fid[b + 1] = fid[b]
    keys = _KEYS[nkeys][fid]
    labels = rng.randint(0, 2, size=R).astype(np.int32)
    return rowptr, keys, labels


def _opt(opt):
    return (capi.OPT_FTRL, O.OPT_FTRL) if opt == "ftrl" else (capi.OPT_SGD, O.OPT_SGD)


def _tables(opt, k, seed=11, cap=1 << 16):
    go, oo = _opt(opt)
    tw = capi.Table(go, 1, capacity=cap)
    tv = capi.Table(go, k, capi.INIT_HASHNORM, 0.0, seed=seed, capacity=cap)
    return tw, tv, F.stores(oo, k, seed)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("k", [4, 7, 10, 16, 32, 64])
def test_steps_state_loss_and_gradient(opt, k):
    _steps_state_loss_and_gradient(opt, k)


@pytest.mark.parametrize("opt,k", [("ftrl", 1), ("sgd", 2), ("ftrl", 80), ("sgd", 300)])
def test_steps_other_factor_counts(opt, k):
    """the forward's P = 1 / 2 paths and its passes of 64 factors (k > 64); the heavy kernels'
    column passes (k + 1 > 256 columns)"""
    _steps_state_loss_and_gradient(opt, k)


def _steps_state_loss_and_gradient(opt, k):
    rng = np.random.RandomState(k + (opt == "sgd"))
    tw, tv, (sw, sv) = _tables(opt, k)
    ws = capi.Workspace(capture=True)
    ws.fm_mode("canonical")
    plans = [(None, False), (1.3, True), (1.3, False), (None, True)]
    saw_heavy = saw_multichunk = False
    for zipf, on_gpu in plans:
        rowptr, keys, labels = synth(rng, 400, 25, 3000, zipf)
        b = capi.Batch(rowptr, keys, labels, on_gpu=on_gpu)
        capi.fm_step(tw, tv, b, ws)
        ukeys, wu, loss, gw = F.step(sw, sv, rowptr, keys, labels)
        h = b.host()
        same(h["ukeys"], ukeys)
        cnt = np.diff(h["segptr"].astype(np.int64))
        saw_heavy |= bool((cnt > capi.HEAVY_SEG).any())
        saw_multichunk |= bool((cnt > 2048).any())
        g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
        same(g_wu, wu)
        same(g_loss, loss)
        same(g_gw, gw)
        same_tables(tw, tv, sw, sv)
    assert saw_heavy and saw_multichunk
    # predict: the pull inserts the new keys, pctr from the checker's forward
    rowptr, keys, labels = synth(rng, 300, 20, 6000, None)
    b = capi.Batch(rowptr, keys, labels)
    same(capi.fm_predict(tw, tv, b, ws), F.predict(sw, sv, rowptr, keys, labels))
    same_tables(tw, tv, sw, sv)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_sharded_one_rank_compile_dev(opt):
    import torch
    k = 16
    rng = np.random.RandomState(3)
    st = capi.Sharded(model="fm", optimizer=opt, k=k, capacity=1 << 16, seed=5,
                      fm_mode="canonical")
    sw, sv = F.stores(_opt(opt)[1], k, 5)
    for zipf in (None, 1.3, None):
        rowptr, keys, labels = synth(rng, 300, 20, 2500, zipf)
        rp32 = rowptr.astype(np.uint32)
        dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
        dr = torch.from_numpy(rp32.view(np.int32)).cuda()
        dl = torch.from_numpy(labels).cuda()
        torch.cuda.synchronize()
        b = st.compile_dev(dk.data_ptr(), dr.data_ptr(), dl.data_ptr(), len(labels),
                           int(rowptr[-1]))
        assert not b.keyed          # the sort-based build (xf_batch_compile_dev): a key list
        st.step(b)
        st.check()
        F.step(sw, sv, rowptr, keys, labels)
        same_tables(st.w, st.v, sw, sv)
    # every key of the last minibatch now in the tables' settled tiers: a reference-form trainer
    # would take the keyed build (xf_batch_compile_fm_dev) for it; the canonical one may not
    ref = capi.Sharded(model="fm", optimizer=opt, k=k, capacity=1 << 16, seed=5)
    ref.step(ref.compile(rowptr, keys, labels))
    ref.defrag()
    st.defrag()
    b_ref = ref.compile_dev(dk.data_ptr(), dr.data_ptr(), dl.data_ptr(), len(labels),
                            int(rowptr[-1]))
    assert b_ref.keyed
    b = st.compile_dev(dk.data_ptr(), dr.data_ptr(), dl.data_ptr(), len(labels), int(rowptr[-1]))
    assert not b.keyed
    st.step(b)
    st.check()
    F.step(sw, sv, rowptr, keys, labels)
    same_tables(st.w, st.v, sw, sv)
    # host arrays through the same trainer (xf_batch_compile_gpu)
    rowptr, keys, labels = synth(rng, 200, 15, 2500, None)
    b = st.compile(rowptr, keys, labels)
    assert not b.keyed
    st.step(b)
    st.check()
    F.step(sw, sv, rowptr, keys, labels)
    same_tables(st.w, st.v, sw, sv)


def test_switching_modes_rebuilds_the_records():
    """reference -> canonical -> reference on the same tables and minibatch: the last steps
    equal the oracle's exact-sum reference update from the state canonical left"""
    k = 16
    rng = np.random.RandomState(21)
    tw, tv, (sw, sv) = _tables("ftrl", k, seed=4)
    ws = capi.Workspace()
    rowptr, keys, labels = synth(rng, 300, 20, 2000, 1.3)
    b = capi.Batch(rowptr, keys, labels)
    ob = O.Batch(rowptr, keys, labels)
    capi.fm_step(tw, tv, b, ws)                  # reference mode: the records are built
    with O.sum_mode(1):
        O.fm_update(sw, sv, ob)
    same_tables(tw, tv, sw, sv)
    ws.fm_mode("canonical")
    capi.fm_step(tw, tv, b, ws)
    F.step(sw, sv, rowptr, keys, labels)
    same_tables(tw, tv, sw, sv)
    ws.fm_mode("reference")
    for _ in range(2):
        capi.fm_step(tw, tv, b, ws)
        with O.sum_mode(1):
            O.fm_update(sw, sv, ob)
        same_tables(tw, tv, sw, sv)


def test_refusals(sample_prefixes):
    ws = capi.Workspace()
    ws.parity("reference_order")
    with pytest.raises(capi.XFError, match="reference-order|REFERENCE_ORDER"):
        ws.fm_mode("canonical")
    ws2 = capi.Workspace()
    ws2.fm_mode("canonical")
    with pytest.raises(capi.XFError, match="canonical"):
        ws2.parity("reference_order")
    # a keyed minibatch (the build against the settled tiers) has no index of its key list
    k = 16
    tw, tv, _ = _tables("ftrl", k)
    rng = np.random.RandomState(2)
    rowptr, keys, labels = synth(rng, 200, 10, 1500, None)
    for t in (tw, tv):
        t.pull(np.unique(keys))
        t.defrag()
    fb = capi.FmBatch(tw, tv, rowptr, keys, labels)
    assert fb.keyed
    with pytest.raises(capi.XFError, match="xf_batch_compile_dev"):
        capi.fm_step(tw, tv, fb, ws2)
    # the trainer's mode is set before the first step
    st = capi.Sharded(model="fm", optimizer="ftrl", k=8, capacity=1 << 14)
    st.step(st.compile(rowptr, keys, labels))
    st.check()
    with pytest.raises(capi.XFError, match="hold keys"):
        st.set_fm_mode("canonical")
    tr, te = sample_prefixes
    with pytest.raises(capi.XFError, match="model 1"):
        capi.XFlow(tr, te, model=0, fm_mode="canonical").train()
    t0 = time.time()
    with pytest.raises(capi.XFError, match="one worker"):
        capi.XFlow(tr, te, model=1, fm_mode="canonical", world=2).train()
    assert time.time() - t0 < 10


def _checker_run(tr, te, opt, k, epochs, hyper=None):
    sw, sv = F.stores(_opt(opt)[1], k, 0)        # the worker's seed: 0
    if hyper is not None:
        hyper.to_store(sw)
        hyper.to_store(sv)
    F.train_worker(sw, sv, tr + "-00000", epochs)
    lab, p = F.predict_file(sw, sv, te + "-00000")
    return sw, sv, O.auc_logloss(lab, p)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_worker_end_to_end(sample_prefixes, tmp_path, opt):
    tr, te = sample_prefixes
    sw, sv, (ll, auc, tp, fp) = _checker_run(tr, te, opt, 10, 3)
    for extra in ({}, {"ingest": "gpu"}):
        x = capi.XFlow(tr, te, model=1, fm_mode="canonical", epochs=3, k=10, optimizer=opt,
                       capacity=4096, pred_path=str(tmp_path / "p.txt"), **extra)
        x.train()
        wh, vh = x.tables()
        go = _opt(opt)[0]
        tw, tv = capi.Table.from_handle(wh, 1, go), capi.Table.from_handle(vh, 10, go)
        same_tables(tw, tv, sw, sv)
        assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
            (np.float32(ll), np.float32(auc))
        assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    if opt == "ftrl":   # the CLI prints the same metric line
        out = subprocess.run([os.path.join(build.LIBDIR, "xflow_lr"), tr, te, "1", "3",
                              "fm_mode=canonical"], capture_output=True, text=True, timeout=300,
                             cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr
        assert O.format_auc_line(ll, auc, tp, fp) in out.stdout.splitlines(), out.stdout


def test_worker_end_to_end_with_another_learning_rate(sample_prefixes, tmp_path):
    """XFlow(lr=0.05) and the command line's lr=0.05 under SGD: the worker hands the value to
    both tables (the checker's stores get it through set_sgd); tables, metrics, the pctr file"""
    tr, te = sample_prefixes
    h = HC.SGD_LO
    sw, sv, (ll, auc, tp, fp) = _checker_run(tr, te, "sgd", 10, 3, hyper=h)
    dw, dv, _ = _checker_run(tr, te, "sgd", 10, 3)
    assert not np.array_equal(sw.export()[1], dw.export()[1])     # not the default's tables
    pred = str(tmp_path / "p.txt")
    x = capi.XFlow(tr, te, model=1, fm_mode="canonical", epochs=3, k=10, optimizer="sgd",
                   capacity=4096, pred_path=pred, **h.kw())
    x.train()
    wh, vh = x.tables()
    go = _opt("sgd")[0]
    same_tables(capi.Table.from_handle(wh, 1, go), capi.Table.from_handle(vh, 10, go), sw, sv)
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    lab, p = F.predict_file(sw, sv, te + "-00000")
    want = ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    assert open(pred).read().split("\n")[:-1] == want
    # the command line's lr=: the same metric line and pctr file
    out = subprocess.run([os.path.join(build.LIBDIR, "xflow_lr"), tr, te, "1", "3",
                          "fm_mode=canonical", "optimizer=sgd", "k=10", "lr=0.05",
                          "pred_path=cli.txt"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert O.format_auc_line(ll, auc, tp, fp) in out.stdout.splitlines(), out.stdout
    assert open(str(tmp_path / "cli.txt")).read().split("\n")[:-1] == want


def test_default_is_the_reference_form(sample_prefixes):
    tr, te = sample_prefixes
    res = []
    for extra in ({}, {"fm_mode": "reference"}):
        x = capi.XFlow(tr, te, model=1, epochs=2, k=8, capacity=4096, **extra)
        x.train()
        wh, vh = x.tables()
        tw, tv = capi.Table.from_handle(wh, 1), capi.Table.from_handle(vh, 8)
        res.append((tw.export(), tv.export(), x.metric("logloss_ref"), x.metric("auc")))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        same(a, b)
    assert res[0][2:] == res[1][2:]


def test_one_large_step_k64_ftrl():
    """>= 2e6 nonzeros, k = 64, FTRL, Zipf 1.1 (the power-law head in many chunks)"""
    k = 64
    rng = np.random.RandomState(64)
    R, nkeys = 20000, 1 << 20
    lens = rng.randint(60, 151, size=R)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(rowptr[-1])
    fid = np.minimum(rng.zipf(1.1, size=n), nkeys) - 1
    keys = capi.hash_decimal_range(0, nkeys)[fid]
    labels = rng.randint(0, 2, size=R).astype(np.int32)
    tw, tv, (sw, sv) = _tables("ftrl", k, seed=9, cap=1 << 21)
    ws = capi.Workspace(capture=True)
    ws.fm_mode("canonical")
    b = capi.Batch(rowptr, keys, labels, on_gpu=True)
    assert b.NNZ >= 2_000_000
    capi.fm_step(tw, tv, b, ws)
    ukeys, wu, loss, gw = F.step(sw, sv, rowptr, keys, labels)
    _, g_loss, g_gw = ws.fetch(b.U, b.R)
    same(g_loss, loss)
    same(g_gw, gw)
    same_tables(tw, tv, sw, sv)
