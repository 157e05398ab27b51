"""Feature values (feature_values=on) on a real MI355X: the valued generic build, valued LR and
valued canonical FM against the numpy checker of tests/_valued_checker.py — bit for bit, after
the checker alone has shown that every one of its sums is exact on these inputs —, the identity
with the binary path when every value is 1, the worker and the CLI end to end, the refusals."""
import os
import subprocess
import time

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import build, capi
from xflow_amd.single import SingleGpuTrainer

from . import _general_cases as GC
from . import _interval as I
from . import _valued_cases as Cs
from . import _valued_checker as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(a, b):
        i = np.flatnonzero((a != b).ravel())
        raise AssertionError("%d of %d differ; first (got, want): %s" % (
            i.size, a.size, [(a.ravel()[j], b.ravel()[j]) for j in i[:6]]))


def same_table(t, s):
    """keys and weights, and FTRL's (n, z)"""
    m = 4 if t.opt == capi.OPT_FTRL else 2
    for a, e in zip(t.export()[:m], s.export()[:m]):
        same(a, e)


def _go(opt):
    return capi.OPT_FTRL if opt == "ftrl" else capi.OPT_SGD


def gpu_tables(model, opt, k, mbs=None, cap=1 << 16):
    """the GPU's tables as Cs.stores makes the oracle's"""
    tw = capi.Table(_go(opt), 1, capacity=cap)
    tv = capi.Table(_go(opt), k, capi.INIT_HASHNORM, 0.0, seed=7, capacity=cap) \
        if model == "fm" else None
    if mbs is not None:
        tw.import_(*Cs.old_state(Cs.stream_keys(mbs), opt, 1, "w"))
        if tv is not None:
            tv.import_(*Cs.old_state(Cs.stream_keys(mbs), opt, k))
    return tw, tv


# ------------------------------------------------------------------------- the build
@pytest.mark.parametrize("case", Cs.CASES)
def test_device_builder_value_arrays_equal_host(case):
    for rowptr, keys, vals, labels in Cs.stream(case)[:2]:
        hb = capi.Batch(rowptr, keys, labels, values=vals)
        db = capi.Batch(rowptr, keys, labels, on_gpu=True, values=vals)
        hh, dh = hb.host(), db.host()
        for n in hh:
            same(dh[n], hh[n])
        for a, e in zip(db.values(), hb.values()):
            same(a, e)
        same(db.values()[0], vals)
        same(db.values()[1], vals[np.argsort(keys, kind="stable")])
        same(db.tiles(), hb.tiles())
        same(db.heavy_chunks(), hb.heavy_chunks())
    # an empty minibatch, and one whose rows are all empty
    for rp in (np.zeros(1, np.uint64), np.zeros(4, np.uint64)):
        db = capi.Batch(rp, np.zeros(0, np.uint64), np.zeros(len(rp) - 1, np.int32), on_gpu=True,
                        values=np.zeros(0, np.float32))
        assert (db.R, db.NNZ, db.U) == (len(rp) - 1, 0, 0) and db.values()[0].size == 0


# ------------------------------------------------------------------- steps vs the checker
def _steps(case, model, opt, k):
    mbs = Cs.stream(case)
    audit = []
    steps, sw, sv, pctr = Cs.run_checker(model, opt, k, mbs, audit)
    V.assert_exact(audit)            # every sum, before the GPU is looked at
    tw, tv = gpu_tables(model, opt, k, mbs)
    ws = capi.Workspace()
    if model == "fm":
        ws.fm_mode("canonical")
    b = None
    for i, ((rowptr, keys, vals, labels), (ukeys, wu, loss, gw)) in enumerate(zip(mbs, steps)):
        b = capi.Batch(rowptr, keys, labels, on_gpu=i != 1, values=vals)   # step 1: host-built
        if model == "fm":
            capi.fm_step(tw, tv, b, ws)
        else:
            capi.lr_step(tw, b, ws)
        same(b.host()["ukeys"], ukeys)
        g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
        same(g_wu, wu)
        same(g_loss, loss)
        same(g_gw, gw)
    same_table(tw, sw)
    if model == "fm":
        same_table(tv, sv)
    same(capi.fm_predict(tw, tv, b, ws) if model == "fm" else capi.lr_predict(tw, b, ws), pctr)
    # a replay of the last minibatch finds its keys' rows where it left them
    rowptr, keys, vals, labels = mbs[-1]
    if model == "fm":
        capi.fm_step(tw, tv, b, ws)
        ukeys, wu, loss, gw = V.fm_step(sw, sv, rowptr, keys, vals, labels, audit)
    else:
        capi.lr_step(tw, b, ws)
        ukeys, wu, loss, gw = V.lr_step(sw, rowptr, keys, vals, labels, audit)
    V.assert_exact(audit)
    g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
    same(g_wu, wu)
    same(g_loss, loss)
    same(g_gw, gw)
    same_table(tw, sw)
    if model == "fm":
        same_table(tv, sv)


@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("case", Cs.CASES)
def test_valued_lr_steps_equal_the_checker(case, opt):
    _steps(case, "lr", opt, 1)


@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("k", Cs.KS)
@pytest.mark.parametrize("case", Cs.CASES)
def test_valued_fm_steps_equal_the_checker(case, k, opt):
    _steps(case, "fm", opt, k)


# ------------------------------------------------------------------------ the identity
@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("case", ["ragged", "zipf_chunks"])
def test_all_values_one_is_the_binary_lr_path(case, opt):
    """fresh tables (zero init, keys inserted by the Pull): valued LR on the generic minibatch
    against LocalBatch + lr_step, the cells path"""
    ta, tb = capi.Table(_go(opt), 1, capacity=1 << 16), capi.Table(_go(opt), 1, capacity=1 << 16)
    wa, wb = capi.Workspace(), capi.Workspace()
    for rowptr, keys, vals, labels in Cs.stream(case) * 2:
        va = capi.Batch(rowptr, keys, labels, on_gpu=True, values=np.ones_like(vals))
        capi.lr_step(ta, va, wa)
        capi.lr_step(tb, capi.LocalBatch(tb, rowptr, keys, labels), wb)
        same(wa.fetch_loss(va.R), wb.fetch_loss(va.R))
        for a, e in zip(ta.export(), tb.export()):
            same(a, e)
    same(capi.lr_predict(ta, va, wa), capi.lr_predict(tb, capi.LocalBatch(tb, rowptr, keys, labels), wb))


@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("k", [1, 4, 7, 16, 64, 80])
def test_all_values_one_is_the_binary_canonical_path(k, opt):
    """fresh tables (hash-normal factors): the valued kernels against the canonical ones"""
    (ta, va_), (tb, vb_) = gpu_tables("fm", opt, k), gpu_tables("fm", opt, k)
    wa, wb = capi.Workspace(), capi.Workspace()
    wa.fm_mode("canonical")
    wb.fm_mode("canonical")
    for case in ("ragged", "zipf_chunks"):
        for rowptr, keys, vals, labels in Cs.stream(case):
            a = capi.Batch(rowptr, keys, labels, on_gpu=True, values=np.ones_like(vals))
            b = capi.Batch(rowptr, keys, labels, on_gpu=True)
            capi.fm_step(ta, va_, a, wa)
            capi.fm_step(tb, vb_, b, wb)
            for x, y in zip(wa.fetch(a.U, a.R), wb.fetch(b.U, b.R)):
                same(x, y)
            for x, y in zip(ta.export() + va_.export(), tb.export() + vb_.export()):
                same(x, y)
    same(capi.fm_predict(ta, va_, a, wa), capi.fm_predict(tb, vb_, b, wb))


# ------------------------------------------------------------- trainers above the kernels
@pytest.mark.parametrize("model,opt,k", [("lr", "ftrl", 1), ("lr", "sgd", 1), ("fm", "ftrl", 16),
                                         ("fm", "sgd", 7)])
def test_sharded_one_rank_and_single_gpu_trainer(model, opt, k):
    import torch
    mbs = Cs.stream("zipf_heavy", seed=3)
    audit = []
    steps, sw, sv, pctr = Cs.run_checker(model, opt, k, mbs, audit)
    V.assert_exact(audit)
    for host_key_build in (False, True):
        st = capi.Sharded(model=model, optimizer=opt, k=k, capacity=1 << 16, seed=7,
                          host_key_build=host_key_build,
                          fm_mode="canonical" if model == "fm" else "reference")
        st.w.import_(*Cs.old_state(Cs.stream_keys(mbs), opt, 1, "w"))
        if model == "fm":
            st.v.import_(*Cs.old_state(Cs.stream_keys(mbs), opt, k))
        for i, (rowptr, keys, vals, labels) in enumerate(mbs):
            if i == 1 and not host_key_build:       # device arrays
                dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
                dv = torch.from_numpy(vals.copy()).cuda()
                dr = torch.from_numpy(rowptr.astype(np.uint32).view(np.int32)).cuda()
                dl = torch.from_numpy(labels).cuda()
                torch.cuda.synchronize()
                b = st.compile_valued_dev(dk.data_ptr(), dv.data_ptr(), dr.data_ptr(),
                                          dl.data_ptr(), len(labels), int(rowptr[-1]))
            else:
                b = st.compile(rowptr, keys, labels, values=vals)
            st.step(b)
            st.check()
        same(st.predict(b), pctr)
        same_table(st.w, sw)
        if model == "fm":
            same_table(st.v, sv)
    # SingleGpuTrainer(feature_values=True) from fresh tables: the identity again, through it
    one = SingleGpuTrainer(model, opt, k, capacity=1 << 16, feature_values=True,
                           fm_mode="canonical" if model == "fm" else "reference")
    two = SingleGpuTrainer(model, opt, k, capacity=1 << 16,
                           fm_mode="canonical" if model == "fm" else "reference")
    for rowptr, keys, vals, labels in mbs:
        one.step(one.compile(rowptr, keys, labels, values=np.ones_like(vals)))
        two.step(two.compile(rowptr, keys, labels))
    for x, y in zip(one.w.export(), two.w.export()):
        same(x, y)
    if model == "fm":
        for x, y in zip(one.v.export(), two.v.export()):
            same(x, y)


# ------------------------------------------------------------------- the worker, the CLI
@pytest.mark.parametrize("model,opt,k", Cs.E2E + ((1, "ftrl", 4),))
def test_worker_end_to_end(sample_prefixes, tmp_path, model, opt, k):
    """Cs.E2E: every sum of the checker is exact (assert_exact).  FM + FTRL from fresh tables
    fails that audit; there the interval rule of tests/_interval.py pins every sum to one fp32
    value — no open sum, asserted here and in tests/test_general_position_cpu.py — and the
    comparison is as exact as for the others"""
    tr, te = sample_prefixes
    if (model, opt) == (1, "ftrl"):
        judge = I.Judge()
        sw, sv, lab, p, (ll, auc, tp, fp) = GC.run_files("fm", opt, 0, k, tr + "-00000",
                                                         te + "-00000", judge)
        assert judge.open_count() == 0, judge.table()
    else:
        audit = []
        sw, sv, lab, p, (ll, auc, tp, fp) = Cs.run_checker_files(model, opt, k, tr + "-00000",
                                                                 te + "-00000", audit)
        V.assert_exact(audit)
    extra = {"fm_mode": "canonical"} if model == 1 else {}
    pred = str(tmp_path / "p.txt")
    x = capi.XFlow(tr, te, model=model, epochs=Cs.E2E_EPOCHS, k=k, optimizer=opt, capacity=4096,
                   pred_path=pred, feature_values="on", **extra)
    x.train()
    wh, vh = x.tables()
    same_table(capi.Table.from_handle(wh, 1, _go(opt)), sw)
    if model == 1:
        same_table(capi.Table.from_handle(vh, k, _go(opt)), sv)
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    want = ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    assert open(pred).read().split("\n")[:-1] == want
    with pytest.raises(capi.XFError, match="feature_values"):
        x.set("feature_values", "off")              # training has started
    # the binary run of the same files differs (the values are read), and is what it was
    y = capi.XFlow(tr, te, model=model, epochs=Cs.E2E_EPOCHS, k=k, optimizer=opt, capacity=4096,
                   pred_path=str(tmp_path / "q.txt"), **extra)
    y.train()
    assert open(pred).read() != open(str(tmp_path / "q.txt")).read()
    # the CLI: the same metric line and pred file
    args = [os.path.join(build.LIBDIR, "xflow_lr"), tr, te, str(model), str(Cs.E2E_EPOCHS),
            "feature_values=on", "optimizer=" + opt, "k=%d" % k, "pred_path=cli.txt"]
    if model == 1:
        args.append("fm_mode=canonical")
    out = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert O.format_auc_line(ll, auc, tp, fp) in out.stdout.splitlines(), out.stdout
    assert open(str(tmp_path / "cli.txt")).read().split("\n")[:-1] == want


# ---------------------------------------------------------------------------- refusals
def test_refusals(sample_prefixes):
    rowptr, keys, vals, labels = Cs.ragged(0)
    vb = capi.Batch(rowptr, keys, labels, on_gpu=True, values=vals)
    tw, tv = gpu_tables("fm", "ftrl", 8)
    # FM in the reference form
    ws = capi.Workspace()
    with pytest.raises(capi.XFError, match=r"feature_values.*fm_mode"):
        capi.fm_step(tw, tv, vb, ws)
    with pytest.raises(capi.XFError, match=r"feature_values.*fm_mode"):
        capi.fm_predict(tw, tv, vb, ws)
    # a parity mode other than exact sums
    ws = capi.Workspace()
    ws.parity("reference_order")
    with pytest.raises(capi.XFError, match=r"feature_values.*parity"):
        capi.lr_step(tw, vb, ws)
    with pytest.raises(capi.XFError, match=r"feature_values.*parity"):
        capi.lr_predict(tw, vb, ws)
    # capture
    ws = capi.Workspace(capture=True)
    with pytest.raises(capi.XFError, match=r"feature_values.*xf_workspace_capture"):
        capi.lr_step(tw, vb, ws)
    ws.fm_mode("canonical")
    with pytest.raises(capi.XFError, match=r"feature_values.*xf_workspace_capture"):
        capi.fm_step(tw, tv, vb, ws)
    assert len(tw) == 0 and len(tv) == 0            # refused by the step itself, before any Pull
    # a binary minibatch keeps every path it has
    capi.lr_step(tw, capi.Batch(rowptr, keys, labels, on_gpu=True), capi.Workspace(capture=True))
    # the trainer: FM in the reference form
    st = capi.Sharded(model="fm", optimizer="ftrl", k=8, capacity=1 << 14)
    with pytest.raises(capi.XFError, match=r"feature_values.*fm_mode"):
        st.compile(rowptr, keys, labels, values=vals)
    # the worker's combinations, each named
    tr, te = sample_prefixes
    t0 = time.time()
    for params, why in (({"model": 1}, "fm_mode"),
                        ({"model": 0, "world": 2}, "one worker"),
                        ({"model": 0, "parity": "reference_order"}, "parity"),
                        ({"model": 0, "block_cache": 1}, "block_cache"),
                        ({"model": 0, "ingest": "gpu"}, "ingest"),
                        ({"model": 1, "fm_mode": "canonical", "block_cache": 1}, "block_cache")):
        with pytest.raises(capi.XFError, match=r"feature_values.*" + why):
            capi.XFlow(tr, te, feature_values="on", **params).train()
    assert time.time() - t0 < 20
    with pytest.raises(capi.XFError, match=r"feature_values.*maybe"):
        capi.XFlow(tr, te, feature_values="maybe")
