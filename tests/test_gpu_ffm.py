"""Field-aware FM (fm_mode=field_aware) on a real MI355X: the fielded generic build, the forward,
the gradient and both Pushes against the numpy checker of tests/_ffm_checker.py — bit for bit,
after the checker alone has shown that every one of its sums is exact on these inputs —, the
touched rule under FTRL, the identity with the binary instantiation when every value is 1, the
trainers, the worker and the CLI end to end with save / load, the refusals."""
import os
import subprocess
import time

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import build, capi
from xflow_amd.single import SingleGpuTrainer

from . import _ffm_checker as F
from . import _general_cases as GC
from . import _hyper_cases as HC
from . import _interval as I
from . import _valued_cases as Cs

pytestmark = pytest.mark.gpu
OPTS = ("ftrl", "sgd")


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


def gpu_tables(opt, Fd, k, mbs=None, cap=1 << 16, seed=7):
    """the GPU's tables as F.stores / F.aged_stores make the oracle's"""
    tw = capi.Table(_go(opt), 1, capacity=cap)
    tv = capi.Table(_go(opt), Fd * k, capi.INIT_HASHNORM, 0.0, seed=seed, capacity=cap)
    if mbs is not None:
        tw.import_(*Cs.old_state(F.stream_keys(mbs), opt, 1, "w"))
        tv.import_(*Cs.old_state(F.stream_keys(mbs), opt, Fd * k))
    return tw, tv


def workspace(Fd):
    ws = capi.Workspace()
    ws.fm_fields(Fd)
    ws.fm_mode("field_aware")
    return ws


def batch(mb, Fd, valued, on_gpu=True):
    rowptr, keys, fg, vals, labels = mb
    return capi.Batch(rowptr, keys, labels, on_gpu=on_gpu, values=vals if valued else None,
                      fields=Fd, fgid=fg)


# ------------------------------------------------------------------------- the build
@pytest.mark.parametrize("case", F.CASES)
def test_device_builder_field_arrays_equal_host(case):
    for mb in F.stream(case, 39)[:2]:
        rowptr, keys, fg, vals, labels = mb
        for valued in (False, True):
            hb, db = batch(mb, 39, valued, on_gpu=False), batch(mb, 39, valued)
            hh, dh = hb.host(), db.host()
            for n in hh:
                same(dh[n], hh[n])
            for a, e in zip(db.field_arrays(), hb.field_arrays()):
                same(a, e)
            for a, e in zip(db.field_arrays(), F.field_arrays(rowptr, keys, fg)):
                same(a, e)
            for a, e in zip(db.values(), hb.values()):
                same(a, e)
            same(db.tiles(), hb.tiles())
            same(db.heavy_chunks(), hb.heavy_chunks())
    # an empty minibatch, and one whose rows are all empty
    for rp in (np.zeros(1, np.uint64), np.zeros(4, np.uint64)):
        db = capi.Batch(rp, np.zeros(0, np.uint64), np.zeros(len(rp) - 1, np.int32), on_gpu=True,
                        fields=7, fgid=np.zeros(0, np.int32))
        assert (db.R, db.NNZ, db.U) == (len(rp) - 1, 0, 0) and db.field_arrays()[0].size == 0
    # an fgid outside [0, fields): refused by name, by the device build too
    with pytest.raises(capi.XFError, match=r"fgid \d+.*fields = 5"):
        batch(mb, 5, False)


# ------------------------------------------------------------------- steps vs the checker
def _steps(case, Fd, k, opt, valued, aged=True, nsteps=F.STEPS):
    mbs = F.stream(case, Fd)[:nsteps]
    audit = []
    sw, sv = F.aged_stores(opt, Fd, k, mbs) if aged else F.stores(opt, Fd, k, 7)
    steps, first = [], None
    for rowptr, keys, fg, vals, labels in mbs:
        steps.append(F.step(sw, sv, Fd, rowptr, keys, fg, vals if valued else None, labels, audit))
        first = first or (sw.export(), sv.export())     # the tables after the first step alone
    rowptr, keys, fg, vals, labels = mbs[-1]
    pctr = F.predict(sw, sv, Fd, rowptr, keys, fg, vals if valued else None, labels, audit)
    F.assert_exact(audit)            # every sum, before the GPU is looked at
    tw, tv = gpu_tables(opt, Fd, k, mbs if aged else None)
    ws = workspace(Fd)
    b = None
    for i, (mb, (ukeys, wu, loss, gw, gv, touched)) in enumerate(zip(mbs, steps)):
        b = batch(mb, Fd, valued, on_gpu=i != 1)                  # step 1: host-built
        capi.fm_step(tw, tv, b, ws)
        same(b.host()["ukeys"], ukeys)
        g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
        same(g_wu, wu)
        same(g_loss, loss)
        same(g_gw, gw)
        if i == 0:
            m = 4 if opt == "ftrl" else 2
            for t, ex in zip((tw, tv), first):
                for x, e in zip(t.export()[:m], ex[:m]):
                    same(x, e)
    same_table(tw, sw)
    same_table(tv, sv)
    same(capi.fm_predict(tw, tv, b, ws), pctr)
    if not aged:
        return
    # a replay of the last minibatch finds its keys' rows where it left them
    rowptr, keys, fg, vals, labels = mbs[-1]
    capi.fm_step(tw, tv, b, ws)
    r = F.step(sw, sv, Fd, rowptr, keys, fg, vals if valued else None, labels, audit)
    F.assert_exact(audit)
    for a, e in zip(ws.fetch(b.U, b.R), r[1:4]):
        same(a, e)
    same_table(tw, sw)
    same_table(tv, sv)


@pytest.mark.parametrize("valued", [False, True], ids=["binary", "valued"])
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("case,Fd,k", F.GRID)
def test_steps_equal_the_checker(case, Fd, k, opt, valued):
    """aged tables (tests/_valued_cases.old_state), three steps and a replay"""
    _steps(case, Fd, k, opt, valued)


@pytest.mark.parametrize("case,Fd,k,opt,valued,nsteps", F.FRESH)
def test_steps_from_fresh_tables(case, Fd, k, opt, valued, nsteps):
    """fresh hash-normal tables, keys inserted by the Pulls"""
    _steps(case, Fd, k, opt, valued, aged=False, nsteps=nsteps)


# ------------------------------------------------------------------------ the touched rule
@pytest.mark.parametrize("aged", [True, False], ids=["aged", "fresh"])
def test_untouched_coordinates_keep_their_state_under_ftrl(aged):
    Fd, k = 39, 4
    mb = F.stream("ragged", Fd)[0]
    rowptr, keys, fg, vals, labels = mb
    sw, sv = F.aged_stores("ftrl", Fd, k, [mb]) if aged else F.stores("ftrl", Fd, k, 7)
    tw, tv = gpu_tables("ftrl", Fd, k, [mb] if aged else None)
    ws = workspace(Fd)
    b = batch(mb, Fd, False)
    capi.fm_predict(tw, tv, b, ws)              # a Pull: the keys are in, at their init
    before = tv.export()
    audit = []
    ukeys, _, _, _, gv, touched = F.step(sw, sv, Fd, rowptr, keys, fg, None, labels, audit)
    F.assert_exact(audit)
    assert 0.02 < 1.0 - touched.mean() < 0.99           # untouched (key, field) pairs exist
    capi.fm_step(tw, tv, b, ws)
    after = tv.export()
    same(after[0], before[0])
    at = np.searchsorted(before[0], ukeys)
    mask = np.repeat(touched, k, axis=1)
    for a, e in zip(after[1:], before[1:]):             # w, n, z of the untouched: bit for bit
        same(a[at][~mask], e[at][~mask])
    same_table(tv, sv)                                  # the touched ones: the checker's
    if aged:
        return
    # from fresh tables, stepping every coordinate is another table: a step with g = 0 leaves
    # n = z = 0 and sets the hash-normal weight to 0 (an aged coordinate, whose w is the one its
    # (n, z) give, would not move)
    sw2, sv2 = F.stores("ftrl", Fd, k, 7)
    F.step(sw2, sv2, Fd, rowptr, keys, fg, None, labels, [], touched_only=False)
    w_all = sv2.export()[1][at]
    assert np.all(w_all[~mask] == 0.0) and np.all(after[1][at][~mask] != 0.0)


# ------------------------------------------------------------------------ the identity
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("Fd,k", [(18, 4), (3, 7), (64, 16), (1, 8)])
def test_all_values_one_is_the_binary_instantiation(Fd, k, opt):
    """fresh tables (hash-normal factors): VAL = true with every x = 1 against VAL = false"""
    (ta, va_), (tb, vb_) = gpu_tables(opt, Fd, k), gpu_tables(opt, Fd, k)
    wa, wb = workspace(Fd), workspace(Fd)
    for case in ("ragged", "zipf_chunks"):
        for rowptr, keys, fg, vals, labels in F.stream(case, Fd):
            a = capi.Batch(rowptr, keys, labels, on_gpu=True, values=np.ones_like(vals),
                           fields=Fd, fgid=fg)
            b = capi.Batch(rowptr, keys, labels, on_gpu=True, fields=Fd, fgid=fg)
            capi.fm_step(ta, va_, a, wa)
            capi.fm_step(tb, vb_, b, wb)
            for x, y in zip(wa.fetch(a.U, a.R), wb.fetch(b.U, b.R)):
                same(x, y)
            for x, y in zip(ta.export() + va_.export(), tb.export() + vb_.export()):
                same(x, y)
    same(capi.fm_predict(ta, va_, a, wa), capi.fm_predict(tb, vb_, b, wb))


# ------------------------------------------------------------- trainers above the kernels
@pytest.mark.parametrize("opt,Fd,k,valued", [("ftrl", 18, 4, True), ("sgd", 39, 7, False)])
def test_sharded_one_rank_and_single_gpu_trainer(opt, Fd, k, valued):
    import torch
    mbs = F.stream("zipf_heavy", Fd, seed=3)
    audit = []
    steps, sw, sv, pctr = F.run_checker(opt, Fd, k, mbs, audit, valued=valued)
    F.assert_exact(audit)
    for host_key_build in (False, True):
        st = capi.Sharded(model="fm", optimizer=opt, k=k, capacity=1 << 16, seed=7,
                          host_key_build=host_key_build, fm_mode="field_aware", fields=Fd)
        st.w.import_(*Cs.old_state(F.stream_keys(mbs), opt, 1, "w"))
        st.v.import_(*Cs.old_state(F.stream_keys(mbs), opt, Fd * k))
        for i, (rowptr, keys, fg, vals, labels) in enumerate(mbs):
            if i == 1 and not host_key_build:       # device arrays
                dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
                dg = torch.from_numpy(fg.astype(np.int32)).cuda()
                dv = torch.from_numpy(vals.copy()).cuda()
                dr = torch.from_numpy(rowptr.astype(np.uint32).view(np.int32)).cuda()
                dl = torch.from_numpy(labels).cuda()
                torch.cuda.synchronize()
                h = capi.vp()
                capi.check(capi.lib().xf_sharded_compile_fielded_dev(
                    st.h, capi.C.byref(h), dk.data_ptr(), dg.data_ptr(),
                    dv.data_ptr() if valued else None, dr.data_ptr(), dl.data_ptr(), len(labels),
                    int(rowptr[-1]), 1))
                b = capi.ShardedBatch(h, st)
            else:
                b = st.compile(rowptr, keys, labels, values=vals if valued else None, fgid=fg)
            st.step(b)
            st.check()
        same(st.predict(b), pctr)
        same_table(st.w, sw)
        same_table(st.v, sv)
    # SingleGpuTrainer from fresh tables: all values 1 against the binary trainer, through it
    one = SingleGpuTrainer("fm", opt, k, capacity=1 << 16, feature_values=True,
                           fm_mode="field_aware", fields=Fd)
    two = SingleGpuTrainer("fm", opt, k, capacity=1 << 16, fm_mode="field_aware", fields=Fd)
    for rowptr, keys, fg, vals, labels in mbs:
        one.step(one.compile(rowptr, keys, labels, values=np.ones_like(vals), fgid=fg))
        two.step(two.compile(rowptr, keys, labels, fgid=fg))
    for x, y in zip(one.w.export() + one.v.export(), two.w.export() + two.v.export()):
        same(x, y)


# ------------------------------------------------------------------- the worker, the CLI
@pytest.mark.parametrize("valued,opt", [(False, "sgd"), (True, "sgd"), (False, "ftrl"),
                                        (True, "ftrl")],
                         ids=["binary", "valued", "ftrl-binary", "ftrl-valued"])
def test_worker_end_to_end(sample_prefixes, tmp_path, valued, opt):
    """the golden files, fields = 18, k = 4, two epochs.  SGD: every sum of the checker is exact
    (assert_exact).  FTRL from fresh tables fails that audit
    (tests/test_ffm_cpu.py::test_golden_files_from_fresh_tables); there the interval rule of
    tests/_interval.py pins every sum to one fp32 value — no open sum, asserted here and in
    tests/test_general_position_cpu.py — and the comparison is as exact as under SGD"""
    tr, te = sample_prefixes
    Fd, k = F.E2E_FIELDS, F.E2E_K
    if opt == "sgd":
        audit = []
        sw, sv, lab, p, (ll, auc, tp, fp) = F.run_checker_files(opt, tr + "-00000", te + "-00000",
                                                                audit, valued)
        F.assert_exact(audit)
    else:
        judge = I.Judge()
        sw, sv, lab, p, (ll, auc, tp, fp) = GC.run_files("ffm", opt, Fd, k, tr + "-00000",
                                                         te + "-00000", judge, valued)
        assert judge.open_count() == 0, judge.table()
    extra = {"feature_values": "on"} if valued else {}
    pred = str(tmp_path / "p.txt")
    ckpt = str(tmp_path / "m.bin")
    x = capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=Fd, epochs=F.E2E_EPOCHS, k=k,
                   optimizer=opt, capacity=4096, pred_path=pred, model_out=ckpt, **extra)
    x.train()
    wh, vh = x.tables()
    same_table(capi.Table.from_handle(wh, 1, _go(opt)), sw)
    same_table(capi.Table.from_handle(vh, Fd * k, _go(opt)), sv)
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    want = ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    assert open(pred).read().split("\n")[:-1] == want
    with pytest.raises(capi.XFError, match="fields"):
        x.set("fields", 3)                          # training has started
    # the block cache carries fgid: the same run from it (binary minibatches only)
    if not valued:
        c = capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=Fd, epochs=F.E2E_EPOCHS,
                       k=k, optimizer=opt, capacity=4096, pred_path=str(tmp_path / "c.txt"),
                       block_cache=1, block_cache_dir=str(tmp_path))
        c.train()
        assert open(str(tmp_path / "c.txt")).read() == open(pred).read()
    # save / load: the F k wide table round-trips, and a loaded worker predicts the same file
    y = capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=Fd, epochs=0, k=k,
                   optimizer=opt, capacity=4096, pred_path=str(tmp_path / "q.txt"),
                   model_in=ckpt, **extra)
    y.train()                                        # no epoch: load, then score the test file
    assert open(str(tmp_path / "q.txt")).read() == open(pred).read()
    y.save(str(tmp_path / "m2.bin"))
    z = capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=Fd, epochs=0, k=k,
                   optimizer=opt, capacity=4096, pred_path=str(tmp_path / "r.txt"),
                   model_in=str(tmp_path / "m2.bin"), **extra)
    z.train()
    assert open(str(tmp_path / "r.txt")).read() == open(pred).read()
    # a model file of another width is refused
    with pytest.raises(capi.XFError):
        capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=Fd, epochs=0, k=k + 1,
                   optimizer=opt, capacity=4096, pred_path=str(tmp_path / "s.txt"),
                   model_in=ckpt).train()
    # the CLI: the same metric line and pred file
    args = [os.path.join(build.LIBDIR, "xflow_lr"), tr, te, "1", str(F.E2E_EPOCHS),
            "fm_mode=field_aware", "fields=%d" % Fd, "optimizer=" + opt, "k=%d" % k,
            "pred_path=cli.txt"] + (["feature_values=on"] if valued else [])
    out = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert O.format_auc_line(ll, auc, tp, fp) in out.stdout.splitlines(), out.stdout
    assert open(str(tmp_path / "cli.txt")).read().split("\n")[:-1] == want
    # fields too small for the files' fgid: refused by name, when the first minibatch is compiled
    with pytest.raises(capi.XFError, match=r"fgid \d+.*fields = 17"):
        capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=17, epochs=1, k=k,
                   optimizer=opt, capacity=4096, pred_path=str(tmp_path / "t.txt")).train()


@pytest.mark.parametrize("valued", [False, True], ids=["binary", "valued"])
def test_worker_and_cli_under_other_ftrl_hyper_parameters(sample_prefixes, tmp_path, valued):
    """XFlow(alpha=, beta=, lambda1=, lambda2=) and the CLI's alpha= beta= lambda1= lambda2=
    options, set A of tests/_hyper_cases.py: the worker hands every value to both tables.  The
    interval rule pins every sum on the golden files under A too (asserted here and in
    tests/test_general_position_cpu.py), so tables, metrics and the pctr file are compared as
    exactly as under the defaults"""
    tr, te = sample_prefixes
    Fd, k, h = F.E2E_FIELDS, F.E2E_K, HC.A
    judge = I.Judge()
    sw, sv, lab, p, (ll, auc, tp, fp) = GC.run_files("ffm", "ftrl", Fd, k, tr + "-00000",
                                                     te + "-00000", judge, valued, hyper=h)
    assert judge.open_count() == 0, judge.table()
    dw, dv = GC.run_files("ffm", "ftrl", Fd, k, tr + "-00000", te + "-00000", I.Judge(), valued)[:2]
    assert not np.array_equal(sw.export()[1], dw.export()[1])     # not the default's tables
    assert not np.array_equal(sv.export()[1], dv.export()[1])
    extra = {"feature_values": "on"} if valued else {}
    pred = str(tmp_path / "p.txt")
    x = capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=Fd, epochs=F.E2E_EPOCHS, k=k,
                   optimizer="ftrl", capacity=4096, pred_path=pred, **extra, **h.kw())
    x.train()
    wh, vh = x.tables()
    same_table(capi.Table.from_handle(wh, 1, capi.OPT_FTRL), sw)
    same_table(capi.Table.from_handle(vh, Fd * k, capi.OPT_FTRL), sv)
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    want = ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    assert open(pred).read().split("\n")[:-1] == want
    if valued:
        return
    args = [os.path.join(build.LIBDIR, "xflow_lr"), tr, te, "1", str(F.E2E_EPOCHS),
            "fm_mode=field_aware", "fields=%d" % Fd, "optimizer=ftrl", "k=%d" % k,
            "pred_path=cli.txt"] + ["%s=%r" % kv for kv in h.kw().items() if kv[0] != "lr"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert O.format_auc_line(ll, auc, tp, fp) in out.stdout.splitlines(), out.stdout
    assert open(str(tmp_path / "cli.txt")).read().split("\n")[:-1] == want


# ---------------------------------------------------------------------------- refusals
def test_refusals(sample_prefixes):
    t0 = time.time()
    mb = F.stream("ragged", 18)[0]
    rowptr, keys, fg, vals, labels = mb
    fb = batch(mb, 18, False)
    plain = capi.Batch(rowptr, keys, labels, on_gpu=True)
    tw, tv = gpu_tables("ftrl", 18, 4)
    ws = workspace(18)
    # a minibatch compiled without fields
    with pytest.raises(capi.XFError, match=r"compiled without fields"):
        capi.fm_step(tw, tv, plain, ws)
    with pytest.raises(capi.XFError, match=r"compiled without fields"):
        capi.fm_predict(tw, tv, plain, ws)
    # ... with another number of fields
    with pytest.raises(capi.XFError, match=r"fields = 39.*fields = 18"):
        capi.fm_step(tw, tv, batch(F.stream("ragged", 39)[0], 39, False), ws)
    # the v table's dim is not fields x k
    t2 = capi.Table(capi.OPT_FTRL, 70, capi.INIT_HASHNORM, 0.0, seed=7, capacity=1 << 12)
    with pytest.raises(capi.XFError, match=r"dim \(70\).*fields \(18\)"):
        capi.fm_step(tw, t2, fb, ws)
    with pytest.raises(capi.XFError, match=r"dim \(70\).*fields \(18\)"):
        capi.fm_predict(tw, t2, fb, ws)
    assert len(tw) == 0 and len(tv) == 0 and len(t2) == 0      # refused before any Pull
    # a fielded minibatch keeps the other forms it has: canonical reads no field
    wc = capi.Workspace()
    wc.fm_mode("canonical")
    capi.fm_step(capi.Table(capi.OPT_FTRL, 1, capacity=1 << 14),
                 capi.Table(capi.OPT_FTRL, 4, capi.INIT_HASHNORM, 0.0, seed=7, capacity=1 << 14),
                 fb, wc)
    # keyed minibatches (xf_batch_compile_fm*): the build against the settled tiers carries no
    # fields (and no index of its key list)
    ka = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 14)
    kb = capi.Table(capi.OPT_FTRL, 16, capi.INIT_HASHNORM, 0.0, seed=7, capacity=1 << 14)
    for t in (ka, kb):
        t.pull(np.unique(keys))
        t.defrag()
    keyed = capi.FmBatch(ka, kb, rowptr, keys, labels)
    assert keyed.keyed
    with pytest.raises(capi.XFError, match=r"xf_batch_compile_fm"):
        capi.fm_step(ka, kb, keyed, ws)
    with pytest.raises(capi.XFError, match=r"xf_batch_compile_fm"):
        capi.fm_predict(ka, kb, keyed, ws)
    # the trainer: world 1 only is reachable here; the form needs its fields, and their product
    st = capi.Sharded(model="fm", optimizer="ftrl", k=8, capacity=1 << 14)
    with pytest.raises(capi.XFError, match=r"xf_sharded_set_fm_fields"):
        st.set_fm_mode("field_aware")
    with pytest.raises(capi.XFError, match=r"field_aware"):
        st.compile(rowptr, keys, labels, fgid=fg)              # the reference form
    capi.check(capi.lib().xf_sharded_set_fm_fields(st.h, 3))
    with pytest.raises(capi.XFError, match=r"width \(8\).*fields \(3\)"):
        st.set_fm_mode("field_aware")
    with pytest.raises(AssertionError, match=r"fields"):
        capi.Sharded(model="fm", fm_mode="field_aware", capacity=1 << 14)      # no fields given
    with pytest.raises(capi.XFError, match=r"not an FM trainer|FM trainer"):
        capi.Sharded(model="lr", fm_mode="field_aware", fields=3, capacity=1 << 14)
    # the worker's combinations, each named
    tr, te = sample_prefixes
    for params, why in (({"model": 0, "fields": 18}, "model 1"),
                        ({"model": 1, "fields": 0}, "fields"),
                        ({"model": 1, "fields": 65}, "fields"),
                        ({"model": 1, "fields": 64, "k": 65}, "4096"),
                        ({"model": 1, "fields": 18, "world": 2}, "one worker"),
                        ({"model": 1, "fields": 18, "parity": "reference_order"}, "parity"),
                        ({"model": 1, "fields": 18, "ingest": "gpu"}, "ingest")):
        with pytest.raises(capi.XFError, match=r"field_aware.*" + why):
            capi.XFlow(tr, te, fm_mode="field_aware", **params).train()
    with pytest.raises(capi.XFError, match=r"feature_values.*block_cache"):
        capi.XFlow(tr, te, model=1, fm_mode="field_aware", fields=18, feature_values="on",
                   block_cache=1).train()
    assert time.time() - t0 < 60
