"""Valued LR, valued canonical FM and field-aware FM on a real MI355X on inputs in general
position (tests/_general_cases.py: full mantissas, signs mixed inside a row, magnitudes over many
binades, fresh tables and four steps under FTRL and SGD, an underflow minibatch), judged by
tests/_general_checker.py: bit for bit wherever tests/_interval.py pins the sum, one of the
candidates where it leaves the sum open, and at most 2 % of any family open in every test."""
import numpy as np
import pytest

from xflow_amd import capi

from . import _general_cases as GC
from . import _general_checker as G
from . import _interval as I

pytestmark = pytest.mark.gpu
bits = G.bits


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
        raise AssertionError("%s: %d of %d differ; first (got, want): %s" % (
            what, i.size, a.size, [(a.ravel()[j], b.ravel()[j]) for j in i[:6]]))


def one_of(got, cands, what):
    """got[...] is one of cands[..., c], bit for bit — the one there is where the sum is pinned"""
    got, cands = np.asarray(got, np.float32), np.asarray(cands, np.float32)
    assert cands.shape[:-1] == got.shape, (what, got.shape, cands.shape)
    ok = (bits(got)[..., None] == bits(cands)).any(axis=-1)
    if not ok.all():
        i = np.flatnonzero(~ok.ravel())
        c = cands.reshape(-1, cands.shape[-1])
        raise AssertionError("%s: %d of %d are no candidate; first (got, candidates): %s" % (
            what, i.size, got.size, [(got.ravel()[j], sorted(set(c[j].tolist()))) for j in i[:4]]))


def table_is(t, e, what):
    """the GPU table against an Expected: the keys; every (w, n, z) — SGD: w — one candidate's;
    what the step does not move (other keys, untouched coordinates) the table before, bit for
    bit.  -> the export"""
    ex = t.export()
    same(ex[0], e.keys, what + " keys")
    cols = [a.reshape(e.pre[0].shape) for a in ex[1:(4 if t.opt == capi.OPT_FTRL else 2)]]
    ok = e.holds(*cols)
    if not ok.all():
        r, c = np.argwhere(~ok)[0]
        raise AssertionError("%s: %d of %d coordinates hold no candidate's state; first: key row "
                             "%d, coordinate %d, got %s, low candidate %s" % (
                                 what, int((~ok).sum()), ok.size, r, c,
                                 [a[r, c] for a in cols], [a[r, c] for a in e.first]))
    for a, p in zip(cols, e.pre):
        same(a[~e.stepped], p[~e.stepped], what + " coordinates the step does not move")
    return ex


def _go(opt):
    return capi.OPT_FTRL if opt == "ftrl" else capi.OPT_SGD


def _run(form, case, fields, k, opt, valued=True):
    mbs = GC.gpu_stream(form, case, fields)
    mbs = mbs if valued else GC.binary(mbs)
    seed = GC.init_seed(case)
    judge = I.Judge()
    sw, sv = GC.stores(form, opt, fields, k, seed)
    run = G.Run(form, sw, sv, judge, fields)
    tw = capi.Table(_go(opt), 1, capacity=1 << 16)
    tv = None if form == "lr" else capi.Table(_go(opt), sv.dim, capi.INIT_HASHNORM, 0.0,
                                              seed=seed, capacity=1 << 16)
    ws = capi.Workspace()
    if form == "ffm":
        ws.fm_fields(fields)
        ws.fm_mode("field_aware")
    elif form == "fm":
        ws.fm_mode("canonical")
    sgd = opt == "sgd"
    b = None
    for i, mb in enumerate(mbs):
        rowptr, keys, fg, vals, labels = mb
        extra = {"fields": fields, "fgid": fg} if form == "ffm" else {}
        b = capi.Batch(rowptr, keys, labels, on_gpu=i != 1, values=vals, **extra)  # step 1: host
        ukeys, wu, loss_c = run.begin(mb)
        if form == "lr":
            capi.lr_step(tw, b, ws)
        else:
            capi.fm_step(tw, tv, b, ws)
        same(b.host()["ukeys"], ukeys, "ukeys")
        g_wu, g_loss, g_gw = ws.fetch(b.U, b.R)
        same(g_wu, wu, "step %d wu" % i)
        one_of(g_loss, loss_c, "step %d loss" % i)
        gw_c, ew, ev = run.finish(g_loss)               # the gradient of the GPU's own loss
        one_of(g_gw, gw_c, "step %d gw" % i)
        xw = table_is(tw, ew, "step %d w table" % i)
        xv = table_is(tv, ev, "step %d v table" % i) if tv is not None else None
        if form == "ffm":
            assert fields <= 3 or not run.touched.all()      # untouched coordinates exist
        # the next step starts from the GPU's state: an open sum does not compound
        run.adopt(xw[:2] if sgd else xw, None if xv is None else (xv[:2] if sgd else xv))
    pctr = capi.lr_predict(tw, b, ws) if form == "lr" else capi.fm_predict(tw, tv, b, ws)
    one_of(pctr, run.predict(mbs[-1]), "pctr")
    print(judge.format("%s %s %dx%d %s %s" % (form, case, fields, k, opt,
                                              "valued" if valued else "binary")))
    judge.assert_cap()


@pytest.mark.parametrize("opt", GC.OPTS)
@pytest.mark.parametrize("case", GC.LR_CASES + ("underflow",))
def test_valued_lr(case, opt):
    _run("lr", case, 0, 1, opt)


@pytest.mark.parametrize("opt", GC.OPTS)
@pytest.mark.parametrize("case,k", GC.FM_GRID + (("underflow", 4),))
def test_valued_canonical_fm(case, k, opt):
    _run("fm", case, 0, k, opt)


@pytest.mark.parametrize("valued", [False, True], ids=["binary", "valued"])
@pytest.mark.parametrize("opt", GC.OPTS)
@pytest.mark.parametrize("case,Fd,k", GC.FFM_GRID)
def test_field_aware_fm(case, Fd, k, opt, valued):
    _run("ffm", case, Fd, k, opt, valued)


@pytest.mark.parametrize("opt", GC.OPTS)
def test_field_aware_fm_underflow(opt):
    _run("ffm", "underflow", 18, 4, opt)
