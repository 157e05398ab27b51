"""Valued LR on the cell kernels, on a real MI355X: the local valued build
(xf_batch_compile_local_valued: raw keys -> state rows -> cells that carry a value per nonzero)
and the valued forward and gradient + Push kernels over them (xf_cells_valued.hip) against the
numpy checker of tests/_valued_checker.py — bit for bit, after the checker alone has shown that
every one of its sums is exact on these inputs (tests/test_valued_cells_cpu.py) —, against the
generic valued path, against the binary local path when every value is 1, on inputs in general
position under the interval rule, at the edges of the cells, across a defrag, the refusals, and
the one-rank trainer's routing between the two builds."""
import numpy as np
import pytest

from xflow_amd import capi

from . import _general_cases as GC
from . import _general_checker as G
from . import _interval as I
from . import _valued_cells_cases as Cs
from . import _valued_checker as V
from . import test_gpu_general_position as GP     # one_of, table_is (the module, not its tests)

pytestmark = pytest.mark.gpu


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


def same_table(t, s, what="table"):
    """keys and weights, and FTRL's (n, z)"""
    m = 4 if t.opt == capi.OPT_FTRL else 2
    for a, e in zip(t.export()[:m], s.export()[:m]):
        same(a, e, what)


def _go(opt):
    return capi.OPT_FTRL if opt == "ftrl" else capi.OPT_SGD


def table_for(opt, mbs, aged=True, cap=1 << 16):
    tw = capi.Table(_go(opt), 1, capacity=cap)
    if aged:
        tw.import_(*Cs.old_state(Cs.stream_keys(mbs), opt, 1, "w"))
    return tw


def local(tw, mb, **kw):
    rowptr, keys, vals, labels = mb
    return capi.LocalBatch(tw, rowptr, keys, labels, values=vals, **kw)


def _steps(mbs, opt, aged=True, cap=1 << 16, look=None):
    """a stream on the local valued path against the checker: the loss of every step, the table
    and the predictions after the stream, a replay of the last minibatch.  look(i, batch, table):
    a test's own assertions on minibatch i.  -> the last minibatch"""
    audit = []
    losses, sw, pctr = Cs.run_checker(opt, mbs, aged, audit)
    V.assert_exact(audit)            # every sum, before the GPU is looked at
    tw = table_for(opt, mbs, aged, cap)
    ws = capi.Workspace()
    b = None
    for i, (mb, loss) in enumerate(zip(mbs, losses)):
        b = local(tw, mb)
        if look:
            look(i, b, tw)
        assert b.cells_info()["segments"] == 1
        capi.lr_step(tw, b, ws)
        same(ws.fetch_loss(b.R), loss, "step %d loss" % i)
    same_table(tw, sw)
    same(capi.lr_predict(tw, b, ws), pctr, "pctr")
    # a replay of the last minibatch is the checker's next step
    rowptr, keys, vals, labels = mbs[-1]
    capi.lr_step(tw, b, ws)
    loss = Cs.expected_loss(V.lr_step(sw, rowptr, keys, vals, labels, audit)[2], labels)
    V.assert_exact(audit)
    same(ws.fetch_loss(b.R), loss, "replay loss")
    same_table(tw, sw, "table after the replay")
    return b


# ------------------------------------------------------- 1. steps against the checker
@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("case", Cs.CASES)
def test_local_valued_steps_equal_the_checker(case, opt):
    _steps(Cs.stream(case), opt)


# ------------------------------------------------------- 2. equal to the generic valued path
@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("case", Cs.CASES)
def test_equal_to_the_generic_valued_path(case, opt):
    mbs = Cs.stream(case)
    ta, tb = table_for(opt, mbs), table_for(opt, mbs)
    wa, wb = capi.Workspace(), capi.Workspace()
    for i, mb in enumerate(mbs):
        rowptr, keys, vals, labels = mb
        ga = capi.Batch(rowptr, keys, labels, on_gpu=True, values=vals)
        lb = local(tb, mb)
        capi.lr_step(ta, ga, wa)
        capi.lr_step(tb, lb, wb)
        same(wb.fetch_loss(lb.R), wa.fetch_loss(ga.R), "step %d loss" % i)
        for a, e in zip(tb.export(), ta.export()):
            same(a, e, "step %d tables" % i)
    same(capi.lr_predict(tb, lb, wb), capi.lr_predict(ta, ga, wa), "pctr")


# ------------------------------------------------------- 3. all values 1: the binary local path
@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("case", ["ragged", "zipf_chunks"])
def test_all_values_one_is_the_binary_local_path(case, opt):
    """fresh tables (zero init, keys inserted by the builds)"""
    ta, tb = capi.Table(_go(opt), 1, capacity=1 << 16), capi.Table(_go(opt), 1, capacity=1 << 16)
    wa, wb = capi.Workspace(), capi.Workspace()
    for rowptr, keys, vals, labels in Cs.stream(case) * 2:
        va = capi.LocalBatch(ta, rowptr, keys, labels, values=np.ones_like(vals))
        bb = capi.LocalBatch(tb, rowptr, keys, labels)
        capi.lr_step(ta, va, wa)
        capi.lr_step(tb, bb, wb)
        same(wa.fetch_loss(va.R), wb.fetch_loss(bb.R), "loss")
        for a, e in zip(ta.export(), tb.export()):
            same(a, e, "tables")
    same(capi.lr_predict(ta, va, wa), capi.lr_predict(tb, bb, wb), "pctr")


# ------------------------------------------------------- 4. general position
@pytest.mark.parametrize("opt", GC.OPTS)
@pytest.mark.parametrize("case", GC.LR_CASES + ("underflow",))
def test_general_position(case, opt):
    """the flow of tests/test_gpu_general_position.py's _run on the local valued path (a cells
    step forms neither the pulled weights nor the per-key gradients): the loss one of the
    candidates, the table one candidate's from the GPU's own loss, the predictions likewise; at
    most 2 % of any family open"""
    mbs = GC.gpu_stream("lr", case, 0)
    judge = I.Judge()
    sw, _ = GC.stores("lr", opt, 0, 1, GC.init_seed(case))
    run = G.Run("lr", sw, None, judge, 0)
    tw = capi.Table(_go(opt), 1, capacity=1 << 16)
    ws = capi.Workspace()
    sgd = opt == "sgd"
    b = None
    for i, mb in enumerate(mbs):
        rowptr, keys, _, vals, labels = mb
        b = capi.LocalBatch(tw, rowptr, keys, labels, values=vals)
        _, _, loss_c = run.begin(mb)
        capi.lr_step(tw, b, ws)
        g_loss = ws.fetch_loss(b.R)
        GP.one_of(g_loss, loss_c, "step %d loss" % i)
        _, ew, _ = run.finish(g_loss)                   # the gradient of the GPU's own loss
        xw = GP.table_is(tw, ew, "step %d w table" % i)
        run.adopt(xw[:2] if sgd else xw, None)          # an open sum does not compound
    GP.one_of(capi.lr_predict(tw, b, ws), run.predict(mbs[-1]), "pctr")
    print(judge.format("lr cells %s %s" % (case, opt)))
    judge.assert_cap()


# ------------------------------------------------------- 5. cell edges
@pytest.mark.parametrize("opt", Cs.OPTS)
@pytest.mark.parametrize("name", Cs.EDGES)
def test_cell_edges(name, opt):
    mbs, aged, cap = Cs.edge(name)
    seen = []

    def look(i, b, tw):
        info = b.cells_info()
        rowptr, keys, vals, labels = mbs[i]
        if name == "two_windows":
            assert b.R == Cs.WIN_MAX + 100 and info["nwin"] >= 2, info
        elif name == "split_chunk":
            assert info["nchunk"] >= 3 and info["nsplit_chunks"] >= 1, info
        elif name == "below_blk":
            assert 0 < b.NNZ < Cs.BLK
        elif name == "blk_plus_one":
            assert b.NNZ > Cs.BLK and b.NNZ % Cs.BLK == 1
        elif name == "empty" and i == 1:
            assert (b.R, b.NNZ) == (0, 0)
        elif name == "empty_rows" and i == 1:
            assert (b.R, b.NNZ) == (3, 0)
        elif name == "twice_in_row":
            a = int(rowptr[1])
            assert keys[a] == keys[a + 2] and vals[a] != vals[a + 2]
        elif name == "fresh_grow":
            distinct = len(np.unique(keys))
            assert distinct < b.NNZ // 2 and distinct * 10 > cap * 6    # duplicates; must grow
            assert tw.capacity > cap and len(tw) == distinct
        seen.append(i)

    _steps(mbs, opt, aged, cap, look)
    assert seen == list(range(len(mbs)))


# ------------------------------------------------------- 6. defrag
@pytest.mark.parametrize("opt", Cs.OPTS)
def test_defrag_between_two_steps(opt):
    mbs = [Cs.stream("ragged")[0]] * 2                  # one minibatch, stepped twice
    audit = []
    losses, sw, pctr = Cs.run_checker(opt, mbs, True, audit)
    V.assert_exact(audit)
    tw = table_for(opt, mbs)
    ws = capi.Workspace()
    b = local(tw, mbs[0], retain_keys=True)
    capi.lr_step(tw, b, ws)
    same(ws.fetch_loss(b.R), losses[0], "loss before the defrag")
    tw.defrag()
    assert tw.defrag_path != capi.DEFRAG_NONE         # the rows were renumbered
    capi.lr_step(tw, b, ws)                             # rebuilt from the retained keys and values
    assert b.cells_info()["segments"] == 1
    same(ws.fetch_loss(b.R), losses[1], "loss after the defrag")
    same_table(tw, sw)
    same(capi.lr_predict(tw, b, ws), pctr, "pctr")
    # without the raw arrays the minibatch cannot follow the renumbering, and says so
    tw = table_for(opt, mbs)
    b = local(tw, mbs[0], retain_keys=False)
    capi.lr_step(tw, b, ws)
    tw.defrag()
    with pytest.raises(capi.XFError, match="did not keep its keys"):
        capi.lr_step(tw, b, ws)


# ------------------------------------------------------- 7. refusals
def test_refusals():
    """refused by the step itself, before any Pull: the minibatch (compiled against one table —
    the build is what enters its keys there — and keeping its keys) meets a second, empty table,
    which stays empty"""
    mb = Cs.stream("ragged")[0]
    home = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 14)
    b = local(home, mb, retain_keys=True)
    tw = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 14)
    tv = capi.Table(capi.OPT_FTRL, 8, capi.INIT_HASHNORM, 0.0, seed=7, capacity=1 << 14)
    ws = capi.Workspace()
    ws.parity("reference_order")
    with pytest.raises(capi.XFError, match=r"feature_values.*parity"):
        capi.lr_step(tw, b, ws)
    with pytest.raises(capi.XFError, match=r"feature_values.*parity"):
        capi.lr_predict(tw, b, ws)
    ws = capi.Workspace(capture=True)
    with pytest.raises(capi.XFError, match=r"feature_values.*xf_workspace_capture"):
        capi.lr_step(tw, b, ws)
    for mode in ("reference", "canonical"):
        ws = capi.Workspace()
        ws.fm_mode(mode)
        with pytest.raises(capi.XFError, match=r"xf_fm_step.*local minibatch with feature values"):
            capi.fm_step(tw, tv, b, ws)
        with pytest.raises(capi.XFError,
                           match=r"xf_fm_predict.*local minibatch with feature values"):
            capi.fm_predict(tw, tv, b, ws)
    assert len(tw) == 0 and len(tv) == 0
    for bad in (3, -1, 0.5):
        with pytest.raises(capi.XFError, match="valued_lr"):
            capi.tune("valued_lr", bad)
    assert len(tw) == 0


# ------------------------------------------------------- 8. the one-rank trainer's routing
@pytest.mark.parametrize("opt", Cs.OPTS)
def test_trainer_routing(opt):
    mbs = Cs.stream("zipf_heavy", seed=3)
    got = {}
    try:
        for sw in (1, 2):
            capi.tune("valued_lr", sw)
            st = capi.Sharded(model="lr", optimizer=opt, capacity=1 << 16, seed=7)
            st.w.import_(*Cs.old_state(Cs.stream_keys(mbs), opt, 1, "w"))
            for rowptr, keys, vals, labels in mbs:
                b = st.compile(rowptr, keys, labels, values=vals)
                if sw == 2:     # the local build: cells over the table's rows, before any step
                    assert b.local_cells_info()["segments"] == 1 and b.U == 0
                else:           # the generic build: a key list, no cells
                    assert b.U > 0
                    with pytest.raises(capi.XFError, match="no cells"):
                        b.local_cells_info()
                st.step(b)
                st.check()
            got[sw] = (st.predict(b), st.w.export())
    finally:
        capi.tune("valued_lr", 0)
    same(got[2][0], got[1][0], "pctr")
    for a, e in zip(got[2][1], got[1][1]):
        same(a, e, "tables")
