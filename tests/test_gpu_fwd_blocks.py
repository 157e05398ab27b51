"""How the LR forward finds an entry's cell (fwd_process: xf_cells_fwd.hip, and its copy in
xf_cells_valued.hip), on a real MI355X: a block of 1024 entries that spans at most 32 cells
decodes the cell from the 5 chunk-number bits the entry carries, a wider one searches cellptr.
The minibatches are placed by state row (tests/_cells_edges.py: fwd_cases; the CPU test holds
their spans to the model): blocks of exactly 31, 32, 33 and 100 cells, a near block whose tag wraps
past 32, blocks that cross from one row window into the next with the next window's first cells
empty or filled, a shorter last window inside a shared block.  The table starts many steps old (a
weight of its own per key: a wrong cell is a wrong loss).  Kept and one-shot minibatches; the
losses of three steps, the table and lr_predict against the exact-sum oracle bit for bit; the two
sides of the 32 / 33 boundary again on valued cells against tests/_valued_checker.py."""
import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _cells_edges as E
from . import _valued_cases as VC
from . import _valued_checker as V
from .test_gpu_entry_streams import same
from .test_gpu_grad_dense import (against, aged, capacity_for, gpu_run, keys_of, launched, reference,
                                  _opt)

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in E.fwd_cases()}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


_REF = {}


def ref_of(name, opt):
    """once per case and optimizer, left unchanged: the minibatch, the oracle's losses and table,
    and its predictions on the table after the steps"""
    if (name, opt) not in _REF:
        c = CASES[name]
        settle = keys_of(c.M)
        raws = [c.raw(settle)]
        ref = reference(raws, opt, settle, state=aged(c.M, opt))
        s = O.Store(_opt(opt)[1], 1)
        s.import_(*ref[1][:4 if opt == "ftrl" else 2])
        ob = O.Batch(*raws[0])
        with O.sum_mode(1):
            pctr = ob.lr_loss(s.pull(ob.ukeys))[1]
        _REF[(name, opt)] = (raws, ref, pctr)
    return _REF[(name, opt)]


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("form", ["kept", "one-shot"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_blocks(name, form, opt):
    c = CASES[name]
    raws, ref, pctr = ref_of(name, opt)
    settle = keys_of(c.M)
    got = gpu_run(raws, opt, settle, form, state=aged(c.M, opt))
    against(got, ref, opt, "%s, %s, %s" % (name, opt, form))
    L = c.layout()
    for info in got[2]:
        assert (info["nwin"], info["W"], info["nchunk"], info["segments"]) == \
            (L["nwin"], L["W"], L["nchunk"], 1), info
    launched(got[3], c.kernel)
    # predict on the table the steps left (the forward alone, both forms of the minibatch)
    t = capi.Table(_opt(opt)[0], 1, capacity=capacity_for(c.M))
    t.import_(*ref[1][:4 if opt == "ftrl" else 2])
    t.defrag()
    ws = capi.Workspace()
    b = capi.LocalBatch(t, *raws[0], retain_keys=form == "kept")
    assert b.cells_info()["nchunk"] == L["nchunk"]
    same(capi.lr_predict(t, b, ws), pctr, "%s: pctr" % name)


# ------------------------------------------------------------------------- valued cells
@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("name", ["fwd-span-32", "fwd-span-33"])
def test_forward_blocks_on_valued_cells(name, opt):
    """xf_cells_valued.hip's copy of fwd_process either side of the boundary: an aged table
    (old_state over every key, settled: key r owns row r), two steps and the predictions against
    the numpy checker, whose sums are asserted exact first"""
    c = CASES[name]
    settle = keys_of(c.M)
    state = VC.old_state(settle, opt, 1, "w")
    sw = O.Store(_opt(opt)[1], 1)
    sw.import_(*state)
    tw = capi.Table(_opt(opt)[0], 1, capacity=capacity_for(c.M))
    tw.import_(*state)
    tw.defrag()
    ws = capi.Workspace()
    audit = []
    rowptr, keys, vals, labels = c.raw_valued(settle, VC._values)
    b = capi.LocalBatch(tw, rowptr, keys, labels, values=vals)
    info = b.cells_info()
    # (the valued build lays its cells over the table's whole row capacity: more chunks than the
    # keys fill, the same chunk numbers — with one window the cells are numbered as in the model)
    assert info["nchunk"] >= c.layout()["nchunk"] and (info["nwin"], info["segments"]) == (1, 1), \
        info
    for i in range(2):
        loss = V.lr_step(sw, rowptr, keys, vals, labels, audit)[2]
        V.assert_exact(audit)
        capi.lr_step(tw, b, ws)
        same(ws.fetch_loss(b.R), loss, "%s: valued loss of step %d" % (name, i))
    m = 4 if opt == "ftrl" else 2
    for a, e in zip(tw.export()[:m], sw.export()[:m]):
        same(a, e, "%s: valued table" % name)
    pctr = V.lr_predict(sw, rowptr, keys, vals, labels, audit)
    V.assert_exact(audit)
    same(capi.lr_predict(tw, b, ws), pctr, "%s: valued pctr" % name)
