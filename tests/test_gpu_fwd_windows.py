"""The forward's own row windows over a kept minibatch's key-sorted copy (xf_cells.h: nwin_f,
xf_common.h: fwd_windows) on a real MI355X.  The copy is regrouped by forward cells — forward
window = global row / W_f, not nested in the gradient's windows — and only the forward kernel and
the finalize read that geometry; no operand changes.  Every case holds the losses of 3 steps and
the table after them against the exact-sum oracle bit for bit (the scheme of
tests/test_gpu_entry_streams.py), FTRL and SGD, and reads from xf_batch_fwd_info that the forward
ran on the geometry the case forces: xf_tune("fwd_windows", n) forces n forward windows whatever
the density of the cells, 1 switches them off, 0 is the rule (tests/test_fwd_windows_cpu.py).

A forced n stays off where the copy would be what it is (n == the gradient's windows) and where
ceil(R / n) rows do not fit a window's LDS (R = 34817, n = 2): expected() says which."""
import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _cells_edges as E
from .test_gpu_entry_streams import (CAP, NKEYS, NKEYS_UNSPLIT, STEPS, mb, pool, ref_windows,
                                     reference, same, split, _opt)
from .test_gpu_fwd_blocks import CASES as FWD_CASES, ref_of as fwd_ref_of
from .test_gpu_grad_dense import aged, capacity_for, keys_of

pytestmark = pytest.mark.gpu
WIN_MAX = E.WIN_MAX


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def expected(R, nf):
    """the forward geometry a kept minibatch of R rows gets under fwd_windows = nf >= 2:
    (split, nwin_f, W_f, G_f)"""
    nwin = max(1, (R + WIN_MAX - 1) // WIN_MAX)
    on = nf >= 2 and nf != nwin and (R + nf - 1) // nf <= WIN_MAX
    n = nf if on else nwin
    return on, n, max(1, (R + n - 1) // n), 32 // n * 8


def run(raws, opt, nf, form="kept", w=1.0, settle=None, state=None, cap=1 << 15, predict=False):
    """STEPS steps under fwd_windows = nf -> losses, table, cells_info and fwd_info per step, and
    (predict) lr_predict of the first minibatch on the table the steps left + its fwd_info.
    settle: keys pulled and settled first; state: a model imported and settled first"""
    capi.tune("fwd_windows", nf)
    try:
        t = capi.Table(_opt(opt)[0], 1, capacity=cap)
        ws = capi.Workspace()
        ws.neg_weight(w)
        if state is not None:
            t.import_(*state)
            t.defrag()
        elif settle is not None:
            t.pull(settle)
            t.defrag()
        kept = [capi.LocalBatch(t, *r) for r in raws] if form == "kept" else None
        losses, infos, fwd = [], [], []
        for i in range(STEPS):
            if kept:
                b = kept[i % len(raws)]
                capi.lr_step(t, b, ws)
            else:
                b = capi.LocalBatch.update(t, ws, *raws[i % len(raws)],
                                           retain_keys=form == "one-call kept")
            losses.append(ws.fetch_loss(b.R))
            infos.append(b.cells_info())
            fwd.append(b.fwd_info())
        t.check()
        table = t.export()
        pctr = pfwd = None
        if predict:
            pctr = capi.lr_predict(t, kept[0], ws)
            pfwd = kept[0].fwd_info()
        return losses, table, infos, fwd, pctr, pfwd
    finally:
        capi.tune("fwd_windows", 0)


def against(got, ref, opt, what):
    for i, (a, e) in enumerate(zip(got[0], ref[0])):
        same(a, e, "%s: loss of step %d" % (what, i))
    m = 4 if opt == "ftrl" else 2
    for nm, a, e in zip(("keys", "w", "n", "z"), got[1][:m], ref[1][:m]):
        same(a, e, "%s: table %s" % (what, nm))


def geometry(got, R, nf, what):
    """the gradient's geometry is what it was, the forward's is expected(); the forward ran on it
    wherever the minibatch is one segment"""
    on, n, W_f, G_f = expected(R, nf)
    nwin = max(1, (R + WIN_MAX - 1) // WIN_MAX)
    used = []
    for info, f in zip(got[2], got[3]):
        assert (info["nwin"], info["W"], info["G"]) == \
            (nwin, max(1, (R + nwin - 1) // nwin), 32 // nwin * 8), (what, info)
        assert (f["split"], f["nwin_f"], f["W_f"], f["G_f"]) == (int(on), n, W_f, G_f), (what, f)
        assert f["used"] == int(on and f["copy_ready"] == 1 and info["segments"] == 1), (what, f, info)
        used.append(f["used"])
    return used


NFS = [2, 5, 8, 16]
_REF = {}


def split_stream(R, opt):
    """two minibatches of 2 R nonzeros over 5 000 keys whose row lengths come from split() (some
    rows are empty), and in which the first row of every forward window of every forced count has
    none (its nonzeros moved to the next row): once per R and optimizer, left unchanged"""
    if (R, opt) not in _REF:
        rng = np.random.RandomState(R)
        raws = []
        for _ in range(2):
            lens = split(rng, 2 * R, R)
            W_fs = [(R + nf - 1) // nf for nf in NFS]
            firsts = {row for W_f in W_fs for row in range(W_f, R - 1, W_f)}
            for row in sorted(firsts):  # (ascending: a neighbour that is a first row passes them on)
                lens[row + 1] += lens[row]
                lens[row] = 0
            raws.append(mb(rng, lens))
        _REF[(R, opt)] = (raws, reference(raws, opt))
    return _REF[(R, opt)]


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("nf", NFS)
@pytest.mark.parametrize("R", [1, 2, 7, 17, 4097, 17408, 17409, 34817])
def test_rows_and_forced_windows(R, nf, opt):
    """1 to 3 nonzeros a row (ref_windows; the rows of the 5 000-key stream from split(): some are
    empty) over 5 000 keys (three chunks, split) and over 40 000 (dense).  R < nf: forward windows
    without a row (W_f = 1); a short last window (4097 = 2 x 2049 - 1, 17409 over 5: 3482 x 5 - 1);
    R = 34817 with three gradient windows of 11606: under 8 forward windows of 4353 the boundaries
    4353 and 8706 fall inside gradient window 0, window 2 (8706 .. 13058) straddles gradient windows
    0 / 1 and window 5 (21765 .. 26117) 1 / 2; R = 17408 = 16 x 1088 = 8 x 2176 = 2 x 8704 meets no
    gradient boundary but its own end; rows without a nonzero sit on boundaries of the split()
    stream.  R = 34817 under 2 windows stays off (17409 rows do not fit) and so does R = 17409 (two
    windows are the gradient's): asserted as such."""
    on = expected(R, nf)[0]
    assert on == ((R, nf) not in ((34817, 2), (17409, 2)))
    for nkeys, seed in ((NKEYS, 0), (NKEYS_UNSPLIT, 50)):
        if nkeys == NKEYS and R >= 17:
            raws, ref = split_stream(R, opt)
            if on:  # the first row of every forward window but window 0 has no nonzero
                W_f = expected(R, nf)[2]
                lens = np.diff(raws[0][0].astype(np.int64))
                assert all(lens[v * W_f] == 0 for v in range(1, nf) if v * W_f < R - 1)
        else:
            raws, ref = ref_windows(R, opt, seed, nkeys)
        got = run(raws, opt, nf, cap=CAP[nkeys])
        what = "R=%d nf=%d %s keys=%d" % (R, nf, opt, nkeys)
        against(got, ref, opt, what)
        used = geometry(got, R, nf, what)
        # the first minibatch settles the fresh table: one segment, steps 0 and 2 run on the split
        assert got[2][0]["segments"] == 1 and (used[0], used[2]) == (int(on), int(on)), (what, used)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("nf", [2, 5])
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_forward_blocks_on_forward_cells(name, nf, opt):
    """every case of _cells_edges.fwd_cases() — block spans of 31 / 32 / 33 / 100 cells, the tag
    wrap, blocks that cross into a window whose first cells are empty, a shorter last window — as a
    kept minibatch under a forced split: the forward decodes (near) and searches (cell_of) on its
    own cell numbering, on an aged table (a wrong cell is a wrong loss); and lr_predict on the
    table the steps left"""
    c = FWD_CASES[name]
    raws, ref, pctr = fwd_ref_of(name, opt)
    got = run(raws, opt, nf, state=aged(c.M, opt), cap=capacity_for(c.M), predict=True)
    what = "%s nf=%d %s" % (name, nf, opt)
    against(got, ref, opt, what)
    on = expected(c.R, nf)[0]
    assert geometry(got, c.R, nf, what) == [int(on)] * STEPS
    same(got[4], pctr, what + ": pctr")
    assert got[5]["used"] == int(on)
    L = c.layout()
    assert all((i["nwin"], i["W"], i["nchunk"], i["segments"]) == (L["nwin"], L["W"], L["nchunk"], 1)
               for i in got[2]), got[2]


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_a_chain_of_two_segments_falls_back(opt):
    """test_gpu_entry_streams.test_a_chain_of_two_segments' shape, "one-call kept": the kept head
    has a split copy, the chain's forward reads the head's `entries` on the base geometry (all
    segments share one partial array) and says so; the oracle's results"""
    rng = np.random.RandomState(7)
    settle = pool()[:4400]
    raws = [mb(rng, rng.randint(1, 4, size=3000), 0, NKEYS) for _ in range(2)]
    got = run(raws, opt, 2, form="one-call kept", settle=settle)
    against(got, reference(raws, opt, settle=settle), opt, "chain " + opt)
    assert [i["segments"] for i in got[2]] == [2, 2, 2], got[2]
    assert [(f["split"], f["nwin_f"], f["used"]) for f in got[3]] == [(1, 2, 0)] * 3, got[3]


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("what", ["predict", "twice-in-a-row", "neg-weight-4"])
def test_other_consumers(what, opt):
    """what else reads a split copy, against the oracle and against fwd_windows = 1: lr_predict;
    the same kept minibatch stepped three times in a row (lr_step then asks for no fetch);
    neg_weight 4 in the finalize's last store.  R = 4097 over 5 forward windows of 820."""
    R, nf = 4097, 5
    rng = np.random.RandomState(41)
    n = 1 if what == "twice-in-a-row" else 2
    raws = [mb(rng, rng.randint(0, 5, size=R)) for _ in range(n)]
    w = 4.0 if what == "neg-weight-4" else 1.0
    ref = reference(raws, opt, w)
    runs = {k: run(raws, opt, k, w=w, predict=True) for k in (nf, 1)}
    for k, got in runs.items():
        against(got, ref, opt, "%s fwd_windows=%d %s" % (what, k, opt))
    assert geometry(runs[nf], R, nf, what)[0] == 1 and runs[nf][5]["used"] == 1
    assert all(f["split"] == 0 and f["used"] == 0 for f in runs[1][3]), runs[1][3]
    if what == "twice-in-a-row":
        assert [f["used"] for f in runs[nf][3]] == [1, 1, 1]
    # predict on the table the steps left (the oracle's table, bit for bit: against())
    s = O.Store(_opt(opt)[1], 1)
    s.import_(*ref[1][:4 if opt == "ftrl" else 2])
    ob = O.Batch(*raws[0])
    with O.sum_mode(1):
        pctr = ob.lr_loss(s.pull(ob.ukeys))[1]
    same(runs[nf][4], pctr, what + ": pctr on the split copy")
    same(runs[1][4], runs[nf][4], what + ": pctr, split against fwd_windows = 1")
    for a, b in zip(runs[nf][0] + list(runs[nf][1]), runs[1][0] + list(runs[1][1])):
        same(a, b, what + ": split against fwd_windows = 1")
