"""Where the LR cells step's entries come from (xf_common.h: entry_streams) on a real MI355X:
the gradient's entries fetched by extra blocks of the finalize launch, and the finalize kernel's
weighted last store.  Neither changes an operand: every case holds the losses of 3 steps and the
table after them against the exact-sum oracle bit for bit (as tests/test_gpu_cells.py does), FTRL
and SGD, under entry_streams = 0 (the product: with the fetch blocks) and = 1 (the finalize
launch alone), and the two against each other.

A KEPT minibatch has the key-sorted copy (retain_keys: xf_batch_compile_local, or xf_lr_update_dev
asked to keep it): its forward reads the copy and the gradient's `entries` are fetched; a ONE-SHOT
minibatch (xf_lr_update_dev, nothing kept) has none: its forward reads `entries` itself and
nothing is fetched."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _negsample_checker as N

pytestmark = pytest.mark.gpu
NKEYS = 5000
STEPS = 3


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


NKEYS_UNSPLIT = 40000      # 1 to 3 nonzeros a row over these: no chunk of 2048 keys is split
CAP = {NKEYS: 1 << 15, NKEYS_UNSPLIT: 1 << 17}
_POOL = {}


def pool(n=NKEYS):
    if n not in _POOL:
        _POOL[n] = capi.hash_decimal_range(0, n)
    return _POOL[n]


def mb(rng, lens, lo=0, hi=NKEYS, nkeys=NKEYS):
    """a minibatch with these row lengths, keys uniform over pool(nkeys)[lo:hi], both labels
    present where there are two rows"""
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    keys = pool(nkeys)[rng.randint(lo, hi, size=int(lens.sum()))]
    labels = rng.randint(0, 2, size=len(lens)).astype(np.int32)
    if len(lens) > 1:
        labels[0], labels[1] = 0, 1
    return rowptr, keys, labels


def _opt(opt):
    return (capi.OPT_FTRL, O.OPT_FTRL) if opt == "ftrl" else (capi.OPT_SGD, O.OPT_SGD)


def reference(raws, opt, w=1.0, settle=None):
    """the oracle's losses of STEPS steps over raws (cycled) and its table after them"""
    s = O.Store(_opt(opt)[1], 1)
    if settle is not None:
        s.pull(settle)
    losses = [N.lr_step(s, *raws[i % len(raws)], np.float32(w)) for i in range(STEPS)]
    return losses, s.export()


def gpu_run(raws, opt, form, es, w=1.0, settle=None, tune=None, cap=1 << 15):
    """STEPS steps on a fresh table under entry_streams = es -> losses, table, cells_info per step,
    launches of the separate weight kernel during the steps, launches of the gradient kernels by
    kind (capi.lr_grad_launches)"""
    assert form in ("kept", "one-shot", "one-call kept")
    capi.tune("entry_streams", es)
    if tune:
        capi.tune(*tune)
    try:
        t = capi.Table(_opt(opt)[0], 1, capacity=cap)
        ws = capi.Workspace()
        ws.neg_weight(w)
        if settle is not None:
            t.pull(settle)
            t.defrag()
        kept = [capi.LocalBatch(t, *r) for r in raws] if form == "kept" else None
        losses, infos = [], []
        n0 = capi.lib().xf_weigh_negatives_launches()
        g0 = capi.lr_grad_launches()
        for i in range(STEPS):
            if kept:
                b = kept[i % len(raws)]
                capi.lr_step(t, b, ws)
            else:
                b = capi.LocalBatch.update(t, ws, *raws[i % len(raws)],
                                           retain_keys=form == "one-call kept")
            losses.append(ws.fetch_loss(b.R) if b.R else np.zeros(0, np.float32))
            infos.append(b.cells_info())
        launches = capi.lib().xf_weigh_negatives_launches() - n0
        g1 = capi.lr_grad_launches()
        t.check()
        return losses, t.export(), infos, launches, {k: g1[k] - g0[k] for k in g1}
    finally:
        capi.tune("entry_streams", 0)
        if tune:
            capi.tune(tune[0], 0)


def check(raws, opt, form, ref, w=1.0, settle=None, tune=None, kernel=None, cap=1 << 15):
    """entry_streams 0 and 1 against the oracle and against each other -> cells_info per step.
    kernel: (launches of k_lr_grad_cells, of k_lr_grad_split_finish, of k_lr_grad_dense in either
    store variant) that each run's STEPS steps must have made, from capi.lr_grad_launches"""
    got = {es: gpu_run(raws, opt, form, es, w, settle, tune, cap) for es in (0, 1)}
    for es, (losses, table, _, launches, grad) in got.items():
        dense = grad["dense_masked"] + grad["dense_full"]
        print(form, opt, tune, grad)
        if kernel is not None:
            assert (grad["cells"], grad["split_finish"], dense) == kernel, (grad, kernel)
        for i, (a, e) in enumerate(zip(losses, ref[0])):
            same(a, e, "entry_streams=%d, %s: loss of step %d" % (es, form, i))
        m = 4 if opt == "ftrl" else 2
        for nm, a, e in zip(("keys", "w", "n", "z"), table[:m], ref[1][:m]):
            same(a, e, "entry_streams=%d, %s: table %s" % (es, form, nm))
        assert launches == 0, "the LR cells step launched the separate weight kernel"
    for a, b in zip(got[0][0], got[1][0]):
        same(a, b, "loss, entry_streams 0 against 1")
    for a, b in zip(got[0][1], got[1][1]):
        same(a, b, "table, entry_streams 0 against 1")
    return got[0][2]


def split(rng, nnz, rows):
    """`rows` row lengths that add up to nnz (some rows may be empty)"""
    cuts = np.sort(rng.randint(0, nnz + 1, size=rows - 1))
    return np.diff(np.concatenate([[0], cuts, [nnz]]))


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("nnz", [0, 1, 3, 4, 5, 1023, 1024, 1025, 4097])
def test_stream_ends(nnz, opt):
    """kept minibatches whose entry stream ends around a 16-byte load (1, 3, 4, 5), a forward
    block (kBlk = 1024) and a fetch block's share (4096 entries); nnz = 0 is R = 0"""
    rng = np.random.RandomState(100 + nnz)
    raws = [mb(rng, split(rng, nnz, min(nnz, 37)) if nnz else [])]
    # (no rows: no losses, and the table stays empty)
    ref = reference(raws, opt) if nnz else ([np.zeros(0, np.float32)] * STEPS,
                                            O.Store(_opt(opt)[1], 1).export())
    info = check(raws, opt, "kept", ref)
    assert nnz == 0 or info[0]["nwin"] == 1


_REF = {}


def ref_windows(R, opt, seed=0, nkeys=NKEYS):
    """computed once per shape and optimizer, shared by the forms, left unchanged"""
    if (R, opt, seed, nkeys) not in _REF:
        rng = np.random.RandomState(R + seed)
        raws = [mb(rng, rng.randint(1, 4, size=R), 0, nkeys, nkeys) for _ in range(2)]
        _REF[(R, opt, seed, nkeys)] = (raws, reference(raws, opt))
    return _REF[(R, opt, seed, nkeys)]


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("form", ["kept", "one-shot"])
@pytest.mark.parametrize("R", [17408, 17409, 34817])
def test_windows(R, form, opt):
    """one, two and three row windows (kWinMax = 17408; the rows are dealt out evenly: 17409 rows
    are windows of 8705 and 8704), 1-3 nonzeros per row over 5 000 keys; kept: the forward over
    the key-sorted copy and the fetch; one-shot: the forward over `entries`, no fetch.
    Over 5 000 keys (three chunks) two or three chunks of every minibatch are split, which sends
    it to k_lr_grad_cells and the finish kernel; the same rows over 40 000 keys split none and run
    k_lr_grad_dense behind the fetch — both asserted from the launch counters
    (tests/test_cells_edges_cpu.py counts the chunks of both)"""
    for nkeys, seed in ((NKEYS, 0), (NKEYS_UNSPLIT, 50)):
        raws, ref = ref_windows(R, opt, seed, nkeys)
        # three steps over two minibatches; the second has a segment of its own over the keys the
        # first did not hold (an arrival segment, never split: dense) — unless the first held them
        # all: 34817 rows draw every one of the 5 000 keys
        new = len(np.setdiff1d(raws[1][1], raws[0][1])) > 0
        assert new == (nkeys == NKEYS_UNSPLIT or R < 34817)
        kernel = (3, 3, int(new)) if nkeys == NKEYS else (0, 0, 3 + int(new))
        info = check(raws, opt, form, ref, kernel=kernel, cap=CAP[nkeys])
        assert info[-1]["nwin"] == (R + 17407) // 17408
        assert info[-1]["G"] == {1: 256, 2: 128, 3: 80}[info[-1]["nwin"]]
        assert all((i["nsplit_chunks"] > 0) == (nkeys == NKEYS) for i in info), info


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_the_general_gradient_kernel(opt):
    """lr_gradient = 1: the one-source k_lr_grad_cells behind the fetch where the dense kernel
    would run — on the stream over 40 000 keys, which has no split chunk (test_windows: it runs
    dense without the knob), and on the one over 5 000, which goes to k_lr_grad_cells anyway"""
    for nkeys, seed in ((NKEYS_UNSPLIT, 50), (NKEYS, 0)):
        raws, ref = ref_windows(17409, opt, seed, nkeys)
        # (three steps and the second minibatch's arrival segment, all through the general kernel)
        info = check(raws, opt, "kept", ref, tune=("lr_gradient", 1),
                     kernel=(4, 3 if nkeys == NKEYS else 0, 0), cap=CAP[nkeys])
        assert all((i["nsplit_chunks"] == 0) == (nkeys == NKEYS_UNSPLIT) for i in info), info


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("form", ["one-shot", "one-call kept"])
def test_a_chain_of_two_segments(form, opt):
    """xf_lr_update_dev on a settled table, a minibatch in which a few hundred keys are new: the
    forward runs again over a second segment of cells; only the first segment's entries are
    fetched (kept), and once: not again by the second forward call"""
    rng = np.random.RandomState(7)
    settle = pool()[:4400]
    raws = [mb(rng, rng.randint(1, 4, size=3000), 0, NKEYS) for _ in range(2)]
    new = np.setdiff1d(np.concatenate([r[1] for r in raws]), settle)
    assert 200 < len(new) < 600, len(new)
    info = check(raws, opt, form, reference(raws, opt, settle=settle), settle=settle)
    assert [i["segments"] for i in info] == [2, 2, 2], info


def _g_of(R):
    return 32 // ((R + 17407) // 17408) * 8


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("R", [1, 15, 16, 17, 63, 65, 69633, 87041])
def test_finalize_rows_and_groups(R, opt):
    """the finalize kernel through the step: rows around a wavefront's 16 (four lanes per row),
    and every G = workgroups per window a shape reaches — 256 (one window), 128 (two), 80 (three)
    in test_windows, 48 (five windows: R = 69633) and 40 (six: R = 87041) here, i.e. 64, 32, 20,
    12 and 10 loads per lane.  Every reachable G is a multiple of 8 (cells_alloc): G that is no
    multiple of 4 is test_finalize_any_group_count's."""
    raws, ref = ref_windows(R, opt, seed=1)
    info = check(raws, opt, "kept", ref)
    assert info[0]["G"] == _g_of(R)


@pytest.mark.parametrize("G", [1, 2, 3, 5, 7, 41, 42, 43, 79, 80, 83])
def test_finalize_any_group_count(G):
    """k_lr_finalize_cells on partial sums made here (xf_cells_finalize_rows): G that is no
    multiple of 4 (1, 2, 3, 5, 7, 41, 42, 43, 79, 83) — no shape reaches one through the forward —
    around the lane's unrolled loop (16 workgroups a trip), R in {1, 15, 16, 17, 63, 65}, a last
    window that is not full, weights 1 and 4.  The partial sums are multiples of 2^-6 below 2^10:
    their fp64 sums are exact in any order, so the reference is fp32(sum) through the oracle's
    sigmoid and the comparison is bit for bit."""
    import torch
    L = capi.lib()
    rng = np.random.RandomState(G)
    for R in (1, 15, 16, 17, 63, 65):
        W = max(1, (R + 1) // 2) if R > 16 else R      # two windows above 16 rows
        nwin = (R + W - 1) // W
        part = (rng.randint(-300, 301, size=(nwin, G, W)) / 64.0).astype(np.float64)
        labels = rng.randint(0, 2, size=R).astype(np.int32)
        rows = part.sum(axis=1).reshape(-1)[:R].astype(np.float32)
        pr = np.array([O.sigmoid(float(x)) for x in rows], np.float32)
        d_part = torch.from_numpy(part.reshape(-1)).cuda()
        d_lab = torch.from_numpy(labels).cuda()
        for w in (1.0, 4.0):
            d_loss = torch.full((R,), 7.0, dtype=torch.float32, device="cuda")
            d_pctr = torch.full((R,), 7.0, dtype=torch.float32, device="cuda")
            capi.check(L.xf_cells_finalize_rows(d_part.data_ptr(), d_lab.data_ptr(), R, W, G,
                                                C.c_float(w), d_loss.data_ptr(),
                                                d_pctr.data_ptr(), None))
            capi.stream_sync()
            torch.cuda.synchronize()
            same(d_pctr.cpu().numpy(), pr, "pctr, R=%d G=%d w=%g" % (R, G, w))
            same(d_loss.cpu().numpy(), N.weigh(pr - labels.astype(np.float32), labels, w),
                 "loss, R=%d G=%d w=%g" % (R, G, w))


@pytest.mark.parametrize("form", ["kept", "one-shot"])
@pytest.mark.parametrize("w", [1.0, 4.0])
def test_the_weight_rides_in_the_finalize(w, form):
    """losses and table equal tests/_negsample_checker.py's weighted step; nothing is launched
    between forward and gradient (xf_weigh_negatives_launches stays where it was: check());
    predict's pctr is the same bits under both weights"""
    rng = np.random.RandomState(31)
    raws = [mb(rng, rng.randint(0, 9, size=700)) for _ in range(2)]
    assert all((r[2] == 0).any() and (r[2] != 0).any() for r in raws)
    for opt in ("ftrl", "sgd"):
        check(raws, opt, form, reference(raws, opt, w), w)
    # predict never weights: the same table scored under both weights
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 15)
    ws = capi.Workspace()
    b = capi.LocalBatch(t, *raws[0])
    capi.lr_step(t, b, ws)
    pctr = []
    for ww in (1.0, 4.0):
        ws.neg_weight(ww)
        pctr.append(capi.lr_predict(t, b, ws))
    same(pctr[0], pctr[1], "pctr under w = 1 and w = 4")


def test_the_launch_counter_counts():
    """the counter test_the_weight_rides_in_the_finalize relies on moves when the separate kernel
    is launched: a weighted reference-form FM step still launches it"""
    rng = np.random.RandomState(3)
    raw = mb(rng, rng.randint(1, 6, size=200))
    tw = capi.Table(capi.OPT_SGD, 1, capacity=1 << 14)
    tv = capi.Table(capi.OPT_SGD, 4, capi.INIT_CONST, 0.001, capacity=1 << 14)
    ws = capi.Workspace()
    ws.neg_weight(4.0)
    n0 = capi.lib().xf_weigh_negatives_launches()
    capi.fm_step(tw, tv, capi.Batch(*raw).upload(), ws)
    tw.check()
    assert capi.lib().xf_weigh_negatives_launches() == n0 + 1
