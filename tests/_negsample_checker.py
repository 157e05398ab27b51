"""Negative subsampling restated in numpy: the only reference of tests/test_negsample_cpu.py and
tests/test_gpu_negsample.py.

    T          = floor(float64(float32(keep)) * 2^32)
    h(ordinal) = mix64(mix64(seed ^ stream) + ordinal)            (64-bit, wrapping)
    a row is kept iff label != 0 or (h >> 32) < T
    w          = float32(1) / float32(keep)
    weighted   loss[r] = loss[r] if label[r] != 0 else float32(w * loss[r])

One apply is one minibatch: row i has ordinal first_ordinal + i, kept rows keep their order,
rowptr / labels / keys / fgid / values are compacted together.
"""
import numpy as np

from ._admit_checker import mix64

U64 = (1 << 64) - 1


def threshold(keep):
    return int(np.floor(np.float64(np.float32(keep)) * np.float64(2.0 ** 32)))


def weight(keep):
    return np.float32(1.0) / np.float32(keep)


def keep_negative(seed, stream, ordinals, keep):
    """bool per ordinal (uint64 array, wrapping): would a NEGATIVE row of this ordinal be kept"""
    ordinals = np.asarray(ordinals, dtype=np.uint64)
    base = mix64(np.array([(int(seed) ^ int(stream)) & U64], np.uint64))[0]
    with np.errstate(over="ignore"):
        h = mix64(base + ordinals)
    # (T can be 2^32: compare as Python-sized integers held in uint64)
    return (h >> np.uint64(32)) < np.uint64(threshold(keep))


def weigh(loss, labels, w):
    """the loss between a step's forward and its gradient"""
    loss = np.asarray(loss, dtype=np.float32)
    return np.where(np.asarray(labels) != 0, loss, (np.float32(w) * loss).astype(np.float32))


class Sampler:
    def __init__(self, keep, seed=0):
        self.keep, self.seed = keep, seed
        self.rows_seen = self.rows_kept = self.neg_seen = self.neg_kept = 0

    def mask(self, stream, first_ordinal, labels):
        labels = np.asarray(labels)
        with np.errstate(over="ignore"):
            ords = np.uint64(int(first_ordinal) & U64) + np.arange(len(labels), dtype=np.uint64)
        return (labels != 0) | keep_negative(self.seed, stream, ords, self.keep)

    def apply(self, stream, first_ordinal, rowptr, keys, labels, fgid=None, values=None):
        """-> (rowptr uint32, keys, labels, fgid or None, values or None) of the sampled minibatch"""
        rowptr = np.asarray(rowptr).astype(np.int64)
        lo = rowptr[0]
        rowptr = rowptr - lo
        labels = np.asarray(labels, dtype=np.int32)
        R = len(rowptr) - 1
        assert len(labels) == R
        m = self.mask(stream, first_ordinal, labels)
        lens = np.diff(rowptr)
        out_rowptr = np.concatenate([[0], np.cumsum(lens[m])]).astype(np.uint32)
        nzmask = np.repeat(m, lens)
        hi = lo + rowptr[-1]
        pick = lambda a, dt: None if a is None else np.asarray(a, dtype=dt)[lo:hi][nzmask]  # noqa: E731
        self.rows_seen += R
        self.rows_kept += int(m.sum())
        self.neg_seen += int((labels == 0).sum())
        self.neg_kept += int((m & (labels == 0)).sum())
        return (out_rowptr, pick(keys, np.uint64), labels[m], pick(fgid, np.int32),
                pick(values, np.float32))

    def stats(self):
        return self.rows_seen, self.rows_kept, self.neg_seen, self.neg_kept


# ---------------------------------------------------------------- weighted steps
# No arithmetic of their own: each mode's existing checker, cut between its forward and its
# gradient, with weigh() on the loss in between.  With w = 1 each is that checker's own step
# (tests/test_negsample_cpu.py).  The imports sit in the functions: the sampler above needs none.
def lr_step(store, rowptr, keys, labels, w):
    """binary LR, the oracle's exact-sum pieces; -> the weighted loss"""
    from oracle import pyoracle as O
    b = O.Batch(rowptr, keys, labels)
    with O.sum_mode(1):
        loss, _ = b.lr_loss(store.pull(b.ukeys))
        loss = weigh(loss, b.labels, w)
        if b.U:
            store.push(b.ukeys, b.lr_grad(loss))
    return loss


def fm_step(sw, sv, rowptr, keys, labels, w):
    """reference-form FM, the oracle's exact-sum pieces; -> the weighted loss"""
    from oracle import pyoracle as O
    b = O.Batch(rowptr, keys, labels)
    k = sv.dim
    with O.sum_mode(1):
        wu, vu = sw.pull(b.ukeys), sv.pull(b.ukeys)
        loss, _, vsum = b.fm_loss(k, wu, vu)
        loss = weigh(loss, b.labels, w)
        if b.U:
            gw, gv = b.fm_grad(k, vu, vsum, loss)
            sw.push(b.ukeys, gw)
            sv.push(b.ukeys, gv)
    return loss


def fmc_step(sw, sv, rowptr, keys, labels, w):
    """canonical FM, tests/_fmc_checker.py's pieces; -> (ukeys, wu, weighted loss, gw)"""
    from . import _fmc_checker as FC
    rowptr = np.asarray(rowptr, np.int64)
    keys = np.asarray(keys, np.uint64)[rowptr[0]:rowptr[-1]]
    rp = rowptr - rowptr[0]
    ukeys, uidx = np.unique(keys, return_inverse=True)
    if len(ukeys) == 0:
        z = np.zeros(0, np.float32)
        return ukeys, z, z, z
    wu, vu = FC.pull(sw, sv, ukeys)
    loss, _, S, _, _ = FC.forward(rp, uidx, labels, wu, vu)
    loss = weigh(loss, labels, w)
    gw, gv = FC.gradient(rp, uidx, len(ukeys), loss, S, vu)
    sw.push(ukeys, gw)
    sv.push(ukeys, gv)
    return ukeys, wu, loss, gw


def valued_lr_step(sw, rowptr, keys, vals, labels, w, audit):
    """valued LR, tests/_valued_checker.py's pieces; -> (ukeys, wu, weighted loss, gw)"""
    from . import _valued_checker as V
    rp, ukeys, uidx, x = V._slice(rowptr, keys, vals)
    if len(ukeys) == 0:
        return ukeys, V._NONE, V._NONE, V._NONE
    wu = V._f32(sw.pull(ukeys)).reshape(len(ukeys))
    loss, _ = V.forward_lr(rp, uidx, x, labels, wu, audit)
    loss = weigh(loss, labels, w)
    gw = V.gradient_w(rp, uidx, len(ukeys), x, loss, audit)[0]
    sw.push(ukeys, gw)
    return ukeys, wu, loss, gw


def ffm_step(sw, sv, F, rowptr, keys, fgid, vals, labels, w, audit):
    """field-aware FM, tests/_ffm_checker.py's pieces; -> (ukeys, wu, weighted loss, gw)"""
    from . import _ffm_checker as FF
    from . import _fmc_checker as FC
    rp, ukeys, uidx, fg, x = FF._slice(rowptr, keys, fgid, vals)
    if len(ukeys) == 0:
        return ukeys, FF._NONE, FF._NONE, FF._NONE
    wu, vu = FC.pull(sw, sv, ukeys)
    loss, _, _, pairs = FF.forward(rp, uidx, fg, x, labels, wu, vu, F, audit)
    loss = weigh(loss, labels, w)
    gw, gv, touched = FF.gradient(rp, uidx, fg, len(ukeys), x, loss, F, pairs, audit)
    sw.push(ukeys, gw)
    FF.push_touched(sv, ukeys, gv, touched, sv.dim // F)
    return ukeys, wu, loss, gw


def sharded_run(mode, opt, k, F, valued, schedule, strs, w, audit, seed=7):
    """tests/_sharded_modes_checker.run with the loss of every rank weighted between its forward
    and its gradient: the same pieces, the same order of the ranks' Pulls and Pushes.
    -> ws, vs, [held-out pctr per rank] (unweighted: predict never weights)"""
    from . import _fmc_checker as FC
    from . import _sharded_modes_checker as M
    assert mode in M.MODES and schedule in ("sequential", "stale1")
    ws, vs = M.stores(mode, opt, k, F, strs, seed)
    world = len(strs)
    outstanding = []
    for s in range(M.STEPS):
        cut = [M._slice(mode, valued, strs[r][0][s]) for r in range(world)]
        pulled = [M._pull(mode, ws, vs, c[1]) if len(c[1]) else (None, None) for c in cut]
        for p in outstanding:
            M._push(mode, ws, vs, F, *p)
        grads = []
        for (rp, ukeys, uidx, fg, x, labels), (wu, vu) in zip(cut, pulled):
            if len(ukeys) == 0:
                grads.append((ukeys, None, None, None))
                continue
            loss, _, aux = M._forward(mode, valued, F, rp, uidx, fg, x, labels, wu, vu, audit)
            loss = weigh(loss, labels, w)
            grads.append((ukeys,) + M._gradient(mode, valued, F, rp, uidx, fg, len(ukeys), x,
                                                loss, aux, vu, audit))
        if schedule == "sequential":
            for p in grads:
                M._push(mode, ws, vs, F, *p)
            outstanding = []
        else:
            outstanding = grads
    for p in outstanding:
        M._push(mode, ws, vs, F, *p)
    pctr = []
    for r in range(world):
        rp, ukeys, uidx, fg, x, labels = M._slice(mode, valued, strs[r][1])
        if len(ukeys) == 0:
            pctr.append(FC._sigmoid(np.zeros(len(rp) - 1, np.float32)))
            continue
        wu, vu = M._pull(mode, ws, vs, ukeys)
        pctr.append(M._forward(mode, valued, F, rp, uidx, fg, x, labels, wu, vu, audit)[1])
    return ws, vs, pctr


def sharded_lr_run(opt, schedule, strs, w):
    """binary LR on several ranks: the oracle's exact-sum pieces in the order
    tests/_sharded_modes_checker.py states (every rank pulls, then the pushes in rank order —
    stale1: after the next step's pulls).  strs: per rank (training (rowptr, keys, labels) list,
    held-out one).  -> the store, [held-out pctr per rank]"""
    from oracle import pyoracle as O
    store = O.Store(O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD, 1)
    outstanding = []
    with O.sum_mode(1):
        for s in range(len(strs[0][0])):
            bs = [O.Batch(*strs[r][0][s]) for r in range(len(strs))]
            pulled = [store.pull(b.ukeys) for b in bs]
            for uk, g in outstanding:
                store.push(uk, g)
            grads = []
            for b, wu in zip(bs, pulled):
                if b.U:
                    grads.append((b.ukeys, b.lr_grad(weigh(b.lr_loss(wu)[0], b.labels, w))))
            if schedule == "sequential":
                for uk, g in grads:
                    store.push(uk, g)
                outstanding = []
            else:
                outstanding = grads
        for uk, g in outstanding:
            store.push(uk, g)
        pctr = []
        for r in range(len(strs)):
            b = O.Batch(*strs[r][1])
            pctr.append(b.lr_loss(store.pull(b.ukeys))[1])
    return store, pctr
