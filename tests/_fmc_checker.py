"""Canonical FM (fm_mode=canonical) restated in numpy: the checker of the new tests.

Every fp64 accumulation adds fp32 values (products rounded to fp32 first), so it is exact and
its order does not matter; the casts to fp32 sit where the definition puts them:
  wx_r    = fp32(sum_j w[u_j])
  S[r,f]  = fp32(sum_j v[u_j,f])
  T_r     = sum_f fp32(S[r,f]^2)          Q_r = sum_f sum_j fp32(v[u_j,f]^2)
  y2_r    = fp32(0.5 (T_r - Q_r))
  p_r     = sigmoid_ref(fp32(wx_r + y2_r)),   loss_r = fp32(p_r - label_r)
  gw[u]   = fp32(fp32(sum_occ loss) / R)
  gv[u,f] = fp32(fp32(sum_occ fp32(loss * fp32(S[r,f] - v[u,f]))) / R)
The optimizer steps and the inits are the oracle's (O.Store pull / push)."""
import numpy as np

from oracle import pyoracle as O

_sigmoid = np.vectorize(O.sigmoid, otypes=[np.float32])


def rows_of(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


class _Seg:
    """sums of fp64 rows per segment id (exact sums: the order is free)"""

    def __init__(self, seg, nseg):
        self.order = np.argsort(seg, kind="stable")
        s = seg[self.order]
        self.starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]]) if len(s) else \
            np.zeros(0, np.int64)
        self.ids = s[self.starts]
        self.nseg = nseg

    def __call__(self, vals):
        vals = np.asarray(vals)
        out = np.zeros((self.nseg,) + vals.shape[1:])
        if len(self.starts):
            out[self.ids] = np.add.reduceat(vals[self.order].astype(np.float64), self.starts,
                                            axis=0)
        return out


_FC = 16  # factors per pass (bounds the checker's memory at millions of nonzeros)


def forward(rowptr, uidx, labels, wu, vu):
    """-> loss[R], pctr[R], S[R, k] (fp32), and T, Q (fp64) for the given pulled rows"""
    rowptr = np.asarray(rowptr, np.int64)
    R, k = len(rowptr) - 1, vu.shape[1]
    by_row = _Seg(rows_of(rowptr), R)
    wx = by_row(wu[uidx]).astype(np.float32)
    S = np.zeros((R, k), np.float32)
    Q = np.zeros(R)
    for f0 in range(0, k, _FC):
        V = vu[uidx, f0:f0 + _FC]                  # fp32
        S[:, f0:f0 + _FC] = by_row(V).astype(np.float32)
        Q += by_row((V * V).astype(np.float64).sum(axis=1))
    T = (S * S).astype(np.float64).sum(axis=1)
    y2 = (0.5 * (T - Q)).astype(np.float32)
    pctr = _sigmoid(wx + y2) if R else np.zeros(0, np.float32)
    loss = pctr - np.asarray(labels, np.float32)
    return loss.astype(np.float32), pctr, S, T, Q


def gradient(rowptr, uidx, U, loss, S, vu):
    R = len(rowptr) - 1
    row = rows_of(rowptr)
    lo = loss[row]
    by_key = _Seg(np.asarray(uidx, np.int64), U)
    gw = (by_key(lo).astype(np.float32).astype(np.float64) / (1.0 * R)).astype(np.float32)
    gv = np.zeros((U, vu.shape[1]), np.float32)
    for f0 in range(0, vu.shape[1], _FC):
        term = lo[:, None] * (S[row, f0:f0 + _FC] - vu[uidx, f0:f0 + _FC])  # fp32 ops
        gv[:, f0:f0 + _FC] = (by_key(term).astype(np.float32).astype(np.float64) /
                              (1.0 * R)).astype(np.float32)
    return gw, gv


def pull(ws, vs, ukeys):
    k = vs.dim
    wu = np.asarray(ws.pull(ukeys), np.float32).reshape(len(ukeys))
    vu = np.asarray(vs.pull(ukeys), np.float32).reshape(len(ukeys), k)
    return wu, vu


def step(ws, vs, rowptr, keys, labels):
    """one canonical update of the oracle stores; -> (ukeys, wu, loss, gw) of the step"""
    rowptr = np.asarray(rowptr, np.int64)
    keys = np.asarray(keys, np.uint64)[rowptr[0]:rowptr[-1]]
    rp = rowptr - rowptr[0]
    ukeys, uidx = np.unique(keys, return_inverse=True)
    U = len(ukeys)
    if U == 0:
        return ukeys, np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)
    wu, vu = pull(ws, vs, ukeys)
    loss, _, S, _, _ = forward(rp, uidx, labels, wu, vu)
    gw, gv = gradient(rp, uidx, U, loss, S, vu)
    ws.push(ukeys, gw)
    vs.push(ukeys, gv)
    return ukeys, wu, loss, gw


def predict(ws, vs, rowptr, keys, labels):
    rowptr = np.asarray(rowptr, np.int64)
    keys = np.asarray(keys, np.uint64)[rowptr[0]:rowptr[-1]]
    rp = rowptr - rowptr[0]
    ukeys, uidx = np.unique(keys, return_inverse=True)
    if len(ukeys) == 0:
        return _sigmoid(np.zeros(len(rp) - 1, np.float32))
    wu, vu = pull(ws, vs, ukeys)
    return forward(rp, uidx, labels, wu, vu)[1]


def stores(opt, k, seed):
    """the canonical mode's two stores: w from zero, v hash-normal for FTRL and SGD alike"""
    return O.Store(opt, 1), O.Store(opt, k, O.INIT_HASHNORM, 0.0, seed)


def train_worker(ws, vs, train_path, epochs, block_bytes=2 << 20):
    """XFlow(model=1, fm_mode=canonical, core_num=1): the key-0 init push (fm_worker.cc:248-252),
    then one update per block and epoch"""
    ws.push(np.zeros(1, np.uint64), np.zeros(1, np.float32))
    vs.push(np.zeros(1, np.uint64), np.zeros(vs.dim, np.float32))
    blocks = list(O.read_blocks(train_path, block_bytes))
    for _ in range(epochs):
        for rowptr, keys, _, labels in blocks:
            step(ws, vs, rowptr, keys, labels)


def predict_file(ws, vs, test_path, block_bytes=2 << 20):
    """the test file's keys pulled first (test-time pulls insert unseen keys), then the forward"""
    labels_all, pctr_all = [], []
    blocks = list(O.read_blocks(test_path, block_bytes))
    for rowptr, keys, _, labels in blocks:
        pull(ws, vs, np.unique(np.asarray(keys, np.uint64)))
    for rowptr, keys, _, labels in blocks:
        pctr_all.append(predict(ws, vs, rowptr, keys, labels))
        labels_all.append(labels)
    return np.concatenate(labels_all), np.concatenate(pctr_all)
