"""Feature values (feature_values=on) restated in numpy: the checker of the valued tests.

x_j is the fp32 value of nonzero j, u_j its key's index, r its row, R the rows of the minibatch.
Every accumulation is an fp64 sum of fp32 values, every product is rounded to fp32 first:
  wx_r    = fp32(sum_j fp32(w[u_j] x_j))
  gw[u]   = fp32(fp32(sum_occ fp32(loss_r x_occ)) / R)
  LR:       p_r = sigmoid_ref(wx_r), loss_r = fp32(p_r - label_r)
  canonical FM, a_jf = fp32(v[u_j,f] x_j):
  S[r,f]  = fp32(sum_j a_jf)
  T_r     = sum_f fp32(S[r,f]^2)          Q_r = sum_f sum_j fp32(a_jf^2)
  y2_r    = fp32(0.5 (T_r - Q_r))
  p_r     = sigmoid_ref(fp32(wx_r + y2_r)),   loss_r = fp32(p_r - label_r)
  gv[u,f] = fp32(fp32(sum_occ fp32(fp32(loss_r x_occ) fp32(S[r,f] - a_occ,f))) / R)
With every x = 1 this is tests/_fmc_checker.py (and, for LR, the oracle's exact-sum update).
The optimizer steps and the inits are the oracle's (O.Store pull / push).

"fp64 sums of fp32 values are exact" is an argument about magnitudes, and values widen the spread
of the addends.  So every family of sums is formed twice — over the addends in ascending and in
descending position order — and every call leaves (family, sums formed, sums that differ) in the
`audit` list it is given: a test asserts that NO sum differs before it compares with the GPU."""
import numpy as np

from oracle import pyoracle as O
from tests import _fmc_checker as F

_sigmoid = F._sigmoid
rows_of = F.rows_of
_FC = 16


class _Seg2:
    """F._Seg twice: the segments' addends in ascending and in descending position order"""

    def __init__(self, seg, nseg):
        seg = np.asarray(seg, np.int64)
        self.up, self.down = F._Seg(seg, nseg), F._Seg(seg, nseg)
        o = self.up.order[::-1]
        s = seg[o]
        self.down.order = o
        self.down.starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]]) if len(s) else \
            np.zeros(0, np.int64)
        self.down.ids = s[self.down.starts]

    def __call__(self, vals, family, audit):
        # (+ 0.0: a sum starts from +0, so one over nothing but -0 addends — loss x with x = 0 and
        # a negative loss — is +0, as IEEE addition has it; reduceat hands a lone addend through)
        a, d = self.up(vals) + 0.0, self.down(vals) + 0.0
        audit.append((family, int(a.size), int(np.count_nonzero(a != d))))
        return a


def _sum_columns(M, family, audit):
    """fp64 row sums of M's columns, added left to right and right to left"""
    M = np.asarray(M, np.float64)
    a, d = np.zeros(M.shape[0]), np.zeros(M.shape[0])
    for f in range(M.shape[1]):
        a += M[:, f]
        d += M[:, M.shape[1] - 1 - f]
    audit.append((family, int(a.size), int(np.count_nonzero(a != d))))
    return a


def disagreements(audit):
    """{family: (sums formed, sums whose two orders differ)} over an audit list"""
    out = {}
    for fam, n, bad in audit:
        a, b = out.get(fam, (0, 0))
        out[fam] = (a + n, b + bad)
    return out


def assert_exact(audit):
    d = disagreements(audit)
    assert d, "nothing was summed"
    bad = {f: v for f, v in d.items() if v[1]}
    assert not bad, "sums that depend on the order of their addends (family: formed, differ): %r" \
        % bad


def _f32(a):
    return np.asarray(a, np.float32)


def forward_lr(rowptr, uidx, x, labels, wu, audit):
    rowptr = np.asarray(rowptr, np.int64)
    R = len(rowptr) - 1
    by_row = _Seg2(rows_of(rowptr), R)
    wx = by_row(_f32(wu[uidx] * x), "wx", audit).astype(np.float32)
    pctr = _sigmoid(wx) if R else np.zeros(0, np.float32)
    loss = pctr - np.asarray(labels, np.float32)
    return _f32(loss), _f32(pctr)


def forward_fm(rowptr, uidx, x, labels, wu, vu, audit):
    """-> loss[R], pctr[R], S[R, k]"""
    rowptr = np.asarray(rowptr, np.int64)
    R, k = len(rowptr) - 1, vu.shape[1]
    by_row = _Seg2(rows_of(rowptr), R)
    wx = by_row(_f32(wu[uidx] * x), "wx", audit).astype(np.float32)
    S = np.zeros((R, k), np.float32)
    Qf = np.zeros((R, k))
    for f0 in range(0, k, _FC):
        A = _f32(vu[uidx, f0:f0 + _FC] * x[:, None])
        S[:, f0:f0 + _FC] = by_row(A, "S", audit).astype(np.float32)
        Qf[:, f0:f0 + _FC] = by_row(_f32(A * A), "Q over j", audit)
    Q = _sum_columns(Qf, "Q over f", audit)
    T = _sum_columns(_f32(S * S), "T", audit)
    y2 = (0.5 * (T - Q)).astype(np.float32)
    pctr = _sigmoid(_f32(wx + y2)) if R else np.zeros(0, np.float32)
    loss = pctr - np.asarray(labels, np.float32)
    return _f32(loss), _f32(pctr), S


def _div_rows(s, R):
    return (s.astype(np.float32).astype(np.float64) / (1.0 * R)).astype(np.float32)


def gradient_w(rowptr, uidx, U, x, loss, audit):
    R = len(rowptr) - 1
    lx = _f32(loss[rows_of(rowptr)] * x)
    by_key = _Seg2(uidx, U)
    return _div_rows(by_key(lx, "gw", audit), R), lx, by_key


def gradient_fm(rowptr, uidx, U, x, loss, S, vu, audit):
    R = len(rowptr) - 1
    row = rows_of(rowptr)
    gw, lx, by_key = gradient_w(rowptr, uidx, U, x, loss, audit)
    gv = np.zeros((U, vu.shape[1]), np.float32)
    for f0 in range(0, vu.shape[1], _FC):
        A = _f32(vu[uidx, f0:f0 + _FC] * x[:, None])
        term = _f32(lx[:, None] * _f32(S[row, f0:f0 + _FC] - A))
        gv[:, f0:f0 + _FC] = _div_rows(by_key(term, "gv", audit), R)
    return gw, gv


def _slice(rowptr, keys, vals):
    rowptr = np.asarray(rowptr, np.int64)
    keys = np.asarray(keys, np.uint64)[rowptr[0]:rowptr[-1]]
    x = np.asarray(vals, np.float32)[rowptr[0]:rowptr[-1]]
    ukeys, uidx = np.unique(keys, return_inverse=True)
    return rowptr - rowptr[0], ukeys, uidx.astype(np.int64), x


_NONE = np.zeros(0, np.float32)


def lr_step(ws, rowptr, keys, vals, labels, audit):
    """one valued LR update of the oracle store; -> (ukeys, wu, loss, gw)"""
    rp, ukeys, uidx, x = _slice(rowptr, keys, vals)
    if len(ukeys) == 0:
        return ukeys, _NONE, _NONE, _NONE
    wu = _f32(ws.pull(ukeys)).reshape(len(ukeys))
    loss, _ = forward_lr(rp, uidx, x, labels, wu, audit)
    gw = gradient_w(rp, uidx, len(ukeys), x, loss, audit)[0]
    ws.push(ukeys, gw)
    return ukeys, wu, loss, gw


def lr_predict(ws, rowptr, keys, vals, labels, audit):
    rp, ukeys, uidx, x = _slice(rowptr, keys, vals)
    if len(ukeys) == 0:
        return _sigmoid(np.zeros(len(rp) - 1, np.float32))
    wu = _f32(ws.pull(ukeys)).reshape(len(ukeys))
    return forward_lr(rp, uidx, x, labels, wu, audit)[1]


def fm_step(ws, vs, rowptr, keys, vals, labels, audit):
    """one valued canonical FM update of the oracle stores; -> (ukeys, wu, loss, gw)"""
    rp, ukeys, uidx, x = _slice(rowptr, keys, vals)
    if len(ukeys) == 0:
        return ukeys, _NONE, _NONE, _NONE
    wu, vu = F.pull(ws, vs, ukeys)
    loss, _, S = forward_fm(rp, uidx, x, labels, wu, vu, audit)
    gw, gv = gradient_fm(rp, uidx, len(ukeys), x, loss, S, vu, audit)
    ws.push(ukeys, gw)
    vs.push(ukeys, gv)
    return ukeys, wu, loss, gw


def fm_predict(ws, vs, rowptr, keys, vals, labels, audit):
    rp, ukeys, uidx, x = _slice(rowptr, keys, vals)
    if len(ukeys) == 0:
        return _sigmoid(np.zeros(len(rp) - 1, np.float32))
    wu, vu = F.pull(ws, vs, ukeys)
    return forward_fm(rp, uidx, x, labels, wu, vu, audit)[1]


# ---------------------------------------------------------------- files
def file_values(path):
    """the values of a text file in token order, by splitting its lines in Python: the third
    field of every token (after the second colon, further colons included), an empty token
    repeating the row's previous value; float32(float(field)), an empty field 0"""
    out = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            if not line:
                continue
            toks = line.split(b"\t", 1)[1].split(b" ")
            if toks and toks[-1] == b"":
                toks.pop()      # a single blank before the newline is not a token
            for t in toks:
                if t == b"":
                    out.append(out[-1])
                    continue
                field = t.split(b":", 2)[2]
                out.append(np.float32(float(field.split(b":")[0] or b"0")))
    return np.asarray(out, np.float32)


def file_blocks(path, block_bytes):
    """(rowptr, keys, labels, values) per block: the oracle's blocks, the values cut by their
    nonzero counts"""
    vals = file_values(path)
    at = 0
    for rowptr, keys, _, labels in O.read_blocks(path, block_bytes):
        n = len(keys)
        yield rowptr, keys, labels, vals[at:at + n]
        at += n
    assert at == len(vals), "the file's tokens and the oracle's nonzeros differ in number"


def train_worker(model, ws, vs, train_path, epochs, audit, block_bytes=2 << 20):
    """XFlow(model, feature_values=on, core_num=1): the key-0 init push, then one update per block
    and epoch"""
    ws.push(np.zeros(1, np.uint64), np.zeros(1, np.float32))
    if model == 1:
        vs.push(np.zeros(1, np.uint64), np.zeros(vs.dim, np.float32))
    blocks = list(file_blocks(train_path, block_bytes))
    for _ in range(epochs):
        for rowptr, keys, labels, vals in blocks:
            if model == 1:
                fm_step(ws, vs, rowptr, keys, vals, labels, audit)
            else:
                lr_step(ws, rowptr, keys, vals, labels, audit)


def predict_file(model, ws, vs, test_path, audit, block_bytes):
    """block by block: a block's Pull inserts its unseen keys, then its forward"""
    labels_all, pctr_all = [], []
    for rowptr, keys, labels, vals in file_blocks(test_path, block_bytes):
        if model == 1:
            pctr_all.append(fm_predict(ws, vs, rowptr, keys, vals, labels, audit))
        else:
            pctr_all.append(lr_predict(ws, rowptr, keys, vals, labels, audit))
        labels_all.append(labels)
    return np.concatenate(labels_all), np.concatenate(pctr_all)
