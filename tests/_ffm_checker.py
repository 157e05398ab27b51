"""Field-aware FM (fm_mode=field_aware) restated in numpy: the checker of the field-aware tests.

Nonzero j of row r: key index u_j, field g_j (its fgid), x_j (1 for a binary minibatch); the v
rows are F k wide, coordinate (h, f) at h k + f; R the rows of the minibatch.  Every accumulation
is an fp64 sum of fp32 values, every product is rounded to fp32 first:
  a_j[h,f]  = fp32(v[u_j,h,f] x_j)
  wx_r      = fp32(sum_j fp32(w[u_j] x_j))
  y2_r      = fp32(sum_{i<j in row r} sum_f fp32(a_i[g_j,f] a_j[g_i,f]))     (pairs of POSITIONS)
  p_r       = sigmoid_ref(fp32(wx_r + y2_r)),   loss_r = fp32(p_r - label_r)
  lx_i      = fp32(loss_r x_i)
  gw[u]     = fp32(fp32(sum_occ lx) / R)
  gv[u,h,f] = fp32(fp32(sum_{occ i of u} sum_{j in row(i), j != i, g_j = h} fp32(lx_i a_j[g_i,f])) / R)
(u, h) is TOUCHED when that double sum has an addend at all; only touched coordinates of v are
stepped, the others keep (w, n, z) bit for bit.  A touched coordinate whose sum is 0 is stepped.
The optimizer steps and the inits are the oracle's (O.Store); the touched rule is laid over
Store.push with Store.export / import_.

Every family of sums is formed over its addends in ascending and in descending order and leaves
(family, sums formed, sums that differ) in `audit`, as tests/_valued_checker.py does: a test
asserts that NO sum differs (assert_exact) before it compares with the GPU."""
import numpy as np

from oracle import pyoracle as O
from tests import _fmc_checker as FC
from tests import _valued_checker as V

_sigmoid = FC._sigmoid
rows_of = FC.rows_of
_Seg2 = V._Seg2
_div_rows = V._div_rows
assert_exact = V.assert_exact
disagreements = V.disagreements
_f32 = V._f32
_NONE = np.zeros(0, np.float32)
_TRIU = {}


def pairs_of(rowptr):
    """(i, j, row) of every pair of positions i < j of one row, over all rows"""
    rowptr = np.asarray(rowptr, np.int64)
    pi, pj, pr = [], [], []
    for r in range(len(rowptr) - 1):
        n = int(rowptr[r + 1] - rowptr[r])
        if n < 2:
            continue
        if n not in _TRIU:
            _TRIU[n] = np.triu_indices(n, 1)
        a, b = _TRIU[n]
        pi.append(a + rowptr[r])
        pj.append(b + rowptr[r])
        pr.append(np.full(len(a), r, np.int64))
    if not pi:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(pi), np.concatenate(pj), np.concatenate(pr)


def _factors(uidx, fg, x, vu, F, pi, pj):
    """a_i[g_j, :] and a_j[g_i, :] of every pair, fp32 [P, k]"""
    v3 = vu.reshape(vu.shape[0], F, -1)
    a_ij = _f32(v3[uidx[pi], fg[pj], :] * x[pi][:, None])
    a_ji = _f32(v3[uidx[pj], fg[pi], :] * x[pj][:, None])
    return a_ij, a_ji


def forward(rowptr, uidx, fg, x, labels, wu, vu, F, audit):
    """-> loss[R], pctr[R], y2[R] (fp32) and the pair list with its factors (for the gradient)"""
    rowptr = np.asarray(rowptr, np.int64)
    R, k = len(rowptr) - 1, vu.shape[1] // F
    by_row = _Seg2(rows_of(rowptr), R)
    wx = by_row(_f32(wu[uidx] * x), "wx", audit).astype(np.float32)
    pi, pj, pr = pairs_of(rowptr)
    a_ij, a_ji = _factors(uidx, fg, x, vu, F, pi, pj)
    term = _f32(a_ij * a_ji).reshape(-1)                     # pair-major, the factor inside
    y2 = _Seg2(np.repeat(pr, k), R)(term, "y2", audit).astype(np.float32)
    pctr = _sigmoid(_f32(wx + y2)) if R else np.zeros(0, np.float32)
    loss = _f32(pctr - np.asarray(labels, np.float32))
    return loss, _f32(pctr), y2, (pi, pj, a_ij, a_ji)


def forward64(rowptr, uidx, fg, x, wu, vu, F):
    """wx + y2 per row in fp64 throughout (no fp32 rounding): the CPU tests' comparisons"""
    rowptr = np.asarray(rowptr, np.int64)
    R = len(rowptr) - 1
    v3 = np.asarray(vu, np.float64).reshape(vu.shape[0], F, -1)
    x = np.asarray(x, np.float64)
    pi, pj, pr = pairs_of(rowptr)
    t = ((v3[uidx[pi], fg[pj], :] * x[pi][:, None]) * (v3[uidx[pj], fg[pi], :] * x[pj][:, None]))
    y2 = np.bincount(pr, t.sum(axis=1), R) if len(pr) else np.zeros(R)
    wx = np.bincount(rows_of(rowptr), np.asarray(wu, np.float64)[uidx] * x, R)
    return wx, y2


def gradient(rowptr, uidx, fg, U, x, loss, F, pairs, audit):
    """-> gw[U], gv[U, F k], touched[U, F] (bool)"""
    R = len(rowptr) - 1
    gw, lx, _ = V.gradient_w(rowptr, uidx, U, x, loss, audit)
    pi, pj, a_ij, a_ji = pairs
    k = a_ij.shape[1]
    # occurrence i gives fp32(lx_i a_j[g_i,:]) to (u_i, g_j); occurrence j the mirror image
    seg = np.r_[uidx[pi] * F + fg[pj], uidx[pj] * F + fg[pi]]
    term = np.concatenate([_f32(lx[pi][:, None] * a_ji), _f32(lx[pj][:, None] * a_ij)])
    touched = np.bincount(seg, minlength=U * F).reshape(U, F) > 0
    if len(seg):
        s = _Seg2(seg, U * F)(term, "gv", audit)
    else:
        s = np.zeros((U * F, k))
    return gw, _div_rows(s, R).reshape(U, F * k), touched


def push_touched(vs, ukeys, gv, touched, k):
    """Store.push on the touched coordinates only: every coordinate of the keys is pushed, then
    the untouched ones get the (w, n, z) back that an export taken before the push holds"""
    mask = np.repeat(touched, k, axis=1)
    kall, w0, n0, z0 = vs.export()
    at = np.searchsorted(kall, ukeys)
    assert np.array_equal(kall[at], ukeys), "the keys were pulled: they are in the store"
    old = [a.reshape(len(kall), -1)[at] for a in (w0, n0, z0)]
    vs.push(ukeys, np.where(mask, gv, np.float32(0.0)))
    kall1, w1, n1, z1 = vs.export()
    assert np.array_equal(kall1, kall)
    new = [a.reshape(len(kall), -1)[at] for a in (w1, n1, z1)]
    vs.import_(ukeys, *[np.where(mask, b, a) for a, b in zip(old, new)])


def _slice(rowptr, keys, fgid, vals):
    rowptr = np.asarray(rowptr, np.int64)
    a, b = rowptr[0], rowptr[-1]
    keys = np.asarray(keys, np.uint64)[a:b]
    fg = np.asarray(fgid, np.int64)[a:b]
    x = np.ones(len(keys), np.float32) if vals is None else np.asarray(vals, np.float32)[a:b]
    ukeys, uidx = np.unique(keys, return_inverse=True)
    return rowptr - a, ukeys, uidx.astype(np.int64), fg, x


def step(ws, vs, F, rowptr, keys, fgid, vals, labels, audit, touched_only=True):
    """one field-aware update of the oracle stores; -> (ukeys, wu, loss, gw, gv, touched).
    touched_only=False steps every coordinate of a pushed key (what the reference's servers would
    do): the rule the tests show to differ under FTRL"""
    rp, ukeys, uidx, fg, x = _slice(rowptr, keys, fgid, vals)
    assert len(fg) == 0 or (fg.min() >= 0 and fg.max() < F), "fgid outside [0, fields)"
    if len(ukeys) == 0:
        return ukeys, _NONE, _NONE, _NONE, _NONE, np.zeros((0, F), bool)
    wu, vu = FC.pull(ws, vs, ukeys)
    loss, _, _, pairs = forward(rp, uidx, fg, x, labels, wu, vu, F, audit)
    gw, gv, touched = gradient(rp, uidx, fg, len(ukeys), x, loss, F, pairs, audit)
    ws.push(ukeys, gw)
    if touched_only:
        push_touched(vs, ukeys, gv, touched, vs.dim // F)
    else:
        vs.push(ukeys, gv)
    return ukeys, wu, loss, gw, gv, touched


def predict(ws, vs, F, rowptr, keys, fgid, vals, labels, audit):
    rp, ukeys, uidx, fg, x = _slice(rowptr, keys, fgid, vals)
    if len(ukeys) == 0:
        return _sigmoid(np.zeros(len(rp) - 1, np.float32))
    wu, vu = FC.pull(ws, vs, ukeys)
    return forward(rp, uidx, fg, x, labels, wu, vu, F, audit)[1]


def stores(opt, F, k, seed):
    """w from zero, the F k wide v hash-normal for FTRL and SGD alike"""
    o = O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD
    return O.Store(o, 1), O.Store(o, F * k, O.INIT_HASHNORM, 0.0, seed)


# ---------------------------------------------------------------- files
def file_blocks(path, block_bytes, valued):
    """(rowptr, keys, fgid, labels, values or None) per block of the oracle's reader"""
    vals = V.file_values(path) if valued else None
    at = 0
    for rowptr, keys, fgid, labels in O.read_blocks(path, block_bytes):
        n = len(keys)
        yield rowptr, keys, fgid, labels, (vals[at:at + n] if valued else None)
        at += n


def train_worker(ws, vs, F, train_path, epochs, audit, valued=False, block_bytes=2 << 20,
                 touched_only=True):
    """XFlow(model=1, fm_mode=field_aware, core_num=1): the key-0 init push (every coordinate of
    key 0, as the worker pushes it), then one update per block and epoch"""
    ws.push(np.zeros(1, np.uint64), np.zeros(1, np.float32))
    vs.push(np.zeros(1, np.uint64), np.zeros(vs.dim, np.float32))
    blocks = list(file_blocks(train_path, block_bytes, valued))
    for _ in range(epochs):
        for rowptr, keys, fgid, labels, vals in blocks:
            step(ws, vs, F, rowptr, keys, fgid, vals, labels, audit, touched_only)


def predict_file(ws, vs, F, test_path, audit, valued=False, block_bytes=2 << 20):
    """block by block: a block's Pull inserts its unseen keys, then its forward"""
    labels_all, pctr_all = [], []
    for rowptr, keys, fgid, labels, vals in file_blocks(test_path, block_bytes, valued):
        pctr_all.append(predict(ws, vs, F, rowptr, keys, fgid, vals, labels, audit))
        labels_all.append(labels)
    return np.concatenate(labels_all), np.concatenate(pctr_all)


# ---------------------------------------------------------------- the builder's arrays
def field_arrays(rowptr, keys, fgid):
    """(xfg, coo_pos) restated: the fields in CSR order; the CSR positions in key order, ascending
    inside a key (a stable sort by key)"""
    rowptr = np.asarray(rowptr, np.int64)
    a, b = rowptr[0], rowptr[-1]
    keys = np.asarray(keys, np.uint64)[a:b]
    return (np.asarray(fgid, np.int64)[a:b].astype(np.uint32),
            np.argsort(keys, kind="stable").astype(np.uint32))


# ---------------------------------------------------------------- the tests' minibatch streams
# (tests/test_ffm_cpu.py runs the checker alone over every one of them and asserts that every sum
# is exact; tests/test_gpu_ffm.py compares the GPU with the checker on the same streams)
STEPS = 3
CASES = ("ragged", "long_rows", "zipf_heavy", "zipf_chunks")
# (case, fields, k): k in {1, 4, 7, 8, 16} x fields in {1, 3, 18, 39, 64}, thinned — every k and
# every field count at least twice, the widest rows (64 x 16) and the chunked heavy keys once each
# — and four shapes with k in {24, 40, 70, 80} for the runtime-k paths
GRID = (("ragged", 1, 4), ("ragged", 3, 1), ("ragged", 18, 4), ("ragged", 39, 7),
        ("ragged", 64, 16), ("ragged", 18, 8), ("long_rows", 3, 16), ("long_rows", 39, 4),
        ("long_rows", 64, 1), ("zipf_heavy", 18, 7), ("zipf_heavy", 1, 8), ("zipf_heavy", 64, 4),
        ("zipf_chunks", 18, 4), ("zipf_chunks", 39, 1),
        # k beyond the compile-time paths: 32 and 64 factor lanes, and passes of 64 (k > 64)
        ("ragged", 3, 24), ("zipf_heavy", 2, 40), ("ragged", 1, 80), ("zipf_heavy", 3, 70))


# from fresh hash-normal tables (the keys inserted by the Pulls): (case, fields, k, optimizer,
# valued, steps).  SGD keeps every sum exact over three steps on these; FTRL for one step (its
# first step leaves factors of any magnitude, after which the y2 sums are not exact)
FRESH = (("ragged", 18, 4, "sgd", False, 3), ("ragged", 18, 4, "sgd", True, 3),
         ("zipf_heavy", 18, 4, "sgd", False, 3), ("ragged", 3, 8, "sgd", False, 3),
         ("ragged", 39, 4, "ftrl", False, 1), ("ragged", 39, 4, "ftrl", True, 1))


def _fields_of(rng, keys, F):
    """a key's home field (from the key), one nonzero in ten under another field: keys under two
    fields, and (key, field) pairs a minibatch never touches"""
    fg = (np.asarray(keys, np.uint64) % np.uint64(F)).astype(np.int32)
    other = rng.rand(len(fg)) < 0.1
    fg[other] = rng.randint(0, F, size=int(other.sum()))
    return fg


def stream(case, F, seed=0):
    """STEPS minibatches (rowptr, keys, fgid, values, labels) whose keys overlap step to step;
    the values are tests/_valued_cases.py's (eight significant bits, 2^-4 ... 4, some zero)"""
    from tests import _valued_cases as Cs
    out = []
    for i in range(STEPS):
        if case == "ragged":        # rows of 0 .. 40, row 1 holds one key twice
            rowptr, keys, vals, labels = Cs.ragged(seed + i)
        elif case == "long_rows":   # rows of 1 to several hundred nonzeros
            rng = np.random.RandomState(100 + seed + i)
            lens = np.r_[1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 257, 331, rng.randint(1, 30, 28)]
            rowptr = np.r_[0, np.cumsum(lens)].astype(np.uint64)
            keys = Cs._keytab(4000)[rng.randint(0, 4000, size=int(rowptr[-1]))]
            # (a 331-long row has 54 615 pairs: the values an eighth of the other cases', so that
            # the second-order term stays below 1 and no loss is tiny beside the others)
            vals = Cs._values(rng, lens) * np.float32(0.125)
            labels = rng.randint(0, 2, size=len(lens)).astype(np.int32)
        elif case == "zipf_heavy":  # head keys beyond XF_HEAVY_SEG, every one in one chunk
            rowptr, keys, vals, labels = Cs.zipf(seed + i, 400, 14, 3000)
        elif case == "zipf_chunks":  # the head key spans several chunks of XF_TILE_NNZ
            rowptr, keys, vals, labels = Cs.zipf(seed + i, 2500, 20, 5000)
        else:
            raise KeyError(case)
        fg = _fields_of(np.random.RandomState(7 + seed + i), keys, F)
        out.append((rowptr, keys, fg, vals, labels))
    return out


def stream_keys(mbs):
    return np.unique(np.concatenate([m[1] for m in mbs]))


def aged_stores(opt, F, k, mbs, seed=7):
    """the oracle's stores holding tests/_valued_cases.old_state for the stream's keys: tables
    "many steps old", whose products add exactly (see there)"""
    from tests import _valued_cases as Cs
    ws, vs = stores(opt, F, k, seed)
    ws.import_(*Cs.old_state(stream_keys(mbs), opt, 1, "w"))
    vs.import_(*Cs.old_state(stream_keys(mbs), opt, F * k))
    return ws, vs


def run_checker(opt, F, k, mbs, audit, valued=True, aged=True, seed=7):
    """the checker over a stream: -> per step (ukeys, wu, loss, gw, gv, touched), the stores, the
    last minibatch's predictions"""
    ws, vs = aged_stores(opt, F, k, mbs, seed) if aged else stores(opt, F, k, seed)
    steps = []
    for rowptr, keys, fg, vals, labels in mbs:
        steps.append(step(ws, vs, F, rowptr, keys, fg, vals if valued else None, labels, audit))
    rowptr, keys, fg, vals, labels = mbs[-1]
    pctr = predict(ws, vs, F, rowptr, keys, fg, vals if valued else None, labels, audit)
    return steps, ws, vs, pctr


# the worker end to end on the golden sample files (18 fields), from fresh tables
E2E_FIELDS, E2E_K, E2E_EPOCHS = 18, 4, 2


def run_checker_files(opt, train_path, test_path, audit, valued=False, touched_only=True):
    """-> the stores after training, (labels, pctr) of the test file, its metrics"""
    ws, vs = stores(opt, E2E_FIELDS, E2E_K, 0)      # the worker's seed: 0
    train_worker(ws, vs, E2E_FIELDS, train_path, E2E_EPOCHS, audit, valued,
                 touched_only=touched_only)
    lab, p = predict_file(ws, vs, E2E_FIELDS, test_path, audit, valued)
    return ws, vs, lab, p, O.auc_logloss(lab, p)
