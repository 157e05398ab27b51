"""The valued and field-aware checkers for inputs whose sums are NOT exact in fp64.

The arithmetic is that of tests/_valued_checker.py and tests/_ffm_checker.py (their docstrings
state the functions; the products, casts and the touched rule are taken from them).  Where those
form a sum twice and demand that the two orders agree, these hand every family of sums to
tests/_interval.py and carry CANDIDATES, every fp32 value from the low to the high end of what the
sum may give in any order: one where the sum is pinned (the GPU is then held to that value bit for
bit), two adjacent ones where it is open — or, where a sum cancels badly, a few more (a heavy
key's gv of 1787 addends that cancel to 10^-6 of their magnitudes spans 7) —, and the GPU must
give one of them.  A Judge collects the counts; every test asserts Judge.assert_cap.

An open sum must not compound: the gradient is formed from a GIVEN loss (the GPU's in the GPU
tests, the low candidate's on the CPU) and the stores are set to given tables after every step
(Run.adopt: the GPU's export), so every step is judged from the state the GPU really holds.  The
canonical gradient reads S[r,f]; an open S would make its addends ambiguous, so no S may be open
(Judge.assert_cap)."""
import numpy as np

from tests import _ffm_checker as F
from tests import _fmc_checker as FC
from tests import _interval as I
from tests import _valued_checker as V

_f32 = V._f32
_div_rows = V._div_rows
_sigmoid = FC._sigmoid
rows_of = FC.rows_of


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ends(seg, nseg, vals, fam, judge, flat=False):
    s = _family(seg, nseg, vals, fam, judge, flat)
    lo, hi = s.ends32()
    judge.note(fam, s.proven, lo, hi)
    return lo, hi


def _family(seg, nseg, vals, fam, judge, flat=False):
    s = I.family(seg, nseg, vals, flat)
    if judge.keep is not None:      # the addends themselves, for the CPU tests of _interval
        judge.keep.append((fam, np.asarray(seg, np.int64), nseg, _f32(vals), flat, s))
    return s


_MAXC = 256      # the most fp32 values one quantity may take before a test gives up on it


def _between(lo, hi, what):
    """every fp32 value from lo to hi, per element: [..., C] with C - 1 the widest gap in steps
    (an element with fewer values repeats its high end)"""
    lo, hi = _f32(lo), _f32(hi)
    assert np.all(lo <= hi), what
    out = [lo]
    while np.any(out[-1] < hi):
        assert len(out) < _MAXC, "%s: a quantity may take more than %d fp32 values" % (what, _MAXC)
        out.append(np.minimum(np.nextafter(out[-1], np.float32(np.inf)), hi))
    if len(out) == 1 and not np.array_equal(bits(lo), bits(hi)):
        out.append(hi)                                  # -0 and +0
    return np.stack(out, axis=-1)


def _candidates(labels, wx, y2=None):
    """pctr and loss for every value t = fp32(wx + y2) may take: fp32 addition is monotone in
    both, so t lies between the sum of the low ends and the sum of the high ends, and every fp32
    value in between is a candidate -> loss[R, C], pctr[R, C] (C = 1: every row is pinned)"""
    lo, hi = (wx[0], wx[1]) if y2 is None else (_f32(wx[0] + y2[0]), _f32(wx[1] + y2[1]))
    t = _between(lo, hi, "wx + y2")
    R = t.shape[0]
    # (sigmoid_ref once per row, and again for the rows with more than one candidate)
    p = np.repeat(_sigmoid(t[:, 0]) if R else np.zeros(0, np.float32), t.shape[1]).reshape(t.shape)
    p = _f32(p)
    odd = np.flatnonzero((bits(t) != bits(t[:, :1])).any(axis=1))
    if len(odd):
        p[odd] = _sigmoid(t[odd])
    loss = _f32(p - np.asarray(labels, np.float32)[:, None])
    return loss, p


def forward_lr(rowptr, uidx, x, labels, wu, judge):
    """-> loss[R, C], pctr[R, C]"""
    R = len(rowptr) - 1
    return _candidates(labels, _ends(rows_of(rowptr), R, _f32(wu[uidx] * x), "wx", judge))


def forward_fm(rowptr, uidx, x, labels, wu, vu, judge):
    """canonical: -> loss[R, C], pctr[R, C], S[R, k] (its low end: no S may be open)"""
    R, row = len(rowptr) - 1, rows_of(rowptr)
    wx = _ends(row, R, _f32(wu[uidx] * x), "wx", judge)
    A = _f32(vu[uidx] * x[:, None])
    S = _ends(row, R, A, "S", judge)[0]
    Q = _family(row, R, _f32(A * A), "Q", judge, flat=True)            # one sum over (j, f)
    T = _family(np.arange(R), R, _f32(S * S), "T", judge, flat=True)
    (t_lo, t_hi), (q_lo, q_hi) = T.ends64(), Q.ends64()
    # fp64 subtraction and the cast are monotone: the ends of T - Q are those of the ends
    y2 = (0.5 * (t_lo - q_hi)).astype(np.float32), (0.5 * (t_hi - q_lo)).astype(np.float32)
    judge.note("y2", T.proven & Q.proven, *y2)
    return _candidates(labels, wx, y2) + (S,)


def forward_ffm(rowptr, uidx, fg, x, labels, wu, vu, Fd, judge):
    """field-aware: -> loss[R, C], pctr[R, C], the pair list with its factors"""
    R, k = len(rowptr) - 1, vu.shape[1] // Fd
    wx = _ends(rows_of(rowptr), R, _f32(wu[uidx] * x), "wx", judge)
    pi, pj, pr = F.pairs_of(rowptr)
    a_ij, a_ji = F._factors(uidx, fg, x, vu, Fd, pi, pj)
    y2 = _ends(pr, R, _f32(a_ij * a_ji).reshape(len(pr), k), "y2", judge, flat=True)
    return _candidates(labels, wx, y2) + ((pi, pj, a_ij, a_ji),)


def _grads(ends, R, what):
    """the gradients of every fp32 value a sum may take: fp32(c / R) -> [..., C]"""
    c = _between(ends[0], ends[1], what)
    return _div_rows(c, R)


def gradient_w(rowptr, uidx, U, x, loss, judge):
    """-> gw candidates [U, C], lx"""
    R = len(rowptr) - 1
    lx = _f32(loss[rows_of(rowptr)] * x)
    return _grads(_ends(uidx, U, lx, "gw", judge), R, "gw"), lx


def gradient_fm(rowptr, uidx, U, x, lx, S, vu, judge):
    R, row = len(rowptr) - 1, rows_of(rowptr)
    A = _f32(vu[uidx] * x[:, None])
    term = _f32(lx[:, None] * _f32(S[row] - A))
    return _grads(_ends(uidx, U, term, "gv", judge), R, "gv")


def gradient_ffm(rowptr, uidx, fg, U, lx, Fd, pairs, judge):
    """-> gv candidates [U, F k, C], touched[U, F]"""
    R = len(rowptr) - 1
    pi, pj, a_ij, a_ji = pairs
    k = a_ij.shape[1]
    seg = np.r_[uidx[pi] * Fd + fg[pj], uidx[pj] * Fd + fg[pi]]
    term = np.concatenate([_f32(lx[pi][:, None] * a_ji), _f32(lx[pj][:, None] * a_ij)])
    touched = np.bincount(seg, minlength=U * Fd).reshape(U, Fd) > 0
    if len(seg):
        ends = _ends(seg, U * Fd, term, "gv", judge)
    else:
        ends = (np.zeros((U * Fd, k), np.float32),) * 2
    g = _grads(ends, R, "gv")
    return g.reshape(U, Fd * k, g.shape[-1]), touched


# ---------------------------------------------------------------- the stores
def _table(store):
    keys, w, n, z = store.export()
    return keys, [a.reshape(len(keys), -1) for a in (w, n, z)]


class Expected:
    """a table after a step: keys; first, the (w, n, z) that the low candidate gradient gives
    ([K, dim] each); more, per further candidate the rows it changes (row numbers, their (w, n,
    z)) — a coordinate's step reads that coordinate alone, so the table may take any candidate
    coordinate by coordinate; pre, the table before the step; stepped, the coordinates the step
    moves"""

    def __init__(self, keys, first, more, pre, stepped):
        self.keys, self.first, self.more, self.pre, self.stepped = keys, first, more, pre, stepped

    def holds(self, w, n=None, z=None):
        """per coordinate: is the given (w, n, z) — FTRL — or w — SGD: n, z None — that of one
        candidate, bit for bit"""
        got = [bits(a).reshape(self.pre[0].shape) for a in (w, n, z) if a is not None]

        def equal(g, e):
            one = np.ones(g[0].shape, bool)
            for x, y in zip(g, e):
                one &= x == bits(y)
            return one

        ok = equal(got, self.first)
        for at, rows in self.more:
            ok[at] |= equal([g[at] for g in got], rows)
        return ok


def _push_all(store, ukeys, g, mask=None):
    """Store.push of every candidate gradient g[..., c] from one state -> Expected; only the
    coordinates of `mask` are stepped (the touched rule, as _ffm_checker.push_touched lays it over
    Store.push).  The store is left holding the first (the low) candidate's table."""
    g = np.asarray(g, np.float32)
    g = g.reshape(len(ukeys), -1, g.shape[-1])
    mask = np.ones(g.shape[:2], bool) if mask is None else mask
    keys, pre = _table(store)
    at = np.searchsorted(keys, ukeys)
    assert np.array_equal(keys[at], ukeys), "the keys were pulled: they are in the store"

    def pushed(c, sel):
        """the rows of ukeys[sel] after candidate c's push, the store put back"""
        old = [a[at[sel]] for a in pre]
        store.push(ukeys[sel], np.where(mask[sel], g[sel, :, c], np.float32(0.0)))
        k1, new = _table(store)
        assert np.array_equal(k1, keys)
        rows = [np.where(mask[sel], b[at[sel]], a) for a, b in zip(old, new)]
        store.import_(ukeys[sel], *old)
        return rows

    every = np.arange(len(ukeys))
    rows = pushed(0, every)
    first = [a.copy() for a in pre]
    for f, r in zip(first, rows):
        f[at] = r
    more = []
    for c in range(1, g.shape[-1]):
        sel = np.flatnonzero((bits(g[..., c]) != bits(g[..., c - 1])).any(axis=1))
        if len(sel):
            more.append((at[sel], pushed(c, sel)))
    store.import_(ukeys, *rows)
    stepped = np.zeros(pre[0].shape, bool)
    stepped[at] = mask
    return Expected(keys, first, more, pre, stepped)


class Run:
    """one form over a stream of minibatches (rowptr, keys, fgid or None, values or None, labels).
    begin() pulls and gives the candidates of the forward; finish(loss) the candidates of the
    gradient of THAT loss and of both tables; adopt() sets the stores to given tables."""

    def __init__(self, form, ws, vs, judge, fields=0):
        assert form in ("lr", "fm", "ffm")
        self.form, self.ws, self.vs, self.judge, self.Fd = form, ws, vs, judge, fields

    def _pull(self, mb):
        rowptr, keys, fg, vals, labels = mb
        rowptr = np.asarray(rowptr, np.int64)
        a, b = rowptr[0], rowptr[-1]
        keys = np.asarray(keys, np.uint64)[a:b]
        x = np.ones(len(keys), np.float32) if vals is None else np.asarray(vals, np.float32)[a:b]
        fg = None if fg is None else np.asarray(fg, np.int64)[a:b]
        ukeys, uidx = np.unique(keys, return_inverse=True)
        self.rp, self.ukeys, self.uidx, self.fg, self.x = rowptr - a, ukeys, uidx.astype(
            np.int64), fg, x
        self.labels = labels
        assert len(ukeys), "the streams hold no empty minibatch"
        self.wu = _f32(self.ws.pull(ukeys)).reshape(len(ukeys))
        self.vu = None if self.form == "lr" else \
            _f32(self.vs.pull(ukeys)).reshape(len(ukeys), self.vs.dim)

    def _forward(self):
        if self.form == "lr":
            loss, p = forward_lr(self.rp, self.uidx, self.x, self.labels, self.wu, self.judge)
            self.aux = None
        elif self.form == "fm":
            loss, p, self.aux = forward_fm(self.rp, self.uidx, self.x, self.labels, self.wu,
                                           self.vu, self.judge)
        else:
            loss, p, self.aux = forward_ffm(self.rp, self.uidx, self.fg, self.x, self.labels,
                                            self.wu, self.vu, self.Fd, self.judge)
        return loss, p

    def begin(self, mb):
        """-> ukeys, wu, loss candidates [R, C]"""
        self._pull(mb)
        return self.ukeys, self.wu, self._forward()[0]

    def finish(self, loss):
        """-> gw candidates [U, C], Expected of w, Expected of v (None for LR)"""
        U = len(self.ukeys)
        gw, lx = gradient_w(self.rp, self.uidx, U, self.x, _f32(loss), self.judge)
        ew = _push_all(self.ws, self.ukeys, gw)
        if self.form == "lr":
            return gw, ew, None
        if self.form == "fm":
            gv = gradient_fm(self.rp, self.uidx, U, self.x, lx, self.aux, self.vu, self.judge)
            return gw, ew, _push_all(self.vs, self.ukeys, gv)
        gv, touched = gradient_ffm(self.rp, self.uidx, self.fg, U, lx, self.Fd, self.aux,
                                   self.judge)
        self.touched = touched
        mask = np.repeat(touched, self.vs.dim // self.Fd, axis=1)
        return gw, ew, _push_all(self.vs, self.ukeys, gv, mask=mask)

    def adopt(self, w_table, v_table=None):
        """(keys, w, n, z) as Table.export gives them"""
        for s, t in ((self.ws, w_table), (self.vs, v_table)):
            if s is not None and t is not None:
                s.import_(*t)

    def predict(self, mb):
        """-> pctr candidates [R, C]"""
        self._pull(mb)
        return self._forward()[1]

    def step(self, mb):
        """the CPU's run: the low candidates throughout"""
        ukeys, wu, loss = self.begin(mb)
        return (ukeys, wu, loss) + self.finish(loss[:, 0])
