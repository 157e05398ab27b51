"""Which fp32 values an fp64 sum of fp32 addends may take, whatever the order of its additions.

The kernels add fp32 values (products already rounded to fp32) in fp64 and cast the sum to fp32.
tests/_valued_checker.py's audit accepts an input only when two orders give the same fp64 sum; this
module reasons about the cast instead, so that inputs in general position can be judged.

Per sum, over its nonzero addends a_1 .. a_n (an addition of 0 is exact):
  PROVEN    q = 2^(e - 24) for the smallest exponent e (frexp: |a| = m 2^e, 1/2 <= m < 1) among
            them: every a_i is a multiple of q.  If sum |a_i| < 2^53 q, every partial sum of every
            order is a multiple of q below 2^53 q, hence an fp64 number: no addition rounds, the
            sum is the exact one in every order.  (The test is made on the computed sum of |a_i|,
            whose own partial sums are then exact too; '<' and not '<=' because a computed 2^53 q
            may be a rounded one.)  A sum with no nonzero addend is proven.
  UNPROVEN  s* = math.fsum of the addends (the correctly rounded exact sum), and Higham's bound for
            any summation tree, |computed - exact| <= gamma_{n-1} sum |a_i| with
            gamma_m = m 2^-53 / (1 - m 2^-53): lanes, shuffle trees, LDS atomics in arrival order
            and chunked partials are all trees.  The computed sum lies in [s* - b, s* + b] and the
            cast to fp32 is monotone, so the fp32 result lies in fp32(s* - b) .. fp32(s* + b).
  PINNED / OPEN  the two ends are one fp32 value (pinned: the GPU must give it bit for bit) or
            not (open: the GPU must give one of them, or an fp32 value between them; `wide` counts
            the open sums whose ends are not ADJACENT, a handful of badly cancelling sums).
The ends are computed in fp64 and moved outward by two fp64 steps and the bound by 2^-30 of
itself, which covers the rounding of s*, of sum |a_i| and of the end itself."""
import math

import numpy as np

_U = 2.0 ** -53
_SLACK = 1.0 + 2.0 ** -30
_NOEXP = 900            # the "exponent" of a zero addend: above every fp32 one


class Sums:
    """one family of sums: s (proven: the exact sum; unproven: fsum), the bound b (0 where
    proven), the mask of the proven, all of one shape"""

    def __init__(self, s, b, proven):
        self.s, self.b, self.proven = s, b, proven

    def ends64(self):
        lo, hi = self.s - self.b, self.s + self.b
        un = ~self.proven
        lo[un] = np.nextafter(np.nextafter(lo[un], -np.inf), -np.inf)
        hi[un] = np.nextafter(np.nextafter(hi[un], np.inf), np.inf)
        return lo, hi

    def ends32(self):
        lo, hi = self.ends64()
        return lo.astype(np.float32), hi.astype(np.float32)


def gamma(m):
    m = np.maximum(np.asarray(m, np.float64), 0.0)
    return m * _U / (1.0 - m * _U)


def family(seg, nseg, vals, flat=False):
    """The sums of vals' rows per segment id -> Sums.  vals[N] gives [nseg]; vals[N, C] gives one
    sum per (segment, column), [nseg, C], or with flat=True one sum per segment over its rows AND
    columns, [nseg]."""
    seg = np.asarray(seg, np.int64)
    a = np.asarray(vals, np.float64)
    assert np.array_equal(a, np.asarray(vals, np.float32)), "the addends are fp32 values"
    one_d = a.ndim == 1
    if one_d:
        a = a[:, None]
    C = a.shape[1]
    order = np.argsort(seg, kind="stable")
    ss = seg[order]
    starts = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1]]) if len(ss) else np.zeros(0, np.int64)
    ids = ss[starts]
    stops = np.r_[starts[1:], len(ss)] if len(ss) else starts
    shape = (nseg,) if (flat or one_d) else (nseg, C)
    s, A = np.zeros(shape), np.zeros(shape)
    n = np.zeros(shape, np.int64)
    emin = np.full(shape, _NOEXP, np.int64)
    if len(starts):
        a = a[order]
        e = np.frexp(a)[1].astype(np.int64)
        e[a == 0.0] = _NOEXP
        parts = [np.add.reduceat(a, starts, axis=0), np.add.reduceat(np.abs(a), starts, axis=0),
                 np.add.reduceat((a != 0.0).astype(np.int64), starts, axis=0),
                 np.minimum.reduceat(e, starts, axis=0)]
        if flat or one_d:
            parts = [parts[0].sum(axis=1), parts[1].sum(axis=1), parts[2].sum(axis=1),
                     parts[3].min(axis=1)]
        s[ids], A[ids], n[ids], emin[ids] = parts
    proven = A < np.ldexp(1.0, 53 + emin - 24)
    b = np.where(proven, 0.0, gamma(n - 1) * A * _SLACK)
    if not proven.all():
        at = np.full(nseg, -1, np.int64)
        at[ids] = np.arange(len(ids))
        for i in zip(*np.nonzero(~proven)):
            j = at[i[0]]
            block = a[starts[j]:stops[j]]
            s[i] = math.fsum(block.ravel() if (flat or one_d) else block[:, i[1]])
    return Sums(s + 0.0, b, proven)      # + 0.0: a sum starts from +0 (see _valued_checker._Seg2)


def adjacent(lo, hi):
    """lo == hi, or hi is the fp32 value next above lo"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return (lo == hi) | (np.nextafter(lo, np.float32(np.inf)) == hi)


class Judge:
    """collects (family, sums formed, unproven, open, wide) and the open masks of a run; passed to
    tests/_general_checker.py's functions where the audit list of the exact checkers goes"""

    CAP = 0.02

    def __init__(self, keep=False):
        self.rows, self.masks = [], []
        self.keep = [] if keep else None    # (family, seg, nseg, addends, flat, Sums) per call

    def note(self, fam, proven, lo, hi):
        """-> the open mask of the family's fp32 ends"""
        open_ = np.asarray(lo, np.float32).view(np.uint32) != np.asarray(hi, np.float32).view(
            np.uint32)
        wide = int(np.count_nonzero(~adjacent(lo, hi)))
        self.rows.append((fam, int(open_.size), int(np.count_nonzero(~proven)),
                          int(np.count_nonzero(open_)), wide))
        self.masks.append((fam, open_))
        return open_

    def table(self):
        """{family: (formed, unproven, open, wide)}"""
        out = {}
        for fam, n, un, op, wide in self.rows:
            a = out.get(fam, (0, 0, 0, 0))
            out[fam] = (a[0] + n, a[1] + un, a[2] + op, a[3] + wide)
        return out

    def format(self, title=""):
        lines = ["%-34s %-4s %9s %9s %6s %5s" % (title, "", "formed", "unproven", "open", "wide")]
        for fam, v in sorted(self.table().items()):
            lines.append("%-34s %-4s %9d %9d %6d %5d" % (("", fam) + v))
        return "\n".join(lines)

    def open_count(self):
        return sum(v[2] for v in self.table().values())

    def assert_cap(self, no_open=("S",)):
        """the condition of every test: at most CAP of each family open, none of `no_open`"""
        t = self.table()
        assert t, "nothing was summed"
        for fam, (n, un, op, wide) in t.items():
            assert op <= self.CAP * n, "%s: %d of %d sums open, beyond the cap" % (fam, op, n)
            assert fam not in no_open or op == 0, "%s: %d of %d sums open" % (fam, op, n)
