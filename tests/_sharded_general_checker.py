"""Canonical FM, field-aware FM and feature values on several ranks on inputs whose sums are NOT
exact in fp64: the checker of tests/test_sharded_general_cpu.py and
tests/test_gpu_sharded_general.py.

No arithmetic of its own.  A rank's forward and gradient are tests/_general_checker.py's
(forward_lr / forward_fm / forward_ffm, gradient_w / gradient_fm / gradient_ffm, _between, _grads,
the Judge of tests/_interval.py) over ONE pair of O.Store, in the order of Pulls and Pushes that
tests/_sharded_modes_checker.py states: every rank pulls first, the pushes are applied in rank
order, each rank divides by its own 1 / R, and for field-aware FM a rank steps coordinate (u, h)
of v only if THAT rank's minibatch touched it.

The several-rank API fetches neither loss nor gradient, so everything is judged from tables and
predictions.  Two rules make that possible.

  * The loss is not observable.  Where a row's loss has more than one candidate (an open wx or
    y2) the gradient's addends fp32(loss x), fp32(lx fp32(S - A)), fp32(lx a) are formed at the
    row's low and at its high loss candidate.  Every addend is monotone in its row's loss (a
    product of two fp32 numbers, rounded), so the per-addend minimum and maximum bound it over
    every combination of candidates; a sum's low end is the interval rule's low end over the
    minimum addends, its high end the rule's high end over the maximum ones, and the Judge counts
    such a sum as unproven.  Rows whose loss is pinned contribute one addend.  S is never open
    (Judge.assert_cap).
  * N pushes compound inside a step.  A coordinate's step reads that coordinate alone, so the
    state after the pushes is, per coordinate, one of the COMBINATIONS of the sources' candidate
    gradients.  They are enumerated by whole-table runs: run j applies the pushes in order from
    the state before the step, every coordinate taking combination j — a mixed-radix index over
    the sources' candidate counts, the first source the least significant digit; a coordinate
    with fewer combinations repeats its last one (so run j pushes only the keys that own a
    coordinate with more than j combinations; the others keep run j - 1's rows).  The number of
    runs is the largest product of candidate counts over any coordinate.

Nothing compounds across judged points: after each the stores take the ranks' exported shards.
sequential is judged after every step.  stale1 lands step t's Push after step t + 1's Pull, so
with a flush after every second step two consecutive steps both compute from the adopted state:
they are judged as a pair, the chain being the N pushes of step t followed by the N of t + 1.

A minibatch is (rowptr, keys, fgid or None, values, labels); a binary trainer ignores the values.
A case is tests/_sharded_modes_checker.py's tuple (mode, world, fields, k, optimizer, schedule,
stream, valued)."""
import numpy as np

from tests import _general_cases as GC
from tests import _general_checker as G
from tests import _hyper_cases as _HC
from tests import _interval as I
from tests import _sharded_modes_checker as M

bits = G.bits
FORM = {"canonical": "fm", "lr": "lr", "field_aware": "ffm"}
case_id = M.case_id
owner_of = M.owner_of


# ---------------------------------------------------------------- streams
def rank_stream(mode, case, rank, F=0):
    """-> (the rank's training minibatches, its held-out minibatch).  The generators' seeds are
    moved by _sharded_modes_checker.rank_seed: ten apart per rank, steps 0 .. 3 and the held-out
    minibatch at + 5, so no two (rank, step) share one; the key universes are the streams' own,
    so the ranks push shared keys in every step"""
    base = M.rank_seed(rank)
    Fd = F if mode == "field_aware" else 0
    if case == "underflow":
        return GC.underflow_stream(Fd, base=base), GC.stream("ragged", Fd, 1, base + 5)[0]
    train = GC.stream(case, Fd, base=base)
    if mode == "field_aware" and case == "ragged":
        train = [M._probe_row(m, rank, F) for m in train]
    return train, GC.stream(case, Fd, 1, base + 5)[0]


def streams(spec, empty_ranks=()):
    mode, world, F, _, _, _, case, _ = spec
    out = []
    for r in range(world):
        train, held = rank_stream(mode, case, r, F)
        if r in empty_ranks:
            e = (M.EMPTY[0], M.EMPTY[1], np.zeros(0, np.int32) if mode == "field_aware" else None,
                 M.EMPTY[3], M.EMPTY[4])
            train, held = [e] * len(train), e
        out.append((train, held))
    return out


def points(schedule, steps):
    """the judged points: the steps each one covers"""
    if schedule == "sequential":
        return [[s] for s in range(steps)]
    assert steps % 2 == 0
    return [[s, s + 1] for s in range(0, steps, 2)]


# ---------------------------------------------------------------- one rank's share of a step
class Share:
    """what one rank pushes in one step: ukeys; R; the candidate gradients gw [U, 1, C] and gv
    [U, dim, C] (None for LR); touched [U, F] (field-aware, else None); ends, {family: (lo, hi)},
    the fp32 ends of the sums before the division by R"""


def _record(run, loss):
    """the gradient's addends for one loss per row: {family: (seg, nseg, addends, flat)}, touched"""
    jk = I.Judge(keep=True)
    U = len(run.ukeys)
    _, lx = G.gradient_w(run.rp, run.uidx, U, run.x, loss, jk)
    touched = None
    if run.form == "fm":
        G.gradient_fm(run.rp, run.uidx, U, run.x, lx, run.aux, run.vu, jk)
    elif run.form == "ffm":
        touched = G.gradient_ffm(run.rp, run.uidx, run.fg, U, lx, run.Fd, run.aux, jk)[1]
    return {fam: (seg, nseg, vals, flat, s) for fam, seg, nseg, vals, flat, s in jk.keep}, touched


def _wide_ends(seg, nseg, a, b, one, fam, judge):
    """the ends of the sums whose addends lie between a and b, element by element; one: the Sums
    of a"""
    if np.array_equal(a, b):
        if judge.keep is not None:
            judge.keep.append((fam, seg, nseg, a, False, one))
        lo, hi = one.ends32()
        judge.note(fam, one.proven, lo, hi)
        return lo, hi
    lo = G._family(seg, nseg, np.minimum(a, b), fam, judge).ends32()[0]
    hi = G._family(seg, nseg, np.maximum(a, b), fam, judge).ends32()[1]
    differ = (a != b).reshape(len(seg), -1).any(axis=1)
    wide = np.bincount(seg[differ], minlength=nseg) > 0
    judge.note(fam, one.proven & ~(wide if lo.ndim == 1 else wide[:, None]), lo, hi)
    return lo, hi


def share(run, mb, valued):
    """Pull, forward and the widened gradient of one rank's minibatch over the Run's stores (no
    Push) -> Share, or None for a rank without rows"""
    if len(mb[4]) == 0:
        return None
    run._pull(mb if valued else GC.binary([mb])[0])
    loss = run._forward()[0]
    lo, hi = loss[:, 0], loss[:, -1]
    rec, touched = _record(run, lo)
    rec_hi = rec if np.array_equal(bits(lo), bits(hi)) else _record(run, hi)[0]
    sh = Share()
    sh.ukeys, sh.R, sh.touched, sh.ends = run.ukeys, len(run.rp) - 1, touched, {}
    U = len(sh.ukeys)
    for fam in ("gw", "gv"):
        if fam in rec:
            seg, nseg, a, flat, one = rec[fam]
            assert not flat
            sh.ends[fam] = _wide_ends(seg, nseg, a, rec_hi[fam][2], one, fam, run.judge)
    sh.gw = G._grads(sh.ends["gw"], sh.R, "gw").reshape(U, 1, -1)
    sh.gv = None
    if run.form != "lr":
        dim = run.vs.dim
        if "gv" not in sh.ends:         # no pair in the whole minibatch: gradient_ffm's zeros
            sh.ends["gv"] = (np.zeros((U * run.Fd, dim // run.Fd), np.float32),) * 2
        g = G._grads(sh.ends["gv"], sh.R, "gv")
        sh.gv = g.reshape(U, dim, g.shape[-1])
    return sh


# ---------------------------------------------------------------- the pushes of a judged point
class Admissible:
    """a table after the pushes of a judged point: keys; tables, per run the (w, n, z), [K, dim]
    each; combos [K, dim], the combinations per coordinate; pre, the table before; stepped, the
    coordinates some source moves"""

    def __init__(self, keys, tables, combos, pre, stepped):
        self.keys, self.tables, self.combos, self.pre, self.stepped = \
            keys, tables, combos, pre, stepped

    def holds(self, w, n=None, z=None):
        """per coordinate: is the given (w, n, z) — FTRL — or w — SGD: n, z None — that of one
        admissible combination, bit for bit"""
        got = [bits(a).reshape(self.pre[0].shape) for a in (w, n, z) if a is not None]
        ok = np.zeros(got[0].shape, bool)
        for t in self.tables:
            one = np.ones(got[0].shape, bool)
            for x, y in zip(got, t):
                one &= x == bits(y)
            ok |= one
        return ok

    def pinned(self):
        return self.combos == 1


def _push(store, ukeys, g, touched):
    if touched is None:
        store.push(ukeys, g)
    else:
        M.FF.push_touched(store, ukeys, g, touched, store.dim // touched.shape[1])


def chain(store, pushes):
    """pushes: (ukeys, g [U, dim, C], touched [U, F] or None) in the order they land, from the
    store's state -> Admissible.  The store is left holding run 0 (every low candidate)."""
    keys, pre = G._table(store)
    K, dim = pre[0].shape
    combos = np.ones((K, dim), np.int64)
    stepped = np.zeros((K, dim), bool)
    ats, cnts = [], []
    for ukeys, g, touched in pushes:
        at = np.searchsorted(keys, ukeys)
        assert np.array_equal(keys[at], ukeys), "the keys were pulled: they are in the store"
        C = g.shape[-1]
        cu = np.ones(g.shape[:2], np.int64)
        if C > 1:
            ch = bits(g[..., 1:]) != bits(g[..., :-1])
            cu = np.where(ch.any(axis=-1), C - np.argmax(ch[..., ::-1], axis=-1), 1)
        mask = np.ones(g.shape[:2], bool) if touched is None else \
            np.repeat(touched, dim // touched.shape[1], axis=1)
        cnt = np.ones((K, dim), np.int64)
        cnt[at] = np.where(mask, cu, 1)
        stepped[at] |= mask
        combos *= cnt
        ats.append(at)
        cnts.append(cnt)
    runs = int(combos.max()) if K else 1
    assert runs <= G._MAXC, "a coordinate's sources combine to %d states, more than %d: the " \
        "stream cancels too badly to be judged" % (runs, G._MAXC)
    tables = []
    for j in range(runs):
        rows = (combos > j).any(axis=1)
        jj = np.minimum(j, combos - 1)
        for (ukeys, g, touched), at, cnt in zip(pushes, ats, cnts):
            idx = jj % cnt
            jj = jj // cnt
            sel = np.flatnonzero(rows[at])
            if len(sel):
                gi = np.take_along_axis(g[sel], idx[at[sel]][..., None], axis=-1)[..., 0]
                _push(store, ukeys[sel], gi, None if touched is None else touched[sel])
        new = G._table(store)[1]
        if j:
            new = [np.where(rows[:, None], b, a) for a, b in zip(tables[-1], new)]
        tables.append(new)
        store.import_(keys, *pre)
    store.import_(keys, *tables[0])
    return Admissible(keys, tables, combos, pre, stepped)


class Point:
    """a judged point: steps; shares[step][rank] (None: no rows); w, v (None for LR): Admissible"""


class Run:
    """one case over the ranks' streams.  point(steps) pulls for every rank and step, forms the
    shares from that one state and chains the pushes; adopt() sets the stores to given tables;
    predict(rank) gives the candidates of a rank's held-out minibatch."""

    def __init__(self, spec, strs, judge, seed=GC.SEED, hyper=None):
        mode, world, F, k, opt, schedule, case, valued = spec
        assert mode in M.MODES and schedule in ("sequential", "stale1") and len(strs) == world
        assert valued or mode != "lr", "binary LR is the reference's: the oracle's own update"
        self.spec, self.strs, self.judge = spec, strs, judge
        self.form, self.valued = FORM[mode], valued
        self.Fd = F if mode == "field_aware" else 0
        self.ws, self.vs = GC.stores(self.form, opt, self.Fd, k, seed)
        if hyper is not None:       # (tests/_hyper_cases.py: a Hyper) one set for both tables
            hyper.to_store(self.ws)
            hyper.to_store(self.vs)

    def _run(self):
        return G.Run(self.form, self.ws, self.vs, self.judge, self.Fd)

    def point(self, steps):
        p = Point()
        p.steps = list(steps)
        # every Pull of the point comes before its first Push: all shares read one state
        p.shares = [[share(self._run(), train[s], self.valued) for train, _ in self.strs]
                    for s in p.steps]
        land = [sh for ranks in p.shares for sh in ranks if sh is not None]
        p.w = chain(self.ws, [(sh.ukeys, sh.gw, None) for sh in land])
        p.v = None if self.vs is None else \
            chain(self.vs, [(sh.ukeys, sh.gv, sh.touched) for sh in land])
        return p

    def adopt(self, w_table, v_table=None):
        """(keys, w, n, z) as Table.export gives them"""
        for s, t in ((self.ws, w_table), (self.vs, v_table)):
            if s is not None and t is not None:
                s.import_(*t)

    def predict(self, rank):
        """-> pctr candidates [R, C] of the rank's held-out minibatch (R = 0: a rank without rows)"""
        mb = self.strs[rank][1]
        if len(mb[4]) == 0:
            return np.zeros((0, 1), np.float32)
        run = self._run()
        run._pull(mb if self.valued else GC.binary([mb])[0])
        return run._forward()[1]


def run_cpu(spec, judge, empty_ranks=(), seed=None, hyper=None):
    """the checker alone, following its low candidates -> Run, [Point], [pctr candidates per rank]"""
    strs = streams(spec, empty_ranks)
    run = Run(spec, strs, judge, init_seed(spec) if seed is None else seed, hyper)
    pts = [run.point(st) for st in points(spec[5], len(strs[0][0]))]
    return run, pts, [run.predict(r) for r in range(spec[1])]


# ---------------------------------------------------------------- what the streams must hold
def shared_keys(p):
    """per step of a point: the keys that two ranks push"""
    out = []
    for ranks in p.shares:
        ks = np.concatenate([sh.ukeys for sh in ranks if sh is not None])
        u, c = np.unique(ks, return_counts=True)
        out.append(u[c > 1])
    return out


def mask_differences(p, F):
    """field-aware: per step bool [F] — for field h, does some key pushed by two ranks have h
    touched on one and not on the other"""
    out = []
    for ranks in p.shares:
        d = np.zeros(F, bool)
        live = [sh for sh in ranks if sh is not None]
        for a in range(len(live)):
            for b in range(a + 1, len(live)):
                _, ia, ib = np.intersect1d(live[a].ukeys, live[b].ukeys, return_indices=True)
                d |= (live[a].touched[ia] != live[b].touched[ib]).any(axis=0)
        out.append(d)
    return out


# ---------------------------------------------------------------- the tests' cases
# (mode, world, fields, k, optimizer, schedule, stream, valued): what
# tests/test_gpu_sharded_general.py steps on the GPU; tests/test_sharded_general_cpu.py asserts the
# caps of every one
CASES = (("canonical", 2, 0, 7, "ftrl", "sequential", "ragged", True),
         ("canonical", 3, 0, 16, "sgd", "stale1", "zipf_chunks", True),
         ("canonical", 2, 0, 64, "ftrl", "stale1", "zipf_heavy", True),
         ("canonical", 2, 0, 4, "ftrl", "sequential", "ragged", False),
         ("lr", 2, 0, 0, "ftrl", "sequential", "zipf_chunks", True),
         ("lr", 3, 0, 0, "sgd", "stale1", "ragged", True),
         ("field_aware", 2, 18, 4, "ftrl", "sequential", "ragged", True),
         ("field_aware", 3, 3, 24, "sgd", "stale1", "zipf_heavy", False),
         ("field_aware", 2, 39, 7, "ftrl", "sequential", "long_rows", True),
         ("field_aware", 2, 64, 4, "ftrl", "stale1", "ragged", True))
UNDERFLOW = (("canonical", 2, 0, 4, "ftrl", "sequential", "underflow", True),
             ("field_aware", 2, 18, 4, "sgd", "sequential", "underflow", True),
             ("lr", 2, 0, 0, "ftrl", "sequential", "underflow", True))
# a group of one on the exchange path (XF_SHARDED_GENERAL=1)
GENERAL = (("canonical", 1, 0, 80, "ftrl", "sequential", "ragged", True),
           ("field_aware", 1, 18, 4, "ftrl", "sequential", "zipf_chunks", True))
# world 2, rank 1 without rows
EMPTY_RANK = (("field_aware", 2, 18, 4, "ftrl", "sequential", "ragged", True),)

# away from the default hyper-parameters (tests/_hyper_cases.py), one set for both tables
HYPER = ((("field_aware", 2, 18, 4, "ftrl", "sequential", "ragged", True), _HC.SPARSE),
         (("canonical", 3, 0, 16, "sgd", "stale1", "zipf_chunks", True), _HC.SGD_HI))


def hyper_id(v):
    return case_id(v) if isinstance(v, tuple) else repr(v)


# The seed of the hash-normal init is GC.SEED = 7 for every case: it is the one
# tests/test_gpu_sharded_modes.py's _trainer gives the GPU tables.  Where a case's open sums do not
# stay under the caps with it, the STREAM is moved instead (INIT_SEED stays empty unless a case
# names its own trainer).
INIT_SEED = {}


def init_seed(spec):
    return INIT_SEED.get(spec, GC.SEED)
