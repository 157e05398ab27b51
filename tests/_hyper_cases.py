"""Hyper-parameter points away from the defaults (alpha 0.05, beta 1, lambda1 5e-5, lambda2 10,
lr 0.001), and the runs that tests/test_gpu_hyper.py drives at them.

Every run here is formed by the oracle alone in tests/test_general_position_cpu.py first: the cap
on open sums per family, the share of exact zeros that SPARSE leaves, and that the checks bite.

A step that takes a weight table and a factor table gives the two DIFFERENT sets (PAIR), so a
kernel that steps one table with the other's values lands on other bits."""
import numpy as np

from oracle import pyoracle as O
from tests import _general_cases as GC
from tests import _general_checker as G
from tests import _interval as I

DEFAULT = (0.05, 1.0, 5e-5, 10.0, 0.001)


def synth(rng, R, nnz_per_row, nkeys, zipf=None, ragged=False):
    """a random minibatch (rowptr, keys, labels): R rows of nnz_per_row nonzeros (ragged: 0 to
    twice that), keys uniform or Zipf over hash_str("0") .. — the generator of the parity, cells
    and hyper-parameter tests (here, because tests/test_gpu_parity.py needs a GPU to import)"""
    lens = rng.randint(0, 2 * nnz_per_row + 1, size=R) if ragged else np.full(R, nnz_per_row)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(lens.sum())
    if zipf:
        fid = np.minimum(rng.zipf(zipf, size=n), nkeys) - 1
    else:
        fid = rng.randint(0, nkeys, size=n)
    table = np.array([O.hash_str(str(i)) for i in range(nkeys)], dtype=np.uint64)
    return rowptr, table[fid], rng.randint(0, 2, size=R).astype(np.int32)


class Hyper:
    """one point: FTRL's (alpha, beta, lambda1, lambda2) or SGD's lr, the rest at the defaults"""

    def __init__(self, name, opt, alpha=DEFAULT[0], beta=DEFAULT[1], lambda1=DEFAULT[2],
                 lambda2=DEFAULT[3], lr=DEFAULT[4]):
        self.name, self.opt = name, opt
        self.alpha, self.beta, self.lambda1, self.lambda2, self.lr = alpha, beta, lambda1, lambda2, lr

    def five(self):
        return self.alpha, self.beta, self.lambda1, self.lambda2, self.lr

    def kw(self):
        """for capi.Table(**kw), capi.Sharded(**kw), XFlow(**kw)"""
        return dict(zip(("alpha", "beta", "lambda1", "lambda2", "lr"), self.five()))

    def to_store(self, s):
        if s is None:
            return
        if self.opt == "ftrl":
            s.set_ftrl(self.alpha, self.beta, self.lambda1, self.lambda2)
        else:
            s.set_sgd(self.lr)

    def to_table(self, t):
        if t is not None:
            t.set_hyper(*self.five())

    def but(self, name, **kw):
        h = Hyper(name, self.opt, *self.five())
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    def __repr__(self):
        return self.name


# lambda1 of SPARSE: chosen with the oracle (test_general_position_cpu.py asserts the condition on
# every stream SPARSE is used on; DESIGN §"Hyper-parameter points" has the measured shares)
SPARSE_L1 = 8.5e-5

A = Hyper("A", "ftrl", 0.1, 0.5, 1e-4, 5.0)
NO_L1 = Hyper("NO_L1", "ftrl", 0.3, 0.25, 0.0, 0.5)
SPARSE = Hyper("SPARSE", "ftrl", 0.01, 2.0, SPARSE_L1, 10.0)
NEG_L1 = Hyper("NEG_L1", "ftrl", 0.05, 1.0, -1e-3, 10.0)
SGD_LO = Hyper("SGD_0.05", "sgd", lr=0.05)
SGD_HI = Hyper("SGD_0.2", "sgd", lr=0.2)
FTRL_DEFAULT = Hyper("DEFAULT", "ftrl")
SGD_DEFAULT = Hyper("SGD_DEFAULT", "sgd")

# (weight table's set, factor table's set)
PAIR = {"ftrl": (NO_L1, SPARSE), "sgd": (SGD_LO, SGD_HI)}
# what the mid-run change goes to: neither table keeps a value it had
PAIR_AFTER = {"ftrl": (A, NO_L1), "sgd": (SGD_HI, SGD_LO)}
SWITCH = 2          # steps 0, 1 under the first pair, 2, 3 under the second


class Plan:
    """one run of tests/_general_checker.py: a stream, a form, and per phase (hyper_w, hyper_v).
    An LR run has one table: the first member."""

    def __init__(self, form, case, fields, k, opt, valued=True, phases=None):
        self.form, self.case, self.fields, self.k, self.opt, self.valued = (
            form, case, fields, k, opt, valued)
        self.phases = phases or [PAIR[opt]]
        if form == "lr":
            self.phases = [(p[0], None) for p in self.phases]
        self.id = "%s-%s-%dx%d-%s-%s-%s" % (
            form, case, fields, k, "valued" if valued else "binary", opt,
            "_then_".join("%s.%s" % p for p in self.phases))

    def stream(self):
        mbs = GC.gpu_stream(self.form, self.case, self.fields)
        return mbs if self.valued else GC.binary(mbs)

    def seed(self):
        return INIT_SEED.get((self.form, self.case, self.fields, self.k), GC.init_seed(self.case))

    def stores(self):
        sw, sv = GC.stores(self.form, self.opt, self.fields, self.k, self.seed())
        self.phases[0][0].to_store(sw)
        if sv is not None:
            self.phases[0][1].to_store(sv)
        return sw, sv

    def phase_at(self, i):
        """the pair that takes effect before step i, or None"""
        return self.phases[1] if len(self.phases) > 1 and i == SWITCH else None


def _both(form, case, fields, k, valued=True, **kw):
    return [Plan(form, case, fields, k, opt, valued, **kw) for opt in GC.OPTS]


def _changed(form, case, fields, k, opt, valued=True, **kw):
    return Plan(form, case, fields, k, opt, valued, phases=[PAIR[opt], PAIR_AFTER[opt]], **kw)


# valued LR has one table: capi.Batch(values=) takes the first members of PAIR, the local valued
# build the members of LR_LOCAL_PAIR
LR_LOCAL_PAIR = {"ftrl": (A, None), "sgd": (SGD_HI, None)}
LR_BATCH = _both("lr", "ragged", 0, 1)
LR_LOCAL = [Plan("lr", "zipf_chunks", 0, 1, opt, phases=[LR_LOCAL_PAIR[opt]]) for opt in GC.OPTS]
FM = _both("fm", "ragged", 0, 7) + _both("fm", "zipf_heavy", 0, 64)
# (18 x 4 binary on the long rows: on the ragged stream a (key, field) coordinate meets a handful
# of pairs in four steps, SPARSE zeroes nine in ten of them at any lambda1 that leaves canonical
# FM's k = 7 a fifth, and the condition on SPARSE could not be met on both)
FFM = _both("ffm", "long_rows", 18, 4, valued=False) + _both("ffm", "ragged", 39, 7)
# heavy keys of the field-aware kernels (k_ffm_heavy_finish).  Not under SPARSE: on this stream it
# zeroes 97 % at the lambda1 the other streams need
FFM_HEAVY_PAIR = {"ftrl": (A, NO_L1), "sgd": (SGD_HI, SGD_LO)}
FFM_HEAVY = [Plan("ffm", "zipf_heavy", 18, 7, opt, phases=[FFM_HEAVY_PAIR[opt]]) for opt in GC.OPTS]
FFM = FFM + FFM_HEAVY
# set_hyper in mid-run: one per form
LR_BATCH_CHANGED = [_changed("lr", "ragged", 0, 1, "ftrl")]
LR_LOCAL_CHANGED = [Plan("lr", "ragged", 0, 1, "ftrl", phases=[(A, None), (NO_L1, None)])]
FM_CHANGED = [_changed("fm", "ragged", 0, 7, "ftrl"), _changed("fm", "ragged", 0, 7, "sgd")]
FFM_CHANGED = [_changed("ffm", "ragged", 18, 4, "ftrl", valued=False)]

PLANS = (LR_BATCH + LR_LOCAL + FM + FFM + LR_BATCH_CHANGED + LR_LOCAL_CHANGED + FM_CHANGED +
         FFM_CHANGED)

# The seed of the hash-normal init per (form, case, fields, k), where tests/_general_cases.py's
# does not keep the open sums under the cap.  The long rows at 18 x 4, binary, under FTRL and SGD:
# seed 8 (_general_cases.INIT_SEED, found at 39 x 4) leaves 4 and 6 of the 200 y2 open, the cap is
# 4; seeds 7, 9, 10, 11 leave 3/4, 3/2, 4/4, 1/4 — at the cap or one open sum of the GPU's own
# trajectory away from it; 12 leaves 2 and 1.
INIT_SEED = {("ffm", "long_rows", 18, 4): 12}


def ids(plans):
    return [p.id for p in plans]


class Track:
    """what SPARSE's condition is about: per key and coordinate of one table, whether a step has
    moved it, whether w was exactly 0 after the first step, and w now"""

    def __init__(self):
        self.keys = None

    def note(self, i, keys, w, stepped):
        keys = np.asarray(keys, np.uint64)
        w = np.asarray(w, np.float32).reshape(len(keys), -1)
        stepped = np.asarray(stepped, bool).reshape(w.shape)
        if self.keys is None:
            self.keys = np.zeros(0, np.uint64)
            self.t, self.z0 = np.zeros((0, w.shape[1]), bool), np.zeros((0, w.shape[1]), bool)
            self.w = np.zeros((0, w.shape[1]), np.float32)
        allk = np.union1d(self.keys, keys)
        if len(allk) != len(self.keys):
            old = np.searchsorted(allk, self.keys)
            for name in ("t", "z0", "w"):
                a = getattr(self, name)
                b = np.zeros((len(allk), a.shape[1]), a.dtype)
                b[old] = a
                setattr(self, name, b)
            self.keys = allk
        at = np.searchsorted(allk, keys)
        self.t[at] |= stepped
        if i == 0:
            self.z0[at] |= stepped & (w == 0)
        self.w[at] = np.where(stepped, w, self.w[at])

    def shares(self):
        """-> (touched coordinates, exact zeros among them now, those that were 0 after the first
        step and are not now)"""
        touched = int(self.t.sum())
        zeros = int((self.t & (self.w == 0)).sum())
        woke = int((self.z0 & (self.w != 0)).sum())
        return touched, zeros, woke


def assert_sparse(track, what):
    touched, zeros, woke = track.shares()
    share = zeros / max(touched, 1)
    print("%s: SPARSE leaves %d of %d touched coordinates at 0 (%.1f %%), %d woke up" % (
        what, zeros, touched, 100 * share, woke))
    assert 0.2 <= share <= 0.8, (what, share)
    assert woke > 0, what
    return share


def sparse_table(plan):
    """which table of the plan's LAST phase runs under SPARSE: 0 (w), 1 (v) or None"""
    last = plan.phases[-1]
    return 0 if last[0] is SPARSE else 1 if last[1] is SPARSE else None


def run_cpu(plan, judge, track=None, wrong=None):
    """the checker alone over a plan, following its low candidates -> the Run.
    track: a Track of the table sparse_table names (the phases before the last count as steps too).
    wrong(phase) -> (hyper_w, hyper_v): a second checker makes every step from the same state
    under those sets instead; -> the Run and the number of coordinates of either table whose
    state no candidate of the right checker holds (a GPU making that mistake fails table_is)."""
    mbs = plan.stream()
    sw, sv = plan.stores()
    run = G.Run(plan.form, sw, sv, judge, plan.fields)
    which = sparse_table(plan)
    sgd = plan.opt == "sgd"
    bad = 0
    if wrong:
        xw, xv = GC.stores(plan.form, plan.opt, plan.fields, plan.k, plan.seed())
        other = G.Run(plan.form, xw, xv, I.Judge(), plan.fields)
        phase = plan.phases[0]
    for i, mb in enumerate(mbs):
        new = plan.phase_at(i)
        if new:
            new[0].to_store(sw)
            if new[1] is not None:
                new[1].to_store(sv)
            phase = new
        if wrong:
            hw, hv = wrong(phase)
            hw.to_store(xw)
            if hv is not None:
                hv.to_store(xv)
            pre = [None if s is None else (s.export()[:2] if sgd else s.export())
                   for s in (sw, sv)]
            other.adopt(*pre)
        _, _, _, _, ew, ev = run.step(mb)
        if wrong:
            _, _, _, _, fw, fv = other.step(mb)
            for e, f in ((ew, fw), (ev, fv)):
                if e is not None:
                    assert np.array_equal(e.keys, f.keys)
                    cols = f.first[:1] if sgd else f.first
                    bad += int(np.count_nonzero(~e.holds(*cols)))
        if track is not None and which is not None:
            e = (ew, ev)[which]
            track.note(i, e.keys, e.first[0], e.stepped)
    run.predict(mbs[-1])
    return (run, bad) if wrong else run


# ------------------------------------------------- steps the oracle itself makes (exact sums)
CELLS_SETS = (NO_L1, SPARSE, NEG_L1, SGD_HI)
CELLS_PATHS = (("lr_gradient", 1), ("lr_gradient", 2), ("lr_gradient", 3), ("old_weight", 2))
CELLS_STEPS = 4


def cells_raw():
    """the three-window power-law shape of tests/test_gpu_cells.py's gradient-kernel test"""
    rng = np.random.RandomState(11)
    return [synth(rng, 40000, 30, 120000, 1.2 if i % 2 else None, True) for i in range(3)]


def cells_raw_unsplit():
    """three windows whose chunks all stay whole (40000 rows of 0 to 12 nonzeros over 100 000
    uniform keys: about 5 000 entries per chunk of 2048 state rows, kSliceMax is 8192).  One split
    chunk sends a whole minibatch to k_lr_grad_cells, and every chunk of cells_raw() is split: this
    is the stream on which the knobs reach k_lr_grad_dense (tests/test_cells_edges_cpu.py counts
    both)."""
    rng = np.random.RandomState(12)
    return [synth(rng, 40000, 6, 100000, None, True) for _ in range(2)]


def old_weight_raw():
    """the stream of the old-weight tests (test_gpu_cells.py, test_gpu_hyper.py): split chunks"""
    rng = np.random.RandomState(23)
    return [synth(rng, 6000, 40, 30000, 1.2 if i else None, True) for i in range(2)]


def old_weight_raw_unsplit():
    """the same rows over 100 000 uniform keys: no chunk is split"""
    rng = np.random.RandomState(23)
    return [synth(rng, 6000, 40, 100000, None, True) for _ in range(2)]


def cells_oracle(raw, phases, track=None):
    """O.lr_update in sum_mode(1) over CELLS_STEPS steps; phases: [hyper] or [hyper, hyper after
    SWITCH] -> the store"""
    s = O.Store(O.OPT_FTRL if phases[0].opt == "ftrl" else O.OPT_SGD, 1)
    phases[0].to_store(s)
    obs = [O.Batch(*x) for x in raw]
    for i in range(CELLS_STEPS):
        if i == SWITCH and len(phases) > 1:
            phases[1].to_store(s)
        with O.sum_mode(1):
            O.lr_update(s, obs[i % len(obs)])
        if track is not None:
            keys, w = s.export()[:2]
            at = np.isin(keys, obs[i % len(obs)].ukeys)
            track.note(i, keys, w, at)
    return s


POOLED_K = 7
POOLED_STEPS = 4


def pooled_raw():
    """the stream of tests/test_gpu_parity.py's test_fm_step_state: the third step power-law"""
    rng = np.random.RandomState(POOLED_K)
    return [synth(rng, 500, 30, 4000, 1.3 if i == 2 else None, True) for i in range(POOLED_STEPS)]


def pooled_stores(opt, seed=99):
    o = O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD
    init = (O.INIT_HASHNORM, 0.0) if opt == "ftrl" else (O.INIT_CONST, 0.001)
    return O.Store(o, 1), O.Store(o, POOLED_K, init[0], init[1], seed), init


def pooled_oracle(raw, opt, phases, track=None, after_step=None):
    """O.fm_update in sum_mode(1) -> (sw, sv, pctr of the last minibatch).  after_step(i, sw, sv)
    is called after every step"""
    sw, sv, _ = pooled_stores(opt)
    phases[0][0].to_store(sw)
    phases[0][1].to_store(sv)
    ob = None
    for i, x in enumerate(raw):
        if i == SWITCH and len(phases) > 1:
            phases[1][0].to_store(sw)
            phases[1][1].to_store(sv)
        ob = O.Batch(*x)
        with O.sum_mode(1):
            O.fm_update(sw, sv, ob)
        if track is not None:
            keys, v = sv.export()[:2]
            at = np.isin(keys, ob.ukeys)
            track.note(i, keys, v, np.repeat(at[:, None], POOLED_K, axis=1))
        if after_step:
            after_step(i, sw, sv)
    with O.sum_mode(1):
        pctr = ob.fm_loss(POOLED_K, sw.pull(ob.ukeys), sv.pull(ob.ukeys))[1]
    return sw, sv, pctr


# the power-law heads of tests/test_gpu_parity.py's test_giant_heavy_keys_chunked_reduction: keys
# of ~15 000, ~4 000 and ~1 000 occurrences (chunked and single-chunk heavy keys of the keyed path)
GIANT_PAIR = {"ftrl": (NO_L1, A), "sgd": PAIR["sgd"]}
GIANT_K, GIANT_STEPS = 16, 3


def giant_raw():
    rng = np.random.RandomState(31)
    R = 6000
    lens = rng.randint(3, 12, size=R)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(lens.sum())
    fid = rng.randint(0, 5000, size=n)
    fid[rng.rand(n) < 0.35] = 7
    fid[rng.rand(n) < 0.10] = 11
    fid[rng.rand(n) < 0.03] = 13
    keytab = np.array([O.hash_str(str(i)) for i in range(5000)], dtype=np.uint64)
    return rowptr, keytab[fid], rng.randint(0, 2, size=R).astype(np.int32)
