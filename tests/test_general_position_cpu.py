"""Inputs in general position without a GPU: tests/_interval.py is sound on the very addends of
the streams of tests/_general_cases.py, wrong arithmetic is caught by its pinned sums, every
(stream, form, optimizer, shape) of tests/test_gpu_general_position.py keeps its open sums under
the cap, and the golden files under FTRL from fresh tables have no open sum at all (what the FTRL
worker runs of tests/test_gpu_ffm.py and tests/test_gpu_values.py rely on)."""
import os

import numpy as np
import pytest

from . import _general_cases as GC
from . import _general_checker as G
from . import _hyper_cases as HC
from . import _interval as I

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAIN, TEST = os.path.join(GOLDEN, "small_train-00000"), os.path.join(GOLDEN, "small_test-00000")
ORDERS = 16


# ------------------------------------------------------------------------ _interval alone
def test_interval_on_hand_made_sums():
    f = np.float32
    seg = np.array([0, 0, 0, 1, 1, 1, 2, 3, 3], np.int64)
    #   0: one magnitude, proven.  1: 1 + 2^-24 + 2^-60: the exact sum lies just above the middle
    #   of two fp32 values, fp64 absorbs 2^-60 and lands ON the middle: unproven and open.
    #   2: a lone addend.  3: 2^60 and 1: unproven, pinned.  4: nothing, proven, +0
    vals = np.array([1.5, -0.25, 3.0, 1.0, 2.0 ** -24, 2.0 ** -60, -7.0, 2.0 ** 60, 1.0], f)
    s = I.family(seg, 5, vals)
    assert s.proven.tolist() == [True, False, True, False, True]
    lo, hi = s.ends32()
    assert (lo[0], hi[0], lo[2], hi[2], lo[4], hi[4]) == (4.25, 4.25, -7.0, -7.0, 0.0, 0.0)
    assert lo[1] == 1.0 and hi[1] == np.nextafter(f(1.0), f(2.0))
    assert lo[3] == hi[3] == f(2.0 ** 60)
    assert not np.signbit(lo[4])
    # a column per factor, and one sum over rows and columns
    M = np.stack([vals, -vals], axis=1)
    two = I.family(seg, 5, M)
    assert np.array_equal(two.s[:, 0], s.s) and np.array_equal(two.s[:, 1], -s.s + 0.0)
    flat = I.family(seg, 5, M, flat=True)
    assert np.all(flat.s == 0.0) and flat.proven.tolist() == [True, False, True, False, True]
    j = I.Judge()
    j.note("x", s.proven, lo, hi)
    assert j.table() == {"x": (5, 2, 1, 0)}
    with pytest.raises(AssertionError, match="beyond the cap"):
        j.assert_cap()
    with pytest.raises(AssertionError, match="fp32 values"):
        I.family(seg, 5, vals.astype(np.float64) + 1e-12)


def _running_sums(seg, nseg, vals, flat, rng):
    """every segment's addends in one random order, added by a plain fp64 running sum"""
    a = np.asarray(vals, np.float64)
    a = a[:, None] if a.ndim == 1 else a
    if flat:
        seg, a = np.repeat(seg, a.shape[1]), a.reshape(-1, 1)
    order = np.lexsort((rng.rand(len(seg)), seg))
    ss, a = seg[order], a[order]
    out = np.zeros((nseg, a.shape[1]))
    if not len(ss):
        return out
    starts = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1]])
    lens = np.diff(np.r_[starts, len(ss)])
    by_len = np.argsort(-lens, kind="stable")
    starts, lens, ids = starts[by_len], lens[by_len], ss[starts][by_len]
    acc = np.zeros((len(ids), a.shape[1]))
    for p in range(int(lens[0])):
        cnt = int(np.searchsorted(-lens, -p, side="left"))      # the segments longer than p
        acc[:cnt] += a[starts[:cnt] + p]
    out[ids] = acc
    return out + 0.0


def _kept(form, opt, fields, k, mbs):
    j = I.Judge(keep=True)
    GC.run_cpu(form, opt, fields, k, mbs, j)
    return j


SOUND = [("lr", "ftrl", 0, 1, "ragged"), ("lr", "sgd", 0, 1, "underflow"),
         ("fm", "ftrl", 0, 7, "ragged"), ("fm", "sgd", 0, 4, "zipf_heavy"),
         ("fm", "ftrl", 0, 4, "underflow"), ("ffm", "ftrl", 3, 4, "ragged"),
         ("ffm", "sgd", 18, 4, "underflow")]


def _sound_stream(form, fields, case):
    if case == "underflow":
        return GC.underflow_stream(fields)
    return GC.stream(case, fields, steps=2 if form == "ffm" else GC.STEPS)


@pytest.mark.parametrize("form,opt,fields,k,case", SOUND)
def test_interval_is_sound_on_the_streams(form, opt, fields, k, case):
    """the addends of every family of a run, in ORDERS random orders: a proven sum is one fp64
    value, an unproven one stays within s* +- b, a pinned one is one fp32 value, an open one lies
    between its ends"""
    j = _kept(form, opt, fields, k, _sound_stream(form, fields, case))
    rng = np.random.RandomState(1)
    seen = {"proven": 0, "unproven": 0, "open": 0}
    for fam, seg, nseg, vals, flat, s in j.keep:
        shape = s.s.shape
        lo, hi = s.ends32()
        pinned = G.bits(lo) == G.bits(hi)
        seen["proven"] += int(s.proven.sum())
        seen["unproven"] += int((~s.proven).sum())
        seen["open"] += int((~pinned).sum())
        for _ in range(ORDERS):
            r = _running_sums(seg, nseg, vals, flat, rng).reshape(shape)
            assert np.array_equal(r[s.proven], s.s[s.proven]), fam
            assert np.all(np.abs(r - s.s) <= s.b), fam
            r32 = r.astype(np.float32)
            assert np.array_equal(G.bits(r32)[pinned], G.bits(lo)[pinned]), fam
            assert np.all((lo <= r32) & (r32 <= hi)), fam
    assert seen["proven"] and seen["unproven"], seen          # real test material


def test_the_underflow_minibatch_underflows():
    """its squares land in fp32's denormal range and below it, its products with w and the loss too
    (numpy keeps gradual underflow: the checker's fp32 products are not flushed)"""
    tiny = np.finfo(np.float32).tiny
    for form, fields, k in (("lr", 0, 1), ("fm", 0, 4), ("ffm", 18, 4)):
        j = _kept(form, "ftrl", fields, k, GC.underflow_stream(fields))
        last = {}
        for fam, seg, nseg, vals, flat, s in j.keep:
            last[fam] = vals
        sub = {f: int(np.count_nonzero((v != 0) & (np.abs(v) < tiny))) for f, v in last.items()}
        print(form, "denormal addends of the last call per family:", sub)
        assert sub["wx"] > 0 and sub["gw"] > 0
        if form == "fm":
            assert sub["S"] > 0 and sub["Q"] > 0 and sub["T"] > 0 and sub["gv"] > 0
            A = last["S"].astype(np.float64)
            assert np.count_nonzero((A != 0) & (last["Q"] == 0)) > 0      # squares below it: 0
        if form == "ffm":
            assert sub["y2"] > 0 and sub["gv"] > 0


# ------------------------------------------------------------------- the checks bite
def test_wrong_arithmetic_fails_a_pinned_comparison():
    """Two kernels that today's exact inputs cannot tell from the right one, restated in numpy on
    the addends of a run: (a) a product rounded late — the square (v x)^2 kept in fp64 when it is
    added to Q; (b) a heavy key's chunk partials kept in fp32.  Each changes pinned results."""
    j = _kept("fm", "ftrl", 0, 7, GC.stream("zipf_chunks")[:2])
    fams = {}
    for rec in j.keep:
        fams.setdefault(rec[0], []).append(rec)
    # (a) Q from the unrounded squares, T as it is: y2 of rows whose y2 is pinned
    bad = 0
    for (_, seg, nseg, A, _, _), (_, _, _, _, _, Q), (_, _, _, _, _, T) in zip(
            fams["S"], fams["Q"], fams["T"]):
        a64 = A.astype(np.float64)
        late = np.bincount(seg, (a64 * a64).sum(axis=1), nseg)
        (t_lo, t_hi), (q_lo, q_hi) = T.ends64(), Q.ends64()
        lo, hi = (0.5 * (t_lo - q_hi)).astype(np.float32), (0.5 * (t_hi - q_lo)).astype(np.float32)
        pinned = G.bits(lo) == G.bits(hi)
        got = (0.5 * (T.s - late)).astype(np.float32)
        bad += int(np.count_nonzero(G.bits(got)[pinned] != G.bits(lo)[pinned]))
    assert bad > 0
    # (b) gv of the heaviest key: chunks of 2048 occurrences, each partial cast to fp32
    bad = 0
    for _, seg, nseg, term, _, s in fams["gv"]:
        u = int(np.argmax(np.bincount(seg, minlength=nseg)))
        t = term[seg == u].astype(np.float64)
        assert len(t) > 2 * 2048
        part = np.stack([t[c:c + 2048].sum(axis=0) for c in range(0, len(t), 2048)])
        got = part.astype(np.float32).astype(np.float64).sum(axis=0).astype(np.float32)
        lo, hi = s.ends32()
        pinned = G.bits(lo[u]) == G.bits(hi[u])
        bad += int(np.count_nonzero(G.bits(got)[pinned] != G.bits(lo[u])[pinned]))
    assert bad > 0


# ------------------------------------------------------------------------ the cap
CAP_CASES = [("lr", c, 0, 1, True) for c in GC.LR_CASES + ("underflow",)] + \
    [("fm", c, 0, k, True) for c, k in GC.FM_GRID + (("underflow", 4),)] + \
    [("ffm", c, Fd, k, v) for c, Fd, k in GC.FFM_GRID for v in (False, True)] + \
    [("ffm", "underflow", 18, 4, True)]


@pytest.mark.parametrize("opt", GC.OPTS)
@pytest.mark.parametrize("form,case,fields,k,valued", CAP_CASES)
def test_open_sums_stay_under_the_cap(form, case, fields, k, valued, opt):
    """every run of tests/test_gpu_general_position.py, the checker alone (its low candidates):
    at most 2 % of each family open, no S open.  A condition on the streams, not a measurement:
    a stream that misses it gets another seed or scale, the cap stays."""
    mbs = GC.gpu_stream(form, case, fields)
    j = I.Judge()
    GC.run_cpu(form, opt, fields, k, mbs if valued else GC.binary(mbs), j, seed=GC.init_seed(case))
    print(j.format("%s %s %dx%d %s %s" % (form, case, fields, k, opt,
                                          "valued" if valued else "binary")))
    j.assert_cap()
    want = {"lr": {"wx", "gw"}, "fm": {"wx", "S", "y2", "gw", "gv"},
            "ffm": {"wx", "y2", "gw", "gv"}}[form]
    assert set(j.table()) == want


# ------------------------------------------------------------------------ the golden files
@pytest.mark.parametrize("form,fields,k,valued", [("ffm", 18, 4, False), ("ffm", 18, 4, True),
                                                  ("fm", 0, 4, True)])
def test_golden_files_under_ftrl_have_no_open_sum(form, fields, k, valued):
    """FTRL from fresh tables, two epochs and the test file: the audit of the exact checkers
    fails here (tests/test_ffm_cpu.py::test_golden_files_from_fresh_tables), the interval rule
    pins every sum.  The FTRL worker tests on the GPU assert the same before they compare."""
    j = I.Judge()
    GC.run_files(form, "ftrl", fields, k, TRAIN, TEST, j, valued)
    print(j.format("golden files, ftrl, %s %s" % (form, "valued" if valued else "binary")))
    t = j.table()
    assert t["y2"][0] == 600 and t["wx"][0] == 600
    assert t["y2"][1] > 0, "every sum is proven: the exact audit would pass too"
    assert j.open_count() == 0, t


# ------------------------------------------------- away from the default hyper-parameters
@pytest.mark.parametrize("plan", HC.PLANS, ids=HC.ids(HC.PLANS))
def test_hyper_streams_stay_under_the_cap(plan):
    """every run of tests/test_gpu_hyper.py that goes through the interval checker, formed by the
    oracle alone under the same hyper-parameters (per table, and changed in mid-run where the GPU
    test changes them): the cap, and SPARSE's condition where a table runs under SPARSE to the
    end — 20 to 80 % of the touched coordinates exactly 0 after the last step, and a coordinate
    that was 0 after the first step is not later"""
    j, track = I.Judge(), HC.Track()
    HC.run_cpu(plan, j, track)
    print(j.format(plan.id))
    j.assert_cap()
    if HC.sparse_table(plan) is not None:
        HC.assert_sparse(track, plan.id)


def test_sparse_condition_on_the_oracle_made_steps():
    """the binary LR cells stream and the pooled FM stream (tests/test_gpu_hyper.py steps them
    against O.lr_update / O.fm_update: exact sums, no cap to hold)"""
    track = HC.Track()
    HC.cells_oracle(HC.cells_raw(), [HC.SPARSE], track)
    HC.assert_sparse(track, "binary LR cells")
    track = HC.Track()
    HC.pooled_oracle(HC.pooled_raw(), "ftrl", [HC.PAIR["ftrl"]], track)
    HC.assert_sparse(track, "pooled FM, the factor table")


@pytest.mark.parametrize("valued", [False, True], ids=["binary", "valued"])
def test_golden_files_under_set_A_have_no_open_sum(valued):
    """what the worker run under A of tests/test_gpu_ffm.py relies on"""
    j = I.Judge()
    GC.run_files("ffm", "ftrl", 18, 4, TRAIN, TEST, j, valued, hyper=HC.A)
    print(j.format("golden files, ftrl A, %s" % ("valued" if valued else "binary")))
    assert j.open_count() == 0, j.table()


BITE = [HC.FM[0], HC.FM[1], HC.FFM[2], HC.FFM[3]]       # canonical k = 7 ragged, 39 x 7 valued


def _swapped(phase):
    return phase[1], phase[0]


def _default_lr(phase):
    return HC.SGD_DEFAULT, HC.SGD_DEFAULT


def _l1_default(phase):
    return tuple(h.but("NO_L1 with the default lambda1", lambda1=HC.DEFAULT[2])
                 if h is HC.NO_L1 else h for h in phase)


@pytest.mark.parametrize("plan,wrong", [(p, w) for p in BITE for w in (
    (_swapped, _l1_default) if p.opt == "ftrl" else (_swapped, _default_lr))],
    ids=lambda v: v.id if isinstance(v, HC.Plan) else v.__name__)
def test_the_hyper_checks_bite(plan, wrong):
    """three mistakes a kernel could make, each restated with a second checker that makes every
    step from the right checker's state under the wrong sets: the two tables' sets swapped, the
    default lr, and NO_L1's lambda1 = 0 taken for the default 5e-5.  Each leaves coordinates whose
    state none of the right checker's candidates holds: the GPU test would fail there."""
    _, bad = HC.run_cpu(plan, I.Judge(), wrong=wrong)
    print("%s, %s: %d coordinates hold no candidate's state" % (plan.id, wrong.__name__, bad))
    assert bad > 0
