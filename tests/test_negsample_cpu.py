"""Negative subsampling without a GPU: the library's keep decision against the numpy restatement
(tests/_negsample_checker.py), the restatement against a loop in plain Python and against the
binomial bound, the weight bit for bit, and every refusal of the worker and of the setters that
needs no device."""
import ctypes as C
import time

import numpy as np
import pytest

from xflow_amd import capi

from . import _negsample_checker as N

MASK = (1 << 64) - 1
KEEPS = (2.0 ** -32, 0.001, 0.25, 0.5, 0.999, 1.0)
SEEDS = (0, 12345, 0xfedcba9876543210)
STREAMS = (0, (3 << 32) | 1)


def _ordinals(n, rng):
    """n ordinals: a run straddling 2^32, a run at the wrap of 2^64, random ones"""
    a = (1 << 32) - n // 4 + np.arange(n // 2, dtype=np.uint64)
    b = np.array([(MASK - 5 + i) & MASK for i in range(16)], np.uint64)
    c = rng.randint(0, 1 << 62, size=n - len(a) - len(b)).astype(np.uint64) * np.uint64(4) + \
        np.uint64(3)
    return np.concatenate([a, b, c])


# ------------------------------------------------------------------ the decision
@pytest.mark.parametrize("keep", KEEPS, ids=["%g" % k for k in KEEPS])
def test_keep_decision_equals_the_restatement(keep):
    rng = np.random.RandomState(7)
    ords = _ordinals(10000, rng)
    assert len(ords) == 10000 and (ords < (1 << 32)).any() and (ords >= (1 << 32)).any()
    f = capi.lib().xf_negsample_keep
    for seed in SEEDS:
        for stream in STREAMS:
            want = N.keep_negative(seed, stream, ords, keep)
            got = np.array([f(seed, stream, int(o), keep) for o in ords], bool)
            assert np.array_equal(got, want), (keep, seed, stream)
            if keep == 1.0:
                assert got.all()
            if keep == 2.0 ** -32:
                assert not got.all()


def test_keep_outside_its_range_keeps_nothing():
    for keep in (0.0, -0.5, 1.5, float("nan")):
        assert not capi.negsample_keep(0, 0, 1, keep)


# ------------------------------------------------------------------ the restatement itself
def _py_mix64(x):
    x = (x + 0x9e3779b97f4a7c15) & MASK
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def _py_keep(seed, stream, ordinal, T):
    return (_py_mix64((_py_mix64(seed ^ stream) + ordinal) & MASK) >> 32) < T


def test_restatement_against_a_plain_loop():
    rng = np.random.RandomState(5)
    seed, stream, first = 77, (2 << 32) | 3, (1 << 32) - 20
    R = 60
    lens = rng.randint(0, 4, size=R)
    lens[[0, 1, 30, R - 1]] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nnz = int(rowptr[-1])
    keys = rng.randint(0, 1 << 40, size=nnz).astype(np.uint64)
    fgid = rng.randint(0, 5, size=nnz).astype(np.int32)
    vals = rng.rand(nnz).astype(np.float32)
    labels = (rng.rand(R) < 0.2).astype(np.int32)
    for keep in (0.25, 0.5, 1.0):
        T = int(np.float64(np.float32(keep)) * 2 ** 32)
        assert T == N.threshold(keep)
        smp = N.Sampler(keep, seed)
        rp, ks, lb, fg, vs = smp.apply(stream, first, rowptr, keys, labels, fgid, vals)
        brp, bks, blb, bfg, bvs = [0], [], [], [], []
        for r in range(R):
            if labels[r] != 0 or _py_keep(seed, stream, (first + r) & MASK, T):
                for i in range(int(rowptr[r]), int(rowptr[r + 1])):
                    bks.append(int(keys[i]))
                    bfg.append(int(fgid[i]))
                    bvs.append(vals[i])
                brp.append(len(bks))
                blb.append(int(labels[r]))
        assert rp.tolist() == brp and ks.tolist() == bks and lb.tolist() == blb
        assert fg.tolist() == bfg and vs.tolist() == bvs
        assert smp.stats() == (R, len(blb), int((labels == 0).sum()),
                               len(blb) - int(labels.sum()))
        if keep == 1.0:
            assert np.array_equal(rp, rowptr.astype(np.uint32)) and np.array_equal(ks, keys)
        else:
            assert 0 < smp.neg_kept < smp.neg_seen


def test_kept_share_of_a_million_ordinals():
    """n = 10^6 consecutive ordinals at keep = 0.25: the kept count is Binomial(n, p) with p =
    T / 2^32 for a hash that mixes, so the share lies within 5 sigma = 5 sqrt(r (1 - r) / n) =
    0.00217 of p — derived, not measured"""
    n, r = 10 ** 6, 0.25
    p = N.threshold(r) / 2.0 ** 32
    assert p == 0.25
    bound = 5 * np.sqrt(r * (1 - r) / n)
    assert abs(bound - 0.0022) < 1e-4
    ords = np.arange(n, dtype=np.uint64)
    for seed, stream in ((0, 0), (12345, (1 << 32) | 1)):
        share = N.keep_negative(seed, stream, ords, r).mean()
        assert abs(share - p) <= bound, (seed, stream, share)


# ------------------------------------------------------------------ the weight
@pytest.mark.parametrize("keep", KEEPS, ids=["%g" % k for k in KEEPS])
def test_weight_is_one_fp32_division(keep):
    s = capi.NegSample(keep, seed=3)
    want = np.float32(1.0) / np.float32(keep)
    assert s.weight.view(np.uint32) == want.view(np.uint32)
    assert N.weight(keep).view(np.uint32) == want.view(np.uint32)
    got_keep, got_seed = s.params()
    assert np.float32(got_keep) == np.float32(keep) and got_seed == 3
    assert s.stats() == (0, 0, 0, 0)


# ------------------------------------------------------------------ refusals without a device
@pytest.mark.parametrize("keep", [0.0, -0.25, 1.5, float("nan"), float("inf")])
def test_sampler_refuses_a_keep_outside_its_range(keep):
    with pytest.raises(capi.XFError) as e:
        capi.NegSample(keep)
    assert "neg_keep" in str(e.value) and "xf_negsample_create" in str(e.value)


@pytest.mark.parametrize("weight", [0.5, 0.0, -4.0, float("nan"), float("inf")])
def test_setters_refuse_a_weight_below_one_or_not_finite(weight):
    ws = capi.Workspace()
    with pytest.raises(capi.XFError) as e:
        ws.neg_weight(weight)
    assert "xf_workspace_neg_weight" in str(e.value)
    ws.neg_weight(1.0)
    ws.neg_weight(4.0)
    assert capi.lib().xf_sharded_set_neg_weight(None, C.c_float(4.0)) == 1       # XF_EINVAL
    assert b"xf_sharded_set_neg_weight" in capi.lib().xf_last_error()


def _start(**params):
    """XFStartTrain through the C ABI itself (capi.XFlow.train asks for a GPU first)"""
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode(), x


def test_the_parameter_and_the_metrics_are_accepted():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test")
    for v in (0.25, 1, 0.001):
        x.set("neg_keep", v)
    assert x.metric("neg_seen") == 0 and x.metric("neg_kept") == 0 and x.metric("rows_kept") == 0


REFUSALS = [
    (dict(neg_keep=0), ["neg_keep", "(0, 1]"]),
    (dict(neg_keep=-0.5), ["neg_keep", "(0, 1]"]),
    (dict(neg_keep=1.25), ["neg_keep", "1.25"]),
    (dict(neg_keep="nan"), ["neg_keep", "(0, 1]"]),
    (dict(neg_keep=0.25, core_num=2), ["neg_keep", "core_num"]),
    (dict(neg_keep=0.25, key_build="host"), ["neg_keep", "key_build"]),
    (dict(neg_keep=0.25, parity="reference_order"), ["neg_keep", "parity"]),
    (dict(neg_keep=0.25, world=2, schedule="owner"), ["neg_keep", "schedule=owner", "world 2"]),
    (dict(neg_keep=0.25, world=2, schedule="owner_stale1"), ["neg_keep", "owner_stale1"]),
]


@pytest.mark.parametrize("params,words", REFUSALS, ids=[",".join("%s=%s" % kv for kv in p.items())
                                                        for p, _ in REFUSALS])
def test_refusals_name_their_parameter(params, words):
    t0 = time.time()
    rc, msg, _ = _start(**params)
    assert rc == 1, (rc, msg)                    # XF_EINVAL
    assert msg.startswith("XFStartTrain:")
    for w in words:
        assert w in msg, msg
    assert time.time() - t0 < 10                 # (before any rendezvous: nobody is waited for)


def test_keep_one_creates_nothing():
    """neg_keep=1: the start gets past the sampling checks whatever else is set (and fails on the
    missing GPU or the missing file); no sampler exists"""
    rc, msg, x = _start(neg_keep=1, core_num=2, world=1)
    assert rc != 0
    assert "neg_keep" not in msg, msg
    assert x.metric("neg_seen") == 0 and x.metric("rows_kept") == 0


# ------------------------------------------------------------------ the weighted checkers
def test_weighted_steps_with_weight_one_are_the_checkers_own_steps():
    """tests/_negsample_checker.py's weighted steps are each mode's checker cut between forward
    and gradient: with w = 1 they leave the stores the checker's own step leaves, bit for bit; with
    w = 4 they do not"""
    from oracle import pyoracle as O

    from . import _ffm_checker as FF
    from . import _fmc_checker as FC
    from . import _valued_cases as Cs
    from . import _valued_checker as V

    def same_stores(a, b, equal=True):
        eq = all(np.array_equal(np.asarray(x).view(np.uint32) if x.dtype == np.float32 else x,
                                np.asarray(y).view(np.uint32) if y.dtype == np.float32 else y)
                 for x, y in zip(a.export(), b.export()))
        assert eq == equal

    mbs = Cs.stream("ragged")
    binary = [(m[0], m[1], m[3]) for m in mbs]
    assert all((m[2] == 0).any() and (m[2] != 0).any() for m in binary)
    for w, equal in ((1.0, True), (4.0, False)):
        # binary LR and the reference-form FM: the oracle's exact-sum updates
        a, b = O.Store(O.OPT_FTRL, 1), O.Store(O.OPT_FTRL, 1)
        av, bv = (O.Store(O.OPT_FTRL, 4, O.INIT_HASHNORM, 0.0, 9) for _ in range(2))
        aw, bw = O.Store(O.OPT_FTRL, 1), O.Store(O.OPT_FTRL, 1)
        for mb in binary:
            N.lr_step(a, *mb, w)
            N.fm_step(aw, av, *mb, w)
            with O.sum_mode(1):
                O.lr_update(b, O.Batch(*mb))
                O.fm_update(bw, bv, O.Batch(*mb))
        same_stores(a, b, equal)
        same_stores(aw, bw, equal)
        same_stores(av, bv, equal)
        # canonical FM
        (aw, av), (bw, bv) = FC.stores(O.OPT_FTRL, 4, 3), FC.stores(O.OPT_FTRL, 4, 3)
        for mb in binary:
            N.fmc_step(aw, av, *mb, w)
            FC.step(bw, bv, *mb)
        same_stores(aw, bw, equal)
        same_stores(av, bv, equal)
        # valued LR and field-aware FM with values, from aged tables
        audit = []
        (aw, _), (bw, _) = Cs.stores("lr", "ftrl", 1, mbs), Cs.stores("lr", "ftrl", 1, mbs)
        for rp, ks, vs, lb in mbs:
            N.valued_lr_step(aw, rp, ks, vs, lb, w, audit)
            V.lr_step(bw, rp, ks, vs, lb, audit)
        same_stores(aw, bw, equal)
        fmbs = FF.stream("ragged", 3)
        (aw, av), (bw, bv) = FF.aged_stores("sgd", 3, 4, fmbs), FF.aged_stores("sgd", 3, 4, fmbs)
        for rp, ks, fg, vs, lb in fmbs:
            N.ffm_step(aw, av, 3, rp, ks, fg, vs, lb, w, audit)
            FF.step(bw, bv, 3, rp, ks, fg, vs, lb, audit)
        same_stores(aw, bw, equal)
        same_stores(av, bv, equal)
