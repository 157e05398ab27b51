"""Held-out validation without a GPU: the library's held decision against the numpy restatement
(tests/_holdout_checker.py), the restatement against a loop in plain Python and against the
binomial bound, its independence from the negative sampler's decision, the stop rule on
hand-written curves, and every refusal of the worker and of the C ABI that needs no device."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from xflow_amd import capi

from . import _holdout_checker as H
from . import _negsample_checker as N

MASK = (1 << 64) - 1
SHARES = (0.0, 2.0 ** -32, 0.001, 0.25, 0.5, 1.0 - 2.0 ** -24)
SEEDS = (0, 12345, 0xfedcba9876543210)
STREAMS = (0, 3)
NAN = float("nan")


def _ordinals(n, rng):
    """n ordinals: a run straddling 2^32, a run at the wrap of 2^64, random ones"""
    a = (1 << 32) - n // 4 + np.arange(n // 2, dtype=np.uint64)
    b = np.array([(MASK - 5 + i) & MASK for i in range(16)], np.uint64)
    c = rng.randint(0, 1 << 62, size=n - len(a) - len(b)).astype(np.uint64) * np.uint64(4) + \
        np.uint64(3)
    return np.concatenate([a, b, c])


# ------------------------------------------------------------------ the decision
@pytest.mark.parametrize("share", SHARES, ids=["%.9g" % s for s in SHARES])
def test_held_decision_equals_the_restatement(share):
    rng = np.random.RandomState(7)
    ords = _ordinals(10000, rng)
    assert len(ords) == 10000 and (ords < (1 << 32)).any() and (ords >= (1 << 32)).any()
    f = capi.lib().xf_holdout_held
    for seed in SEEDS:
        for stream in STREAMS:
            want = H.held(seed, stream, ords, share)
            got = np.array([f(seed, stream, int(o), share) for o in ords], bool)
            assert np.array_equal(got, want), (share, seed, stream)
            if share == 0.0:
                assert not got.any()
            if share == 1.0 - 2.0 ** -24:
                assert got.mean() > 0.999
    assert capi.holdout_held(SEEDS[2], 3, MASK, share) == bool(H.held(SEEDS[2], 3, [MASK], share)[0])


def test_share_outside_its_range_holds_nothing():
    for share in (-0.5, 1.0, 1.5, NAN):
        assert not any(capi.holdout_held(0, 0, o, share) for o in range(64))


def test_the_salt_is_the_headers():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "xflow_amd.h")).read()
    assert "#define XF_HOLDOUT_SALT 0x%xull" % H.SALT in src


# ------------------------------------------------------------------ the restatement itself
def _py_mix64(x):
    x = (x + 0x9e3779b97f4a7c15) & MASK
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def _py_held(seed, stream, ordinal, T):
    return (_py_mix64((_py_mix64(seed ^ stream ^ H.SALT) + ordinal) & MASK) >> 32) < T


def test_restatement_against_a_plain_loop():
    rng = np.random.RandomState(5)
    seed, stream, first = 77, 3, (1 << 32) - 20
    R = 60
    lens = rng.randint(0, 4, size=R)
    lens[[0, 1, 30, R - 1]] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nnz = int(rowptr[-1])
    keys = rng.randint(0, 1 << 40, size=nnz).astype(np.uint64)
    fgid = rng.randint(0, 5, size=nnz).astype(np.int32)
    vals = rng.rand(nnz).astype(np.float32)
    labels = (rng.rand(R) < 0.2).astype(np.int32)
    for share in (0.0, 0.25, 0.5):
        T = int(np.float64(np.float32(share)) * 2 ** 32)
        assert T == H.threshold(share)
        sp = H.Splitter(share, seed)
        parts = sp.split(stream, first, rowptr, keys, labels, fgid, vals)
        want = [([0], [], [], [], []), ([0], [], [], [], [])]
        for r in range(R):
            brp, bks, blb, bfg, bvs = want[1 if _py_held(seed, stream, (first + r) & MASK, T) else 0]
            for i in range(int(rowptr[r]), int(rowptr[r + 1])):
                bks.append(int(keys[i]))
                bfg.append(int(fgid[i]))
                bvs.append(vals[i])
            brp.append(len(bks))
            blb.append(int(labels[r]))
        for (rp, ks, lb, fg, vs), (brp, bks, blb, bfg, bvs) in zip(parts, want):
            assert rp.tolist() == brp and ks.tolist() == bks and lb.tolist() == blb
            assert fg.tolist() == bfg and vs.tolist() == bvs
        assert sp.stats() == (R, len(want[1][2]), len(want[1][1]))
        if share == 0.0:
            assert len(parts[1][2]) == 0 and np.array_equal(parts[0][1], keys)
        else:
            assert 0 < sp.rows_held < R


def test_held_share_of_a_million_ordinals():
    """n = 10^6 consecutive ordinals at share = 0.25: the held count is Binomial(n, p) with p =
    T / 2^32 for a hash that mixes, so the share lies within 5 sigma = 5 sqrt(r (1 - r) / n) =
    0.00217 of p — derived, not measured"""
    n, r = 10 ** 6, 0.25
    p = H.threshold(r) / 2.0 ** 32
    assert p == 0.25
    bound = 5 * np.sqrt(r * (1 - r) / n)
    ords = np.arange(n, dtype=np.uint64)
    for seed, stream in ((0, 0), (12345, 1)):
        share = H.held(seed, stream, ords, r).mean()
        assert abs(share - p) <= bound, (seed, stream, share)


def test_independent_of_the_negative_samplers_decision():
    """kept AND held at keep = share = 0.5 on the same seed and stream: Binomial(n, 0.25) for
    independent decisions — within 5 sigma = 5 sqrt(0.25 * 0.75 / n); without the salt the two
    hashes are one and the joint share is 0.5"""
    n = 10 ** 6
    bound = 5 * np.sqrt(0.25 * 0.75 / n)
    ords = np.arange(n, dtype=np.uint64)
    for seed, stream in ((0, 0), (12345, 1)):
        kept = N.keep_negative(seed, stream, ords, 0.5)
        held = H.held(seed, stream, ords, 0.5)
        assert abs((kept & held).mean() - 0.25) <= bound, (seed, stream)
        lib = np.array([capi.negsample_keep(seed, stream, o, 0.5) and
                        capi.holdout_held(seed, stream, o, 0.5) for o in range(4000)])
        assert np.array_equal(lib, (kept & held)[:4000])


# ------------------------------------------------------------------ the stop rule
CURVES = [
    # (curve, patience, delta, stop, best)
    ([0.5, 0.4, 0.3, 0.2], 1, 0.0, False, 3),           # strict improvement throughout
    ([0.5, 0.4, 0.41], 1, 0.0, True, 1),                # one epoch worse, P = 1
    ([0.5, 0.4, 0.41], 2, 0.0, False, 1),               # ... P = 2 waits
    ([0.5, 0.4, 0.41, 0.42], 2, 0.0, True, 1),
    ([0.5, 0.4, 0.4], 1, 0.0, True, 1),                 # a tie is no improvement
    ([0.5, 0.4, 0.41, 0.39], 2, 0.0, False, 3),         # improves in time
    ([0.5, 0.45], 1, 0.1, True, 0),                     # delta: 0.45 is not below 0.5 - 0.1
    ([0.5, 0.39], 1, 0.1, False, 1),
    ([0.5, 0.4], 1, 0.1, True, 0),                      # exactly best - delta: no improvement
    ([0.5, NAN], 1, 0.0, False, 0),                     # a NaN never stops ...
    ([0.5, NAN, NAN, NAN], 1, 0.0, False, 0),
    ([0.5, NAN, 0.6], 1, 0.0, True, 0),                 # ... and never improves
    ([0.5, NAN, 0.4], 1, 0.0, False, 2),
    ([0.5, 0.6, NAN], 1, 0.0, False, 0),                # (the decision at a NaN epoch is no)
    ([NAN, NAN], 1, 0.0, False, -1),
    ([0.5], 1, 0.0, False, 0),                          # n < P + 1: nothing to compare
    ([0.5, 0.6], 3, 0.0, False, 0),                     # n < P
    ([0.5, 0.6, 0.7, 0.8], 0, 0.0, False, 0),           # P = 0: off
    ([], 1, 0.0, False, -1),
]


@pytest.mark.parametrize("curve,patience,delta,stop,best", CURVES,
                         ids=["%d" % i for i in range(len(CURVES))])
def test_stop_rule(curve, patience, delta, stop, best):
    assert capi.holdout_should_stop(curve, patience, delta) == (stop, best)
    assert H.should_stop(curve, patience, delta) == (stop, best)


def test_stop_rule_on_random_curves_equals_the_restatement():
    rng = np.random.RandomState(3)
    for _ in range(300):
        n = rng.randint(0, 9)
        curve = np.round(rng.rand(n), 1)
        curve[rng.rand(n) < 0.15] = np.nan
        P, d = int(rng.randint(0, 4)), float(rng.choice([0.0, 0.1]))
        assert capi.holdout_should_stop(curve, P, d) == H.should_stop(curve.tolist(), P, d)


def test_stop_rule_refuses_quietly():
    f = capi.lib().xf_holdout_should_stop
    best = C.c_int(7)
    one = (C.c_double * 1)(0.5)
    assert f(None, 3, 1, 0.0, C.byref(best)) == 0 and best.value == -1
    assert f(one, 1, 1, -0.1, C.byref(best)) == 0 and best.value == -1
    assert f(one, 1, 1, NAN, C.byref(best)) == 0 and best.value == -1
    assert f(one, 1, 1, 0.0, None) == 0


# ------------------------------------------------------------------ refusals without a device
@pytest.mark.parametrize("share", [-0.25, 1.0, 1.5, NAN, float("inf")])
def test_split_refuses_a_share_outside_its_range(share):
    with pytest.raises(capi.XFError) as e:
        capi.Holdout(share)
    assert "holdout" in str(e.value) and "xf_holdout_create" in str(e.value)


def test_the_object_needs_no_device_until_its_first_split():
    s = capi.Holdout(0.25, seed=3)
    assert s.params() == (0.25, 3) and s.stats() == (0, 0, 0)
    assert capi.holdout_shape()["tile"] == 256
    lib = capi.lib()
    assert lib.xf_sharded_holdout(None, 1) == 1 and b"xf_sharded_holdout" in lib.xf_last_error()
    assert lib.xf_sharded_validate(None, None) == 1
    assert b"xf_sharded_validate" in lib.xf_last_error()
    assert lib.xf_lr_validate(None, None, None, None) == 1
    assert b"xf_lr_validate" in lib.xf_last_error()
    assert lib.xf_fm_validate(None, None, None, None, None) == 1
    assert b"xf_fm_validate" in lib.xf_last_error()


def _start(**params):
    """XFStartTrain through the C ABI itself (capi.XFlow.train asks for a GPU first)"""
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode(), x


REFUSALS = [
    (dict(holdout=1), ["holdout", "[0, 1)"]),
    (dict(holdout=-0.5), ["holdout", "[0, 1)"]),
    (dict(holdout=1.25), ["holdout", "1.25"]),
    (dict(holdout="nan"), ["holdout", "[0, 1)"]),
    (dict(holdout=0.25, holdout_every=0), ["holdout_every"]),
    (dict(holdout=0.25, early_stop=-1), ["early_stop"]),
    (dict(holdout=0.25, early_stop=1, early_stop_delta=-0.1), ["early_stop_delta"]),
    (dict(early_stop=2), ["early_stop=2", "without holdout"]),
    (dict(holdout=0.25, core_num=2), ["holdout", "core_num"]),
    (dict(holdout=0.25, key_build="host"), ["holdout", "key_build"]),
    (dict(holdout=0.25, parity="reference_order"), ["holdout", "parity"]),
    (dict(holdout=0.25, world=2, schedule="owner"), ["holdout", "schedule=owner", "world 2"]),
    (dict(holdout=0.25, world=2, schedule="owner_stale1"), ["holdout", "owner_stale1"]),
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


def test_holdout_zero_creates_nothing():
    """holdout=0: the start gets past the holdout checks whatever else is set (and fails on the
    missing GPU or the missing file); no metric exists"""
    rc, msg, x = _start(holdout=0, core_num=2, world=1)
    assert rc != 0
    assert "holdout" not in msg, msg
    assert x.metric("epochs_run") == 0
    with pytest.raises(capi.XFError, match="no epoch has been validated"):
        x.metric("holdout_logloss")
