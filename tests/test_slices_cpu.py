"""Sliced progressive validation without a GPU: the host-side definitions of the library — the home
slot, the table of fixed-point row terms, the summary, the parameter checks — against the
restatement (tests/_slices_checker.py) with ==, and every refusal that needs no device."""
import math

import numpy as np
import pytest

from xflow_amd import capi

from . import _progress_checker as P
from . import _slices_checker as S

# splitmix64 from state 0: its first two outputs (public test vectors) are mix64(0) and
# mix64(0x9e3779b97f4a7c15)
MIX_0 = 0xE220A8397B1DCDAF
MIX_GOLDEN = 0x6E789E6AA1B965F4


def test_home_known_answers():
    assert S.mix64(0) == MIX_0 and S.mix64(0x9E3779B97F4A7C15) == MIX_GOLDEN
    for b in (2, 3, 16, 26):
        assert capi.slices_home(0, b) == MIX_0 >> (64 - b)
        assert capi.slices_home(0x9E3779B97F4A7C15, b) == MIX_GOLDEN >> (64 - b)
    assert capi.slices_home(0, 2) == 3 and capi.slices_home(0, 16) == 0xE220
    assert capi.slices_home(0x9E3779B97F4A7C15, 26) == 0x6E789E6AA1B965F4 >> 38


def test_home_against_the_restatement():
    rng = np.random.default_rng(7)
    keys = [0, 1, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1] + [int(k) for k in
                                                          rng.integers(0, 2 ** 63, 300) * 2 + 1]
    for b in (2, 5, 9, 16, 20, 26):
        for k in keys:
            h = capi.slices_home(k, b)
            assert h == S.home(k, b) and 0 <= h < 2 ** b
    # outside 2 .. 26 there is no table: 0
    assert capi.slices_home(12345, 1) == 0 and capi.slices_home(12345, 27) == 0
    assert capi.slices_home(12345, 64) == 0 and capi.slices_home(12345, -1) == 0


def test_terms_against_the_restatement():
    got, want = capi.slices_terms(), S.terms()
    assert got.dtype == want.dtype == np.uint32 and got.shape == want.shape == (P.RANKS,)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    # the edges: rank 0 (q = 0: the midpoint of [0, 2^-126 ...) rounds to 0), C (ln 2), 2C (25 ln 2)
    assert got[P.C] == int(round(math.log(2.0) * 2 ** 24))
    assert got[2 * P.C] == int(round(25 * math.log(2.0) * 2 ** 24))
    # (the largest term any bucket can have is -ln of the smallest denormal, < 104: 31 bits)
    assert got[0] == 0 and got.max() < 104 * 2 ** 24 < 2 ** 31
    assert np.all(np.diff(got[:2 * P.C // 2 + 1].astype(np.int64)) >= 0), "monotone up to C"


CASES = {
    "both classes": [10, 5, 3 * 2 ** 30, 2 ** 31 + 12345, 7 * 2 ** 24 + 1, 9 * 2 ** 23, 2],
    "negatives only": [1000, 0, 123456789012, 0, 98765432101, 0, 0],
    "positives only": [0, 3, 0, 2 ** 31, 0, 3 * 11629080, 0],
    "no rows": [0, 0, 0, 0, 0, 0, 0],
    "other only": [0, 0, 0, 0, 0, 0, 41],
    "large": [2 ** 40 + 3, 2 ** 39 + 1, (2 ** 40 + 3) * 2 ** 23 - 5, 2 ** 63 + 12345,
              2 ** 62 + 7, 2 ** 61 + 9, 2 ** 33],
}


@pytest.mark.parametrize("w", [1.0, 4.0, float(np.float32(1) / np.float32(0.3))])
@pytest.mark.parametrize("case", sorted(CASES))
def test_summary_against_python_ints(case, w):
    words = CASES[case]
    got = capi.slices_summary(np.array(words, np.uint64), w)
    S.same(got, S.summary(words, w))
    n0, n1 = words[0], words[1]
    if n0 == 0 and n1 == 0:
        assert all(math.isnan(got[k]) for k in ("ctr", "pctr", "logloss")) and got["rows"] == 0
        assert got["other"] == words[6]
    else:
        assert got["rows"] == n1 + float(np.float32(w)) * n0
        assert 0.0 <= got["ctr"] <= 1.0 and 0.0 <= got["pctr"] <= 1.0
    if case == "positives only":
        # q sums to 2^31 over 3 rows: p = 1 - 1/3 a row; w plays no part
        assert got["ctr"] == 1.0 and got["pctr"] == (3 * 2 ** 31 - 2 ** 31) / 2.0 ** 31 / 3.0
        assert got["logloss"] == (3 * 11629080) / 2.0 ** 24 / 3.0
    assert got["logloss_bound"] == P.LOGLOSS_BOUND + 2.0 ** -25 and got["pctr_bound"] == 2.0 ** -31


def test_summary_of_rows_equals_the_weighted_mean():
    """the fixed-point sums stand for what they say: pctr within 2^-31 a row of the weighted mean
    of the rows' p, logloss within the bound of the mean of -log1p(-q)"""
    rng = np.random.default_rng(11)
    p = (1.0 / (1.0 + np.exp(-rng.normal(0, 3, size=5000)))).astype(np.float32)
    y = (rng.random(5000) < 0.3).astype(np.int32)
    loss = (p - y.astype(np.float32)).astype(np.float32)
    for w in (1.0, 4.0):
        words = S.total(S.words_of(loss, y, np.zeros(5000, np.uint64)))
        got = capi.slices_summary(np.array(words, np.uint64), w)
        wt = np.where(y != 0, 1.0, w)
        q = np.abs(loss).astype(np.float64)
        pr = np.where(y != 0, 1.0 - q, q)
        # (+ 1e-15: the fp64 rounding of numpy's own sum of 5000 terms below 1)
        assert abs(got["pctr"] - float((wt * pr).sum() / wt.sum())) <= got["pctr_bound"] + 1e-15
        ll = float((wt * -np.log1p(-q)).sum() / wt.sum())
        assert abs(got["logloss"] - ll) <= got["logloss_bound"]
        assert got["rows"] == float((y != 0).sum()) + w * float((y == 0).sum())


def test_refusals_without_a_device():
    for field, b, piece in [(-1, 16, "field id"), (2 ** 31, 16, "field id"), (3, 1, "2^b"),
                            (3, 27, "2^b"), (3, -5, "2^b"), (2 ** 40, 16, "field id")]:
        with pytest.raises(capi.XFError) as e:
            capi.slices_check(field, b)
        assert piece in str(e.value), str(e.value)
    for field, b in [(0, 2), (2 ** 31 - 1, 26), (7, 16)]:
        capi.slices_check(field, b)
    words = np.array(CASES["both classes"], np.uint64)
    for w in (0.5, float("nan"), float("inf"), -1.0):
        with pytest.raises(capi.XFError) as e:
            capi.slices_summary(words, w)
        assert "weight" in str(e.value)
    with pytest.raises(capi.XFError) as e:     # qsum1 beyond what n1 rows can hold
        capi.slices_summary(np.array([0, 1, 0, 2 ** 31 + 1, 0, 0, 0], np.uint64), 1.0)
    assert "qsum[1]" in str(e.value)
    assert capi.lib().xf_slices_summary(None, 1.0, None) != 0
    assert capi.lib().xf_slices_terms(None) != 0


# ------------------------------------------------------------------ the worker's parameters
def _start(**params):
    """XFStartTrain through the C ABI itself (capi.XFlow.train asks for a GPU first): -> (rc,
    xf_last_error)"""
    import ctypes as C
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode()


WORKER_REFUSALS = [
    (dict(progress_by=3), "progress=0"),
    (dict(progress_by=3, progress=0), "progress=0"),
    (dict(progress_by=3, progress=1, ingest="gpu"), "ingest=gpu"),
    (dict(progress_by=3, progress=1, core_num=2), "core_num=1"),
    (dict(progress_by=3, progress=1, key_build="host"), "key_build=host"),
    (dict(progress_by=3, progress=1, parity="reference_order"), "parity=reference_order"),
    (dict(progress_by=-1, progress=1), "progress_by must be a field id"),
    (dict(progress_by=2 ** 31, progress=1), "progress_by must be a field id"),
    (dict(progress_by=3, progress=1, progress_slots=1), "progress_slots must be in 2 .. 26"),
    (dict(progress_by=3, progress=1, progress_slots=27), "progress_slots must be in 2 .. 26"),
    (dict(progress_by=3, progress=1, progress_top=-1), "progress_top"),
    (dict(progress_by=3, progress=1, world=2, schedule="owner"), "schedule=owner"),
    (dict(progress_by=3, progress=1, world=2, schedule="owner_stale1"), "schedule=owner"),
]


@pytest.mark.parametrize("params,piece", WORKER_REFUSALS,
                         ids=["%d" % i for i in range(len(WORKER_REFUSALS))])
def test_worker_refusals_before_any_rendezvous(params, piece):
    rc, msg = _start(**params)
    assert rc != 0 and piece in msg and "XFStartTrain" in msg, msg
    if "progress_by" in msg:
        assert "progress_by=%d" % params["progress_by"] in msg or "progress_by must" in msg


def test_worker_parameters():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test")
    x.set("progress_by", 0)
    x.set("progress_by", 2 ** 31 - 1)
    x.set("progress_slots", 2)
    x.set("progress_top", 0)
    x.set("progress_slices_out", "/tmp/slices.tsv")
    with pytest.raises(capi.XFError, match="progress_by must be a field id"):
        x.set("progress_by", "site")
    with pytest.raises(capi.XFError):           # nothing has been summarised
        x.metric("slices")
