"""Progressive validation without a GPU: the library's rank and summary (host code) against the
restatement (tests/_progress_checker.py), the rank's edge values, monotonicity and mirror identity,
the summary's bound and slack against exact fp64 figures on synthetic logistic rows, and the
refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

from xflow_amd import capi

from . import _progress_checker as P


def _lib_ranks(loss):
    f = capi.lib().xf_progress_rank
    return np.array([f(float(x)) for x in np.asarray(loss, np.float32)], np.int64)


def test_the_constants():
    assert capi.PROGRESS_RANKS == P.RANKS == 258049 and capi.PROGRESS_CENTER == P.C == 0x1F800


def test_rank_edges():
    for q, want in P.EDGES:
        for loss in (q, -q):                       # a negative's loss is p, a positive's p - 1
            assert capi.progress_rank(loss) == want, (q, loss)
            assert int(P.ranks([loss])[0]) == want, (q, loss)
    assert capi.progress_rank(-0.0) == 0
    for bad in (float("nan"), 1.0000001, -1.0000001, 2.0, -3.5, float("inf"), float("-inf")):
        assert capi.progress_rank(bad) == P.RANKS
        assert int(P.ranks([bad])[0]) == P.RANKS


def test_rank_on_random_patterns():
    rng = np.random.default_rng(7)
    # fp32 bit patterns of [0, 1]: 0 .. bits(1.0f), with both signs
    bits = rng.integers(0, 0x3F800000 + 1, size=100_000, dtype=np.uint64).astype(np.uint32)
    bits |= rng.integers(0, 2, size=bits.size, dtype=np.uint64).astype(np.uint32) << np.uint32(31)
    loss = bits.view(np.float32)
    got, want = _lib_ranks(loss), P.ranks(loss)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() <= 2 * P.C
    # uniform values too (the patterns above are mostly tiny numbers)
    u = rng.random(20_000).astype(np.float32)
    assert np.array_equal(_lib_ranks(u), P.ranks(u))


def test_rank_is_monotone_and_mirrored():
    rng = np.random.default_rng(8)
    q = np.sort(np.concatenate([
        rng.integers(0, 0x3F800000 + 1, size=50_000, dtype=np.uint64).astype(np.uint32)
        .view(np.float32), rng.random(50_000).astype(np.float32),
        np.array([e[0] for e in P.EDGES], np.float32)]))
    r = _lib_ranks(q)
    assert np.all(np.diff(r) >= 0)
    # rank(1 - q) = 2C - rank(q) wherever 1 - q is exact
    one_minus = (np.float32(1) - q).astype(np.float32)
    q64, m64 = q.astype(np.float64), one_minus.astype(np.float64)
    exact = (m64 == 1.0 - q64) & (q64 == 1.0 - m64)   # (a tiny q rounded away fails the second)
    assert exact.sum() > 20_000
    assert np.array_equal(_lib_ranks(one_minus[exact]), 2 * P.C - r[exact])


def _crafted():
    rng = np.random.default_rng(9)
    out = {}
    z = np.zeros((2, P.RANKS), np.uint64)
    out["empty"] = (z.copy(), np.zeros(2, np.uint64))
    c = z.copy()
    c[1, [0, 5, P.C, 2 * P.C]] = [3, 1, 4, 2]
    out["positives_only"] = (c, np.array([0, 2], np.uint64))
    c = z.copy()
    c[0, [7, P.C - 1, P.C + 1]] = [1, 1, 9]
    out["negatives_only"] = (c, np.array([1, 0], np.uint64))
    c = z.copy()
    c[0, P.C] = 40
    c[1, P.C] = 24
    out["all_at_C"] = (c, np.zeros(2, np.uint64))
    c = z.copy()
    idx = rng.integers(0, P.RANKS, size=3000)
    c[0, idx] += rng.integers(1, 1000, size=3000).astype(np.uint64)
    idx = rng.integers(0, P.RANKS, size=3000)
    c[1, idx] += rng.integers(1, 50, size=3000).astype(np.uint64)
    c[:, 2 * P.C] += np.uint64(5)
    c[:, 0] += np.uint64(6)
    out["random"] = (c, np.array([3, 4], np.uint64))
    c = z.copy()                                   # U2 needs more than 64 bits
    c[0, [100, 129000, 200000]] = [1 << 40, (1 << 40) + 12345, 1 << 39]
    c[1, [2 * P.C - 100, 129500, 150000]] = [(1 << 40) + 7, 1 << 38, (1 << 40) - 1]
    out["near_2^40"] = (c, np.array([1 << 41, 1], np.uint64))
    return out


CRAFTED = _crafted()


@pytest.mark.parametrize("name", list(CRAFTED))
@pytest.mark.parametrize("w", [1.0, 4.0, float(np.float32(1) / np.float32(0.3))],
                         ids=["w1", "w4", "w1/0.3"])
def test_summary_against_the_restatement(name, w):
    counts, other = CRAFTED[name]
    got = capi.progress_summary(counts, other, w)
    assert P.same(got, P.summary(counts, other, w))
    if name == "empty":
        for k in ("logloss", "auc", "ctr", "pctr"):
            assert math.isnan(got[k])
        assert got["rows_pos"] == 0 and got["rows_neg"] == 0
    if name in ("positives_only", "negatives_only"):
        assert math.isnan(got["auc"])
        assert not any(math.isnan(v) for k, v in got.items() if k != "auc")
    if name == "all_at_C":
        assert got["logloss"] == math.log(2.0) and got["auc"] == 0.5 and got["auc_slack"] == 0.5
        assert got["pctr"] == 0.5
    if name == "near_2^40":
        assert 0.0 < got["auc"] < 1.0


def test_summary_refuses_a_bad_weight():
    counts, other = CRAFTED["random"]
    for w in (0.5, float("nan"), float("inf")):
        with pytest.raises(capi.XFError) as e:
            capi.progress_summary(counts, other, w)
        assert "xf_progress_summary" in str(e.value)


def _exact_auc(p, y):
    """the tie-aware rank AUC of scores p: (sum of the positives' average ranks - P(P+1)/2) / PN"""
    order = np.argsort(p, kind="stable")
    ps = p[order]
    _, first, cnt = np.unique(ps, return_index=True, return_counts=True)
    avg = np.repeat(first + (cnt + 1) / 2.0, cnt)     # 1-based average rank of each tie group
    ranks = np.empty(len(p))
    ranks[order] = avg
    npos = int(y.sum())
    nneg = len(y) - npos
    return (ranks[y != 0].sum() - npos * (npos + 1) / 2.0) / (npos * nneg)


def test_bound_and_slack_on_logistic_rows():
    rng = np.random.default_rng(10)
    n = 200_000
    logit = rng.normal(0.0, 6.0, size=n)
    p = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)      # what a forward would store
    y = (rng.random(n) < p).astype(np.int32)
    loss = (p - y.astype(np.float32)).astype(np.float32)        # sigmoid - label, in fp32
    counts, other = P.counts_of(loss, y)
    assert other.sum() == 0
    m = capi.progress_summary(counts, other, 1.0)
    assert m["rows_pos"] + m["rows_neg"] == n
    assert m["auc_slack"] < 1e-3, m["auc_slack"]
    # logloss: against the exact fp64 mean of -log1p(-q) over the rows outside the saturated bucket
    q = np.abs(loss).astype(np.float64)
    r = P.ranks(loss)
    unsat = r != 2 * P.C
    exact = -np.log1p(-q[unsat])
    sat_term = -math.log(2.0 ** -25) * (~unsat).sum()
    ours_unsat = (m["logloss"] * n - sat_term) / unsat.sum()
    print("logloss", m["logloss"], "unsaturated mean", ours_unsat, "exact", exact.mean(),
          "bound", m["logloss_bound"], "saturated rows", int((~unsat).sum()))
    assert abs(ours_unsat - exact.mean()) <= m["logloss_bound"]
    # auc: the score whose ties the contract speaks of is p as the loss carries it: q for a
    # negative, 1 - q (exact or the stored fl(1 - p)'s mirror) for a positive
    score = np.where(y != 0, 1.0 - q, q)
    exact_auc = _exact_auc(score, y)
    print("auc", m["auc"], "exact", exact_auc, "slack", m["auc_slack"])
    assert abs(m["auc"] - exact_auc) <= m["auc_slack"]
    assert abs(m["ctr"] - y.mean()) < 1e-12
    assert abs(m["pctr"] - p.astype(np.float64).mean()) < 1e-3


# ------------------------------------------------------------------ refusals that need no device
def _start(**params):
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode(), x


def test_the_parameter_is_accepted_and_checked():
    capi.XFlow("/nonexistent/train", "/nonexistent/test", progress=1)
    capi.XFlow("/nonexistent/train", "/nonexistent/test", progress=0)
    with pytest.raises(capi.XFError) as e:
        capi.XFlow("/nonexistent/train", "/nonexistent/test", progress=2)
    assert "progress must be 0 or 1" in str(e.value)


def test_metrics_before_training_are_refused_by_name():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", progress=1)
    for name in ("progress_logloss", "progress_auc_first"):
        with pytest.raises(capi.XFError) as e:
            x.metric(name)
        assert name in str(e.value)


@pytest.mark.parametrize("schedule", ["owner", "owner_stale1"])
def test_owner_schedules_on_several_workers_are_refused_before_any_rendezvous(schedule):
    """world=2 with nobody to meet: the refusal returns at once instead of waiting for a peer"""
    rc, msg, _ = _start(progress=1, schedule=schedule, world=2, rank=0)
    assert rc != 0 and "progress=1" in msg and "owner" in msg, msg


def test_null_arguments_are_refused():
    L = capi.lib()
    assert L.xf_progress_create(None) != 0 and "xf_progress_create" in L.xf_last_error().decode()
    assert L.xf_progress_summary(None, None, 1.0, None) != 0
    assert L.xf_progress_read(None, None, None, 0) != 0
    assert L.xf_progress_accumulate_dev(None, None, None, 0, None) != 0
    assert L.xf_workspace_progress(None, None) != 0
    assert L.xf_sharded_progress(None, 1) != 0
    assert L.xf_progress_destroy(None) == 0
