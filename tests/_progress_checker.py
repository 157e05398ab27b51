"""The numpy / Python-int restatement of progressive validation (include/xflow_amd.h, "progressive
validation"): the rank of a loss, the counts of a minibatch, the summary of the counts.  Written
from the header's text, not from the library's code: the tests compare the two with ==."""
import math

import numpy as np

MANT = 10
SH = 23 - MANT
C = 0x3F000000 >> SH                 # bits(0.5f) >> SH
RANKS = 2 * C + 1
LOGLOSS_BOUND = -math.log(1.0 - 2.0 ** -(MANT + 1))

# the issue's edge values of q and their ranks
EDGES = [(0.0, 0), (float(np.float32(1e-45)), 0), (2.0 ** -126, 1024), (2.0 ** -24, 105472),
         (0.25, 128000), (float(np.nextafter(np.float32(0.5), np.float32(0))), 129023),
         (0.5, 129024), (float(np.nextafter(np.float32(0.5), np.float32(1))), 129025),
         (1.0 - 2.0 ** -24, 152576), (1.0, 258048)]


def ranks(loss):
    """rank of every loss (float32 array): 0 .. 2C, RANKS for NaN and |loss| > 1"""
    loss = np.ascontiguousarray(loss, dtype=np.float32)
    q = np.abs(loss)
    ok = q <= np.float32(1.0)                      # (False for NaN)
    qs = np.where(ok, q, np.float32(0))
    low = qs < np.float32(0.5)
    m = (np.float32(1.0) - qs).astype(np.float32)  # exact for q >= 0.5
    r_low = (qs.view(np.uint32) >> SH).astype(np.int64)
    r_high = 2 * C - (m.view(np.uint32) >> SH).astype(np.int64)
    r = np.where(low, r_low, r_high)
    return np.where(ok, r, RANKS)


def counts_of(loss, labels):
    """(counts [2, RANKS] uint64, other [2] uint64) of one minibatch; class 1 = label != 0"""
    r = ranks(loss)
    cls = (np.asarray(labels) != 0).astype(np.int64)
    counts = np.zeros((2, RANKS), np.uint64)
    other = np.zeros(2, np.uint64)
    part = r < RANKS
    np.add.at(counts, (cls[part], r[part]), np.uint64(1))
    np.add.at(other, cls[~part], np.uint64(1))
    return counts, other


def _edge(r):
    return float(np.array([r << SH], np.uint32).view(np.float32)[0])


def bucket_m(rank):
    """the bucket's representative: of q below C, of 1 - q above"""
    if rank == C:
        return 0.5
    if rank == 2 * C:
        return 2.0 ** -25
    r = rank if rank < C else 2 * C - rank
    return 0.5 * (_edge(r) + _edge(r + 1))


def summary(counts, other, w=1.0):
    """the metrics from the counts: sums per class by ascending rank, sum += float(count) * term;
    the AUC's U2 in Python ints"""
    w = float(np.float32(w))
    neg = [int(x) for x in counts[0]]
    pos = [int(x) for x in counts[1]]
    P = N = 0
    loss_pos = loss_neg = p_pos = p_neg = 0.0
    for r in np.flatnonzero((counts[0] != 0) | (counts[1] != 0)):
        r = int(r)
        m = bucket_m(r)
        term = -math.log1p(-m) if r < C else -math.log(m)
        q = m if r < C else 1.0 - m
        pq = 1.0 - m if r < C else m
        P += pos[r]
        N += neg[r]
        loss_pos += float(pos[r]) * term
        loss_neg += float(neg[r]) * term
        p_pos += float(pos[r]) * pq
        p_neg += float(neg[r]) * q
    U2 = T2 = below = 0
    for s in range(RANKS):
        ps, ns = pos[2 * C - s], neg[s]
        if ps:
            U2 += ps * (2 * below + ns)
            T2 += ps * ns
        below += ns
    nan = float("nan")
    rows = float(P) + w * float(N)
    any_, both = (P or N) != 0, P != 0 and N != 0
    out = {
        "rows_pos": float(P), "rows_neg": w * float(N),
        "saturated": float(pos[2 * C]) + w * float(neg[2 * C]),
        "other": float(int(other[1])) + w * float(int(other[0])),
        "logloss_bound": LOGLOSS_BOUND,
        "logloss": (loss_pos + w * loss_neg) / rows if any_ else nan,
        "ctr": float(P) / rows if any_ else nan,
        "pctr": (p_pos + w * p_neg) / rows if any_ else nan,
        "auc": float(U2) / float(2 * P * N) if both else nan,
        "auc_slack": float(T2) / float(2 * P * N) if both else (0.0 if any_ else nan),
    }
    return out


def same(a, b):
    """two summaries equal field for field (NaN == NaN)"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert (math.isnan(x) and math.isnan(y)) or x == y, (k, x, y)
    return True
