"""The numpy / Python-int restatement of the grouped AUC (include/xflow_amd.h, "grouped AUC,
held-out"): the code of a row's record, the figures of the groups, the summary.  Written from the
header's text, not from the library's code: the tests compare the two with ==."""
import math

import numpy as np

from . import _progress_checker as pchk

C = pchk.C
OTHER = 2**32 - 1
NONE = 2**64 - 1
CODE_MAX = ((2 * C) << 1) | 1
WORDS = 4


def codes(loss, labels):
    """the code of every row (uint32 array): (score << 1) | pos, OTHER for NaN and |loss| > 1"""
    r = pchk.ranks(loss)
    pos = (np.asarray(labels) != 0).astype(np.int64)
    score = np.where(pos == 1, 2 * C - r, r)
    return np.where(r == pchk.RANKS, OTHER, (score << 1) | pos).astype(np.uint32)


def records(loss, labels, ids):
    """(ids, codes) of the rows that leave a record, none [2], other [2]"""
    c = codes(loss, labels)
    ids = np.asarray(ids, dtype=np.uint64)
    pos = (np.asarray(labels) != 0).astype(np.int64)
    is_other = c == OTHER
    is_none = ~is_other & (ids == np.uint64(NONE))
    keep = ~is_other & ~is_none
    none = np.array([np.sum(is_none & (pos == q)) for q in (0, 1)], np.uint64)
    other = np.array([np.sum(is_other & (pos == q)) for q in (0, 1)], np.uint64)
    return ids[keep], c[keep], none, other


def figures(ids, codes_):
    """(distinct ids ascending, [n, 4] = P, N, U2, T) by np.lexsort and Python ints"""
    ids = np.asarray(ids, dtype=np.uint64)
    codes_ = np.asarray(codes_, dtype=np.uint32)
    order = np.lexsort((codes_, ids))
    sid, sc = ids[order], codes_[order]
    out_ids, out = [], []
    i, n = 0, len(sid)
    while i < n:
        j = i
        while j < n and sid[j] == sid[i]:
            j += 1
        P = N = U2 = T = below = 0
        a = i
        while a < j:                      # one run of equal score at a time, ascending
            b = a
            score = int(sc[a]) >> 1
            while b < j and int(sc[b]) >> 1 == score:
                b += 1
            pos_b = int(np.sum(sc[a:b] & np.uint32(1)))
            neg_b = (b - a) - pos_b
            U2 += pos_b * (2 * below + neg_b)
            T += pos_b * neg_b
            P += pos_b
            N += neg_b
            below += neg_b
            a = b
        out_ids.append(int(sid[i]))
        out.append((P, N, U2, T))
        i = j
    return (np.array(out_ids, np.uint64),
            np.array(out, np.uint64).reshape(-1, WORDS))


def figures_fast(ids, codes_):
    """the same figures vectorised (for the tests' larger inputs); checked against figures() by
    the CPU tests"""
    ids = np.asarray(ids, dtype=np.uint64)
    codes_ = np.asarray(codes_, dtype=np.uint32)
    n = len(ids)
    if n == 0:
        return np.zeros(0, np.uint64), np.zeros((0, WORDS), np.uint64)
    order = np.lexsort((codes_, ids))
    sid, sc = ids[order], codes_[order].astype(np.int64)
    pos, score = sc & 1, sc >> 1
    ghead = np.ones(n, bool)
    ghead[1:] = sid[1:] != sid[:-1]
    rhead = ghead.copy()
    rhead[1:] |= score[1:] != score[:-1]
    grp = np.cumsum(ghead) - 1
    run = np.cumsum(rhead) - 1
    G, Rn = grp[-1] + 1, run[-1] + 1
    pos_b = np.bincount(run, weights=pos, minlength=Rn).astype(np.int64)
    cnt_b = np.bincount(run, minlength=Rn).astype(np.int64)
    neg_b = cnt_b - pos_b
    run_grp = grp[rhead]
    neg_cum = np.cumsum(neg_b) - neg_b                 # negatives in runs before, whole log
    g_first_run = np.flatnonzero(np.r_[True, run_grp[1:] != run_grp[:-1]])
    below = neg_cum - neg_cum[g_first_run][run_grp]    # (all < 2^31: int64 products are exact)
    out = np.zeros((G, WORDS), np.int64)
    np.add.at(out[:, 0], run_grp, pos_b)
    np.add.at(out[:, 1], run_grp, neg_b)
    np.add.at(out[:, 2], run_grp, pos_b * (2 * below + neg_b))
    np.add.at(out[:, 3], run_grp, pos_b * neg_b)
    return sid[ghead].copy(), out.astype(np.uint64)


def summary(ids, fig, none=(0, 0), other=(0, 0)):
    """the metrics from the figures, the groups in the order given (ascending id); also the
    per-group auc and slack (NaN for a group that is not scored)"""
    nan = float("nan")
    gauc = gauc_slack = sum_auc = 0.0
    rows = scored = 0
    aucs, slacks = [], []
    fig = [[int(x) for x in row] for row in fig]
    rows_scored = sum(P + N for P, N, _, _ in fig if P > 0 and N > 0)
    for P, N, U2, T in fig:
        rows += P + N
        a = s = nan
        if P > 0 and N > 0:
            a = float(U2) / float(2 * P * N)
            s = float(T) / float(2 * P * N)
            w = float(P + N) / float(rows_scored)    # the group's share of the scored rows
            gauc += w * a
            gauc_slack += w * s
            sum_auc += a
            scored += 1
        aucs.append(a)
        slacks.append(s)
    out = {
        "gauc": gauc if scored else nan,
        "gauc_slack": gauc_slack if scored else nan,
        "macro_auc": sum_auc / float(scored) if scored else nan,
        "groups": len(fig), "groups_scored": scored, "rows": rows, "rows_scored": rows_scored,
        "rows_one_class": rows - rows_scored,
        "none_rows": int(none[0]) + int(none[1]), "other_rows": int(other[0]) + int(other[1]),
    }
    return out, np.array(aucs, np.float64), np.array(slacks, np.float64)


def same(a, b):
    """two summaries equal field for field (floats as their bits: NaN == NaN)"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, float) or isinstance(y, float):
            assert (math.isnan(x) and math.isnan(y)) or \
                np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64), (k, x, y)
        else:
            assert int(x) == int(y), (k, x, y)
    return True


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def pair_count(scores, pos):
    """the plain O(m^2) count of one group: pairs (positive, negative) with the positive's score
    above the negative's, ties counted 1/2 — returned doubled, an integer"""
    twice = 0
    for i in range(len(scores)):
        if not pos[i]:
            continue
        for j in range(len(scores)):
            if pos[j]:
                continue
            twice += 2 if scores[i] > scores[j] else (1 if scores[i] == scores[j] else 0)
    return twice


def from_progress_counts(counts):
    """(P, N, U2, T) of ONE group that holds every row, from progressive validation's counts
    [2, RANKS] (class 0 first, indexed by the rank of q): a positive's score is 2C - rank"""
    neg = [int(x) for x in counts[0]]
    pos = [int(x) for x in counts[1]]
    P = N = U2 = T = below = 0
    for s in np.flatnonzero((counts[0] != 0) | (counts[1][::-1] != 0)):
        s = int(s)
        ps, ns = pos[2 * C - s], neg[s]
        U2 += ps * (2 * below + ns)
        T += ps * ns
        P += ps
        N += ns
        below += ns
    return P, N, U2, T
