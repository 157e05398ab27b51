"""The numpy / Python-int restatement of sliced progressive validation (include/xflow_amd.h,
"sliced progressive validation"): the slice id of a row, the home slot of a key, the fixed-point
row terms, what a minibatch adds to every slice, the summary of a slice's seven words.  Written
from the header's text, not from the library's code: the tests compare the two with ==."""
import math

import numpy as np

from . import _progress_checker as P

NONE = 2 ** 64 - 1
WORDS = 7                    # n0 n1 qsum0 qsum1 llsum0 llsum1 other
M64 = 2 ** 64 - 1
LOGLOSS_BOUND = P.LOGLOSS_BOUND + 2.0 ** -25
PCTR_BOUND = 2.0 ** -31


def mix64(x):
    """admission's mix64: add the golden constant, then the splitmix64 finaliser"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def home(key, b):
    return mix64(int(key) & M64) >> (64 - b)


def probes(b):
    return min(2 ** b, 128)


def ids_of(rowptr, keys, fgid, F, nnz=None):
    """id[r]: the key of the first nonzero of row r with fgid == F; NONE without one; a row whose
    offsets descend or leave the arrays is empty.  rowptr: R + 1 offsets into keys / fgid"""
    rowptr = np.asarray(rowptr).astype(np.int64)
    keys = np.asarray(keys, dtype=np.uint64)
    fgid = np.asarray(fgid, dtype=np.int64)
    nnz = len(keys) if nnz is None else nnz
    out = np.full(len(rowptr) - 1, NONE, np.uint64)
    for r in range(len(rowptr) - 1):
        a, e = int(rowptr[r]), int(rowptr[r + 1])
        if e < a or e > nnz:
            continue
        hit = np.flatnonzero(fgid[a:e] == F)
        if len(hit):
            out[r] = keys[a + hit[0]]
    return out


_TERMS = None


def terms():
    """ll_fix[rank] = round-half-even(term(rank) * 2^24), from the progress checker's terms"""
    global _TERMS
    if _TERMS is None:
        t = np.zeros(P.RANKS, np.uint32)
        for r in range(P.RANKS):
            m = P.bucket_m(r)
            term = -math.log1p(-m) if r < P.C else -math.log(m)
            t[r] = int(round(term * 2.0 ** 24))     # (the scaling is exact; round: half to even)
        _TERMS = t
    return _TERMS


def rows_words(loss, labels):
    """what every row adds: an int64-safe uint64 array [R, 7]"""
    loss = np.ascontiguousarray(loss, dtype=np.float32)
    cls = (np.asarray(labels) != 0).astype(np.int64)
    r = P.ranks(loss)
    part = r < P.RANKS
    q = np.where(part, np.abs(loss), np.float32(0)).astype(np.float32)
    qfix = (q.astype(np.float64) * 2.0 ** 31).astype(np.uint64)     # exact product, truncated
    ll = terms()[np.where(part, r, 0)].astype(np.uint64)
    w = np.zeros((len(loss), WORDS), np.uint64)
    rows = np.arange(len(loss))
    w[rows[part], cls[part]] = 1
    w[rows[part], 2 + cls[part]] = qfix[part]
    w[rows[part], 4 + cls[part]] = ll[part]
    w[rows[~part], 6] = 1
    return w


def words_of(loss, labels, ids, into=None):
    """{id: [7 Python ints]} of one minibatch, added into `into` when given"""
    out = {} if into is None else into
    w = rows_words(loss, labels)
    ids = np.asarray(ids, dtype=np.uint64)
    for key in np.unique(ids):
        s = [int(x) for x in w[ids == key].sum(axis=0, dtype=np.uint64)]
        old = out.get(int(key))
        out[int(key)] = s if old is None else [a + b for a, b in zip(old, s)]
    return out


def total(truth):
    return [sum(v[i] for v in truth.values()) for i in range(WORDS)]


def check_table(got, truth, b, complete=None):
    """the table's contract against the truth {id: words}: every resident key's words are exactly
    its truth, `none` is the NONE id's, `overflow` the summed truth of the keys not resident, and
    the sum of everything is the whole stream's.  complete=True: also no overflow"""
    keys, words, none, overflow = got
    keys = [int(k) for k in keys]
    assert keys == sorted(set(keys)) and NONE not in keys, "keys ascending, distinct, none apart"
    assert len(keys) <= 2 ** b
    for k, w in zip(keys, words):
        assert k in truth, ("a resident key nobody fed", hex(k))
        assert [int(x) for x in w] == truth[k], (hex(k), list(w), truth[k])
    assert [int(x) for x in none] == truth.get(NONE, [0] * WORDS), "none"
    rest = {k: v for k, v in truth.items() if k != NONE and k not in set(keys)}
    want_over = total(rest) if rest else [0] * WORDS
    assert [int(x) for x in overflow] == want_over, ("overflow", list(overflow), want_over)
    if complete is not None:
        assert (not rest) == complete, (len(rest), complete)
    return len(rest)


def summary(words, w=1.0):
    """the figures of one slice in Python ints and fp64"""
    w = float(np.float32(w))
    n0, n1, q0, q1, l0, l1, other = [int(x) for x in words]
    rows = float(n1) + w * float(n0)
    nan = float("nan")
    any_ = (n0 or n1) != 0
    return {
        "rows": rows, "other": float(other),
        "ctr": float(n1) / rows if any_ else nan,
        "pctr": (float(n1 * 2 ** 31 - q1) + w * float(q0)) / 2.0 ** 31 / rows if any_ else nan,
        "logloss": (float(l1) + w * float(l0)) / 2.0 ** 24 / rows if any_ else nan,
        "logloss_bound": LOGLOSS_BOUND, "pctr_bound": PCTR_BOUND,
    }


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert (math.isnan(x) and math.isnan(y)) or x == y, (k, x, y)
    return True
