"""Table eviction restated in numpy (xf_table_evict): a row is dropped iff w == 0 (either sign of
zero) and n < x, in float32; a NaN n compares false and is kept.  Applied to an export (keys
ascending, w, n, z), so the survivors keep their order.  Also the crafted tables and the training
stream that tests/test_gpu_evict.py and tests/test_evict_cpu.py share."""
import numpy as np

from tests._hyper_cases import synth

SPARE = np.uint64(2**64 - 1)      # the reserved key value: judged like any other


def keep_mask(w, n, x):
    w, n = np.asarray(w, np.float32), np.asarray(n, np.float32)
    with np.errstate(invalid="ignore"):
        return ~((w == np.float32(0)) & (n < np.float32(x)))


def evict(state, x):
    """state = (keys, w, n, z) of an export -> (the survivors' state, rows seen, rows dropped);
    x == 0 does nothing and judges nothing"""
    keys, w, n, z = state
    if float(x) == 0.0:
        return state, 0, 0
    keep = keep_mask(w, n, x)
    return tuple(a[keep] for a in state), len(keys), int((~keep).sum())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_state(got, want, what=""):
    for name, g, r in zip(("keys", "w", "n", "z"), got, want):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.shape, r.shape)
        assert np.array_equal(bits(g), bits(r)), (what, name)


# ------------------------------------------------------------------ crafted tables
X = 1.0       # the threshold of the crafted tables: dropped rows hold n = 0.5, kept zero rows 2.0
PATTERNS = ("none", "all", "every_other", "first", "last", "blocks", "one_per_wave",
            "one_per_block_last", "random_half")


def sizes(B, S):
    """the row counts: around a wavefront, around a block, several blocks, and more blocks than
    the scan has threads (257 blocks + 1 row)"""
    return [1, S - 1, S, S + 1, B - 1, B, B + 1, 2 * B + 1, 5 * B + 37, 257 * B + 1]


def drop_pattern(name, n, B, S):
    """which of the n rows (rank order == key order) go"""
    r = np.arange(n)
    if name == "none":
        return np.zeros(n, bool)
    if name == "all":
        return np.ones(n, bool)
    if name == "every_other":
        return r % 2 == 0
    if name == "first":
        return r == 0
    if name == "last":
        return r == n - 1
    if name == "blocks":                       # whole blocks dropped between kept ones
        return (r // B) % 2 == 1
    if name == "one_per_wave":                 # the survivor's lane moves from wave to wave
        return r % S != ((r // S) * 7 + 3) % S
    if name == "one_per_block_last":           # (a ragged last block keeps nothing)
        return r % B != B - 1
    if name == "random_half":
        return np.random.default_rng(n).random(n) < 0.5
    raise KeyError(name)


def crafted(n, drop, seed=1):
    """(keys ascending, w, n, z) of n rows of which drop[r] go at x = X.  Dropped rows: w = +0 or
    -0, n = 0.5, z anything; kept rows: a nonzero w, or w = 0 with n = 2."""
    rng = np.random.default_rng(seed + n)
    keys = np.unique(rng.integers(1, 2**63, size=n + n // 8 + 16, dtype=np.uint64))[:n]
    assert len(keys) == n
    w = rng.normal(0, 1, n).astype(np.float32)
    w[w == 0] = 1.0
    nn = rng.random(n).astype(np.float32) * 4
    z = rng.normal(0, 1, n).astype(np.float32)
    kept_zero = ~drop & (rng.random(n) < 0.5)
    w[kept_zero] = 0.0
    nn[kept_zero] = 2.0
    w[drop] = np.where(rng.random(int(drop.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    nn[drop] = 0.5
    return keys, w, nn, z


# ------------------------------------------------------------------ the training stream
# lambda1 of the training tests: the oracle's CPU run of T1 steps of stream() leaves 59.5 % of the
# 4783 keys at w == 0 (tests/test_evict_cpu.py asserts 10 % .. 90 %); at the default 5e-5 .. 8e-4
# it is 19.8 % (a minibatch of 600 rows: one occurrence moves z by ~8e-4)
L1 = 1.6e-3
HYPER = dict(alpha=0.05, beta=1.0, lambda1=L1, lambda2=10.0)
T1, T2 = 3, 2
X_TRAIN = 5e-6        # a finite threshold inside the zero rows' n (0 .. 2.4e-5)


def stream():
    """T1 + T2 training minibatches and a held one (the suite's exact-sum inputs)"""
    rng = np.random.RandomState(41)
    return [synth(rng, 600, 12, 5000, 1.2 if i % 2 else None, True) for i in range(T1 + T2 + 1)]


def oracle_after_t1():
    from oracle import pyoracle as O
    s = O.Store(O.OPT_FTRL, 1)
    s.set_ftrl(HYPER["alpha"], HYPER["beta"], HYPER["lambda1"], HYPER["lambda2"])
    for raw in stream()[:T1]:
        with O.sum_mode(1):
            O.lr_update(s, O.Batch(*raw))
    return s.export()
