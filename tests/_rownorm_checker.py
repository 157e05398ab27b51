"""Row normalisation restated in numpy: the definition of include/xflow_amd.h ("row
normalisation"), a second derivation beside csrc/xf_rownorm.h.

* the tree: the squares in float64 (each exact), zero-padded to a power of two, then repeated
  reshape(-1, 2).sum(1) — level 0 adds positions (0,1), (2,3), ..., level 1 those sums in pairs;
* the branch on s: scaled iff s > 0 and finite;
* y = float32(float64(x) * (1.0 / sqrt(s))): the product in float64, one cast to float32.

tests/test_rownorm_cpu.py pins it to a plain Python loop that walks the tree recursively."""
import numpy as np


def sumsq(x):
    """s of one row (float64)"""
    d = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sq = d * d                                               # exact in float64
    if len(sq) == 0:
        return np.float64(0.0)
    width = 1
    while width < len(sq):
        width *= 2
    level = np.zeros(width, np.float64)
    level[:len(sq)] = sq
    with np.errstate(invalid="ignore", over="ignore"):
        while len(level) > 1:
            level = level.reshape(-1, 2).sum(1)
    return np.float64(level[0])


def scales(s):
    return bool(s > 0.0 and np.isfinite(s))


def row(x):
    """(y float32, s float64, scaled) of one row"""
    x = np.asarray(x, np.float32)
    s = sumsq(x)
    if not scales(s):
        return x.copy(), s, False
    rs = np.float64(1.0) / np.sqrt(s)
    return (x.astype(np.float64) * rs).astype(np.float32), s, True


def apply(rowptr, vals):
    """a minibatch: (normalised values, the rows' s, rows scaled)"""
    rowptr = np.asarray(rowptr, np.int64)
    vals = np.asarray(vals, np.float32)
    out = np.empty(int(rowptr[-1] - rowptr[0]), np.float32)
    ss = np.zeros(len(rowptr) - 1, np.float64)
    scaled = 0
    for r in range(len(rowptr) - 1):
        a, e = int(rowptr[r]), int(rowptr[r + 1])
        y, s, sc = row(vals[a:e])
        out[a - int(rowptr[0]):e - int(rowptr[0])] = y
        ss[r] = s
        scaled += int(sc)
    return out, ss, scaled


def tree_loop(sq):
    """the tree walked recursively over a Python list of floats (the plain-loop derivation): the
    sum of positions [lo, lo + width) of the zero-padded squares"""
    n = len(sq)
    width = 1
    while width < n:
        width *= 2

    def go(lo, w):
        if lo >= n:
            return 0.0
        if w == 1:
            return sq[lo]
        return go(lo, w // 2) + go(lo + w // 2, w // 2)
    return go(0, width) if n else 0.0


def same_bits(a, b):
    """float arrays equal bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


def same_sums(a, b):
    """the rows' s equal with ==, a NaN matching a NaN (whose payload is not part of the
    definition: which of two NaNs an addition passes on differs between processors)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------- the tests' rows
def general_values(rng, n):
    """tests/_general_cases.values: exp(N(0, 1)) as fp32, mixed signs, a tenth exact zeros, some
    scaled by 2^-20 and 2^5"""
    from tests import _general_cases as Gc
    return Gc.values(rng, n)


def special_rows():
    """[(name, values)]: the rows whose branch or range is the point"""
    f = np.float32
    tiny, big = f(1e-45), np.finfo(np.float32).max      # the smallest subnormal, FLT_MAX
    rng = np.random.RandomState(3)
    sub = (rng.randint(1, 1 << 23, size=37).astype(np.uint32)).view(np.float32).copy()
    sub[::3] *= f(-1.0)
    return [
        ("zeros", np.array([0.0, -0.0, 0.0, -0.0, -0.0], f)),
        ("one_subnormal", np.array([tiny], f)),
        ("one_negative_subnormal", np.array([-tiny], f)),
        ("subnormals", sub),
        ("flt_max", np.array([big, -big, big, big, 1.0, -big], f)),
        ("nan", np.array([1.0, 2.0, np.nan, -3.0], f)),
        ("inf", np.array([1.0, -np.inf, 0.5], f)),
        ("nan_and_inf", np.array([np.inf, np.nan], f)),
    ]


def recipe_row(rng, target, b=None):
    """a row of a values +-1 and b values +-2 with a + 4 b = target in {4, 16, 64}, shuffled:
    s = target exactly, so the normalised values are exactly +-2^-k"""
    assert target in (4, 16, 64)
    b = int(rng.randint(0, target // 4 + 1)) if b is None else b
    a = target - 4 * b
    x = np.r_[np.ones(a), np.full(b, 2.0)].astype(np.float32)
    x *= np.where(rng.rand(a + b) < 0.3, -1.0, 1.0).astype(np.float32)
    return x[rng.permutation(a + b)]
