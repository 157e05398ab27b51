"""Feature admission restated in numpy: the only reference of tests/test_admit_cpu.py and
tests/test_gpu_admit.py.  A filter is 2^L saturating 8-bit counters, h slots per key, a threshold
N and a seed:

    slot_j(key) = mix64(key ^ mix64(seed + j)) >> (64 - L)         j = 0 .. h - 1
    count:   c[s] = min(N, c[s] + #{(nonzero, j) : slot_j(key) = s})
    filter:  a nonzero is kept iff all h of its counters equal N (after the whole count);
             kept nonzeros keep their order, rowptr is rebuilt from the rows' kept counts
"""
import numpy as np

GOLDEN = np.uint64(0x9e3779b97f4a7c15)
M1 = np.uint64(0xbf58476d1ce4e5b9)
M2 = np.uint64(0x94d049bb133111eb)


def mix64(x):
    """add the golden constant, then the splitmix64 finaliser; uint64 arrays, wrapping"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + GOLDEN
        x = (x ^ (x >> np.uint64(30))) * M1
        x = (x ^ (x >> np.uint64(27))) * M2
        return x ^ (x >> np.uint64(31))


def slots(keys, seed, L, h):
    """[h, len(keys)] slot numbers (uint64)"""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.empty((h, len(keys)), np.uint64)
    for j in range(h):
        with np.errstate(over="ignore"):
            salt = mix64(np.array([seed], np.uint64) + np.uint64(j))[0]
        out[j] = mix64(keys ^ salt) >> np.uint64(64 - L)
    return out


class Filter:
    def __init__(self, L, N, h=3, seed=0):
        self.L, self.N, self.h, self.seed = L, N, h, seed
        self.c = np.zeros(1 << L, np.uint8)
        self.seen = self.kept = 0

    def count(self, keys):
        s = slots(keys, self.seed, self.L, self.h).astype(np.int64).ravel()
        add = np.bincount(s, minlength=len(self.c))
        self.c = np.minimum(self.N, self.c.astype(np.int64) + add).astype(np.uint8)

    def keep_mask(self, keys):
        s = slots(keys, self.seed, self.L, self.h).astype(np.int64)
        return (self.c[s] == self.N).all(axis=0) if len(keys) else np.zeros(0, bool)

    def filter(self, rowptr, keys, fgid=None, values=None, update=True):
        """-> (rowptr uint32, keys, fgid or None, values or None) of the filtered minibatch"""
        rowptr = np.asarray(rowptr).astype(np.int64)
        lo, hi = rowptr[0], rowptr[-1]
        keys = np.asarray(keys, dtype=np.uint64)[lo:hi]
        rowptr = rowptr - lo
        if update:
            self.count(keys)
        keep = self.keep_mask(keys)
        before = np.concatenate([[0], np.cumsum(keep)])      # kept nonzeros in front of position i
        out_rowptr = before[rowptr].astype(np.uint32)
        if update:
            self.seen += len(keys)
            self.kept += int(keep.sum())
        pick = lambda a, dt: None if a is None else np.asarray(a, dtype=dt)[lo:hi][keep]  # noqa: E731
        return out_rowptr, keys[keep], pick(fgid, np.int32), pick(values, np.float32)
