"""Held-out validation restated in numpy: the only reference of tests/test_holdout_cpu.py and
tests/test_gpu_holdout.py.

    T          = floor(float64(float32(share)) * 2^32)
    h(ordinal) = mix64(mix64(seed ^ stream ^ SALT) + ordinal)     (64-bit, wrapping)
    a row is HELD iff (h >> 32) < T

One split is one minibatch: row i has ordinal first_ordinal + i; the rows go, in order, into a
train and a held minibatch, rowptr / labels / keys / fgid / values compacted together.

The stop rule: an epoch improves iff L < best - delta; a NaN neither improves nor counts as an
epoch without improvement; stop iff patience > 0, at least `patience` epochs since the best one did
not improve, and the last value is not NaN.

The counts of a validate: the ranks (tests/_progress_checker.py) of loss = float32(pctr - label).
"""
import numpy as np

from ._admit_checker import mix64

U64 = (1 << 64) - 1
SALT = 0x6a09e667f3bcc909


def threshold(share):
    return int(np.floor(np.float64(np.float32(share)) * np.float64(2.0 ** 32)))


def held(seed, stream, ordinals, share):
    """bool per ordinal (uint64 array, wrapping): is the row of this ordinal held"""
    ordinals = np.asarray(ordinals, dtype=np.uint64)
    base = mix64(np.array([(int(seed) ^ int(stream) ^ SALT) & U64], np.uint64))[0]
    with np.errstate(over="ignore"):
        h = mix64(base + ordinals)
    return (h >> np.uint64(32)) < np.uint64(threshold(share))


def should_stop(curve, patience, delta=0.0):
    """-> (stop, index of the best epoch or -1)"""
    best, low, since = -1, float("inf"), 0
    for i, L in enumerate(curve):
        if L != L:
            continue
        if L < low - delta:
            best, low, since = i, L, 0
        else:
            since += 1
    n = len(curve)
    return bool(n and patience > 0 and since >= patience and curve[-1] == curve[-1]), best


class Splitter:
    def __init__(self, share, seed=0):
        self.share, self.seed = share, seed
        self.rows_seen = self.rows_held = self.nnz_held = 0

    def mask(self, stream, first_ordinal, R):
        with np.errstate(over="ignore"):
            ords = np.uint64(int(first_ordinal) & U64) + np.arange(R, dtype=np.uint64)
        return held(self.seed, stream, ords, self.share)

    def split(self, stream, first_ordinal, rowptr, keys, labels, fgid=None, values=None):
        """-> (train, held), each (rowptr uint32, keys, labels, fgid or None, values or None)"""
        rowptr = np.asarray(rowptr).astype(np.int64)
        lo = rowptr[0]
        rowptr = rowptr - lo
        labels = np.asarray(labels, dtype=np.int32)
        R = len(rowptr) - 1
        assert len(labels) == R
        m = self.mask(stream, first_ordinal, R)
        lens = np.diff(rowptr)
        hi = lo + rowptr[-1]
        parts = []
        for part in (~m, m):
            nz = np.repeat(part, lens)
            pick = lambda a, dt: None if a is None else np.asarray(a, dtype=dt)[lo:hi][nz]  # noqa: E731
            parts.append((np.concatenate([[0], np.cumsum(lens[part])]).astype(np.uint32),
                          pick(keys, np.uint64), labels[part], pick(fgid, np.int32),
                          pick(values, np.float32)))
        self.rows_seen += R
        self.rows_held += int(m.sum())
        self.nnz_held += int(lens[m].sum())
        return parts[0], parts[1]

    def stats(self):
        return self.rows_seen, self.rows_held, self.nnz_held


def write_split(src, train_out, held_out, seed, stream, share):
    """the text file `src` (one row a line, row i has ordinal i) written as two files: the rows
    that are not held and the held ones, in order -> the held mask"""
    lines = open(src, "rb").read().split(b"\n")
    assert lines[-1] == b""
    lines = lines[:-1]
    m = held(seed, stream, np.arange(len(lines), dtype=np.uint64), share)
    for path, part in ((train_out, ~m), (held_out, m)):
        with open(path, "wb") as f:
            f.write(b"".join(ln + b"\n" for ln, p in zip(lines, part) if p))
    return m


def counts_of(pctr, labels):
    """what a validate adds for rows scored `pctr`: the forward stores one fp32 pctr - label"""
    from . import _progress_checker as P
    pctr = np.asarray(pctr, np.float32)
    labels = np.asarray(labels)
    loss = (pctr - labels.astype(np.float32)).astype(np.float32)
    return P.counts_of(loss, labels)
