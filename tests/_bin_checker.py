"""Value binning restated in numpy and Python ints: the definition of include/xflow_amd.h ("value
binning"), a second derivation beside csrc/xf_bin.h.  Everything is integer-exact."""
import numpy as np

CODES, NAN_CODE = 4096, 4095
SALT = 0x62696e5f76616c73
M64 = (1 << 64) - 1


def code(vals):
    """the 12-bit codes of float32 values (an array)"""
    u = np.ascontiguousarray(vals, np.float32).view(np.uint32).astype(np.int64)
    nan = (u & 0x7fffffff) > 0x7f800000
    u = np.where(u == 0x80000000, 0, u)                          # -0.0 counts as +0.0
    k = np.where(u >> 31 == 1, ~u & 0xffffffff, u | 0x80000000)
    return np.where(nan, NAN_CODE, k >> 20).astype(np.int64)


def lut(counts, bins):
    """one field's LUT from its 4096 counts, in Python ints; None where T >= 2^56 is refused"""
    counts = [int(c) for c in counts]
    T = sum(counts[:NAN_CODE])
    if T >= 1 << 56:
        return None
    out, C = np.zeros(CODES, np.uint8), 0
    for c in range(NAN_CODE):
        out[c] = min(bins - 1, C * bins // T) if T else 0
        C += counts[c]
    out[NAN_CODE] = bins
    return out


def mix64(x):
    x = (x + 0x9e3779b97f4a7c15) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def key(k, f, b):
    return mix64((mix64(int(k) ^ SALT) + ((int(f) & 0xffffffff) << 32 | int(b))) & M64)


def counts(spec, fgid, vals):
    """(fields, 4096) uint64: numpy.bincount of the listed fields' codes"""
    c = code(vals)
    return np.stack([np.bincount(c[fgid == f], minlength=CODES).astype(np.uint64)
                     for f, _ in spec])


def fit(spec, cnt):
    return np.stack([lut(cnt[p], b) for p, (_, b) in enumerate(spec)])


def mix64_np(x):
    """mix64 on a uint64 array (numpy's unsigned arithmetic wraps)"""
    U = np.uint64
    x = x + U(0x9e3779b97f4a7c15)
    x = (x ^ (x >> U(30))) * U(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> U(27))) * U(0x94d049bb133111eb)
    return x ^ (x >> U(31))


def apply(spec, luts, keys, fgid, vals):
    """(keys, values, nonzeros binned) of the rewrite"""
    ok, ov, c = keys.copy(), vals.copy(), code(vals)
    binned = 0
    for p, (f, _) in enumerate(spec):
        at = np.flatnonzero(fgid == f)
        b = luts[p][c[at]].astype(np.uint64)
        ok[at] = mix64_np(mix64_np(keys[at] ^ np.uint64(SALT)) + (np.uint64(f << 32) | b))
        ov[at] = 1.0
        binned += len(at)
    return ok, ov, binned
