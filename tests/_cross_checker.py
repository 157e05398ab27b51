"""Feature crosses restated in numpy: the definition of include/xflow_amd.h ("feature crosses"),
nothing of the library's code.  tests/test_cross_cpu.py pins it to a loop in plain Python ints and
to the known answers; the GPU tests compare the stage with it bit for bit."""
import numpy as np

GOLD = np.uint64(0x9e3779b97f4a7c15)
M1 = np.uint64(0xbf58476d1ce4e5b9)
M2 = np.uint64(0x94d049bb133111eb)
LIMIT = (1 << 32) - 1            # a crossed minibatch holds fewer nonzeros than this


def mix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + GOLD
        x = (x ^ (x >> np.uint64(30))) * M1
        x = (x ^ (x >> np.uint64(27))) * M2
    return x ^ (x >> np.uint64(31))


def salt(fa, fb):
    return mix64(np.uint64(((int(fa) & 0xffffffff) << 32) | (int(fb) & 0xffffffff)))


def cross_key(ka, kb, fa, fb):
    """arrays (or scalars) of keys of field fa and of field fb -> the crossed keys"""
    ka, kb = np.asarray(ka, dtype=np.uint64), np.asarray(kb, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64(mix64(ka ^ salt(fa, fb)) + kb)


def parse(spec):
    """"2*3,16*17" -> [(2, 3), (16, 17)] (a well-formed spec only: the refusals are the library's)"""
    return [tuple(int(x) for x in piece.split("*")) for piece in spec.split(",")]


class Cross:
    def __init__(self, spec_or_pairs, fgid_base=0):
        self.pairs = parse(spec_or_pairs) if isinstance(spec_or_pairs, str) else \
            [(int(a), int(b)) for a, b in spec_or_pairs]
        self.base = int(fgid_base)
        self.rows_seen = self.nnz_in = self.nnz_crossed = 0

    def apply(self, rowptr, keys, fgid, values=None):
        """(rowptr uint32, keys, fgid, values or None) of the crossed minibatch; rowptr is
        row-relative (its first entry may be an offset into keys: a slice of a block)"""
        rowptr = np.asarray(rowptr, dtype=np.uint64).astype(np.int64)
        keys = np.asarray(keys, dtype=np.uint64)
        fgid = np.asarray(fgid, dtype=np.int32)
        R = len(rowptr) - 1
        ok, ofg, ov, orp = [], [], [], [0]
        for r in range(R):
            a, b = int(rowptr[r]), int(rowptr[r + 1])
            if b < a or b > len(keys):
                a = b = 0                              # length 0
            k, f = keys[a:b], fgid[a:b]
            v = values[a:b] if values is not None else None
            ok.append(k)
            ofg.append(f)
            if v is not None:
                ov.append(np.asarray(v, np.float32))
            n = b - a
            for p, (fa, fb) in enumerate(self.pairs):
                ia, ib = np.flatnonzero(f == fa), np.flatnonzero(f == fb)
                if len(ia) == 0 or len(ib) == 0:
                    continue
                i, j = np.repeat(ia, len(ib)), np.tile(ib, len(ia))
                ok.append(cross_key(k[i], k[j], fa, fb))
                ofg.append(np.full(len(i), self.base + p, np.int32))
                if v is not None:
                    ov.append((np.asarray(v, np.float32)[i] *
                               np.asarray(v, np.float32)[j]).astype(np.float32))
                n += len(i)
            orp.append(orp[-1] + n)
            self.nnz_in += b - a
            self.nnz_crossed += n - (b - a)
        assert orp[-1] < LIMIT
        self.rows_seen += R
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
        return (np.asarray(orp, np.uint32), cat(ok, np.uint64), cat(ofg, np.int32),
                cat(ov, np.float32) if values is not None else None)

    def stats(self):
        return self.rows_seen, self.nnz_in, self.nnz_crossed
