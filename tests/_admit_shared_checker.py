"""One admission filter shared by the ranks of a group, restated with tests/_admit_checker.py: the
reference of tests/test_admit_shared_cpu.py and tests/test_gpu_admit_shared.py.

One collective apply = the minibatches the ranks hand in at the same call.  The counters are those
of ONE Filter that counts the concatenation of the ranks' nonzeros; rank r's output is what that
filter keeps of r's arrays.  The slot partition (which rank holds which counters) is restated here
too; it decides nothing about the result."""
import numpy as np

from . import _admit_checker as A

SEED = 0x5eed


# ------------------------------------------------------------------ the slot partition
def per(L, world):
    """slots per rank: 4 * ceil(ceil(2^L / world) / 4) — whole 32-bit counter words"""
    slots = 1 << L
    return 4 * -(-(-(-slots // world)) // 4)


def admit_range(L, world, rank):
    """(first, n): rank owns [rank * per, min((rank + 1) * per, 2^L)), possibly nothing"""
    slots, p = 1 << L, per(L, world)
    lo = min(slots, rank * p)
    return lo, min(slots, lo + p) - lo


def owner(slot, L, world):
    return slot // per(L, world)


# ------------------------------------------------------------------ the applies of one filter
def pool(n=3000):
    """arbitrary 64-bit keys (no library needed)"""
    return A.mix64(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(7919))


def _csr(lens, keys):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(rowptr[-1]) == len(keys)
    return rowptr, np.asarray(keys, np.uint64)


NO_ROWS = (np.zeros(1, np.uint64), np.zeros(0, np.uint64))


def _no_nonzeros(R=5):
    return np.zeros(R + 1, np.uint64), np.zeros(0, np.uint64)


def _zipf(rng, P, n, a):
    return P[np.minimum(rng.zipf(a, size=n), len(P)) - 1]


def _small(rng, P, rows=40):
    lens = rng.randint(0, 9, size=rows)
    return _csr(lens, _zipf(rng, P, int(lens.sum()), 1.4))


def keys_on_slots(targets, L, exclude=()):
    """for every slot in `targets` a key whose slot 0 (seed SEED) is that slot, found by search"""
    cand = A.mix64(np.arange(1 << 20, (1 << 20) + 200000, dtype=np.uint64))
    s0 = A.slots(cand, SEED, L, 1)[0]
    out = []
    for t in targets:
        hit = [k for k in cand[s0 == np.uint64(t)][:8].tolist() if k not in exclude]
        assert hit, "no key on slot %d" % t
        out.append(hit[0])
    return np.array(out, np.uint64)


def boundary_slots(L, world):
    """the first and the last slot of every non-empty range"""
    out = []
    for r in range(world):
        first, n = admit_range(L, world, r)
        if n:
            out += [first, first + n - 1]
    return out


def word_mates(L, want=4):
    """`want` distinct keys whose slot 0 falls into one 32-bit counter word"""
    cand = A.mix64(np.arange(1 << 22, (1 << 22) + 100000, dtype=np.uint64))
    s0 = A.slots(cand, SEED, L, 1)[0] >> np.uint64(2)
    words, counts = np.unique(s0, return_counts=True)
    return cand[s0 == words[np.argmax(counts >= want)]][:want]


def covered_keys(hot, L, h, want=6):
    """keys outside `hot` whose h slots are all slots of `hot` keys: once the hot keys' counters
    are full these are admitted without having occurred — false admissions"""
    full = np.zeros(1 << L, bool)
    full[A.slots(hot, SEED, L, h).astype(np.int64).ravel()] = True
    cand = A.mix64(np.arange(1 << 24, (1 << 24) + 200000, dtype=np.uint64))
    ok = full[A.slots(cand, SEED, L, h).astype(np.int64)].all(axis=0) & ~np.isin(cand, hot)
    assert ok.sum() >= want, "no key covered by the hot keys' slots"
    return cand[ok][:want]


def sequence(world, N, h, L):
    """[(name, update, [per rank (rowptr, keys)])]: the applies of one filter, in order"""
    rng = np.random.RandomState(1000 * world + 10 * h + L)
    P = pool()
    last = world - 1
    seq = []

    def add(name, parts, update=True):
        assert len(parts) == world
        seq.append((name, update, parts))

    # ragged rows on every rank: empty rows first, last and in runs; power-law keys
    parts = []
    for r in range(world):
        lens = rng.randint(0, 21, size=300)
        lens[:3] = 0
        lens[-2:] = 0
        lens[100:120] = 0
        parts.append(_csr(lens, _zipf(rng, P, int(lens.sum()), 1.3)))
    add("ragged", parts)
    # a key N - 1 times on rank 0 and once on the last rank: N occurrences in all — a filter of
    # rank 0's or of the last rank's own would not admit it (world > 1, N > 1)
    split = np.uint64(0xabcdef0123456789)
    parts = [_small(rng, P) for _ in range(world)]
    rp, ks = parts[0]
    parts[0] = _csr(np.concatenate([np.diff(rp.astype(np.int64)), [N - 1]]),
                    np.concatenate([ks, np.full(N - 1, split, np.uint64)]))
    rp, ks = parts[last]
    parts[last] = _csr(np.concatenate([[1], np.diff(rp.astype(np.int64))]),
                       np.concatenate([[split], ks]))
    add("split_key", parts)
    # one rank without nonzeros, then one without rows, then nobody brings anything
    add("rank_nnz0", [_no_nonzeros() if r == 0 else _small(rng, P) for r in range(world)])
    add("rank_r0", [NO_ROWS if r == last else _small(rng, P) for r in range(world)])
    add("all_empty", [NO_ROWS if r % 2 else _no_nonzeros(3) for r in range(world)])
    # one key 20 000 times on rank 0, the same key on rank 1 as well: one counter word under
    # contention from two ranks' slots
    hot = P[2999]
    keys = P[rng.randint(0, len(P), size=24000)]
    keys[rng.permutation(24000)[:20000]] = hot
    parts = [_small(rng, P) for _ in range(world)]
    parts[0] = _csr(np.full(480, 50), keys)
    if world > 1:
        keys1 = P[rng.randint(0, len(P), size=600)]
        keys1[::3] = hot
        parts[1] = _csr(np.full(60, 10), keys1)
    add("hot_key", parts)
    # 40 keys 300 times each, dealt out to the ranks: their counters are full whatever N ...
    hots = pool(4000)[3000:3040]
    deal = np.repeat(hots, 300)[rng.permutation(12000)]
    add("hot_set", [_csr(np.full(12000 // world // 20, 20), deal[r::world])    # (12000 = 2^5 3 5^3)
                    for r in range(world)])
    # ... so keys that only hit those counters are admitted unseen, next to fresh keys that are not
    probes = np.concatenate([covered_keys(hots, L, h), A.mix64(np.arange(1 << 26, (1 << 26) + 6, dtype=np.uint64))])
    add("probes", [_csr([len(probes[r::world])], probes[r::world]) for r in range(world)])
    # four keys of one counter word spread over the ranks
    m = np.tile(word_mates(L), 3)
    add("word_mates", [_csr([len(m[r::world])], m[r::world]) for r in range(world)])
    # keys on the first and the last slot of every non-empty range, spread over the ranks
    b = np.tile(keys_on_slots(boundary_slots(L, world), L), 2)
    add("boundary", [_csr([0, len(b[r::world]), 0], b[r::world]) for r in range(world)])
    # the tile of the test and the scatter (2048 nonzeros) on one rank
    for n in (2047, 2048, 2049):
        parts = [_small(rng, P) for _ in range(world)]
        parts[last] = _csr([n - n // 2, 0, n // 2], _zipf(rng, P, n, 1.2))
        add("nnz%d" % n, parts)
    # a read-only apply: fresh and seen keys, filtered by the present state
    parts = []
    for r in range(world):
        lens = rng.randint(0, 15, size=80)
        n = int(lens.sum())
        ks = _zipf(rng, P, n, 1.3)
        ks[::5] = A.mix64(np.arange(r << 20, (r << 20) + len(ks[::5]), dtype=np.uint64) + np.uint64(1 << 30))
        parts.append(_csr(lens, ks))
    add("read_only", parts, update=False)
    add("ragged_again", seq[0][2])
    return seq


def companions(keys, t):
    """(fgid, values) of apply number t: none, fgid, values, both in turn; each says where its
    nonzero came from"""
    n = len(keys)
    fg = np.arange(n, dtype=np.int32) % 977
    vs = (np.arange(n, dtype=np.float32) * np.float32(0.25) - np.float32(3)).astype(np.float32)
    return (fg if t % 4 in (1, 3) else None), (vs if t % 4 in (2, 3) else None)


def expected(seq, N, h, L):
    """per apply: (counters after it, [per rank (rowptr, keys, fgid, values, keep mask)]) — one
    Filter counting the concatenation, then every rank's arrays against it"""
    flt = A.Filter(L, N, h, SEED)
    out = []
    for t, (name, update, parts) in enumerate(seq):
        if update:
            flt.count(np.concatenate([ks for _, ks in parts]))
        ranks = []
        for rp, ks in parts:
            fg, vs = companions(ks, t)
            keep = flt.keep_mask(ks)
            before = np.concatenate([[0], np.cumsum(keep)])
            ranks.append((before[rp.astype(np.int64)].astype(np.uint32), ks[keep],
                          None if fg is None else fg[keep], None if vs is None else vs[keep], keep))
        out.append((flt.c.copy(), ranks))
    return out


def global_stream():
    """minibatches of a stream that the world-independence test deals out to 1, 2 and 3 ranks"""
    rng = np.random.RandomState(99)
    P = pool()
    out = []
    for _ in range(5):
        lens = rng.randint(0, 12, size=120)
        out.append(_csr(lens, _zipf(rng, P, int(lens.sum()), 1.3)))
    return out


def deal(mb, world):
    """a minibatch's rows in `world` contiguous parts"""
    rp, ks = mb
    rp = rp.astype(np.int64)
    R = len(rp) - 1
    cuts = [R * r // world for r in range(world + 1)]
    return [((rp[a:b + 1] - rp[a]).astype(np.uint64), ks[rp[a]:rp[b]]) for a, b in zip(cuts, cuts[1:])]
