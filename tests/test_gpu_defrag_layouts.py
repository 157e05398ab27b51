"""The sort-free table defrag (xf_table.hip "defrag without a library sort": k_df_count / _scan /
_list / _fix / _merge) at the layouts where a block of kDfBlock = 16384 index positions decides
which entries are its own: a cluster across a block end (lead / ext), a block that is all lead,
the 4 * kDfMax = 32768 limit of an extension, the kDfCluster = 1024 limit of k_df_fix, the wrap
rule with several blocks, a wrapped cluster that covers block 0, sharded geometries, rows of
dim > 1, a rehash in between, and the kMgTile = 4096 tile cuts of the merge with the settled tier.

The keys are crafted: the order-preserving home map is restated here in Python integers (Geo)
and inverted, so that a key set lands where the case wants it; every case asserts on a simulated
index (Geo.occupied: linear probing fills the same positions in any arrival order) that its own
inputs do reach the edge it names.  The reference is the oracle's Store, a plain CPU map fed the
same push calls; every comparison is bit for bit.  Every case runs under key_build = 0 (the
sort-free path) and key_build = 1 (the radix defrag), and the two tables are compared as well.
The radix sort is right for any index, and xf_table_defrag falls back to it when the blocks'
counts do not add up — which would hide a wrong ownership decision.  So every defrag is also held
to the way it must go (xf_table_defrag_path): SORTFREE where the layout is the sort-free path's
to the end, RADIX_CLUSTER / RADIX_EXTENT where a limit hands it over, never RADIX_COUNT.

Wall time per test on an MI355X, measured once with the shapes as they are here (pytest
--durations, the module run alone: 38 cases in 5.7 s):
  test_the_wrapped_cluster_covers_block_0 (each order)        0.45 - 0.47 s
  test_an_inner_block_that_is_all_lead[homed_at]              0.41 s   [one_per_home] 0.04 s
  test_a_cluster_across_a_block_end                           0.20 s (first use of the GPU)
  test_an_extension_at_its_limit                              0.17 s, 0.08 s
  test_a_cluster_at_the_limit_of_the_in_place_sort[...-1024]  0.14 s
  test_keys_that_arrive_in_minibatches[wrap-over-block0]      0.10 s
  every other case                                            under 0.04 s
(the slow ones are the pushes of 17000 keys with one home: every key probes past the others).
"""
import numpy as np
import pytest
import torch

from oracle import pyoracle as O
from xflow_amd import capi

from .test_gpu_keybuild import steps_vs_oracle
from .test_gpu_parity import same

pytestmark = pytest.mark.gpu

B = 16384                 # kDfBlock
RESERVED = 2**64 - 1      # the reserved key value: lives at the spare position, never in the index
MARGIN = 64               # homes kept free of background keys around a crafted run


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


class Geo:
    """home = min(((key - lo) * mult) >> 64, cap - 1), mult = (cap << 64) // span,
    span = (2**64 - 1) // nshards, lo = span * shard (xf_device.h home_of, set_geometry)"""

    def __init__(self, cap, shard=0, nshards=1):
        self.cap, self.shard, self.nshards = cap, shard, nshards
        self.span = (2**64 - 1) // nshards
        self.lo = self.span * shard
        self.mult = (cap << 64) // self.span
        assert self.mult < 2**64
        # the largest ordinary key of the range (the last shard takes the remainder too)
        self.top = 2**64 - 2 if shard == nshards - 1 else self.lo + self.span - 1

    def home(self, key):
        return min(((int(key) - self.lo) * self.mult) >> 64, self.cap - 1)

    def first_key(self, h):
        """the smallest key whose home is h (h below the clamp)"""
        return self.lo + -((-(h << 64)) // self.mult)

    def _checked(self, keys, homes):
        assert len(set(keys)) == len(keys) and all(self.lo <= k <= self.top for k in keys)
        assert [self.home(k) for k in keys] == list(homes)      # (the test's own inputs)
        return np.array(keys, dtype=np.uint64)

    def homed_at(self, h, count, skip=0):
        """the keys number skip .. skip + count - 1 (ascending) of home h: one cluster, one home"""
        k0 = self.first_key(h) + skip
        return self._checked([k0 + i for i in range(count)], [h] * count)

    def one_per_home(self, h0, count, skip=0):
        """a key for each home h0 .. h0 + count - 1: an occupied run with nothing displaced"""
        homes = range(h0, h0 + count)
        return self._checked([self.first_key(h) + skip for h in homes], homes)

    def largest(self, count, skip=0):
        """the ordinary keys number skip .. skip + count - 1 from the top of the range"""
        keys = [self.top - skip - i for i in range(count)]
        return self._checked(keys, [self.cap - 1] * count)

    def smallest(self, count, skip=0):
        keys = [self.lo + skip + i for i in range(count)]
        return self._checked(keys, [0] * count)

    def background(self, start, n, clear=()):
        """about n hashed keys of this shard's range whose homes avoid the `clear` ranges"""
        out = []
        for k in capi.hash_decimal_range(start, n * self.nshards):
            k = int(k)
            if not self.lo <= k <= self.top:
                continue
            h = self.home(k)
            if not any(a - MARGIN <= h < b + MARGIN for a, b in clear):
                out.append(k)
        return np.array(out, dtype=np.uint64)

    def occupied(self, keys):
        """which index positions hold a key once `keys` are in (linear probing from the home:
        the SET of positions does not depend on the arrival order)"""
        h = np.sort(np.array([self.home(k) for k in keys if int(k) != RESERVED], dtype=np.int64))
        i = np.arange(len(h), dtype=np.int64)
        p = i + np.maximum.accumulate(h - i)            # p[i] = max(h[i], p[i-1] + 1)
        wrapped = int((p >= self.cap).sum())            # they run on from position 0
        if wrapped:
            h = np.concatenate([np.zeros(wrapped, np.int64), h])
            i = np.arange(len(h), dtype=np.int64)
            p = i + np.maximum.accumulate(h - i)
            assert int((p >= self.cap).sum()) == wrapped
            p = p[p < self.cap]
        occ = np.zeros(self.cap, dtype=bool)
        occ[p] = True
        assert int(occ.sum()) == len(p)
        return occ


class Wave:
    """what arrives between two defrags: key sets in push order (the background first), what
    the index must then look like: (first, last, occupied?) runs of positions, and which way
    xf_table_defrag must take under key_build = 0 (xf_table_defrag_path)"""

    def __init__(self, geo, sets, bg_start, bg=2000, clear=(), expect=(),
                 path=capi.DEFRAG_SORTFREE):
        self.path = path      # how the sort-free defrag must come to order these keys
        self.sets = [geo.background(bg_start, bg, clear)] if bg else []
        self.sets += [np.asarray(k, dtype=np.uint64) for k in sets]
        allk = np.concatenate(self.sets)
        assert len(np.unique(allk)) == len(allk)
        if expect:
            occ = geo.occupied(allk)
            for first, last, want in expect:
                assert bool(occ[first:last + 1].all() if want else not occ[first:last + 1].any()), \
                    (first, last, want)


def run_of(h0, n):
    """positions h0 .. h0 + n - 1 occupied, the position before and the one after empty"""
    return [(h0 - 1, h0 - 1, False), (h0, h0 + n - 1, True), (h0 + n, h0 + n, False)]


def compare(t, s):
    for a, e in zip(t.export(), s.export()):
        same(a, e)
    assert len(t) == len(s)


def check_settled(t, s):
    """the table is the Store's, and every ordinary key is settled at the row of its rank"""
    compare(t, s)
    keys = s.export()[0]
    ordinary = keys[keys != np.uint64(RESERVED)]
    assert np.all(ordinary[1:] > ordinary[:-1])
    assert t.settled == len(ordinary)
    dk = torch.from_numpy(ordinary.view(np.int64)).cuda()
    rows = torch.empty(len(ordinary), dtype=torch.int32, device="cuda")
    t.resolve_dev(dk.data_ptr(), len(ordinary), rows.data_ptr())
    t.check()
    assert np.array_equal(rows.cpu().numpy(), np.arange(len(ordinary)))
    same(t.pull(keys), s.pull(keys))
    return keys


def settle_and_check(t, s, rng, dim, path):
    """defrag — the way the layout is meant to make it go —, check_settled, and the rows moved
    together with their keys (a push on all of them says so)"""
    t.defrag()
    assert t.defrag_path == path, (t.defrag_path, path)
    keys = check_settled(t, s)
    g = rng.randn(len(keys), dim).astype(np.float32)
    t.push(keys, g)
    s.push(keys, g)
    compare(t, s)


def make_pair(cap, opt=capi.OPT_FTRL, dim=1, init=capi.INIT_ZERO, seed=0, shard=0, nshards=1):
    t = capi.Table(opt, dim, init, 0.0, seed, capacity=cap, shard=shard, nshards=nshards)
    assert t.capacity == cap
    return t, O.Store(opt, dim, init, 0.0, seed)


def push_wave(t, s, wave, rng, dim):
    for keys in wave.sets:
        g = rng.randn(len(keys), dim).astype(np.float32)
        t.push(keys, g)
        s.push(keys, g)


def check_layout(cap, waves, seed=1, **table):
    dim = table.get("dim", 1)
    allk = np.concatenate([k for wave in waves for k in wave.sets])
    assert len(np.unique(allk)) == len(allk)     # (a wave's keys are new to the table)
    exports = []
    for mode in (0, 1):
        capi.tune("key_build", mode)
        try:
            rng = np.random.RandomState(seed)
            t, s = make_pair(cap, **table)
            for wave in waves:
                push_wave(t, s, wave, rng, dim)
                settle_and_check(t, s, rng, dim,
                                 wave.path if mode == 0 else capi.DEFRAG_RADIX_ASKED)
            exports.append(t.export())
        finally:
            capi.tune("key_build", 0)
    for a, b in zip(*exports):
        same(a, b)


# ------------------------------------------------------------------------------ the layouts
def straddle(geo, bg=2000):
    """one home, 300 keys, from B - 100: block 0 extends by 200, block 1 has a lead of 200; the
    second copy at the next block end"""
    return [Wave(geo, [geo.homed_at(b - 100, 300)], w * 10**6, bg, [(b - 100, b + 200)],
                 run_of(b - 100, 300)) for w, b in ((0, B), (1, 2 * B))]


def test_a_cluster_across_a_block_end():
    cap = 3 * B + 1000
    check_layout(cap, straddle(Geo(cap)))


@pytest.mark.parametrize("count", [1024, 1025])
@pytest.mark.parametrize("h", [B // 2, 2 * B - 500], ids=["mid-block", "across-a-block-end"])
def test_a_cluster_at_the_limit_of_the_in_place_sort(h, count):
    """k_df_fix sorts a cluster of up to kDfCluster = 1024 keys in place; 1025 set the flag and
    the radix sort runs.  The cluster stands alone: its neighbours are empty."""
    cap = 3 * B + 1000
    geo = Geo(cap)
    h2 = h + B if h < B else h - B
    path = capi.DEFRAG_SORTFREE if count <= 1024 else capi.DEFRAG_RADIX_CLUSTER
    waves = [Wave(geo, [geo.homed_at(x, count)], w * 10**6, 2000, [(x, x + count)],
                  run_of(x, count), path) for w, x in ((0, h), (1, h2))]
    check_layout(cap, waves)


def test_a_block_filled_from_its_first_to_its_last_position():
    """lead = 0 (the position before the block is empty), the last position occupied, ext = 0;
    the blocks' counts must add up — and then one cluster of 16384 keys is the radix sort's"""
    cap = 3 * B + 1000
    geo = Geo(cap)
    waves = [Wave(geo, [geo.one_per_home(b, B)], w * 10**6, 2000, [(b, b + B)], run_of(b, B),
                  capi.DEFRAG_RADIX_CLUSTER) for w, b in ((0, B), (1, 2 * B))]
    check_layout(cap, waves)


@pytest.mark.parametrize("kind", ["one_per_home", "homed_at"])
def test_an_inner_block_that_is_all_lead(kind):
    """a run of 17500 positions from B - 384: block 0 carries it, every position of block 1 is
    lead, block 2 has a lead — as a run of keys at their homes, and as one home's keys.  The
    blocks' counts must add up (RADIX_COUNT otherwise); the cluster then is the radix sort's.
    (4B + 1000 positions: two such runs need more than the 37615 state rows of 3B + 1000.)"""
    cap = 4 * B + 1000
    geo = Geo(cap)
    # (the runs overlap: the second copy takes the next key of every home, a key of its own)
    waves = [Wave(geo, [getattr(geo, kind)(b - 384, 17500, w)], w * 10**6, 2000,
                  [(b - 384, b - 384 + 17500)], run_of(b - 384, 17500),
                  capi.DEFRAG_RADIX_CLUSTER) for w, b in ((0, B), (1, 2 * B))]
    check_layout(cap, waves)


@pytest.mark.parametrize("ext", [32768, 32769])
def test_an_extension_at_its_limit(ext):
    """block 0's last cluster runs on for exactly 4 * kDfMax = 32768 positions (followed and
    counted: it is k_df_fix that then hands the long cluster to the radix sort) and for one more
    (k_df_count flags it).  Two such runs and the background need
    more rows than 4B + 1000 positions give: 6B + 1000, the partial last block kept."""
    cap = 6 * B + 1000
    geo = Geo(cap)
    path = capi.DEFRAG_RADIX_CLUSTER if ext <= 32768 else capi.DEFRAG_RADIX_EXTENT
    # (the runs overlap: the second copy takes the next key of every home, a key of its own)
    waves = [Wave(geo, [geo.one_per_home(b - 10, 10 + ext, w)], w * 10**6, 2000,
                  [(b - 10, b + ext)], run_of(b - 10, 10 + ext), path)
             for w, b in ((0, B), (1, 3 * B))]
    check_layout(cap, waves)


def wrap_multi(geo, bg=2000):
    """the top of the key range piles up at the last position and runs on into the first ones,
    where the smallest keys live; key 0 and the reserved key value among them"""
    n = 300
    waves = []
    for w in (0, 1):
        sets = [geo.largest(n, w * n), geo.smallest(n, 1 + w * n)]
        if w == 0 and geo.nshards == 1:
            sets.append(np.array([0, RESERVED], dtype=np.uint64))
        extra = len(sets[-1]) - 1 if len(sets) == 3 else 0
        # the top keys take cap - 1 and 0 .. n - 2, the small ones follow them
        waves.append(Wave(geo, sets, w * 10**6, bg, [(0, 2 * n + 2), (geo.cap - 1, geo.cap)],
                          [(geo.cap - 1, geo.cap - 1, True), (0, 2 * n - 2 + extra, True),
                           (2 * n - 1 + extra, 2 * n - 1 + extra, False)]))
    return waves


@pytest.mark.parametrize("cap", [2 * B, 2 * B + 1, 3 * B + 1000])
def test_the_wrapped_cluster_with_several_blocks(cap):
    """... a whole number of blocks, a last block of one position, a partial last block"""
    check_layout(cap, wrap_multi(Geo(cap)))


@pytest.mark.parametrize("order", ["top_then_small", "small_then_top", "one_push"])
def test_the_wrapped_cluster_covers_block_0(order):
    """17000 keys from the top of the key space home at cap - 1 and fill block 0 and the start
    of block 1; 50 small keys belong to the same cluster.  Pushed after the top keys they sit in
    block 1's lead and have not wrapped: block 1 skips its lead, the past-the-end rule of the
    last block takes wrapped entries only — they are block 0's, which extends although its every
    position is lead.  The blocks' counts must add up in every order of arrival; the 17000 keys
    of one home then are the radix sort's.  (4B + 1000 positions: two such clusters need more
    than the 37615 state rows of 3B + 1000.)"""
    cap = 4 * B + 1000
    geo = Geo(cap)
    ntop, nsmall = 17000, 50
    waves = []
    for w in (0, 1):
        top, small = geo.largest(ntop, w * ntop), geo.smallest(nsmall, 1 + w * nsmall)
        sets = {"top_then_small": [top, small], "small_then_top": [small, top],
                "one_push": [np.random.RandomState(w).permutation(np.concatenate([top, small]))]}
        waves.append(Wave(geo, sets[order], w * 10**6, 2000,
                          [(0, ntop + nsmall), (cap - 1, cap)],
                          [(cap - 1, cap - 1, True), (0, ntop + nsmall - 2, True),
                           (ntop + nsmall - 1, ntop + nsmall - 1, False)],
                          capi.DEFRAG_RADIX_CLUSTER))
    check_layout(cap, waves)


@pytest.mark.parametrize("shard", [2, 5])
def test_the_wrapped_cluster_of_a_shard(shard):
    """lo != 0 and a rounded mult; the last shard's range is longer than span: its top keys'
    homes clamp at cap - 1"""
    cap = 3 * B + 1000
    geo = Geo(cap, shard, 6)
    if shard == 5:
        assert ((geo.top - geo.lo) * geo.mult) >> 64 >= cap       # (clamped)
    check_layout(cap, wrap_multi(geo), shard=shard, nshards=6)


@pytest.mark.parametrize("table", [
    dict(opt=capi.OPT_FTRL, dim=4, init=capi.INIT_HASHNORM, seed=99),
    dict(opt=capi.OPT_SGD, dim=4),
], ids=["ftrl-hashnorm", "sgd"])
@pytest.mark.parametrize("layout", [straddle, wrap_multi], ids=["straddle", "wrap-multi"])
def test_whole_rows_move_with_their_keys(layout, table):
    """k_move_rows with dim = 4; a first-touch value (a hash of the key) travels with the key"""
    cap = 3 * B + 1000
    check_layout(cap, layout(Geo(cap)), **table)


def test_a_rehash_between_two_defrags():
    """2B + 1 positions: a wrapped cluster, defrag, a second one, then reserve(5B + 7) — k_rehash
    must leave every key inside the cluster of its home, and the second state buffer (of the old
    size) is dropped — and a cluster across a block end of the new geometry, defrag"""
    cap, cap2 = 2 * B + 1, 5 * B + 7
    old, new = Geo(cap), Geo(cap2)
    first, second = wrap_multi(old)
    third = Wave(new, [new.homed_at(3 * B - 100, 300)], 2 * 10**6, 2000,
                 [(3 * B - 100, 3 * B + 200)])
    both = np.concatenate(second.sets + third.sets)
    occ = new.occupied(both)
    assert occ[3 * B - 100:3 * B + 200].all() and occ[cap2 - 1] and occ[0]   # (it wraps again)
    exports = []
    for mode in (0, 1):
        capi.tune("key_build", mode)
        try:
            rng = np.random.RandomState(5)
            t, s = make_pair(cap)
            push_wave(t, s, first, rng, 1)
            settle_and_check(t, s, rng, 1, first.path if mode == 0 else capi.DEFRAG_RADIX_ASKED)
            push_wave(t, s, second, rng, 1)
            t.reserve(cap2)
            assert t.capacity == cap2
            compare(t, s)
            push_wave(t, s, third, rng, 1)
            settle_and_check(t, s, rng, 1, third.path if mode == 0 else capi.DEFRAG_RADIX_ASKED)
            exports.append(t.export())
        finally:
            capi.tune("key_build", 0)
    for a, b in zip(*exports):
        same(a, b)


@pytest.mark.parametrize("where", ["below", "above", "interleaved", "one"])
@pytest.mark.parametrize("total", [4096, 4097, 8192])
def test_the_merge_with_the_settled_tier_at_tile_cuts(total, where):
    """k_df_merge / merge_split: nA settled keys and nB new ones, nA + nB a whole tile, a tile
    and one key, two tiles; the new keys all below the tier's, all above, in between, or one"""
    cap = 1 << 16
    geo = Geo(cap)
    keys = np.sort(capi.hash_decimal_range(0, total))
    assert len(np.unique(keys)) == total
    new = {"below": np.arange(total) < 1000, "above": np.arange(total) >= total - 1000,
           "interleaved": np.arange(total) % 2 == 1, "one": np.arange(total) == total // 2}[where]
    waves = [Wave(geo, [keys[~new]], 0, 0), Wave(geo, [keys[new]], 0, 0)]
    check_layout(cap, waves)


# --------------------------------------------------------------- the second door: minibatches
def as_minibatch(rng, keys, per_row=4):
    """every key once, in any order, rows of per_row keys"""
    keys = rng.permutation(np.asarray(keys, dtype=np.uint64))
    R = (len(keys) + per_row - 1) // per_row
    rowptr = np.minimum(np.arange(R + 1, dtype=np.uint64) * np.uint64(per_row),
                        np.uint64(len(keys)))
    return rowptr, keys, rng.randint(0, 2, size=R).astype(np.int32)


def _mb_straddle(geo):
    k = geo.homed_at(B - 100, 300)
    return [k[::2], k[1::2]], [(B - 100, B + 200)], run_of(B - 100, 300), capi.DEFRAG_SORTFREE


def _mb_wrap_multi(geo):
    n = 300
    return ([np.concatenate([geo.largest(n), [np.uint64(RESERVED)]]),
             np.concatenate([[np.uint64(0)], geo.smallest(n, 1)])],
            [(0, 2 * n + 2), (geo.cap - 1, geo.cap)],
            [(geo.cap - 1, geo.cap - 1, True), (0, 2 * n - 1, True), (2 * n, 2 * n, False)],
            capi.DEFRAG_SORTFREE)


def _mb_wrap_over_block0(geo):
    ntop, nsmall = 17000, 50
    return ([geo.largest(ntop), geo.smallest(nsmall, 1)],
            [(0, ntop + nsmall), (geo.cap - 1, geo.cap)],
            [(geo.cap - 1, geo.cap - 1, True), (0, ntop + nsmall - 2, True),
             (ntop + nsmall - 1, ntop + nsmall - 1, False)], capi.DEFRAG_RADIX_CLUSTER)


@pytest.mark.parametrize("layout", [_mb_straddle, _mb_wrap_multi, _mb_wrap_over_block0],
                         ids=["straddle", "wrap-multi", "wrap-over-block0"])
def test_keys_that_arrive_in_minibatches(layout):
    """Table.push inserts through k_resolve; a training step inserts through the arrival build
    of xf_keybuild.hip (key_build = 3: no first-minibatch settle; a few settled keys to begin
    with, so that the minibatches are built against a tier: holes + an arrival segment).  The
    crafted keys come in two minibatches; defrag after the second, then two more steps."""
    cap = 3 * B + 1000
    geo = Geo(cap)
    rng = np.random.RandomState(11)
    halves, clear, expect, path = layout(geo)
    seedk = geo.background(5 * 10**6, 40, clear)
    mbs = [np.concatenate([geo.background(w * 10**6, 1000, clear), halves[w]]) for w in (0, 1)]
    Wave(geo, mbs, 0, 0, expect=expect)          # (the index the defrag reads: both minibatches)
    raws = [as_minibatch(rng, k) for k in mbs]
    ws = capi.Workspace()
    capi.tune("key_build", 3)
    try:
        t, s = make_pair(cap)
        g = rng.randn(len(seedk)).astype(np.float32)
        t.push(seedk, g)
        s.push(seedk, g)
        t.defrag()
        assert t.defrag_path == capi.DEFRAG_SORTFREE
        segs = steps_vs_oracle(t, s, raws, ws, 4, defrag_at=1)
        # new keys: a second segment over arrival rows (after the defrag only the reserved key
        # value, which is never settled, still makes one)
        assert segs[:2] == [2, 2], segs
        assert t.capacity == cap and t.defrag_path == path, (t.capacity, t.defrag_path)
        check_settled(t, s)
    finally:
        capi.tune("key_build", 0)
