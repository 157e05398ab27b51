"""The edge streams of the valued cells tests (tests/test_valued_cells_cpu.py runs the checker of
tests/_valued_checker.py alone over them and asserts that every one of its sums is exact;
tests/test_gpu_valued_cells.py compares the GPU's local valued build and cell kernels with it on
the same streams, bit for bit).

Built from the generators of tests/_valued_cases.py — its values (_values), its key table, its
"many steps old" table state (old_state) — so that the exactness argument made there holds here:
only the row structure differs, chosen to hit the edges of the cells (xf_cells.h): a second row
window, a chunk cut into slices, fewer entries than one forward block, one entry more than whole
blocks, no nonzero at all, a key twice in one row, a fresh table that has to grow.

Every stream is a list of minibatches (rowptr, keys, values, labels); EDGES[name] says whether its
table starts aged (old_state over the stream's keys) or fresh, and with what capacity."""
import numpy as np

from tests import _valued_cases as Cs
from tests import _valued_checker as V

CASES = Cs.CASES
OPTS = Cs.OPTS
old_state = Cs.old_state
stream = Cs.stream
stream_keys = Cs.stream_keys

WIN_MAX = 17408         # xf::kWinMax: rows per window
BLK = 1024              # xf::kBlk: entries per forward block
SLICE_MAX = 8192        # xf::kSliceMax: entries of a chunk one gradient work item takes


def _rows(rng, lens, K, p=None):
    """a minibatch of the given row lengths over the first K keys of the key table"""
    lens = np.asarray(lens, np.int64)
    rowptr = np.r_[0, np.cumsum(lens)].astype(np.uint64)
    n = int(rowptr[-1])
    tab = Cs._keytab(K)
    keys = tab[rng.choice(K, size=n, p=p)] if n else np.zeros(0, np.uint64)
    vals = Cs._values(rng, lens) if n else np.zeros(0, np.float32)
    labels = rng.randint(0, 2, size=len(lens)).astype(np.int32)
    return rowptr, keys, vals, labels


def two_windows(seed=0):
    """kWinMax + 100 rows of 1 to 3 nonzeros: two row windows"""
    rng = np.random.RandomState(100 + seed)
    R = WIN_MAX + 100
    return _rows(rng, rng.randint(1, 4, size=R), 3000)


def split_chunk(seed=0, R=10000, K=5000, rows_with_head=9000):
    """Zipf(1.1) keys as zipf_chunks, about 50 000 nonzeros over K keys (three chunks of state
    rows), plus one more key that 9000 of the rows hold once each: its chunk holds more than
    kSliceMax entries and is cut into slices"""
    rng = np.random.RandomState(200 + seed)
    p = 1.0 / np.arange(1, K + 1) ** 1.1
    p /= p.sum()
    lens = rng.randint(3, 8, size=R)                      # 5 on average
    rowptr, keys, vals, labels = _rows(rng, lens, K, p)
    head = Cs._keytab(K + 1)[K]                           # a key of its own
    rows = np.sort(rng.choice(R, size=rows_with_head, replace=False))
    keys[rowptr[rows + 1].astype(np.int64) - 1] = head    # the last nonzero of those rows
    return rowptr, keys, vals, labels


def below_blk(seed=0):
    """fewer nonzeros than one forward block"""
    rng = np.random.RandomState(300 + seed)
    mb = _rows(rng, rng.randint(0, 12, size=90), 400)
    assert 0 < len(mb[1]) < BLK
    return mb


def blk_plus_one(seed=0, k=3):
    """1024 k + 1 nonzeros: the last block holds one entry"""
    rng = np.random.RandomState(400 + seed)
    lens = rng.randint(1, 30, size=400)
    want = BLK * k + 1
    cut = int(np.searchsorted(np.cumsum(lens), want))     # rows [0, cut] reach `want`
    lens = lens[:cut + 1].copy()
    lens[-1] -= int(lens.sum()) - want
    assert lens.sum() == want and lens[-1] > 0
    return _rows(rng, lens, 2500)


def empty():
    """no row at all"""
    return (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.float32),
            np.zeros(0, np.int32))


def empty_rows(R=3):
    """rows without a nonzero"""
    return (np.zeros(R + 1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.float32),
            np.array([1, 0, 1][:R], np.int32))


# name -> (minibatches, aged table?, table capacity)
def edge(name):
    if name == "two_windows":
        return [two_windows(0), two_windows(1)], True, 1 << 16
    if name == "split_chunk":
        return [split_chunk(0), split_chunk(1)], True, 1 << 16
    if name == "below_blk":
        return [below_blk(0), below_blk(1)], True, 1 << 16
    if name == "blk_plus_one":
        return [blk_plus_one(0), blk_plus_one(1)], True, 1 << 16
    if name == "empty":             # (between two minibatches that hold something)
        return [Cs.ragged(0), empty(), Cs.ragged(1)], True, 1 << 16
    if name == "empty_rows":
        return [Cs.ragged(0), empty_rows(), Cs.ragged(1)], True, 1 << 16
    if name == "twice_in_row":      # row 1 of ragged: key A with 0.75, ..., key A with -1.5
        return [Cs.ragged(5)], True, 1 << 16
    if name == "fresh_grow":        # a fresh table's first minibatch, its keys many times over,
        return [Cs.zipf(9, 400, 14, 3000)], False, 1024   # more keys than 0.6 of the capacity
    raise KeyError(name)


EDGES = ("two_windows", "split_chunk", "below_blk", "blk_plus_one", "empty", "empty_rows",
         "twice_in_row", "fresh_grow")


def expected_loss(loss, labels):
    """the checker's loss of a step; a minibatch without a key (the checker returns nothing): every
    row's sum is +0"""
    if len(loss) == len(labels):
        return loss
    return (V._sigmoid(np.zeros(len(labels), np.float32)) - labels.astype(np.float32)) \
        .astype(np.float32)


def run_checker(opt, mbs, aged, audit):
    """the checker over a stream: -> the loss per step, the store after the stream, the last
    minibatch's predictions (a caller replays with V.lr_step on the store it is given)"""
    ws, _ = Cs.stores("lr", opt, 1, mbs if aged else None)
    losses = []
    for rowptr, keys, vals, labels in mbs:
        loss = V.lr_step(ws, rowptr, keys, vals, labels, audit)[2]
        losses.append(expected_loss(loss, labels))
    rowptr, keys, vals, labels = mbs[-1]
    return losses, ws, V.lr_predict(ws, rowptr, keys, vals, labels, audit)
