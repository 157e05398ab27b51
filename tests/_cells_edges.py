"""Minibatches placed by state row, and a numpy model of the cell layout they compile to.

After `t.pull(keys); t.defrag()` the key of rank r in sorted order owns state row r
(include/xflow_amd.h: xf_table_settled), so a list of (row of the minibatch, state row) pairs
decides every (row window, chunk) cell's entry count exactly.  layout() is the model (xf_cells.h:
windows of W rows, cellptr in window-major order, forward blocks of kBlk entries, gradient work
items per chunk); the cases below state what structure they have, tests/test_cells_edges_cpu.py
holds the model to every statement, and the GPU tests (tests/test_gpu_grad_dense.py,
tests/test_gpu_fwd_blocks.py) run them against the exact-sum oracle and read from the launch
counters (capi.lr_grad_launches) which gradient kernel took them.  No GPU is needed here."""
import numpy as np

CHUNK = 2048        # xf::kChunk: state rows per chunk
WIN_MAX = 17408     # xf::kWinMax: rows per window at the most
SLICE_MAX = 8192    # xf::kSliceMax: entries of a chunk one gradient work item takes
BLK = 1024          # xf::kBlk: entries per forward block
TAG_MASK = 31       # xf::kTagMask: the chunk-number bits an entry carries
DENSE_WIN = 4       # xf::kDenseWin: row windows k_lr_grad_dense keeps in registers
ROUND = 2048        # entries per trip of k_lr_grad_dense's accumulate loop (256 threads x 8)


def geometry(R):
    """-> (nwin, W) as cells_alloc deals the rows out"""
    nwin = max(1, (R + WIN_MAX - 1) // WIN_MAX)
    return nwin, max(1, (R + nwin - 1) // nwin)


def dense_touch(NNZ, nitems):
    """launch_grad's choice of whole-line stores, computed the way the code computes it"""
    return float(NNZ) >= 0.3 * float(nitems) * float(CHUNK)


def layout(R, M, rows, srows):
    """the model: rows / srows are the entries' minibatch rows and state rows (any order)"""
    rows, srows = np.asarray(rows, np.int64), np.asarray(srows, np.int64)
    assert rows.shape == srows.shape
    assert not len(rows) or (0 <= rows.min() and rows.max() < R and 0 <= srows.min()
                             and srows.max() < M)
    nwin, W = geometry(R)
    nchunk = max(1, (M + CHUNK - 1) // CHUNK)
    cell = (rows // W) * nchunk + srows // CHUNK
    counts = np.bincount(cell, minlength=nwin * nchunk).reshape(nwin, nchunk)
    cellptr = np.concatenate([[0], np.cumsum(counts.ravel())])
    per_chunk = counts.sum(axis=0)
    slices = (per_chunk + SLICE_MAX - 1) // SLICE_MAX
    nsplit = int((slices > 1).sum())
    nitems = int(slices.sum())
    cs = np.sort(cell)
    nblk = (len(cs) + BLK - 1) // BLK
    blk_cell = np.concatenate([cs[::BLK][:nblk], [nwin * nchunk - 1]])
    # a forward block's span in every window it lies in: fwd_process clamps (lo, hi) to the window
    spans = []
    for b in range(nblk):
        lo, hi = int(blk_cell[b]), int(blk_cell[b + 1])
        last = int(cs[min(len(cs), (b + 1) * BLK) - 1])      # (the block's own last entry)
        for v in range(lo // nchunk, last // nchunk + 1):
            l, h = max(lo, v * nchunk), min(hi, (v + 1) * nchunk - 1)
            spans.append((b, v, l - v * nchunk, h - l + 1))
    if nwin > DENSE_WIN or nsplit:
        kernel = "cells"
    else:
        kernel = "dense_full" if dense_touch(len(rows), nitems) else "dense_masked"
    return dict(nwin=nwin, W=W, nchunk=nchunk, counts=counts, cellptr=cellptr,
                per_chunk=per_chunk, nsplit=nsplit, nitems=nitems, blk_cell=blk_cell,
                spans=spans, kernel=kernel, NNZ=len(rows))


def win_rows(R, v):
    """[first, end) rows of window v"""
    nwin, W = geometry(R)
    return v * W, min(R, (v + 1) * W)


class Case:
    """name, shape (R rows, M state rows), the entries, and what the case claims:
    cells {(window, chunk): entries}, the kernel launch_grad picks by itself, and, for the forward
    cases, spans: {(block, window): cells spanned}"""

    def __init__(self, name, R, M, rows, srows, cells, kernel, spans=None, totals=None):
        self.name, self.R, self.M = name, R, M
        self.rows, self.srows = np.asarray(rows, np.int64), np.asarray(srows, np.int64)
        self.cells, self.kernel, self.spans, self.totals = dict(cells), kernel, spans, totals

    def __repr__(self):
        return self.name

    def layout(self):
        return layout(self.R, self.M, self.rows, self.srows)

    def raw(self, sorted_keys, seed=0, more=None):
        """(rowptr, keys, labels): the entries grouped by row (a row keeps their given order),
        both labels present.  more: (rows, keys) of further entries, appended to their rows —
        keys the table has not seen make a second segment of cells"""
        assert len(sorted_keys) == self.M
        rows, keys = self.rows, np.asarray(sorted_keys, np.uint64)[self.srows]
        if more is not None:
            rows = np.concatenate([rows, np.asarray(more[0], np.int64)])
            keys = np.concatenate([keys, np.asarray(more[1], np.uint64)])
        order = np.argsort(rows, kind="stable")
        lens = np.bincount(rows, minlength=self.R)
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        labels = np.random.RandomState(1000 + seed).randint(0, 2, size=self.R).astype(np.int32)
        if self.R > 1:
            labels[0], labels[1] = 0, 1
        return rowptr, keys[order], labels

    def raw_valued(self, sorted_keys, values, seed=0):
        """(rowptr, keys, vals, labels) with values(rng, row lengths) per nonzero
        (tests/_valued_cases.py: _values, the values in general position)"""
        rowptr, keys, labels = self.raw(sorted_keys, seed=seed)
        lens = np.diff(rowptr.astype(np.int64))
        return rowptr, keys, values(np.random.RandomState(50 + seed), lens), labels


def place(name, R, M, cells, kernel, seed=0, rin=None, pos=None, **kw):
    """a case from {(window, chunk): n}: n entries in that cell, rows and positions random within
    it, or rin(v, c, n, nrows) / pos(v, c, n, npos) choose the rows-in-window / positions"""
    rng = np.random.RandomState(seed)
    rows, srows = [], []
    for (v, c), n in sorted(cells.items()):
        r0, r1 = win_rows(R, v)
        npos = min(CHUNK, M - c * CHUNK)
        assert r1 > r0 and npos > 0, (name, v, c)
        a = rin(v, c, n, r1 - r0) if rin else rng.randint(0, r1 - r0, size=n)
        p = pos(v, c, n, npos) if pos else rng.randint(0, npos, size=n)
        rows.append(r0 + np.asarray(a, np.int64))
        srows.append(c * CHUNK + np.asarray(p, np.int64))
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, np.int64)   # noqa: E731
    return Case(name, R, M, cat(rows), cat(srows), {k: n for k, n in cells.items() if n}, kernel,
                **kw)


def deal(total, parts):
    """total entries dealt over `parts` cells as evenly as integers allow"""
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


R4 = 4 * WIN_MAX            # 69632: four full windows
R2 = WIN_MAX + 1            # 17409: windows of 8705 and 8704
R4S = 3 * WIN_MAX + 1       # 52225: four windows of 13057, 13057, 13057 and 13054 (a shorter last)
M3 = 3 * CHUNK


# ------------------------------------------------------------------------------ the gate
def gate_cases():
    out = []
    for R in (17408, 17409, 34817, 52225, 69632, 69633):
        nwin, _ = geometry(R)
        cells = {(v, c): 40 + 7 * v + 3 * c for v in range(nwin) for c in range(3)}
        out.append(place("gate-R%d" % R, R, M3, cells,
                         "dense_masked" if nwin <= DENSE_WIN else "cells", seed=R))
    for n in (SLICE_MAX, SLICE_MAX + 1):
        q = deal(n, 2)
        cells = {(0, 0): 10, (1, 0): 20, (0, 1): q[0], (1, 1): q[1], (1, 2): 5}
        # (8192 entries over three chunks: more than 0.3 a row, whole-line stores)
        out.append(place("gate-chunk-of-%d" % n, R2, M3, cells,
                         "dense_full" if n <= SLICE_MAX else "cells", seed=n,
                         totals={1: n}))
    return out


# ------------------------------------------------------------------------- store variant
def store_cases():
    """five chunks touched, one entry either side of NNZ >= 0.3 * nitems * kChunk = 3072"""
    out = []
    for nnz in (3071, 3072):
        cells = dict(zip([(v, c) for c in range(5) for v in range(2)], deal(nnz, 10)))
        out.append(place("store-%d" % nnz, R2, 5 * CHUNK, cells,
                         "dense_full" if dense_touch(nnz, 5) else "dense_masked", seed=nnz))
    assert [c.kernel for c in out] == ["dense_masked", "dense_full"]
    return out


# ------------------------------------------------------------------------------- windows
def window_cases():
    """one minibatch per window count: every chunk has its own pattern of occupied windows"""
    out = []
    for R, tag in ((R4S, "four"), (R2, "two")):
        nwin, W = geometry(R)
        last = nwin - 1
        mid = list(range(1, last)) or [0]
        pats = [list(range(nwin)), [0], [last], sorted({0, last}), mid]
        cells = {}
        for c, wins in enumerate(pats):
            for v in wins:
                cells[(v, c)] = 60 + 11 * v + c
        for v in range(nwin):
            cells[(v, 5)] = 1                                   # one entry per window
        out.append(place("windows-%s" % tag, R, 7 * CHUNK, cells, "dense_masked", seed=nwin))
        # row-in-window 0 and W - 1 of every window, and row R - 1 of the (shorter) last one
        ends = {(v, c): 2 for v in range(nwin) for c in range(2)}

        def rin(v, c, n, nrows):
            return [0, nrows - 1]
        out.append(place("window-ends-%s" % tag, R, 2 * CHUNK, ends, "dense_masked", seed=nwin,
                         rin=rin))
        assert out[-1].rows.max() == R - 1 and win_rows(R, last)[1] - win_rows(R, last)[0] < W
    return out


# -------------------------------------------------------------------------------- rounds
ROUND_TOTALS = (1, 2047, 2048, 2049, 4096, 4097, 8191, 8192)


def round_cases():
    """chunk c of one four-window minibatch holds ROUND_TOTALS[c] entries; a second minibatch
    puts a round boundary inside a window's cell (chunk 0: cells of 1000, 1500, ...) and exactly
    on a cell boundary (chunk 1: c1 = 2048)"""
    cells = {}
    for c, n in enumerate(ROUND_TOTALS):
        for v, q in enumerate(deal(n, 4)):
            cells[(v, c)] = q
    a = place("round-totals", R4, len(ROUND_TOTALS) * CHUNK, cells, "dense_full", seed=5,
              totals=dict(enumerate(ROUND_TOTALS)))
    cells = {(0, 0): 1000, (1, 0): 1500, (2, 0): 700, (3, 0): 900,
             (0, 1): 2048, (1, 1): 2048, (2, 1): 1, (3, 1): 2047}
    b = place("round-boundaries", R4, 2 * CHUNK, cells, "dense_full", seed=6,
              totals={0: 4100, 1: 6144})
    return [a, b]


# ----------------------------------------------------------------------------- positions
def position_cases():
    out = []
    out.append(place("positions-0-1-2047", R2, CHUNK, {(0, 0): 3, (1, 0): 3}, "dense_masked",
                     pos=lambda v, c, n, npos: [0, 1, 2047]))
    # a key twice in one row (and once in another)
    out.append(Case("key-twice-in-a-row", R2, CHUNK, [5, 5, 9000, 5], [77, 77, 77, 3],
                    {(0, 0): 3, (1, 0): 1}, "dense_masked"))
    out.append(place("one-key-8192-times", R2, CHUNK, {(0, 0): 4096, (1, 0): 4096}, "dense_full",
                     seed=2, pos=lambda v, c, n, npos: np.full(n, 1234), totals={0: 8192}))
    out.append(place("all-2048-positions-once", R2, CHUNK, {(0, 0): 1024, (1, 0): 1024},
                     "dense_full", seed=3,
                     pos=lambda v, c, n, npos: np.arange(n) * 2 + v, totals={0: 2048}))
    out.append(place("first-and-last-of-30-chunks", R2, 30 * CHUNK,
                     {(0, 0): 50, (1, 0): 50, (0, 29): 50, (1, 29): 50}, "dense_masked", seed=4))
    return out


# -------------------------------------------------------------- the end of the index space
def end_cases():
    """M = 2048c - 1, 2048c, 2048c + 1 (c = 2) with the last state row touched"""
    out = []
    for M in (2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):
        nchunk = (M + CHUNK - 1) // CHUNK
        lastc = nchunk - 1
        cells = {(v, c): 30 for v in range(2) for c in range(nchunk)}
        cells[(1, lastc)] = 3

        def pos(v, c, n, npos, lastc=lastc):
            if c == lastc:      # (17 entries on the last row: an odd number of +-0.5 never cancels)
                k = (n + 1) // 2
                return np.concatenate([np.full(k, npos - 1), np.arange(n - k) % npos])
            return np.random.RandomState(c + 10 * v).randint(0, npos, size=n)
        out.append(place("end-M%d" % M, R2, M, cells, "dense_masked", pos=pos))
        assert out[-1].srows.max() == M - 1
    return out


def grad_cases():
    return (gate_cases() + store_cases() + window_cases() + round_cases() + position_cases() +
            end_cases())


# ------------------------------------------------------------------- forward cell decode
def _fwd(name, R, nchunk, cells, spans, seed=0):
    return place(name, R, nchunk * CHUNK, cells, "dense_masked", seed=seed, spans=spans)


def fwd_cases():
    """forward blocks of kBlk entries by the cells they span: fwd_process decodes a cell from the
    entry's 5 chunk-number bits when hi - lo <= kTagMask (a span of at most 32 cells) and searches
    cellptr otherwise.  spans: {(block, window): cells}."""
    out = []
    # block 0 spans exactly 31, 32, 33 and 100 cells: entry 1024 (the next block's first) lies in
    # the span's last cell, and so do entries of block 0 itself except at 32 (31 cells of 33 are
    # 1023 entries) — at 33 cells the 32 of 31 entries leave block 0 thirty-two entries in cell 32,
    # which a tag decode taken one cell too far (hi - lo <= 32) would put into cell 0
    for span, per in ((31, 34), (32, 33), (33, 31), (100, 10)):
        cells = {(0, c): per for c in range(span - 1)}
        cells[(0, span - 1)] = BLK + 1 - per * (span - 1)
        assert 0 < cells[(0, span - 1)]
        out.append(_fwd("fwd-span-%d" % span, 300, span + 2, cells, {(0, 0): span}, seed=span))
    # a near block whose cells start at chunk 40: the tag wraps past 32
    cells = {(0, c): 33 for c in range(40, 71)}
    cells[(0, 71)] = BLK + 1 - 31 * 33
    out.append(_fwd("fwd-near-from-chunk-40", 300, 80, cells, {(0, 0): 32}, seed=40))
    # two windows, nchunk = 37: a block that begins in window 0's last cells (700 entries) and
    # ends in window 1, whose cells before `first` are empty.  first = 0 / 20: the block ends in
    # window 1's 9th filled cell (9 and 29 cells: both decoded from the tag); first = 30: the
    # minibatch's only block, closed by the last cell of all (37 cells of window 1: searched)
    for first, span in ((0, 9), (20, 29), (30, 37)):
        cells = {(0, c): 100 for c in range(30, 37)}
        for c in range(first, 37):
            cells[(1, c)] = 40
        out.append(_fwd("fwd-across-windows-first-%d" % first, R2, 37, cells,
                        {(0, 0): 7, (0, 1): span}, seed=37 + first))
    # a shorter last window (13054 rows of 13057) whose entries all lie in a block shared with
    # its neighbour.  (A last window of ONE row cannot be compiled from a minibatch: cells_alloc
    # deals R rows over nwin windows of ceil(R / nwin), so the last holds more than W - nwin.)
    out.append(_fwd("fwd-short-last-window", R4S, 3, {(2, 0): 200, (2, 2): 300, (3, 1): 6},
                    {(0, 2): 3, (0, 3): 3}, seed=1))
    return out


# ------------------------------------------- the streams of the tests from before (the table
# of DESIGN "Which gradient kernel the tests reach"): entries per chunk of kChunk state rows
def stream_chunk_counts(keys, known=None):
    """a minibatch's entries per chunk when the table holds exactly the keys seen so far (known:
    the keys of the minibatches before) and state rows are dealt out in key order"""
    keys = np.asarray(keys, np.uint64)
    table = np.unique(keys if known is None else np.concatenate([known, keys]))
    srow = np.searchsorted(table, keys)
    return np.bincount(srow // CHUNK, minlength=(len(table) + CHUNK - 1) // CHUNK)
