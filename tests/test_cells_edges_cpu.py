"""tests/_cells_edges.py's cases have the structure they claim (no GPU): per-cell entry counts,
chunk totals, split chunks, the kernel launch_grad picks by itself, the span of the forward blocks;
and the random streams of the GPU tests from before this file split their chunks — which is why
they never reached k_lr_grad_dense — while the unsplit streams added beside them do not."""
import numpy as np
import pytest

from oracle import pyoracle as O

from . import _cells_edges as E
from . import _hyper_cases as HC
from . import _valued_cases as VC
from . import _valued_checker as V

GRAD = E.grad_cases()
FWD = E.fwd_cases()


def by_name(name):
    return next(c for c in GRAD + FWD if c.name == name)


@pytest.mark.parametrize("case", GRAD + FWD, ids=repr)
def test_the_model_has_the_cells_the_case_names(case):
    L = case.layout()
    got = {(v, c): int(L["counts"][v, c]) for v in range(L["nwin"]) for c in range(L["nchunk"])
           if L["counts"][v, c]}
    assert got == case.cells
    assert L["cellptr"][-1] == L["NNZ"] == len(case.rows) and len(L["cellptr"]) == \
        L["nwin"] * L["nchunk"] + 1
    assert L["kernel"] == case.kernel
    assert (L["per_chunk"] == sum(L["counts"][v] for v in range(L["nwin"]))).all()
    for c, n in (case.totals or {}).items():
        assert L["per_chunk"][c] == n, (c, L["per_chunk"][c], n)
    spans = {(b, v): n for b, v, _, n in L["spans"]}
    for k, n in (case.spans or {}).items():
        assert spans[k] == n, (k, spans[k], n)
    # the minibatch it compiles from holds the same entries, row by row
    rowptr, keys, labels = case.raw(np.arange(case.M, dtype=np.uint64) * 3 + 1)
    assert len(labels) == case.R and rowptr[-1] == len(keys) == len(case.rows)
    rows = np.repeat(np.arange(case.R), np.diff(rowptr.astype(np.int64)))
    again = E.layout(case.R, case.M, rows, (keys.astype(np.int64) - 1) // 3)
    assert (again["counts"] == L["counts"]).all()


def test_the_gate():
    want = {17408: 1, 17409: 2, 34817: 3, 52225: 4, 69632: 4, 69633: 5}
    for R, nwin in want.items():
        L = by_name("gate-R%d" % R).layout()
        assert L["nwin"] == nwin and L["nsplit"] == 0
        assert (L["kernel"] == "cells") == (nwin > E.DENSE_WIN)
    a, b = by_name("gate-chunk-of-8192").layout(), by_name("gate-chunk-of-8193").layout()
    assert a["per_chunk"].max() == E.SLICE_MAX and a["nsplit"] == 0 and a["nitems"] == 3
    assert b["per_chunk"].max() == E.SLICE_MAX + 1 and b["nsplit"] == 1 and b["nitems"] == 4


def test_the_store_threshold():
    a, b = by_name("store-3071").layout(), by_name("store-3072").layout()
    assert a["nitems"] == b["nitems"] == 5 and (a["NNZ"], b["NNZ"]) == (3071, 3072)
    assert 0.3 * 5.0 * 2048.0 == 3072.0
    assert (a["kernel"], b["kernel"]) == ("dense_masked", "dense_full")


@pytest.mark.parametrize("tag,nwin", [("four", 4), ("two", 2)])
def test_the_window_patterns(tag, nwin):
    L = by_name("windows-%s" % tag).layout()
    assert L["nwin"] == nwin
    occ = [tuple(np.flatnonzero(L["counts"][:, c])) for c in range(L["nchunk"])]
    last = nwin - 1
    assert occ[0] == tuple(range(nwin)) and occ[1] == (0,) and occ[2] == (last,)
    assert occ[3] == (0, last)
    assert occ[4] == (tuple(range(1, last)) if nwin > 2 else (0,))
    assert (L["counts"][:, 5] == 1).all() and occ[6] == ()
    c = by_name("window-ends-%s" % tag)
    rin = c.rows % L["W"]
    for v in range(nwin):
        r0, r1 = E.win_rows(c.R, v)
        assert set(rin[c.rows // L["W"] == v]) == {0, r1 - r0 - 1}
    assert c.rows.max() == c.R - 1 and E.win_rows(c.R, last)[1] - E.win_rows(c.R, last)[0] < L["W"]


def test_the_rounds():
    L = by_name("round-totals").layout()
    assert tuple(L["per_chunk"]) == E.ROUND_TOTALS == (1, 2047, 2048, 2049, 4096, 4097, 8191, 8192)
    assert L["nwin"] == 4 and L["nsplit"] == 0
    L = by_name("round-boundaries").layout()
    cum = np.cumsum(L["counts"], axis=0)           # c1, c2, c3, total of every chunk
    # chunk 0: the boundaries at 2048 and 4096 fall strictly inside cells
    assert cum[0, 0] < E.ROUND < cum[1, 0] and cum[2, 0] < 2 * E.ROUND < cum[3, 0]
    # chunk 1: c1 == 2048 and c2 == 4096: boundaries exactly between two cells
    assert cum[0, 1] == E.ROUND and cum[1, 1] == 2 * E.ROUND and cum[3, 1] == 3 * E.ROUND


def test_the_positions():
    c = by_name("positions-0-1-2047")
    assert sorted(set(c.srows)) == [0, 1, 2047]
    c = by_name("key-twice-in-a-row")
    rp, keys, _ = c.raw(np.arange(c.M, dtype=np.uint64))
    assert list(keys[int(rp[5]):int(rp[6])]) == [77, 77, 3]
    c = by_name("one-key-8192-times")
    assert len(c.srows) == 8192 and set(c.srows) == {1234}
    c = by_name("all-2048-positions-once")
    assert sorted(c.srows) == list(range(2048))
    c = by_name("first-and-last-of-30-chunks")
    assert sorted(np.flatnonzero(c.layout()["per_chunk"])) == [0, 29]


def test_the_end_of_the_index_space():
    for M in (4095, 4096, 4097):
        c = by_name("end-M%d" % M)
        assert c.M == M and c.srows.max() == M - 1 and c.layout()["nchunk"] == (M + 2047) // 2048


def test_the_forward_blocks():
    for span in (31, 32, 33, 100):
        L = by_name("fwd-span-%d" % span).layout()
        b, v, first, n = L["spans"][0]
        assert (first, n) == (0, span) and L["blk_cell"][1] - L["blk_cell"][0] == span - 1
        # the decision of fwd_process: hi - lo <= kTagMask
        assert (L["blk_cell"][1] - L["blk_cell"][0] <= E.TAG_MASK) == (span <= 32)
        if span == 33:      # block 0 holds entries of its own in cell 32, whose tag is cell 0's
            assert L["cellptr"][32] == 992 and L["cellptr"][33] == 1025
    L = by_name("fwd-near-from-chunk-40").layout()
    assert L["spans"][0] == (0, 0, 40, 32)
    for first, span in ((0, 9), (20, 29), (30, 37)):
        L = by_name("fwd-across-windows-first-%d" % first).layout()
        assert L["nchunk"] == 37 and L["nwin"] == 2
        assert L["spans"][0] == (0, 0, 30, 7) and L["spans"][1] == (0, 1, 0, span)
        assert not L["counts"][1, :first].any() and L["counts"][1, first:].all()
    L = by_name("fwd-short-last-window").layout()
    assert len(L["blk_cell"]) == 2 and L["counts"][3].sum() == 6 and L["counts"][2].sum() == 500


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("name", ["fwd-span-32", "fwd-span-33"])
def test_the_valued_forward_cases_have_exact_sums(name, opt):
    """the checker alone over what tests/test_gpu_fwd_blocks.py runs on valued cells: every sum it
    forms is exact, so the comparison there is bit for bit"""
    c = by_name(name)
    settle = np.sort(np.array([O.hash_str(str(i)) for i in range(c.M)], np.uint64))
    sw = O.Store(O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD, 1)
    sw.import_(*VC.old_state(settle, opt, 1, "w"))
    rowptr, keys, vals, labels = c.raw_valued(settle, VC._values)
    audit = []
    for _ in range(2):
        V.lr_step(sw, rowptr, keys, vals, labels, audit)
    V.lr_predict(sw, rowptr, keys, vals, labels, audit)
    V.assert_exact(audit)


def test_no_minibatch_has_a_last_window_of_one_row():
    """the rows are dealt out evenly (cells_alloc): above one window the last holds thousands"""
    for nwin in range(2, 8):
        for R in ((nwin - 1) * E.WIN_MAX + 1, nwin * E.WIN_MAX):
            assert E.geometry(R)[0] == nwin
            assert E.win_rows(R, nwin - 1)[1] - E.win_rows(R, nwin - 1)[0] > E.WIN_MAX // 2 - nwin


# ------------------------------------------------------ the streams of the tests from before
def _chunks(raws):
    """per minibatch: (chunks, largest entry count of a chunk, chunks over kSliceMax), the table
    holding every key of the stream in key order"""
    known = np.unique(np.concatenate([r[1] for r in raws]))
    out = []
    for r in raws:
        pc = E.stream_chunk_counts(r[1], known)
        out.append((len(pc), int(pc.max()), int((pc > E.SLICE_MAX).sum())))
    return out


def test_the_random_streams_split_their_chunks_and_the_unsplit_ones_do_not():
    """Counted with the real hashed keys.  A minibatch with ONE split chunk goes to
    k_lr_grad_cells whole (launch_grad), so none of these streams reaches k_lr_grad_dense; the
    second streams (HC.cells_raw_unsplit, HC.old_weight_raw_unsplit) keep every chunk whole."""
    # test_gpu_cells.py::test_every_variant..., test_gpu_hyper.py::...under_every_set
    assert _chunks(HC.cells_raw()) == [(59, 20881, 59), (59, 222808, 34), (59, 20732, 59)]
    # test_the_old_weight_is_derived..., test_import_vouches_for_w...
    assert _chunks(HC.old_weight_raw()) == [(15, 16598, 15), (15, 50334, 9)]
    for raws in (HC.cells_raw_unsplit(), HC.old_weight_raw_unsplit()):
        for n, most, over in _chunks(raws):
            assert over == 0 and most <= 0.85 * E.SLICE_MAX, (n, most)
    # test_gpu_entry_streams.py::ref_windows: 1 to 3 nonzeros a row over 5 000 keys (three chunks)
    # split two or three of them; over 40 000 keys (its second stream) none
    keys = {n: np.array([O.hash_str(str(i)) for i in range(n)], np.uint64) for n in (5000, 40000)}
    rank = {n: np.argsort(np.argsort(k)) for n, k in keys.items()}
    for R, want in ((17408, 2), (17409, 2), (34817, 3)):
        for nkeys in (5000, 40000):
            rng = np.random.RandomState(R + (0 if nkeys == 5000 else 50))
            for _ in range(2):
                lens = rng.randint(1, 4, size=R)                    # (mb()'s draws, in its order)
                srow = rank[nkeys][rng.randint(0, nkeys, size=int(lens.sum()))]
                rng.randint(0, 2, size=R)
                pc = np.bincount(srow // E.CHUNK)
                over = int((pc > E.SLICE_MAX).sum())
                assert over == (want if nkeys == 5000 else 0), (R, nkeys, pc)
