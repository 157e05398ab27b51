"""Sliced progressive validation on real hardware, everything with == against the restatement
(tests/_slices_checker.py): the extract kernel (host and device entry), the accumulate kernel and
the table's contract (resident keys exact, none apart, overflow = the rest, the sum = the whole
stream), the tap of the training steps (tables bit for bit those without slices), two ranks on one
GPU with a merged read."""
import os
import re
import shutil
import subprocess
import traceback

import numpy as np
import pytest

from xflow_amd import build, capi

from . import _progress_checker as P
from . import _sharded_modes_checker as M
from . import _slices_checker as S
from . import test_gpu_progress as TP          # the step paths' runners (the module, not its tests)
from . import test_gpu_sharded_modes as SM     # _spawn, _trainer, _import_old
from .conftest import GOLDEN
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
NONE = S.NONE


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def _dev(a, as_type):
    """a numpy array on the device (torch has no unsigned 32 / 64: same bytes, signed)"""
    import torch
    a = np.ascontiguousarray(a)
    if len(a) == 0:
        return None, 0
    t = torch.from_numpy(a.view(as_type)).cuda()
    return t, t.data_ptr()


# ------------------------------------------------------------------ extract
def _csr(lengths, member_at, F, rng, other_fields=(0, 1, 2, 5, 2 ** 31 - 1)):
    """rows of the given lengths; member_at[r]: the positions of row r that carry field F"""
    rowptr = np.zeros(len(lengths) + 1, np.uint64)
    rowptr[1:] = np.cumsum(np.asarray(lengths, np.uint64))
    nnz = int(rowptr[-1])
    keys = rng.integers(1, 2 ** 62, size=nnz, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    others = np.array([f for f in other_fields if f != F], np.int32)
    fgid = others[rng.integers(0, len(others), size=nnz)].astype(np.int32)
    for r, pos in enumerate(member_at):
        for p in pos:
            fgid[int(rowptr[r]) + p] = F
    return rowptr, keys, fgid


def _extract_every_way(F, rowptr, keys, fgid, row_begin=0, row_end=None):
    """the host entry and the device entry on the same row slice, both against the restatement"""
    row_end = len(rowptr) - 1 if row_end is None else row_end
    s = capi.Slices(F, 2)
    want = S.ids_of(rowptr, keys, fgid, F)[row_begin:row_end]
    got = s.extract(rowptr, keys, fgid, row_begin, row_end)
    assert got.dtype == np.uint64 and got.tolist() == want.tolist(), "host entry"
    base, end = int(rowptr[row_begin]), int(rowptr[row_end])
    rp32 = (rowptr[row_begin:row_end + 1] - np.uint64(base)).astype(np.uint32)
    tk, pk = _dev(keys[base:end], np.int64)
    tf, pf = _dev(fgid[base:end], np.int32)
    tr, pr = _dev(rp32, np.int32)
    R = row_end - row_begin
    d = s.extract_dev(pk or None, pf or None, pr or None, R, end - base)
    got = capi.Slices.download_ids(d, R)
    assert got.tolist() == want.tolist(), "device entry"
    # the inputs pass through unchanged
    if tk is not None:
        assert np.array_equal(tk.cpu().numpy().view(np.uint64), keys[base:end])
        assert np.array_equal(tf.cpu().numpy(), fgid[base:end])
    return want


LENS = [1, 63, 64, 65, 128, 129, 5000]


@pytest.mark.parametrize("F", [0, 3, 2 ** 31 - 1])
def test_extract_lengths_and_member_positions(F):
    rng = np.random.default_rng(F % 1000)
    lengths, member_at = [], []
    for n in LENS:
        for pos in ([0], [min(63, n - 1)], [min(64, n - 1)], [n - 1], []):
            lengths.append(n)
            member_at.append(sorted(set(pos)))
        lengths.append(n)                                    # several members: the first wins
        member_at.append(sorted({n // 3, n // 2, n - 1}))
    lengths += [5000, 5000]                                  # deep inside a long row
    member_at += [[4999], [2 * 64, 77 * 64 + 5]]
    rowptr, keys, fgid = _csr(lengths, member_at, F, rng)
    want = _extract_every_way(F, rowptr, keys, fgid)
    for r, pos in enumerate(member_at):
        assert int(want[r]) == (int(keys[int(rowptr[r]) + pos[0]]) if pos else NONE)
    _extract_every_way(F, rowptr, keys, fgid, 5, len(lengths) - 3)    # a row slice


def test_extract_empty_inputs_and_empty_rows():
    rng = np.random.default_rng(1)
    s = capi.Slices(3, 2)
    assert s.extract(np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32)).size == 0
    assert capi.Slices.download_ids(s.extract_dev(None, None, None, 0, 0), 0).size == 0
    # NNZ = 0 with rows
    ids = _extract_every_way(3, np.zeros(6, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32))
    assert ids.tolist() == [NONE] * 5
    # empty rows first, last and in runs
    lengths = [0, 0, 3, 0, 0, 0, 2, 70, 0, 1, 0]
    member_at = [[], [], [1], [], [], [], [], [69], [], [0], []]
    rowptr, keys, fgid = _csr(lengths, member_at, 3, rng)
    ids = _extract_every_way(3, rowptr, keys, fgid)
    assert [int(i) != NONE for i in ids] == [bool(m) for m in member_at]
    _extract_every_way(3, rowptr, keys, fgid, 3, 6)          # a slice of empty rows only
    _extract_every_way(3, rowptr, keys, fgid, 4, 4)          # R = 0 inside


def test_extract_a_key_equal_to_none_and_module_function():
    rowptr = np.array([0, 2, 4], np.uint64)
    keys = np.array([5, NONE, 7, 9], np.uint64)
    fgid = np.array([1, 3, 3, 3], np.int32)
    ids = _extract_every_way(3, rowptr, keys, fgid)
    assert ids.tolist() == [NONE, 7]         # row 0 has a member whose key IS the none value
    assert capi.slice_ids(rowptr, keys, fgid, 3).tolist() == [NONE, 7]
    assert capi.slice_ids(rowptr, keys, fgid, 1).tolist() == [5, NONE]


def test_extract_around_the_launch_tile_and_descending_offsets():
    tile = capi.slices_shape()["extract_rows"]
    rng = np.random.default_rng(2)
    for R in (tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1):
        lengths = rng.integers(0, 6, size=R).tolist()
        member_at = [[int(rng.integers(0, n))] if n and rng.random() < 0.7 else [] for n in lengths]
        _extract_every_way(4, *_csr(lengths, member_at, 4, rng))
    # the device entry on offsets that descend or leave the arrays: those rows count as empty
    keys = (np.arange(10, dtype=np.uint64) + np.uint64(100))
    fgid = np.full(10, 4, np.int32)
    rp = np.array([0, 5, 3, 8, 20, 8, 10, 4294967295, 2], np.uint32)
    want = S.ids_of(rp, keys, fgid, 4, nnz=10)
    assert want.tolist() == [100, NONE, 103, NONE, NONE, 108, NONE, NONE]
    s = capi.Slices(4, 2)
    tk, pk = _dev(keys, np.int64)
    tf, pf = _dev(fgid, np.int32)
    tr, pr = _dev(rp, np.int32)
    got = capi.Slices.download_ids(s.extract_dev(pk, pf, pr, len(rp) - 1, 10), len(rp) - 1)
    assert got.tolist() == want.tolist()
    with pytest.raises(capi.XFError) as e:                  # the host entry names them instead
        s.extract(np.array([0, 5, 3], np.uint64), keys, fgid)
    assert "descend" in str(e.value)


# ------------------------------------------------------------------ accumulate
def _accumulate(s, p, loss, labels, ids, truth):
    """feed the slices, a progress (the whole stream's totals) and the truth the same rows"""
    import torch
    loss = np.ascontiguousarray(loss, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    ids = np.ascontiguousarray(ids, np.uint64)
    before = capi.slices_launches()
    if len(loss) == 0:
        s.accumulate(None, None, None, 0)
        assert capi.slices_launches() == before
        return
    tl, pl = _dev(loss, np.float32)
    ty, py = _dev(labels, np.int32)
    ti, pi = _dev(ids, np.int64)
    s.accumulate(pl, py, pi, len(loss))
    p.accumulate(pl, py, len(loss))
    torch.cuda.synchronize()
    assert capi.slices_launches() == before + 1
    S.words_of(loss, labels, ids, into=truth)


def _totals_from_progress(p):
    """n0 n1 . . llsum0 llsum1 other of the whole stream, from the progress's counts"""
    counts, other = p.read()
    t = S.terms().astype(object)
    ll = [int((counts[c].astype(object) * t).sum()) for c in (0, 1)]
    return int(counts[0].sum()), int(counts[1].sum()), ll[0], ll[1], int(other.sum())


def _check(s, p, truth, b, complete=None, reset=False):
    got = s.read(reset=reset)
    left = S.check_table(got, truth, b, complete)
    keys, words, none, overflow = got
    tot = [int(words[:, i].sum(dtype=np.uint64)) + int(none[i]) + int(overflow[i])
           for i in range(S.WORDS)]
    assert tot == S.total(truth), "entries + none + overflow = the whole stream"
    n0, n1, ll0, ll1, other = _totals_from_progress(p)
    assert (tot[0], tot[1], tot[4], tot[5], tot[6]) == (n0, n1, ll0, ll1, other), "the progress's totals"
    return got, left


def _random_rows(rng, R, pool):
    loss, y = TP._random_losses(rng, R)
    return loss, y, np.asarray(pool, np.uint64)[rng.integers(0, len(pool), size=R)]


def test_accumulate_sequence_on_one_object():
    rng = np.random.default_rng(3)
    shape = capi.slices_shape()
    s, p, truth = capi.Slices(3, 12), capi.Progress(), {}
    pool = [11, 22, 2 ** 64 - 2, 2 ** 63, NONE, 0]
    _accumulate(s, p, [], [], [], truth)                                   # R = 0: no launch
    _accumulate(s, p, [0.25], [0], [11], truth)                            # R = 1
    _accumulate(s, p, [-0.75], [1], [NONE], truth)                         # R = 1, no id
    loss, y = TP._random_losses(rng, 3000)
    _accumulate(s, p, loss, y, np.full(3000, 22, np.uint64), truth)        # one slice: the fold
    loss, y = TP._random_losses(rng, 64)
    _accumulate(s, p, loss, y, np.arange(64, dtype=np.uint64) + np.uint64(1000), truth)  # 64 ids a wave
    for R in (63, 65, shape["rows"] - 1, shape["rows"], shape["rows"] + 1, 2 * shape["rows"] + 17):
        _accumulate(s, p, *_random_rows(rng, R, pool), truth)              # mixed labels and ids
    edge = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, float("nan"), 1.5, -1.5, 1e-45, -1e-45,
                     2.0 ** -126, float("inf")], np.float32)
    lab = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 2, -1], np.int32)
    _accumulate(s, p, edge, lab, np.full(len(edge), 777, np.uint64), truth)
    _accumulate(s, p, edge, lab[::-1].copy(), np.full(len(edge), NONE, np.uint64), truth)
    assert truth[777][6] == 4 and truth[777][0] + truth[777][1] == len(edge) - 4   # NaN, +-1.5, inf
    assert truth[777][2] + truth[777][3] == 2 * 2 ** 30 + 2 * 2 ** 31      # 0.5 x 2 + 1.0 x 2 (+ tiny -> 0)
    got, _ = _check(s, p, truth, 12, complete=True)
    again, _ = _check(s, p, truth, 12, complete=True, reset=True)          # a read changes nothing
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    keys, words, none, overflow = s.read()                                 # ... a reset empties
    assert len(keys) == 0 and words.size == 0 and not none.any() and not overflow.any()
    assert s.count() == 0
    truth2, p2 = {}, capi.Progress()
    _accumulate(s, p2, *_random_rows(rng, 500, pool), truth2)
    _check(s, p2, truth2, 12, complete=True)
    # the summary of a slice: the library's against the restatement's, on real counters
    keys, words, none, _ = s.read()
    for w in (1.0, 4.0):
        for row in list(words[:3]) + [none]:
            S.same(capi.slices_summary(row, w), S.summary(row, w))


def test_more_distinct_ids_than_the_lds_table_holds():
    """one workgroup's rows on more ids than its LDS table has entries: rows that find no entry
    within the probes go to the global table directly"""
    shape = capi.slices_shape()
    rows, slots = shape["rows"], shape["slots"]
    assert rows > slots + shape["probe"]
    rng = np.random.default_rng(4)
    R = 2 * rows + 17
    ids = (np.arange(R, dtype=np.uint64) % np.uint64(rows + 300)) * np.uint64(0x9E3779B97F4A7C15) \
        + np.uint64(12345)
    assert len(np.unique(ids[:rows])) == rows > slots
    loss, y = TP._random_losses(rng, R)
    s, p, truth = capi.Slices(0, 16), capi.Progress(), {}
    _accumulate(s, p, loss, y, ids, truth)
    _accumulate(s, p, loss[::-1].copy(), y, ids, truth)
    _check(s, p, truth, 16, complete=True)


def _ids_with_home(b, home, n, start=1):
    out, k = [], start
    while len(out) < n:
        if S.home(k, b) == home:
            assert capi.slices_home(k, b) == home
            out.append(k)
        k += 1
    return out


def test_probing_wraps_at_the_last_entry():
    b = 6
    ids = _ids_with_home(b, 2 ** b - 1, 5)       # one home slot, the last: four of them wrap
    rng = np.random.default_rng(5)
    s, p, truth = capi.Slices(0, b), capi.Progress(), {}
    for _ in range(2):
        _accumulate(s, p, *_random_rows(rng, 700, ids + [NONE]), truth)
    got, _ = _check(s, p, truth, b, complete=True)
    assert [int(k) for k in got[0]] == sorted(ids)


def test_overflow_property():
    b = 2
    rng = np.random.default_rng(6)
    # four ids, whatever their home slots: all resident (the probe limit is the whole table)
    four = [5, 6, 7, 2 ** 64 - 2]
    s, p, truth = capi.Slices(0, b), capi.Progress(), {}
    _accumulate(s, p, *_random_rows(rng, 900, four + [NONE]), truth)
    got, left = _check(s, p, truth, b, complete=True)
    assert left == 0 and len(got[0]) == 4 and not got[3].any() and got[2].any()
    # seven ids: exactly four resident, each exact; overflow = the summed truth of the other three
    seven = four + [8, 9, 10]
    s, p, truth = capi.Slices(0, b), capi.Progress(), {}
    for _ in range(3):
        _accumulate(s, p, *_random_rows(rng, 1500, seven + [NONE]), truth)
    got, left = _check(s, p, truth, b, complete=False)
    assert left == 3 and len(got[0]) == 4 and got[3].any()
    assert [int(x) for x in got[2]] == truth[NONE], "none stays separate"
    # a read that cannot hold the entries says so and resets nothing
    n = capi.C.c_uint64()
    small = np.zeros((2, 8), np.uint64)
    rc = capi.lib().xf_slices_read(s.h, capi._p(small, capi.u64p), 2, capi.C.byref(n), None, None, 1)
    assert rc != 0 and n.value == 4
    _check(s, p, truth, b, complete=False)


def test_refusals_on_the_device():
    for field, b in [(-1, 16), (3, 1), (3, 27)]:
        with pytest.raises(capi.XFError) as e:
            capi.Slices(field, b)
        assert "xf_slices_create" in str(e.value)
    assert capi.Slices(2 ** 31 - 1, 2).params() == (2 ** 31 - 1, 2)
    ws = capi.Workspace()
    with pytest.raises(capi.XFError) as e:     # ids without a slices object and a progress
        ws.slice_ids(1234, 5)
    assert "xf_workspace_slice_ids" in str(e.value)


# ------------------------------------------------------------------ the tap
POOL = [101, 202, 2 ** 64 - 2, 303, NONE]
TAP_PATHS = ["lr_cells", "valued_lr_generic", "canonical_fm", "field_aware_fm_values"]


def _run_tapped(path, w, monkeypatch, with_ids):
    """TP's runner of a step path, its workspace carrying a progress and a slices; every step is
    given ids for its rows first (with_ids)"""
    ws = capi.Workspace()
    if w != 1.0:
        ws.neg_weight(w)
    p, s = capi.Progress(), capi.Slices(3, 9)
    ws.progress(p)
    ws.slices(s)
    fed, alive = [], []
    real = {"lr_step": capi.lr_step, "fm_step": capi.fm_step}

    def give_ids(ws_, R):
        rng = np.random.default_rng(1000 + len(fed))
        ids = np.asarray(POOL, np.uint64)[rng.integers(0, len(POOL), size=R)]
        t, ptr = _dev(ids, np.int64)
        alive.append(t)
        fed.append(ids)
        ws_.slice_ids(ptr, R)

    def lr_step(t, b, ws_, stream=None):
        if with_ids:
            give_ids(ws_, b.R)
        return real["lr_step"](t, b, ws_, stream)

    def fm_step(wt, vt, b, ws_, stream=None):
        if with_ids:
            give_ids(ws_, b.R)
        return real["fm_step"](wt, vt, b, ws_, stream)

    monkeypatch.setattr(capi, "lr_step", lr_step)
    monkeypatch.setattr(capi, "fm_step", fm_step)
    before = capi.slices_launches()
    tables, steps = TP.PATHS[path](ws)
    launches = capi.slices_launches() - before
    monkeypatch.undo()
    bits = TP._table_bits(tables)
    counts, got = p.read(), s.read()
    ws.slices(None)
    ws.progress(None)
    return bits, steps, counts, got, fed, launches


@pytest.mark.parametrize("w", [1.0, 4.0], ids=["w1", "w4"])
@pytest.mark.parametrize("path", TAP_PATHS)
def test_tap_of_the_step_paths(path, w, monkeypatch):
    base_bits, base_steps, base_counts = TP._run(path, True, w)          # progress alone
    bits, steps, counts, got, fed, launches = _run_tapped(path, w, monkeypatch, True)
    assert launches == len(steps) == len(fed) == 3
    assert bits == base_bits, "tables with slices attached"
    TP.same_counts(counts, base_counts, "the progress beside the slices")
    truth = {}
    for (loss, labels), (loss0, _), ids in zip(steps, base_steps, fed):
        TP.eq(loss, loss0, "the step's (weighted) losses")
        labels = np.asarray(labels)
        # the tap sees the unweighted losses: undoing w = 4 on the negatives is exact
        plain = np.where(labels == 0, loss / np.float32(w), loss).astype(np.float32)
        S.words_of(plain, labels, ids, into=truth)
    S.check_table(got, truth, 9, complete=True)
    tot = S.total(truth)
    assert (tot[0], tot[1], tot[6]) == (int(counts[0][0].sum()), int(counts[0][1].sum()),
                                        int(counts[1].sum()))
    # steps without ids: no accumulate launch, nothing counted, the same tables
    bits2, _, counts2, got2, _, launches2 = _run_tapped(path, w, monkeypatch, False)
    assert launches2 == 0 and bits2 == base_bits and len(got2[0]) == 0
    assert not got2[2].any() and not got2[3].any()
    TP.same_counts(counts2, base_counts)


def test_tap_ids_name_one_step_only_and_must_fit():
    raws = TP._lr_raws()
    t = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 17)
    ws, p, s = capi.Workspace(), capi.Progress(), capi.Slices(3, 9)
    ws.progress(p)
    ws.slices(s)
    R = len(raws[0][2])
    ids = np.full(R, 42, np.uint64)
    ti, pi = _dev(ids, np.int64)
    ws.slice_ids(pi, R)
    capi.lr_step(t, capi.LocalBatch(t, *raws[0]), ws)
    capi.lr_step(t, capi.LocalBatch(t, *raws[1]), ws)        # no ids: not counted
    keys, words, none, overflow = s.read()
    assert keys.tolist() == [42] and int(words[0][0] + words[0][1] + words[0][6]) == R
    ws.slice_ids(pi, R - 1)                                  # ids of another row count
    with pytest.raises(capi.XFError) as e:
        capi.lr_step(t, capi.LocalBatch(t, *raws[2]), ws)
    assert "slice ids" in str(e.value)


# ------------------------------------------------------------------ two ranks on one GPU
TWO = (("lr", 2, 0, 0, "ftrl", "sequential", "ragged", False),
       ("lr", 2, 0, 0, "ftrl", "stale1", "ragged", False))
POOL2 = [7, 8, 9, NONE, 2 ** 64 - 2, 10, 11]


def _pack(got):
    keys, words, none, overflow = got
    return np.concatenate([keys.reshape(-1, 1), words], axis=1), none, overflow


def _slices_rank(rank, world, port, spec, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        mode, _, F, k, opt, schedule, case, valued = spec
        strs = M.streams(mode, case, world, F)
        st = SM._trainer(g, spec)
        st.set_progress(True)
        st.set_slices(True, 3, 3)             # eight entries a rank hold its four or five ids
        SM._import_old(st, spec, strs, rank, world)
        train, _ = strs[rank]
        alive, losses, labels, fed = [], [], [], []
        for i, mb in enumerate(train):
            b = st.compile(mb[0], mb[1], mb[4])
            R = len(mb[4])
            pool = np.asarray(POOL2[:5 + rank] if i % 2 == 0 else POOL2[rank:4], np.uint64)
            ids = pool[np.random.default_rng(100 * rank + i).integers(0, len(pool), size=R)]
            if i != 1:                         # (the second minibatch has no ids: not counted)
                t = torch.from_numpy(ids.view(np.int64)).cuda()
                torch.cuda.synchronize()
                st.batch_slices(b, t.data_ptr(), R)
                st.flush()
                del t                          # the minibatch keeps its own copy
            alive.append(b)
            st.step(b)
            if i != 1:
                losses.append(st.last_loss(b))
                labels.append(np.asarray(mb[4], np.int32))
                fed.append(ids)
        own = _pack(st.slices_read())
        mer = _pack(st.slices_read(reset=True, merged=True))
        left = st.slices_read()
        st.check()
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), own_e=own[0], own_n=own[1], own_o=own[2],
                 mer_e=mer[0], mer_n=mer[1], mer_o=mer[2],
                 left=np.array([len(left[0]) + int(left[2].sum()) + int(left[3].sum())]),
                 loss=np.concatenate(losses), labels=np.concatenate(labels),
                 ids=np.concatenate(fed))
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("spec", TWO, ids=["%s-%s" % (s[0], s[5]) for s in TWO])
def test_two_ranks_merged_read(tmp_path, spec):
    world = 2
    port = free_port()
    SM._spawn(_slices_rank, [(r, world, port, spec, str(tmp_path)) for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    both = {}
    for r in range(world):
        truth = S.words_of(parts[r]["loss"], parts[r]["labels"], parts[r]["ids"])
        S.words_of(parts[r]["loss"], parts[r]["labels"], parts[r]["ids"], into=both)
        e = parts[r]["own_e"]
        S.check_table((e[:, 0], e[:, 1:], parts[r]["own_n"], parts[r]["own_o"]), truth, 3,
                      complete=True)
        assert parts[r]["left"][0] == 0 and len(parts[r]["labels"]) > 0
    for r in range(world):
        e = parts[r]["mer_e"]
        S.check_table((e[:, 0], e[:, 1:], parts[r]["mer_n"], parts[r]["mer_o"]), both, 4,
                      complete=True)
        assert np.array_equal(e, parts[0]["mer_e"]), "the same list on every rank"
    assert 10 in parts[0]["mer_e"][:, 0] and 10 not in parts[0]["own_e"][:, 0]   # rank 1's alone


def _owner_refusal(port, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"       # a group of one on the exchange path
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        seen = []
        for sched in ("owner", "owner_stale1"):
            st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule=sched)
            st.set_slices(False)                     # (off is the default: accepted)
            try:
                st.set_slices(True, 3, 8)
            except capi.XFError as e:
                assert re.search(r"xf_sharded_slices.*schedule %s\b" % sched, str(e)) \
                    and "sequential" in str(e), str(e)
                seen.append(sched)
            st.close()
        st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule="stale1")
        try:
            st.set_slices(True, 3, 8)                # progress is off
        except capi.XFError as e:
            assert "xf_sharded_progress" in str(e), str(e)
            seen.append("needs progress")
        st.set_progress(True)
        for field, b in ((-1, 8), (3, 27)):
            try:
                st.set_slices(True, field, b)
            except capi.XFError as e:
                assert "xf_sharded_slices" in str(e), str(e)
                seen.append("bad parameter")
        st.set_slices(True, 3, 8)
        try:
            st.set_schedule("owner")
        except capi.XFError as e:
            assert "xf_sharded_set_schedule" in str(e), str(e)
            seen.append("then owner")
        try:
            st.set_progress(False)
        except capi.XFError as e:
            assert "xf_sharded_slices" in str(e), str(e)
            seen.append("progress off under slices")
        try:
            capi.Sharded(g, model="lr", capacity=1 << 12).slices_read()
        except capi.XFError as e:
            assert "is off" in str(e), str(e)
            seen.append("read while off")
        st.close()
        g.close()
        q.put((0, ("ok", seen)))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_owner_schedules_refuse_slices():
    res = SM._spawn(_owner_refusal, [(free_port(),)])
    assert res[0][1] == ("ok", ["owner", "owner_stale1", "needs progress", "bad parameter",
                                "bad parameter", "then owner", "progress off under slices",
                                "read while off"]), res


# ------------------------------------------------------------------ the worker end to end
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(build.LIBDIR, "xflow_lr")
FIELD, SEED, KEEP = 3, 5, 0.5
STAGES = dict(neg_keep=KEEP, cross="2*3", admit_count=2, admit_log2_slots=16)
CONFIGS = {
    "host": dict(ingest="host"),
    "gpu_fields": dict(ingest="gpu_fields"),
    "host-nocache": dict(ingest="host", cache_batches=0),
    "gpu_fields-nocache": dict(ingest="gpu_fields", cache_batches=0),
    "host-stages": dict(ingest="host", **STAGES),
    "gpu_fields-stages": dict(ingest="gpu_fields", **STAGES),
    "host-stages-nocache": dict(ingest="host", cache_batches=0, **STAGES),
}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("slices")
    shutil.copy(os.path.join(GOLDEN, "small_train-00000"), str(d / "train-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "test-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "train-00001"))   # (two workers)
    return d


_parsed = {}


def _file_rows(data, name):
    """(labels, slice ids) of a training file's rows, from the host parser and the restatement"""
    if name not in _parsed:
        labels, ids = [], []
        for rp, keys, fg, lab, vals in capi.read_blocks(str(data / name), 2 << 20, values=True):
            labels.append(np.asarray(lab))
            ids.append(S.ids_of(rp, keys, fg, FIELD))
        _parsed[name] = (np.concatenate(labels), np.concatenate(ids))
    return _parsed[name]


def _expected_counts(labels, ids, keep_mask):
    """{id: (n0, n1)} over the kept rows"""
    out = {}
    for y, i, k in zip(labels, ids, keep_mask):
        if k:
            n = out.setdefault(int(i), [0, 0])
            n[1 if y != 0 else 0] += 1
    return out


def _kept(labels, epoch, sampled, rank=0):
    if not sampled:
        return np.ones(len(labels), bool)
    return np.array([y != 0 or capi.negsample_keep(SEED, (epoch << 32) | rank, r, KEEP) == 1
                     for r, y in enumerate(labels)])


def _read_tsv(path):
    """{epoch: [(key, n0, n1, other, ctr, pctr, logloss)]} in file order"""
    out = {}
    for ln in open(path).read().strip().split("\n"):
        f = ln.split("\t")
        assert len(f) == 8, ln
        out.setdefault(int(f[0]), []).append((int(f[1], 16), int(f[2]), int(f[3]), int(f[4]),
                                              float(f[5]), float(f[6]), float(f[7])))
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_worker_counts_per_slice(data, name):
    cfg = CONFIGS[name]
    tsv = str(data / ("slices_%s.tsv" % name))
    x = capi.XFlow(str(data / "train"), str(data / "test"), model=0, capacity=1 << 14, epochs=2,
                   seed=SEED, progress=1, progress_by=FIELD, progress_slices_out=tsv,
                   pred_path=str(data / ("pred_%s.txt" % name)), **cfg)
    x.train()
    if cfg["ingest"] == "gpu_fields":
        assert x.metric("blocks_gpu") > 0
    labels, ids = _file_rows(data, "train-00000")
    sampled = "neg_keep" in cfg
    w = float(np.float32(1) / np.float32(KEEP)) if sampled else 1.0
    got = _read_tsv(tsv)
    assert sorted(got) == [0, 1]
    for epoch in (0, 1):
        # a cached minibatch replays epoch 0's sample; without the cache epoch 1 samples again
        want = _expected_counts(labels, ids, _kept(labels, epoch if cfg.get("cache_batches", 1) == 0
                                                   else 0, sampled))
        none = want.pop(NONE, [0, 0])
        rows = got[epoch]
        assert [r[0] for r in rows] == sorted(want), "one line a slice, by key"
        for key, n0, n1, other, ctr, pctr, logloss in rows:
            assert [n0, n1] == want[key] and other == 0, hex(key)
            assert ctr == n1 / (n1 + w * n0) and 0.0 < pctr < 1.0 and logloss > 0.0
        if epoch == 1:
            total = sum(r[2] + w * r[1] for r in rows) + none[1] + w * none[0]
            assert total == x.metric("progress_rows") == x.metric("slice_rows")
            assert x.metric("slices") == len(rows)
            assert x.metric("slice_none_rows") == none[1] + w * none[0]
            assert x.metric("slice_overflow_rows") == 0
    if not sampled and cfg.get("cache_batches", 1) == 1 and cfg["ingest"] == "host":
        # a fresh LR table: every row's p is 0.5 in epoch 0, in every slice
        for key, n0, n1, other, ctr, pctr, logloss in got[0]:
            assert pctr == 0.5 and logloss == float(capi.slices_terms()[P.C]) / 2.0 ** 24


def test_worker_off_is_the_parent(data):
    """tables, predictions and progress figures with progress_by are those without it"""
    out = {}
    for tag, extra in (("off", {}), ("on", dict(progress_by=FIELD, progress_slots=3))):
        pred, mdl = str(data / ("p_%s.txt" % tag)), str(data / ("m_%s.bin" % tag))
        x = capi.XFlow(str(data / "train"), str(data / "test"), model=0, capacity=1 << 14,
                       epochs=2, progress=1, pred_path=pred, model_out=mdl, **extra)
        x.train()
        out[tag] = (open(pred, "rb").read(), open(mdl, "rb").read(),
                    [x.metric("progress_" + n) for n in ("logloss", "auc", "ctr", "pctr", "rows")])
        if tag == "on":        # 8 entries for the file's 11 slices: the rest is in overflow
            assert x.metric("slices") == 8 and x.metric("slice_overflow_rows") > 0
            assert x.metric("slice_rows") == x.metric("progress_rows")
        else:
            with pytest.raises(capi.XFError):
                x.metric("slices")
    assert out["on"] == out["off"]


def _run_cli(args, cwd, prefix=(), env=None):
    out = subprocess.run(list(prefix) + [CLI] + args, capture_output=True, text=True, timeout=300,
                         cwd=str(cwd), env=env)
    assert out.returncode == 0, out.stderr
    return out.stdout.split("\n")


def _check_printed(lines, tsv, epochs, top, field=FIELD):
    heads = [i for i, ln in enumerate(lines) if ln.startswith("progress slices epoch ")]
    assert len(heads) == epochs, lines
    for e, at in enumerate(heads):
        rows = tsv[e]
        assert lines[at - 1].startswith("progress epoch %d: " % e), "after the progress line"
        assert lines[at].startswith("progress slices epoch %d: field = %d slices = %d rows = "
                                    % (e, field, len(rows))), lines[at]
        assert "overflow_rows = 0" in lines[at] and "incomplete" not in lines[at]
        want = sorted(rows, key=lambda r: (-(r[1] + r[2]), r[0]))[:top]      # (w = 1)
        printed = lines[at + 1:at + 1 + top]
        assert all(ln.startswith("  key = 0x") for ln in printed), printed
        assert not lines[at + 1 + len(want)].startswith("  key = ")
        for ln, (key, n0, n1, other, ctr, pctr, logloss) in zip(printed, want):
            assert ln == "  key = 0x%016x rows = %.12g ctr = %.6f pctr = %.6f logloss = %.6f" % (
                key, n0 + n1, ctr, pctr, logloss), ln


def test_cli_prints_the_heaviest_slices(data, tmp_path):
    args = [str(data / "train"), str(data / "test"), "0", "2", "capacity=16384",
            "pred_path=on.txt", "progress=1", "progress_by=%d" % FIELD, "progress_top=5",
            "progress_slices_out=s.tsv"]
    lines = _run_cli(args, tmp_path)
    tsv = _read_tsv(str(tmp_path / "s.tsv"))
    _check_printed(lines, tsv, 2, 5)
    labels, ids = _file_rows(data, "train-00000")
    want = _expected_counts(labels, ids, np.ones(len(labels), bool))
    want.pop(NONE, None)
    assert {r[0]: [r[1], r[2]] for r in tsv[1]} == want
    off = _run_cli(args[:7], tmp_path)
    assert not any("slices" in ln for ln in off)
    bad = subprocess.run([CLI] + args[:6] + ["progress_by=3"], capture_output=True, text=True,
                         timeout=300, cwd=str(tmp_path))
    assert bad.returncode != 0 and "progress=0" in bad.stdout + bad.stderr


def test_local_sh_two_workers_merge_their_slices(data, tmp_path):
    args = [str(data / "train"), str(data / "test"), "0", "2", "transport=host", "capacity=16384",
            "pred_path=two.txt", "progress=1", "progress_by=%d" % FIELD, "progress_top=3",
            "progress_slices_out=two.tsv"]   # (host transport: both ranks share one GPU)
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI] + args,
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path),
                         env=dict(os.environ, DMLC_PS_ROOT_PORT=str(free_port())))
    assert out.returncode == 0, out.stderr
    tsv = _read_tsv(str(tmp_path / "two.tsv"))           # rank 0 alone writes
    lines = out.stdout.split("\n")
    heads = [ln for ln in lines if ln.startswith("progress slices epoch ")]
    assert len(heads) == 2, out.stdout                   # ... and prints
    want = {}
    for f in ("train-00000", "train-00001"):
        labels, ids = _file_rows(data, f)
        for k, n in _expected_counts(labels, ids, np.ones(len(labels), bool)).items():
            old = want.setdefault(k, [0, 0])
            old[0] += n[0]
            old[1] += n[1]
    none = want.pop(NONE, [0, 0])
    for e in (0, 1):
        assert {r[0]: [r[1], r[2]] for r in tsv[e]} == want
        assert heads[e].startswith("progress slices epoch %d: field = %d slices = %d rows = 400 "
                                   "none_rows = %d " % (e, FIELD, len(want), sum(none))), heads[e]
