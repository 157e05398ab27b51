"""Held-out validation (xf_holdout.hip, xf_sharded_validate, the worker's holdout=) on a real
MI355X.  The only reference of the split is the numpy restatement tests/_holdout_checker.py (pinned
to a plain loop by tests/test_holdout_cpu.py); validate is held to predict's own pctr of the same
minibatch; the worker to a plain run on the training file with the held rows deleted.  Every
comparison is exact — integer arrays, float arrays as their bits.

* the split: both parts' arrays and the statistics over share x companions, on minibatches chosen
  where the passes can go wrong, one after the other on ONE object with running ordinals;
* validate on every step path, across a defrag and an eviction, beside predict, on two ranks;
* the worker end to end."""
import os
import re
import shutil
import subprocess
import traceback

import numpy as np
import pytest

from xflow_amd import build, capi

from . import _admit_checker as A
from . import _cross_checker as X
from . import _ffm_checker as FF
from . import _holdout_checker as H
from . import _progress_checker as P
from . import _sharded_modes_checker as M
from . import _valued_cases as Cs
from . import test_gpu_fm_canonical as TC      # synth (the module, not its tests)
from . import test_gpu_progress as TP          # the step paths' tables (the module, not its tests)
from . import test_gpu_sharded_modes as SM     # _spawn, _trainer, _import_old
from .conftest import GOLDEN
from .test_gpu_parity import synth
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(build.LIBDIR, "xflow_lr")
eq, same_counts = TP.eq, TP.same_counts


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def tile_size():
    """the row tile of the flag and the place pass, read from the source"""
    src = open(os.path.join(ROOT, "xflow_amd", "csrc", "xf_holdout.hip")).read()
    return int(re.search(r"constexpr uint32_t kHoTile = (\d+);", src).group(1))


# ------------------------------------------------------------------ the split's minibatches
STREAM = 2
TINY, QUARTER, NEARLY = 2.0 ** -32, 0.25, 1.0 - 2.0 ** -24
LONG_ROW_AT = 1 << 20          # the first ordinal of the `long_row` minibatch
EDGE_AT = 1 << 21              # ... and where the searched cases start
POOL = None


def pool():
    global POOL
    if POOL is None:
        POOL = capi.hash_decimal_range(0, 3000)
    return POOL


def _mb(rng, lens, labels=None):
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    keys = pool()[rng.randint(0, len(pool()), size=int(rowptr[-1]))]
    if labels is None:
        labels = (rng.rand(len(lens)) < 0.3).astype(np.int32)
    return rowptr, keys, np.asarray(labels, np.int32)


def long_row_seeds():
    """two seeds under which the row of 5000 nonzeros (row 2 of `long_row`) is held, respectively
    not held, at share 0.25 — found with the restatement"""
    at = np.uint64(LONG_ROW_AT) + np.arange(5, dtype=np.uint64)
    masks = [(s, H.held(s, STREAM, at, QUARTER)) for s in range(1, 1000)]
    held = next(s for s, m in masks if m[2] and not m.all())      # (both parts have rows)
    kept = next(s for s, m in masks if not m[2] and m.any())
    return held, kept


def _find(seed, share, start, want):
    """the first ordinal f >= start with held(f + i) == want[i] for every i in want (a dict)"""
    offs = np.array(sorted(want), np.uint64)
    flags = np.array([want[int(o)] for o in offs], bool)
    for f in range(start, start + 100000):
        if np.array_equal(H.held(seed, STREAM, np.uint64(f) + offs, share), flags):
            return f
    raise AssertionError("no such place")


def sequence(seed, share):
    """[(name, first_ordinal, rowptr, keys, labels)] in the order they go through one object:
    ordinals run on from minibatch to minibatch, with jumps forward to the places some cases need"""
    rng = np.random.RandomState(29)
    T = tile_size()
    out, at = [], [7]

    def add(name, mb, first=None):
        if first is not None:
            assert first >= at[0]
            at[0] = first
        out.append((name, at[0]) + mb)
        at[0] += len(mb[2])

    add("no_rows", (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32)))
    add("all_rows_empty", _mb(rng, np.zeros(40, np.int64)))
    lens = rng.randint(0, 40, size=700)            # empty rows first, last and in runs
    lens[:3] = 0
    lens[-2:] = 0
    lens[300:340] = 0
    lens[rng.rand(700) < 0.05] = 0
    add("ragged", _mb(rng, lens))
    add("long_run", _mb(rng, rng.randint(1, 6, size=T + 40)))   # (held / kept at the edge shares)
    for R in (T - 1, T, T + 1, 2 * T + 1):
        add("rows%d" % R, _mb(rng, rng.randint(0, 5, size=R)))
    add("long_row", _mb(rng, [3, 0, 5000, 0, 7]), first=LONG_ROW_AT)
    add("short_rows", _mb(rng, rng.randint(1, 4, size=300)))
    if share == QUARTER:                           # (searched: the edge shares hold all or nothing)
        add("one_row_held", _mb(rng, [9]), first=_find(seed, share, EDGE_AT, {0: True}))
        add("one_row_kept", _mb(rng, [9]), first=_find(seed, share, at[0], {0: False}))
        R = 90
        add("first_row_held", _mb(rng, rng.randint(1, 6, size=R)),
            first=_find(seed, share, at[0], {0: True, R - 1: False}))
        add("last_row_held", _mb(rng, rng.randint(1, 6, size=R)),
            first=_find(seed, share, at[0], {0: False, R - 1: True}))
    else:
        add("one_row", _mb(rng, [9]))
    add("across_2^32", _mb(rng, rng.randint(0, 6, size=50)), first=(1 << 32) - 3)
    return out


def companions(keys):
    """an fgid and a value per nonzero that say where the nonzero came from"""
    n = len(keys)
    return (np.arange(n, dtype=np.int32) % 977,
            (np.arange(n, dtype=np.float32) * np.float32(0.25) - np.float32(3)).astype(np.float32))


COMP = {"none": (False, False), "fgid": (True, False), "vals": (False, True), "both": (True, True)}
GRID = [(QUARTER, c, w) for c in COMP for w in (0, 1)] + \
       [(s, c, 0) for s in (TINY, NEARLY) for c in COMP]


@pytest.mark.parametrize("share,comp,which", GRID,
                         ids=["share%.3g-%s-seed%s" % (s, c, "AB"[w]) for s, c, w in GRID])
def test_split_arrays_and_stats(share, comp, which):
    seed = long_row_seeds()[which]
    mbs = sequence(seed, share)
    with_fg, with_vs = COMP[comp]
    T = tile_size()
    # the restatement first: the expected arrays of every call, and that each case has the property
    # it is named for — before the GPU is asked anything
    ref, expect = H.Splitter(share, seed), []
    for name, first, rowptr, keys, labels in mbs:
        fg, vs = companions(keys)
        tr, he = ref.split(STREAM, first, rowptr, keys, labels, fg, vs)
        expect.append((tr, he, ref.stats()))
        m = ref.mask(STREAM, first, len(labels))
        assert len(tr[2]) + len(he[2]) == len(labels) and len(tr[1]) + len(he[1]) == len(keys)
        if share == TINY:
            assert not m.any(), name                      # nothing held: a kept run > a tile
        elif share == NEARLY:
            assert m.all(), name                          # everything held: a held run > a tile
        elif name not in ("no_rows", "one_row_held", "one_row_kept"):
            assert m.any() and not m.all(), name          # both parts have rows
        if name == "long_run":
            assert len(labels) > T
        if name == "all_rows_empty":
            assert len(keys) == 0 and len(labels) > 0
        if name == "ragged":
            lens = np.diff(rowptr.astype(np.int64))
            assert lens[0] == 0 and lens[-1] == 0 and (lens[300:340] == 0).all()
        if name == "long_row" and share == QUARTER:
            assert (len(he[1]) >= 5000) == (which == 0) and (len(tr[1]) >= 5000) == (which == 1)
        if name == "one_row_held":
            assert m.tolist() == [True]
        if name == "one_row_kept":
            assert m.tolist() == [False]
        if name == "first_row_held":
            assert m[0] and not m[-1]
        if name == "last_row_held":
            assert m[-1] and not m[0]
        if name == "across_2^32":
            assert first < (1 << 32) < first + len(labels)
    obj = capi.Holdout(share, seed=seed)
    for (name, first, rowptr, keys, labels), (tr, he, stats) in zip(mbs, expect):
        fg, vs = companions(keys)
        got = obj.split(STREAM, first, rowptr, keys, labels, fgid=fg if with_fg else None,
                        values=vs if with_vs else None)
        for part, g, (rp, ks, lb, efg, evs) in zip(("train", "held"), got, (tr, he)):
            what = "%s %s " % (name, part)
            eq(g[0], rp, what + "rowptr")
            eq(g[1], ks, what + "keys")
            eq(g[2], lb, what + "labels")
            at = 3
            if with_fg:
                eq(g[at], efg, what + "fgid")
                at += 1
            if with_vs:
                eq(g[at], evs, what + "values")
                at += 1
            assert len(g) == at
        assert obj.stats() == stats, name


def test_row_slice_of_a_block_and_the_device_entry():
    """host arrays whose first offset is not 0 — rows [100, 300) of a block — and the same rows
    through xf_holdout_split_dev from device arrays; the parts' device arrays are aligned"""
    import torch
    name, first, rowptr, keys, labels = sequence(1, QUARTER)[2]
    obj, ref = capi.Holdout(QUARTER, seed=9), H.Splitter(QUARTER, 9)
    want = ref.split(STREAM, 1000, rowptr[100:301], keys, labels[100:300])
    got = obj.split(STREAM, 1000, rowptr[100:301], keys, labels[100:300])
    for g, e in zip(got, want):
        for a, b in zip(g, e[:3]):
            eq(a, b)
    assert 0 < len(got[1][2]) < 200
    lo, hi = int(rowptr[100]), int(rowptr[300])
    d_rp = torch.from_numpy((rowptr[100:301] - rowptr[100]).astype(np.uint32).view(np.int32)).cuda()
    d_keys = torch.from_numpy(keys[lo:hi].view(np.int64)).cuda()
    d_lab = torch.from_numpy(labels[100:300]).cuda()
    tr, he = obj.part_dev(STREAM, 1000, d_keys.data_ptr(), d_rp.data_ptr(), d_lab.data_ptr(), 200,
                          hi - lo)
    align = capi.holdout_shape()["align"]
    assert he.d_keys % (8 * align) == 0 and he.d_rowptr % (4 * align) == 0 and \
        he.d_labels % (4 * align) == 0 and tr.d_fgid is None and he.d_vals is None
    for d, e in zip((tr, he), want):
        for a, b in zip(capi.Holdout.download(d), e[:3]):
            eq(a, b)
    with pytest.raises(capi.XFError, match="descend"):
        obj.split(STREAM, 0, np.array([0, 3, 2], np.uint64), np.zeros(3, np.uint64),
                  np.zeros(2, np.int32))


def test_broken_row_offsets_on_the_device_entry():
    """xf_holdout_split_dev takes what a caller hands it: a row whose offsets descend or leave the
    arrays counts as empty; rows that overlap past NNZ are refused, nothing written out of bounds"""
    import torch
    keys = np.arange(100, 110, dtype=np.uint64)
    labels = np.array([0, 1, 0, 1], np.int32)
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    d_lab = torch.from_numpy(labels).cuda()
    obj = capi.Holdout(0.5, seed=4)
    m = H.held(4, STREAM, np.arange(4, dtype=np.uint64), 0.5)
    assert m.any() and not m.all()
    # rows: [0, 4); [4, 2) descends; [2, 50) leaves the arrays; [50, 10) descends: three empty rows
    rp = np.array([0, 4, 2, 50, 10], np.uint32)
    d_rp = torch.from_numpy(rp.view(np.int32)).cuda()
    tr, he = obj.part_dev(STREAM, 0, d_keys.data_ptr(), d_rp.data_ptr(), d_lab.data_ptr(), 4, 10)
    lens = np.array([4, 0, 0, 0])
    for d, part in ((tr, ~m), (he, m)):
        g = capi.Holdout.download(d)
        eq(g[0], np.concatenate([[0], np.cumsum(lens[part])]).astype(np.uint32))
        eq(g[1], keys[:4] if part[0] else keys[:0])
        eq(g[2], labels[part])
    # rows 0 and 2 are both [0, 10): 20 nonzeros of 10 — refused; the object goes on working
    bad = np.array([0, 10, 0, 10, 0], np.uint32)
    d_rp = torch.from_numpy(bad.view(np.int32)).cuda()
    with pytest.raises(capi.XFError, match="overlap"):
        obj.part_dev(STREAM, 0, d_keys.data_ptr(), d_rp.data_ptr(), d_lab.data_ptr(), 4, 10)
    d_rp = torch.from_numpy(np.array([0, 10, 10, 10, 10], np.uint32).view(np.int32)).cuda()
    tr, he = obj.part_dev(STREAM, 0, d_keys.data_ptr(), d_rp.data_ptr(), d_lab.data_ptr(), 4, 10)
    assert tr.NNZ + he.NNZ == 10 and tr.R + he.R == 4


# ------------------------------------------------------------------ validate, one GPU
# (every forward stores one fp32 loss = pctr - (float)label beside pctr — k_lr_forward,
# k_lr_finalize*, k_fm_forward*, k_fmc_forward, k_ffm_forward, k_val_lr_forward, the cells' finalize
# with weight 1 — so the losses a validate counts are formed here from predict's pctr)
def check_validate(predict, validate, labels):
    p = capi.Progress()
    at = capi.progress_launches()
    pctr = predict()
    assert capi.progress_launches() == at                 # predict never accumulates
    validate(p)
    assert capi.progress_launches() == at + 1             # one launch, nothing else of its own
    got = p.read(reset=True)
    same_counts(got, H.counts_of(pctr, labels), "validate against predict's pctr")
    assert int(got[0].sum()) == len(labels) > 0 and int(got[1].sum()) == 0
    eq(predict(), pctr, "predict after a validate")
    assert len(np.unique(pctr)) > 1                       # (a trained model: not all sigmoid(0))
    return got


def _lr(t, ws, b, labels):
    return check_validate(lambda: capi.lr_predict(t, b, ws),
                          lambda p: capi.lr_validate(t, b, ws, p), labels)


def _fm(tw, tv, ws, b, labels):
    return check_validate(lambda: capi.fm_predict(tw, tv, b, ws),
                          lambda p: capi.fm_validate(tw, tv, b, ws, p), labels)


def test_validate_lr_cells_and_local():
    ws = capi.Workspace()
    (t,), _ = TP._run_lr_cells(ws)
    held = synth(np.random.RandomState(77), 1000, 40, 45000, None, True)   # (a third unseen keys)
    _lr(t, ws, capi.Batch(*held), held[2])                 # the generic build's cells
    _lr(t, ws, capi.LocalBatch(t, *held), held[2])         # the local build's


@pytest.mark.parametrize("path", ["generic", "local"])
def test_validate_valued_lr(path):
    ws = capi.Workspace()
    (t,), _ = TP._run_valued(ws, path)
    rp, ks, vs, lb = Cs.stream("ragged", seed=50)[0]
    b = capi.LocalBatch(t, rp, ks, lb, values=vs) if path == "local" else \
        capi.Batch(rp, ks, lb, on_gpu=True, values=vs)
    _lr(t, ws, b, lb)


@pytest.mark.parametrize("k", [4, 10], ids=["k4-records", "k10"])
def test_validate_reference_fm(k):
    ws = capi.Workspace()
    (tw, tv), _ = TP._run_reference_fm(ws, k)
    held = synth(np.random.RandomState(78), 300, 30, 6000, None, True)
    _fm(tw, tv, ws, capi.Batch(*held), held[2])


def test_validate_canonical_fm():
    ws = capi.Workspace()
    (tw, tv), _ = TP._run_canonical(ws)
    held = TC.synth(np.random.RandomState(79), 300, 20, 6000, None)
    _fm(tw, tv, ws, capi.Batch(*held, on_gpu=True), held[2])


def test_validate_field_aware_fm():
    ws = capi.Workspace()
    (tw, tv), _ = TP._run_ffm(ws)
    Fd = 18
    rp, ks, fg, vs, lb = FF.stream("ragged", Fd)[-1]
    _fm(tw, tv, ws, capi.Batch(rp, ks, lb, on_gpu=True, values=vs, fields=Fd, fgid=fg), lb)


def test_validate_across_a_defrag_and_an_eviction():
    """the same held minibatch — compiled once, kept — validated before and after the table is
    renumbered and after its dead rows are dropped: equal counts (an evicted key returns at first
    touch: w = 0, as it left), and equal to predict's"""
    raws = TP._lr_raws()
    held = synth(np.random.RandomState(77), 1000, 40, 45000, None, True)
    st = capi.Sharded(model="lr", capacity=1 << 17)
    st.set_holdout(True)
    with pytest.raises(capi.XFError, match="progressive validation is off"):
        st.progress_read()                                 # (the two progresses are apart)
    hb = st.compile(*held)
    for raw in raws:
        st.step(st.compile(*raw))
    pctr = st.predict(hb)
    want = H.counts_of(pctr, held[2])
    st.validate(hb)
    same_counts(st.holdout_read(reset=True), want, "before")
    st.defrag()
    st.validate(hb)
    same_counts(st.holdout_read(reset=True), want, "after the defrag")
    seen, dropped = st.evict(float("inf"))
    assert 0 < dropped < seen
    st.validate(hb)
    st.validate(hb)
    twice = st.holdout_read()
    same_counts((twice[0] // 2, twice[1] // 2), want, "after the eviction, summed over two")
    assert (twice[0] % 2 == 0).all()
    same_counts(st.holdout_read(reset=True), twice, "a read without reset keeps the counts")
    assert int(st.holdout_read()[0].sum()) == 0
    eq(st.predict(hb), pctr, "predict after it all")
    st.set_holdout(False)
    with pytest.raises(capi.XFError, match="held-out validation is off"):
        st.validate(hb)
    st.close()


# ------------------------------------------------------------------ validate, two ranks
TWO = (("lr", 2, 0, 0, "ftrl", "sequential", "ragged", False),
       ("lr", 2, 0, 0, "ftrl", "stale1", "ragged", False),
       ("canonical", 2, 0, 4, "ftrl", "stale1", "ragged", False))


def _validate_rank(rank, world, port, spec, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        mode, _, F, k, opt, schedule, case, valued = spec
        strs = M.streams(mode, case, world, F)
        st = SM._trainer(g, spec)
        st.set_holdout(True)
        SM._import_old(st, spec, strs, rank, world)
        train, held = strs[rank]
        alive = []
        for mb in train:
            b = st.compile(mb[0], mb[1], mb[4])
            alive.append(b)
            st.step(b)
        hb = st.compile(held[0], held[1], held[4])
        pctr = st.predict(hb)
        st.validate(hb)
        own_c, own_o = st.holdout_read()
        mer_c, mer_o = st.holdout_read(reset=True, merged=True)
        zero_c, zero_o = st.holdout_read()
        st.check()
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), own_c=own_c, own_o=own_o, mer_c=mer_c,
                 mer_o=mer_o, left=np.array([zero_c.sum() + zero_o.sum()]), pctr=pctr,
                 again=st.predict(hb), labels=np.asarray(held[4], np.int32))
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("spec", TWO, ids=["%s-%s" % (s[0], s[5]) for s in TWO])
def test_validate_on_two_ranks(tmp_path, spec):
    world = 2
    port = free_port()
    SM._spawn(_validate_rank, [(r, world, port, spec, str(tmp_path)) for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    sum_c = parts[0]["own_c"] + parts[1]["own_c"]
    sum_o = parts[0]["own_o"] + parts[1]["own_o"]
    for r in range(world):
        same_counts((parts[r]["mer_c"], parts[r]["mer_o"]), (sum_c, sum_o), "merged, rank %d" % r)
        same_counts((parts[r]["own_c"], parts[r]["own_o"]),
                    H.counts_of(parts[r]["pctr"], parts[r]["labels"]), "rank %d's own" % r)
        eq(parts[r]["again"], parts[r]["pctr"])
        assert parts[r]["left"][0] == 0
        assert parts[r]["own_c"].sum() == len(parts[r]["labels"]) > 0


def _owner_refusal(port, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"       # a group of one on the exchange path
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        seen = []
        for sched in ("owner", "owner_stale1"):
            st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule=sched)
            st.set_holdout(False)                    # (off is the default: accepted)
            try:
                st.set_holdout(True)
            except capi.XFError as e:
                assert re.search(r"xf_sharded_holdout.*schedule %s\b" % sched, str(e)) \
                    and "sequential" in str(e), str(e)
                seen.append(sched)
            st.close()
        st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule="stale1")
        st.set_holdout(True)
        try:
            st.set_schedule("owner")
        except capi.XFError as e:
            assert "xf_sharded_set_schedule" in str(e), str(e)
            seen.append("then owner")
        st.set_schedule("sequential")
        try:
            capi.Sharded(g, model="lr", capacity=1 << 12).holdout_read()
        except capi.XFError as e:
            assert "held-out validation is off" in str(e), str(e)
            seen.append("read while off")
        st.close()
        g.close()
        q.put((0, ("ok", seen)))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_owner_schedules_refuse_holdout():
    res = SM._spawn(_owner_refusal, [(free_port(),)])
    assert res[0][1] == ("ok", ["owner", "owner_stale1", "then owner", "read while off"]), res


# ------------------------------------------------------------------ the worker end to end
EPOCHS = 3
SHARE = 0.25
ADMIT = dict(admit_count=2, admit_log2_slots=12, admit_hashes=3)
CROSS = "2*3"
VARIANTS = {
    "plain": {},
    "neg_keep": dict(neg_keep=0.5),
    "admit": dict(ADMIT),
    "cross": dict(cross=CROSS),
}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """full/: the golden training file (one block) and, as its test file, its held rows;
    reduced/: the training file with the held rows deleted, written by the checker, and the same
    test file — a plain run there is the reference of a holdout run on full/"""
    d = tmp_path_factory.mktemp("holdout")
    (d / "full").mkdir()
    (d / "reduced").mkdir()
    shutil.copy(os.path.join(GOLDEN, "small_train-00000"), str(d / "full" / "train-00000"))
    m = H.write_split(str(d / "full" / "train-00000"), str(d / "reduced" / "train-00000"),
                      str(d / "reduced" / "test-00000"), 0, 0, SHARE)   # the worker's seed, rank 0
    shutil.copy(str(d / "reduced" / "test-00000"), str(d / "full" / "test-00000"))
    blocks = list(capi.read_blocks(str(d / "full" / "train-00000"), 2 << 20))
    assert len(blocks) == 1 and len(blocks[0][3]) == len(m)             # a row a line, one block
    assert 20 < int(m.sum()) < len(m) // 2
    return d


def run(data, where, tag, **params):
    pred = str(data / where / ("pred_%s.txt" % tag))
    x = capi.XFlow(str(data / where / "train"), str(data / where / "test"), capacity=1 << 14,
                   pred_path=pred, **params)
    x.train()
    return x, pred


def table_of(x):
    """{key: (w, n, z)} of a worker's LR table"""
    t = capi.Table.from_handle(x.tables()[0], 1, capi.OPT_FTRL)
    keys, w, n, z = t.export()[:4]
    return {int(k): (np.float32(a).tobytes(), np.float32(b).tobytes(), np.float32(c).tobytes())
            for k, a, b, c in zip(keys, w, n, z)}


def staged_held(data, variant):
    """the held rows as validate sees them: crossed, then filtered by the admission filter that
    has counted the (crossed) train part once — the restatements"""
    (rp, keys, fg, labels), = list(capi.read_blocks(str(data / "reduced" / "test-00000"), 2 << 20))
    (trp, tkeys, tfg, _), = list(capi.read_blocks(str(data / "reduced" / "train-00000"), 2 << 20))
    rp, trp = rp.astype(np.uint64), trp.astype(np.uint64)
    if variant == "cross":
        rp, keys, fg, _ = X.Cross(CROSS).apply(rp, keys, fg)
    if variant == "admit":
        flt = A.Filter(ADMIT["admit_log2_slots"], ADMIT["admit_count"], ADMIT["admit_hashes"], 0)
        flt.filter(trp, tkeys, update=True)
        rp, keys, _, _ = flt.filter(rp, keys, update=False)
    return rp.astype(np.uint64), keys, labels


_refs = {}


def reference(data, variant):
    """per epoch count e = 1 .. EPOCHS: a plain run on reduced/ with the variant's parameters;
    its table scores the staged held rows -> the counts and the summary a holdout run must print
    after that epoch; and the last run itself"""
    if variant not in _refs:
        rp, keys, labels = staged_held(data, variant)
        out = []
        for e in range(1, EPOCHS + 1):
            x, pred = run(data, "reduced", "%s_ref%d" % (variant, e), epochs=e, **VARIANTS[variant])
            table = table_of(x)
            t = capi.Table.from_handle(x.tables()[0], 1, capi.OPT_FTRL)
            pctr = capi.lr_predict(t, capi.Batch(rp, keys, labels), capi.Workspace())
            counts, other = H.counts_of(pctr, labels)
            s = capi.progress_summary(counts, other)
            assert P.same(s, P.summary(counts, other))
            out.append((s, table, open(pred, "rb").read(),
                        {n: x.metric(n) for n in ("logloss_ref", "auc", "tp", "fp", "rows_trained",
                                                  "neg_seen", "neg_kept", "admit_seen",
                                                  "admit_kept")}))
        assert out[-1][0]["logloss"] < out[0][0]["logloss"]              # (it learns)
        _refs[variant] = out
    return _refs[variant]


def line_of(e, s):
    return ("holdout epoch %d: rows = %.12g logloss = %.6f (+- %.1e) auc = %.6f (+- %.1e) "
            "ctr = %.6f pctr = %.6f" % (e, s["rows_pos"] + s["rows_neg"], s["logloss"],
                                        s["logloss_bound"], s["auc"], s["auc_slack"], s["ctr"],
                                        s["pctr"]))


def check_run(x, pred, out, ref, epochs_run=EPOCHS):
    lines = [ln for ln in out.split("\n") if ln.startswith("holdout epoch ")]
    assert lines == [line_of(e, ref[e][0]) for e in range(epochs_run)], (lines, out)
    s, table, pred_bytes, metrics = ref[epochs_run - 1]
    for n in ("logloss", "auc", "ctr", "pctr"):
        assert x.metric("holdout_" + n) == s[n], n
    assert x.metric("holdout_rows") == s["rows_pos"] + s["rows_neg"]
    assert x.metric("holdout_logloss_first") == ref[0][0]["logloss"]
    assert x.metric("epochs_run") == epochs_run
    # the keys of the run on the reduced file: bit for bit; whatever else the table holds (keys
    # that only held rows carry) is at first-touch state
    got = table_of(x)
    zero = (np.float32(0).tobytes(),) * 3
    for k, v in table.items():
        assert got[k] == v, k
    assert all(v == zero for k, v in got.items() if k not in table)
    assert len(table) > 100
    assert open(pred, "rb").read() == pred_bytes
    for n, v in metrics.items():
        assert x.metric(n) == v, n


@pytest.mark.parametrize("ingest", ["host", "gpu_fields"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_worker_end_to_end(data, capfd, variant, ingest):
    ref = reference(data, variant)
    capfd.readouterr()
    x, pred = run(data, "full", "%s_%s" % (variant, ingest), epochs=EPOCHS, holdout=SHARE,
                  ingest=ingest, **VARIANTS[variant])
    out = capfd.readouterr().out
    assert x.metric("blocks_gpu") == (0 if ingest == "host" else 1)
    check_run(x, pred, out, ref)
    curve = [r[0]["logloss"] for r in ref]
    best = int(np.argmin(curve))
    assert (x.metric("holdout_best_epoch"), x.metric("holdout_best_logloss")) == (best, curve[best])


@pytest.mark.parametrize("variant", ["plain", "neg_keep"])
def test_worker_without_the_batch_cache(data, capfd, variant):
    """cache_batches=0: every epoch reads the text again and splits it again — the same rows are
    held (no epoch in the split's stream), the held list of the first epoch stays; under negative
    subsampling the later epochs draw other negatives, on both runs alike"""
    key = variant + "_nocache"
    VARIANTS[key] = dict(VARIANTS[variant], cache_batches=0)
    ref = reference(data, key)
    capfd.readouterr()
    x, pred = run(data, "full", key, epochs=EPOCHS, holdout=SHARE, **VARIANTS[key])
    check_run(x, pred, capfd.readouterr().out, ref)


def test_holdout_every_and_early_stop(data, capfd):
    ref = reference(data, "plain")
    curve = [r[0]["logloss"] for r in ref]
    # holdout_every=2 of 3 epochs: after epoch 1 and after the last one
    capfd.readouterr()
    x, pred = run(data, "full", "every2", epochs=EPOCHS, holdout=SHARE, holdout_every=2)
    lines = [ln for ln in capfd.readouterr().out.split("\n") if ln.startswith("holdout epoch ")]
    assert lines == [line_of(1, ref[1][0]), line_of(2, ref[2][0])]
    assert x.metric("holdout_logloss_first") == curve[1] and x.metric("epochs_run") == EPOCHS
    # a delta no epoch improves by: the checker says the rule stops after the second epoch
    delta = 2.0 * (curve[0] - min(curve)) + 1.0
    stops = [e for e in range(EPOCHS) if H.should_stop(curve[:e + 1], 1, delta)[0]]
    assert stops[0] == 1 and H.should_stop(curve[:2], 1, delta) == (True, 0)
    capfd.readouterr()
    x, pred = run(data, "full", "stop", epochs=EPOCHS, holdout=SHARE, early_stop=1,
                  early_stop_delta=delta)
    out = capfd.readouterr().out
    check_run(x, pred, out, ref, epochs_run=2)
    assert "early stop after epoch 1: best epoch 0 logloss = %.6f" % curve[0] in out.split("\n")
    assert (x.metric("holdout_best_epoch"), x.metric("holdout_best_logloss")) == (0, curve[0])
    # ... and with delta = 0 on this curve (it improves every epoch) it never does
    assert not any(H.should_stop(curve[:e + 1], 1, 0.0)[0] for e in range(EPOCHS))
    capfd.readouterr()
    x, pred = run(data, "full", "nostop", epochs=EPOCHS, holdout=SHARE, early_stop=1)
    out = capfd.readouterr().out
    check_run(x, pred, out, ref)
    assert "early stop" not in out


def test_holdout_zero_is_the_run_without_it(data, capfd):
    """holdout=0: output, table, metrics and the launch counters of a run that never heard of it"""
    def launches():
        grads = np.zeros(5, np.uint64)
        capi.lib().xf_lr_grad_launches(grads.ctypes.data_as(capi.u64p))
        return np.concatenate([grads, np.array([capi.progress_launches(),
                                                capi.lib().xf_weigh_negatives_launches()],
                                               np.uint64)]).astype(np.int64)

    def counted(tag, **params):
        at = launches()
        capfd.readouterr()
        x, pred = run(data, "full", tag, epochs=EPOCHS, **params)
        return x, open(pred, "rb").read(), capfd.readouterr().out, (launches() - at).tolist()
    x, pred_x, out_x, n_x = counted("zero", holdout=0)
    y, pred_y, out_y, n_y = counted("never")
    strip = lambda s: [ln for ln in s.split("\n") if not ln.startswith("examples/sec")]  # noqa: E731
    assert pred_x == pred_y and strip(out_x) == strip(out_y) and n_x == n_y
    assert "holdout" not in out_x
    assert table_of(x) == table_of(y)
    for n in ("logloss_ref", "auc", "tp", "fp", "keys", "rows_trained", "epochs_run"):
        assert x.metric(n) == y.metric(n), n
    assert x.metric("epochs_run") == EPOCHS and x.metric("rows_trained") == EPOCHS * 200
    with pytest.raises(capi.XFError, match="no epoch has been validated"):
        x.metric("holdout_logloss")


def test_cli_prints_one_line_per_epoch(data, tmp_path):
    ref = reference(data, "plain")
    out = subprocess.run([CLI, str(data / "full" / "train"), str(data / "full" / "test"), "0",
                          str(EPOCHS), "capacity=16384", "pred_path=cli.txt",
                          "holdout=%r" % SHARE],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.split("\n") if ln.startswith("holdout epoch ")]
    assert lines == [line_of(e, ref[e][0]) for e in range(EPOCHS)]
    assert open(str(tmp_path / "cli.txt"), "rb").read() == ref[-1][2]


# ---- two workers: scripts/local.sh 2 2 xflow_lr ... holdout=0.25
def _local_sh(cwd, train, test, epochs, *args):
    env = dict(os.environ, DMLC_PS_ROOT_PORT=str(free_port()))
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI,
                          train, test, "0", str(epochs), "transport=host", "capacity=16384",
                          "model_out=" + os.path.join(cwd, "model"),
                          "pred_path=" + os.path.join(cwd, "pred.txt"), *args],
                         capture_output=True, text=True, timeout=240, env=env, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    one = capi.Sharded(None, model="lr", optimizer="ftrl", capacity=1 << 15)
    one.load(os.path.join(cwd, "model"))                   # two shard files -> one table
    return out.stdout.split("\n"), one


def test_local_sh_two_workers(tmp_path):
    """each rank splits its own file under its own stream; the merged counts are those of both
    ranks' held rows scored by the table of a two-worker run on the two reduced files"""
    full, red = tmp_path / "full", tmp_path / "reduced"
    full.mkdir()
    red.mkdir()
    held = []
    for r, src in enumerate(("small_train-00000", "small_test-00000")):
        shutil.copy(os.path.join(GOLDEN, src), str(full / ("train-%05d" % r)))
        H.write_split(str(full / ("train-%05d" % r)), str(red / ("train-%05d" % r)),
                      str(red / ("held-%05d" % r)), 0, r, SHARE)
        (blk,) = list(capi.read_blocks(str(red / ("held-%05d" % r)), 2 << 20))
        held.append((blk[0].astype(np.uint64), blk[1], blk[3]))
        assert len(blk[3]) > 20
    for d in (full, red):
        shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "test-00000"))
    want, tables = [], []
    for e in (1, 2):
        cwd = tmp_path / ("ref%d" % e)
        cwd.mkdir()
        _, one = _local_sh(str(cwd), str(red / "train"), str(red / "test"), e)
        tables.append({int(k): (np.float32(a).tobytes(), np.float32(b).tobytes(),
                                np.float32(c).tobytes())
                       for k, a, b, c in zip(*one.w.export()[:4])})
        counts = np.zeros((2, P.RANKS), np.uint64)
        other = np.zeros(2, np.uint64)
        for rp, keys, labels in held:
            c, o = H.counts_of(one.predict(one.compile(rp, keys, labels)), labels)
            counts += c
            other += o
        want.append(line_of(e - 1, capi.progress_summary(counts, other)))
        one.close()
    cwd = tmp_path / "run"
    cwd.mkdir()
    lines, one = _local_sh(str(cwd), str(full / "train"), str(full / "test"), 2,
                           "holdout=%r" % SHARE)
    assert [ln for ln in lines if ln.startswith("holdout epoch ")] == want   # rank 0 alone prints
    got = {int(k): (np.float32(a).tobytes(), np.float32(b).tobytes(), np.float32(c).tobytes())
           for k, a, b, c in zip(*one.w.export()[:4])}
    zero = (np.float32(0).tobytes(),) * 3
    for k, v in tables[-1].items():
        assert got[k] == v, k
    assert all(v == zero for k, v in got.items() if k not in tables[-1])
    assert len(tables[-1]) > 100
    one.close()
