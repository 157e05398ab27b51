"""Feature crosses (xf_cross.hip, the worker's cross=) on a real MI355X.  The only reference of the
stage is the numpy restatement tests/_cross_checker.py (pinned to a plain loop and to the known
answers by tests/test_cross_cpu.py); the trainers are each mode's existing checker, fed from the
restatement's arrays.  Every comparison is exact — integer arrays, float arrays as their bits.

* the stage: the crossed arrays and the statistics on minibatches chosen where the passes can go
  wrong, one after the other on ONE stage, with and without values and fgid output; again with
  every row forced through the long-row emit and its lists in the global scratch;
* identity, the 2^32 - 1 limit, a missing fgid, a row slice of a block;
* LR (cells, both optimizers), valued LR, canonical and field-aware FM, LR on two ranks, each
  stepped on the stage's device arrays;
* the worker end to end on the golden sample files."""
import os
import re
import shutil
import subprocess
import traceback

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import build, capi

from . import _admit_checker as A
from . import _cross_checker as X
from . import _ffm_checker as F
from . import _negsample_checker as N
from . import _valued_cases as Cs
from . import _valued_checker as V
from . import test_gpu_sharded_modes as SM     # _spawn, _check_tables, _export (the module)
from .conftest import GOLDEN
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(build.LIBDIR, "xflow_lr")
BIG = 2147483647


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


def same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(a, b):
        i = np.flatnonzero((a != b).ravel())
        raise AssertionError("%s: %d of %d differ; first (at, got, want): %s" % (
            what, i.size, a.size, [(j, a.ravel()[j], b.ravel()[j]) for j in i[:6]]))


def tile_size():
    """the row tile of the count and the emit pass, read from the source"""
    src = open(os.path.join(ROOT, "xflow_amd", "csrc", "xf_cross.hip")).read()
    return int(re.search(r"constexpr uint32_t kCxTile = (\d+);", src).group(1))


# ------------------------------------------------------------------ the stage's minibatches
# 32 pairs: field 1 in several pairs and on both sides, (1, 2) together with (2, 1), the two ends
# of the id range on both sides, a pair one of whose fields never occurs (5 * 6), and pairs none
# of whose fields occur.  Field 7 is in no pair.
SPEC = [(1, 2), (2, 1), (1, 3), (4, 1), (0, BIG), (BIG, 0), (5, 6), (3, 4)] + \
    [(100 + p, 200 + p) for p in range(24)]
FIELDS = np.array([0, 1, 2, 3, 4, 5, 7, 7, 7, BIG], np.int32)      # what a random nonzero draws from
BASE = 40


def _keys(rng, n):
    return rng.randint(0, 1 << 62, size=n).astype(np.uint64) * np.uint64(4) + \
        rng.randint(0, 4, size=n).astype(np.uint64)


def _vals(rng, n):
    """full mantissas, mixed signs, a spread of exponents"""
    return (rng.randn(n) * np.exp2(rng.randint(-8, 9, size=n))).astype(np.float32)


def _mb(rng, lens, fgid=None):
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(rowptr[-1])
    fg = FIELDS[rng.randint(0, len(FIELDS), size=n)] if fgid is None else \
        np.asarray(fgid, np.int32)
    assert len(fg) == n
    return rowptr, _keys(rng, n), fg, _vals(rng, n)


def _explicit(rng, rows):
    return _mb(rng, [len(r) for r in rows], np.concatenate([np.asarray(r, np.int64) for r in rows]))


def sequence():
    """[(name, rowptr, keys, fgid, values)] in the order they are applied to one stage"""
    rng = np.random.RandomState(41)
    T = tile_size()
    out = []
    add = lambda name, mb: out.append((name,) + mb)  # noqa: E731
    add("no_rows", (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32),
                    np.zeros(0, np.float32)))
    add("no_nonzeros", (np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32),
                        np.zeros(0, np.float32)))
    lens = rng.randint(0, 40, size=700)
    lens[:3] = 0
    lens[-2:] = 0
    lens[300:340] = 0
    lens[rng.rand(700) < 0.05] = 0
    add("ragged", _mb(rng, lens))
    add("explicit", _explicit(rng, [
        [1, 1, 7, 7],                      # only A members (of 1*2), only B members (of 2*1)
        [2, 2, 2, 7],
        [7, 7, 7],                         # neither
        [1, 7, 1, 2, 2, 7, 2],             # 2 x 3
        [7, 1, 2, 2, 2, 2, 2],             # 1 x 5
        [1, 7, 7, 7, 2],                   # the members are the first and the last nonzero
        [0, BIG],                          # fgids 0 and 2^31 - 1, both orders of the pair
        [BIG, 7, 0, 0],
        [5, 5, 5],                         # a pair whose other field never occurs
        [],
        [3, 4, 1],                         # field 1 on the B side (4*1) and the A side (1*3); 3*4
        [7]]))
    add("lengths", _mb(rng, [1, 63, 64, 65, 127, 128, 129, 0, 64, 64]))
    # 40 x 30 members of one pair (and 30 x 40 of its mirror), 7 x 0 of another, the rest field 7
    fg = np.full(5000, 7, np.int64)
    at = rng.permutation(5000)
    fg[at[:40]], fg[at[40:70]], fg[at[70:77]] = 1, 2, 5
    add("long_row", _mb(rng, [3, 0, 5000, 0, 7], np.concatenate([
        FIELDS[rng.randint(0, len(FIELDS), size=3)], fg, FIELDS[rng.randint(0, len(FIELDS), size=7)]])))
    add("short_rows", _mb(rng, rng.randint(1, 4, size=300)))
    for R in (T - 1, T, T + 1, 2 * T + 1):
        add("rows%d" % R, _mb(rng, rng.randint(0, 20, size=R)))
    add("click_rows", _mb(rng, np.full(150, 17), np.tile(np.r_[0:6, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, BIG], 150)))
    add("no_rows_again", out[0][1:])
    return out


COMP = [(False, False), (True, False), (False, True), (True, True)]


def _expect(mbs, with_vs):
    ref, expect = X.Cross(SPEC, BASE), []
    for name, rowptr, keys, fg, vs in mbs:
        e = ref.apply(rowptr, keys, fg, vs if with_vs else None)
        expect.append(e + (ref.stats(),))
        n_in = len(keys)
        if name == "long_row":
            assert len(e[1]) - n_in >= 2 * 1200
        if name == "lengths":          # crossed rows longer than one 64-position chunk of the emit
            assert (np.diff(e[0].astype(np.int64)) - np.diff(rowptr.astype(np.int64)) > 64).any()
        if name == "explicit":
            d = np.diff(e[0].astype(np.int64)) - np.diff(rowptr.astype(np.int64))
            assert d.tolist() == [0, 0, 0, 12, 10, 2, 2, 4, 0, 0, 3, 0], d
    assert ref.stats()[2] > ref.stats()[1] // 4
    return expect


def _apply_all(mbs, expect, with_fg, with_vs):
    st = capi.Cross(SPEC, fgid_base=BASE)
    assert st.params() == (SPEC, BASE)
    for (name, rowptr, keys, fg, vs), (rp, ks, efg, evs, stats) in zip(mbs, expect):
        got = st.apply(rowptr, keys, fg, values=vs if with_vs else None, want_fgid=with_fg)
        same(got[0], rp, name + " rowptr")
        same(got[1], ks, name + " keys")
        at = 2
        if with_fg:
            same(got[at], efg, name + " fgid")
            at += 1
        if with_vs:
            same(got[at], evs, name + " values")
            at += 1
        assert len(got) == at and st.stats() == stats, name


@pytest.mark.parametrize("with_fg,with_vs", COMP, ids=["keys", "fgid", "vals", "both"])
def test_crossed_arrays_and_stats(with_fg, with_vs):
    mbs = sequence()
    _apply_all(mbs, _expect(mbs, with_vs), with_fg, with_vs)


@pytest.mark.parametrize("short_max,lds_chunks", [(0, 2048), (0, 1), (16, 4)],
                         ids=["all_long", "all_long_spilled", "mixed"])
def test_the_emit_paths_agree(short_max, lds_chunks):
    """xf_tune moves rows between the wave-per-row emit, the workgroup-per-row emit with its
    member lists in LDS, and the same with the lists in the global scratch: the result is the
    restatement's whichever path a row takes"""
    mbs = sequence()
    expect = _expect(mbs, True)
    try:
        capi.tune("cross_short_max", short_max)
        capi.tune("cross_lds_chunks", lds_chunks)
        _apply_all(mbs, expect, True, True)
    finally:
        capi.tune("cross_short_max", 64)
        capi.tune("cross_lds_chunks", 2048)


def test_a_spec_whose_fields_never_occur_is_the_identity():
    st = capi.Cross("300*301,302*300")
    for name, rowptr, keys, fg, vs in sequence():
        got = st.apply(rowptr, keys, fg, values=vs)
        for g, want in zip(got, (rowptr.astype(np.uint32), keys, fg, vs)):
            assert g.dtype == want.dtype and g.tobytes() == want.tobytes(), name
    assert st.stats()[2] == 0
    # binary LR: a table stepped on the stage's device arrays is the table stepped on the minibatch
    name, rowptr, keys, fg, _ = sequence()[2]
    keys = capi.hash_decimal_range(0, 3000)[np.random.RandomState(1).randint(0, 3000, size=len(keys))]
    labels = np.random.RandomState(5).randint(0, 2, size=len(rowptr) - 1).astype(np.int32)
    a = capi.Sharded(model="lr", capacity=1 << 14)
    b = capi.Sharded(model="lr", capacity=1 << 14)
    for _ in range(3):
        d = st.apply_dev(rowptr, keys, fg, labels=labels, want_fgid=False, stream=a.stream())
        assert (d.R, d.NNZ) == (len(labels), len(keys))
        a.step(a.compile_dev(*d[:5]))
        a.check()
        b.step(b.compile(rowptr, keys, labels))
        b.check()
    for x, y in zip(a.w.export(), b.w.export()):
        same(x, y)
    assert len(a.w) > 100


def test_a_total_of_2_to_the_32_is_refused_and_the_stage_lives_on():
    n = 66000
    rowptr = np.array([0, 2 * n], np.uint64)
    keys = np.arange(2 * n, dtype=np.uint64)
    fg = np.r_[np.full(n, 1), np.full(n, 2)].astype(np.int32)
    st = capi.Cross("1*2")
    with pytest.raises(capi.XFError, match=r"xf_cross_apply_dev.*\b4356132000\b"):
        st.apply(rowptr, keys, fg)
    assert st.stats() == (0, 0, 0)
    got = st.apply(np.array([0, 2, 3], np.uint64), np.array([5, 6, 7], np.uint64),
                   np.array([1, 2, 2], np.int32))
    e = X.Cross("1*2").apply(np.array([0, 2, 3], np.uint64), np.array([5, 6, 7], np.uint64),
                             np.array([1, 2, 2], np.int32))
    for g, w in zip(got, e[:3]):
        same(g, w)
    assert len(got[1]) == 4 and st.stats() == (2, 3, 1)


def test_bad_arguments():
    st = capi.Cross("1*2")
    d = st.apply_dev(np.array([0, 2], np.uint64), np.array([5, 6], np.uint64),
                     np.array([1, 2], np.int32))
    with pytest.raises(capi.XFError, match=r"xf_cross_apply_dev.*d_fgid is NULL"):
        st.cross_dev(d.d_keys, d.d_rowptr, 1, 2, None)
    with pytest.raises(capi.XFError, match=r"xf_cross_apply.*fgid is NULL"):
        st.apply_dev(np.array([0, 2], np.uint64), np.array([5, 6], np.uint64), None)
    with pytest.raises(capi.XFError, match="descend"):
        st.apply(np.array([0, 3, 2], np.uint64), np.zeros(3, np.uint64), np.zeros(3, np.int32))


def test_row_slice_of_a_block():
    """host arrays whose first offset is not 0: rows [100, 300) of a block"""
    name, rowptr, keys, fg, vs = sequence()[2]
    labels = np.arange(len(rowptr) - 1, dtype=np.int32)
    st, ref = capi.Cross(SPEC, BASE), X.Cross(SPEC, BASE)
    got = st.apply(rowptr, keys, fg, labels=labels, values=vs, row_begin=100, row_end=300)
    e = ref.apply(rowptr[100:301], keys, fg, vs)
    same(got[0], e[0], "rowptr")
    same(got[1], e[1], "keys")
    same(got[2], labels[100:300], "labels")
    same(got[3], e[2], "fgid")
    same(got[4], e[3], "values")
    assert len(e[1]) > int(rowptr[300] - rowptr[100]) and st.stats() == ref.stats()


# ------------------------------------------------------------------ trainers fed from the stage
TSPEC, TBASE, TRAW = "0*1,2*3", 4, 4     # raw fgids in [0, 4); field-aware: fields = 4 + 2


def trainer_stream(seed=0):
    """three minibatches (rowptr, keys, fgid, values, labels): tests/_valued_cases.py's ragged
    rows with a field per nonzero"""
    out = []
    for i, (rowptr, keys, vals, labels) in enumerate(Cs.stream("ragged", seed=seed)):
        fg = np.random.RandomState(90 + seed + i).randint(0, TRAW, size=len(keys)).astype(np.int32)
        out.append((rowptr, keys, fg, vals, labels))
    return out


def crossed(mbs, base=0):
    """the restatement's arrays of a stream: (rowptr u64, keys, fgid, values, labels)"""
    chk, out = X.Cross(TSPEC, base), []
    for rowptr, keys, fg, vals, labels in mbs:
        rp, ks, cfg, cv = chk.apply(rowptr, keys, fg, vals)
        assert len(ks) > len(keys) * 3 // 2
        out.append((rp.astype(np.uint64), ks, cfg, cv, labels))
    return out


def export_same(table, store, opt, what):
    for a, e in zip(table.export()[:4 if opt == "ftrl" else 2], store.export()):
        same(a, e, what)


@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
def test_lr_on_cells_from_the_stage(opt):
    mbs = trainer_stream()
    s = O.Store(O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD, 1)
    with O.sum_mode(1):
        for rp, ks, _, _, labels in crossed(mbs):
            O.lr_update(s, O.Batch(rp, ks, labels))
        held = crossed(mbs)[0]
        ob = O.Batch(held[0], held[1], held[4])
        pctr = ob.lr_loss(s.pull(ob.ukeys))[1]
    st, x = capi.Sharded(model="lr", optimizer=opt, capacity=1 << 18), capi.Cross(TSPEC)
    for rowptr, keys, fg, _, labels in mbs:
        d = x.apply_dev(rowptr, keys, fg, labels=labels, want_fgid=False, stream=st.stream())
        st.step(st.compile_dev(*d[:5]))
        st.check()
    d = x.apply_dev(mbs[0][0], mbs[0][1], mbs[0][2], labels=mbs[0][4], want_fgid=False,
                    stream=st.stream())
    same(st.predict(st.compile_dev(*d[:5])), pctr, "pctr")
    export_same(st.w, s, opt, "w")


@pytest.mark.parametrize("model,opt,k", [("lr", "ftrl", 1), ("fm", "sgd", 4)],
                         ids=["valued_lr", "canonical_fm_values"])
def test_valued_trainers_from_the_stage(model, opt, k):
    """valued LR on the cells and canonical FM with values: the crossed value is the product"""
    mbs = trainer_stream()
    cm = [(rp, ks, cv, labels) for rp, ks, _, cv, labels in crossed(mbs)]
    audit = []
    _, sw, sv, pctr = Cs.run_checker(model, opt, k, cm, audit)
    V.assert_exact(audit)
    st = capi.Sharded(model=model, optimizer=opt, k=k, capacity=1 << 18, seed=7,
                      fm_mode="canonical" if model == "fm" else "reference")
    st.w.import_(*Cs.old_state(Cs.stream_keys(cm), opt, 1, "w"))
    if model == "fm":
        st.v.import_(*Cs.old_state(Cs.stream_keys(cm), opt, k))
    x = capi.Cross(TSPEC)
    for rowptr, keys, fg, vals, labels in mbs:
        d = x.apply_dev(rowptr, keys, fg, labels=labels, values=vals, want_fgid=False,
                        stream=st.stream())
        b = st.compile_valued_dev(d.d_keys, d.d_vals, d.d_rowptr, d.d_labels, d.R, d.NNZ)
        st.step(b)
        st.check()
    same(st.predict(b), pctr, "pctr")
    export_same(st.w, sw, opt, "w")
    if model == "fm":
        export_same(st.v, sv, opt, "v")


def test_field_aware_fm_from_the_stage():
    """fields = base + pairs, fgid_base = base: a crossed nonzero is a member of its pair's field"""
    opt, k, Fd = "sgd", 4, TBASE + 2
    mbs = trainer_stream()
    cm = crossed(mbs, TBASE)
    assert max(int(m[2].max()) for m in cm) == Fd - 1
    audit = []
    _, sw, sv, pctr = F.run_checker(opt, Fd, k, cm, audit, valued=False)
    F.assert_exact(audit)
    st = capi.Sharded(model="fm", optimizer=opt, k=k, capacity=1 << 18, seed=7,
                      fm_mode="field_aware", fields=Fd)
    st.w.import_(*Cs.old_state(F.stream_keys(cm), opt, 1, "w"))
    st.v.import_(*Cs.old_state(F.stream_keys(cm), opt, Fd * k))
    x = capi.Cross(TSPEC, fgid_base=TBASE)
    for rowptr, keys, fg, _, labels in mbs:
        d = x.apply_dev(rowptr, keys, fg, labels=labels, stream=st.stream())
        h = capi.vp()
        capi.check(capi.lib().xf_sharded_compile_fielded_dev(
            st.h, capi.C.byref(h), d.d_keys, d.d_fgid, None, d.d_rowptr, d.d_labels, d.R, d.NNZ, 1))
        b = capi.ShardedBatch(h, st)
        st.step(b)
        st.check()
    same(st.predict(b), pctr, "pctr")
    export_same(st.w, sw, opt, "w")
    export_same(st.v, sv, opt, "v")


def rank_streams(world):
    """per rank: (three training minibatches, a held-out one), each (rowptr, keys, fgid, labels)"""
    out = []
    for r in range(world):
        train, held = trainer_stream(seed=10 + 7 * r), trainer_stream(seed=15 + 7 * r)[0]
        four = lambda m: (m[0], m[1], m[2], m[4])  # noqa: E731
        out.append(([four(m) for m in train], four(held)))
    return out


def _crossed_lr_rank(rank, world, port, opt, schedule, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        st = capi.Sharded(g, model="lr", optimizer=opt, capacity=1 << 18, schedule=schedule,
                          seed=7)
        x = capi.Cross(TSPEC)
        train, held = rank_streams(world)[rank]
        alive = []
        for rowptr, keys, fg, labels in train:
            d = x.apply_dev(rowptr, keys, fg, labels=labels, want_fgid=False, stream=st.stream())
            b = st.compile_dev(*d[:5])
            alive.append(b)
            st.step(b)
        st.check()
        d = x.apply_dev(held[0], held[1], held[2], labels=held[3], want_fgid=False,
                        stream=st.stream())
        out = {"pctr": st.predict(st.compile_dev(*d[:5]))}
        st.check()
        SM._export(st, out)
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("schedule", ["sequential", "owner"])
def test_lr_on_two_ranks_from_the_stage(tmp_path, schedule):
    """every rank crosses its own rows; the trainers see keys only, the owner-compute schedule
    included (its rank-ordered update is the sequential schedule's table)"""
    world, opt = 2, "ftrl"
    strs = []
    for train, held in rank_streams(world):
        chk = X.Cross(TSPEC)
        cr = lambda m: (lambda e: (e[0].astype(np.uint64), e[1], m[3]))(chk.apply(m[0], m[1], m[2]))  # noqa: E731
        strs.append(([cr(m) for m in train], cr(held)))
    store, pctr = N.sharded_lr_run(opt, "sequential", strs, np.float32(1.0))
    port = free_port()
    SM._spawn(_crossed_lr_rank, [(r, world, port, opt, schedule, str(tmp_path))
                                 for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    SM._check_tables(parts, world, store, None, opt)
    for r in range(world):
        same(parts[r]["pctr"], np.asarray(pctr[r], np.float32), "rank %d pctr" % r)


# ------------------------------------------------------------------ the worker end to end
from . import test_gpu_admit as TA             # noqa: E402  (Model, ADMIT: the module)
from . import test_gpu_negsample as TN         # noqa: E402  (WeightedModel)

WSPEC = "2*3,16*17"        # the golden rows hold fields 1 .. 17, 16 and 17 more than once in places
KEEP = 0.25


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("cross")
    shutil.copy(os.path.join(GOLDEN, "small_train-00000"), str(d / "train-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "test-00000"))
    shutil.copy(os.path.join(GOLDEN, "small_test-00000"), str(d / "train-00001"))   # (two workers)
    return d


_refs = {}


def reference(data, admit, neg):
    """the restatement does what the worker does: every training block sampled (when on), crossed,
    filtered by admission (when on), stepped; the second epoch replays; the test blocks crossed and
    filtered read-only"""
    if (admit, neg) in _refs:
        return _refs[admit, neg]
    smp = N.Sampler(KEEP, 0) if neg else None                     # the worker's seed: 0
    chk = X.Cross(WSPEC)
    flt = A.Filter(12, 2, 3, 0) if admit else None
    m = TN.WeightedModel("lr", N.weight(KEEP)) if neg else TA.Model("lr")
    mbs, ordinal = [], 0
    for rp, keys, fg, labels, vals in capi.read_blocks(str(data / "train-00000"), 2 << 20,
                                                       values=True):
        if smp is not None:
            rp, keys, labels, fg, vals = smp.apply(0, ordinal, rp, keys, labels, fg, vals)
            ordinal += len(labels)
        n_in = len(keys)
        rp, keys, fg, vals = chk.apply(rp, keys, fg, vals)
        assert len(keys) > n_in + len(labels)       # (fields 16 and 17 are multi-valued in places)
        if flt is not None:
            rp, keys, fg, vals = flt.filter(rp.astype(np.uint64), keys, fg, vals, update=True)
        mbs.append((rp.astype(np.uint64), keys, fg, vals, labels))
    assert len(mbs) == 1
    for epoch in range(2):
        for mb in mbs:
            m.step(mb)
    labs, ps = [], []
    for rp, keys, fg, labels, vals in capi.read_blocks(str(data / "test-00000"), 4 << 20,
                                                       values=True):
        rp, keys, fg, vals = chk.apply(rp, keys, fg, vals)
        if flt is not None:
            rp, keys, fg, vals = flt.filter(rp.astype(np.uint64), keys, fg, vals, update=False)
        ps.append(m.predict((rp.astype(np.uint64), keys, fg, vals, labels)))
        labs.append(labels)
    lab, p = np.concatenate(labs), np.concatenate(ps)
    _, nin, ncross = chk.stats()
    _refs[admit, neg] = (m, lab, p, O.auc_logloss(lab, p), (nin, nin + ncross),
                         (flt.seen, flt.kept) if flt is not None else (0, 0))
    return _refs[admit, neg]


def check_worker(x, pred, ref):
    m, lab, p, (ll, auc, tp, fp), cstats, admitted = ref
    wh, _ = x.tables()
    for a, e in zip(capi.Table.from_handle(wh, 1, capi.OPT_FTRL).export()[:4], m.ws.export()):
        same(a, e, "table")
    assert open(pred).read().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]
    assert (np.float32(x.metric("logloss_ref")), np.float32(x.metric("auc"))) == \
        (np.float32(ll), np.float32(auc))
    assert (x.metric("tp"), x.metric("fp")) == (tp, fp)
    assert x.metric("keys") == len(m.ws)
    assert (x.metric("cross_in"), x.metric("cross_out")) == cstats
    assert (x.metric("admit_seen"), x.metric("admit_kept")) == admitted


def run_worker(data, ingest, tag, admit, neg, **extra):
    pred = str(data / ("pred_%s.txt" % tag))
    p = dict(model=0, cross=WSPEC, epochs=2)
    if admit:
        p.update(TA.ADMIT)
    if neg:
        p["neg_keep"] = KEEP
    p.update(extra)
    x = capi.XFlow(str(data / "train"), str(data / "test"), capacity=1 << 14, ingest=ingest,
                   pred_path=pred, **p)
    x.train()
    return x, pred


@pytest.mark.parametrize("neg", [False, True], ids=["all_rows", "neg_keep"])
@pytest.mark.parametrize("admit", [False, True], ids=["plain", "admission"])
@pytest.mark.parametrize("ingest", ["host", "gpu_fields"])
def test_worker_end_to_end(data, ingest, admit, neg):
    ref = reference(data, admit, neg)
    x, pred = run_worker(data, ingest, "%s%d%d" % (ingest, admit, neg), admit, neg)
    check_worker(x, pred, ref)


def test_crossed_keys_enter_the_table(data):
    """... beside the plain run's: cross off is the worker without the stage"""
    x = capi.XFlow(str(data / "train"), str(data / "test"), capacity=1 << 14, epochs=2,
                   pred_path=str(data / "pred_plain.txt"))
    x.train()
    assert (x.metric("cross_in"), x.metric("cross_out")) == (0, 0)
    assert len(reference(data, False, False)[0].ws) > x.metric("keys")


def test_block_cache_gives_the_same_run(data, tmp_path):
    ref = reference(data, False, False)
    for tag in ("write", "read"):                                # the cache is written, then read
        x, pred = run_worker(data, "host", "cache_" + tag, False, False, block_cache=1,
                             block_cache_dir=str(tmp_path))
        check_worker(x, pred, ref)


def test_cli_prints_the_same_metric_line(data, tmp_path):
    _, lab, p, (ll, auc, tp, fp), cstats, _ = reference(data, False, False)
    out = subprocess.run([CLI, str(data / "train"), str(data / "test"), "0", "2",
                          "capacity=16384", "pred_path=cli.txt", "cross=" + WSPEC],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert O.format_auc_line(ll, auc, tp, fp) in lines, out.stdout
    assert "rank 0 cross_in = %d cross_out = %d" % cstats in lines, out.stdout
    assert open(str(tmp_path / "cli.txt")).read().split("\n")[:-1] == \
        ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, lab)]


def test_local_sh_two_workers(data, tmp_path):
    """scripts/local.sh 2 2 ... cross=: a turn is one block of every rank, each crossed by its own
    rank; both ranks pull, then push in rank order; the second epoch replays"""
    chk = [X.Cross(WSPEC), X.Cross(WSPEC)]
    turn = []
    for r in range(2):
        (rp, keys, fg, labels), = capi.read_blocks(str(data / ("train-%05d" % r)), 2 << 20)
        crp, ck, _, _ = chk[r].apply(rp, keys, fg)
        turn.append((crp.astype(np.uint64), ck, labels))
    with O.sum_mode(1):
        s = O.Store(O.OPT_FTRL, 1)
        s.push(np.array([0], np.uint64), np.zeros(1, np.float32))
        for epoch in range(2):
            obs = [O.Batch(*mb) for mb in turn]
            pulled = [s.pull(ob.ukeys) for ob in obs]
            grads = [ob.lr_grad(ob.lr_loss(pw)[0]) for ob, pw in zip(obs, pulled)]
            for ob, g in zip(obs, grads):
                s.push(ob.ukeys, g)
        trained = s.export()
        (rp, keys, fg, labels), = capi.read_blocks(str(data / "test-00000"), 4 << 20)
        stats0 = chk[0].stats()
        crp, ck, _, _ = chk[0].apply(rp, keys, fg)                 # rank 0 scores the test file
        b = O.Batch(crp.astype(np.uint64), ck, labels)
        p = b.lr_loss(s.pull(b.ukeys))[1]
    ll, auc, tp, fp = O.auc_logloss(labels, p)
    ckpt, pred = str(tmp_path / "model"), str(tmp_path / "pred.txt")
    env = dict(os.environ, DMLC_PS_ROOT_PORT=str(free_port()))
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI,
                          str(data / "train"), str(data / "test"), "0", "2", "transport=host",
                          "capacity=16384", "model_out=" + ckpt, "pred_path=" + pred,
                          "cross=" + WSPEC],
                         capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert O.format_auc_line(ll, auc, tp, fp) in lines, lines
    assert open(pred).read().split("\n")[:-1] == ["%g\t%d\t%d" % (a, 1 - b, b) for a, b in zip(p, labels)]
    want = sorted("rank %d cross_in = %d cross_out = %d" % (r, c.stats()[1], sum(c.stats()[1:]))
                  for r, c in enumerate(chk))
    assert sorted(ln for ln in lines if "cross_in" in ln) == want and stats0[1] > 0
    one = capi.Sharded(None, model="lr", optimizer="ftrl", capacity=1 << 15)
    one.load(ckpt)                                               # two shard files -> one table
    for a, e in zip(one.w.export(), trained):
        same(a, e)
    assert len(trained[0]) > 100


REFUSALS = [
    (dict(core_num=2), r"cross=2\*3,16\*17 needs core_num=1, not core_num=2"),
    (dict(key_build="host"), r"cross=.*key_build=host"),
    (dict(parity="reference_order"), r"cross=.*parity=reference_order"),
    (dict(ingest="gpu"), r"cross=.*ingest=gpu:.*ingest=gpu_fields"),
    (dict(cross="2*3,3x4"), r"xf_cross_parse: '3x4'"),
    (dict(model=1, fm_mode="field_aware", fields=18, cross_fgid_base=17),
     r"cross_fgid_base=17 with 2 pairs needs fields >= 19, not fields=18"),
]


@pytest.mark.parametrize("params,msg", REFUSALS, ids=[
    "core_num", "key_build", "parity", "ingest", "malformed", "fields"])
def test_refusals_by_name_in_and_outside_training(data, tmp_path, params, msg):
    p = dict(cross=WSPEC)
    p.update(params)
    with pytest.raises(capi.XFError, match=msg):
        capi.XFlow(str(data / "train"), str(data / "test"), **p).train()
    # XFLoadModel builds the tables without XFStartTrain's checks in front: the same refusal
    with pytest.raises(capi.XFError, match=msg):
        capi.XFlow(str(data / "train"), str(data / "test"), **p).load(str(tmp_path / "no_model"))


def test_cross_cannot_change_once_the_stage_exists(data):
    x, _ = run_worker(data, "host", "change", False, False)
    for name, value in (("cross", "4*5"), ("cross_fgid_base", 3)):
        with pytest.raises(capi.XFError, match=r"XFSetParam: %s cannot change" % name):
            x.set(name, value)
