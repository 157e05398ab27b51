"""A row slice of a block through the host-array front ends of the device key build.

Every front end (xf_batch_compile_gpu / _valued_gpu / _fielded_gpu / _fm / _local, and
xf_sharded_compile* above them) takes the reader's block arrays and a slice [row_begin, row_end):
it rebases the 64-bit row offsets to 32-bit slice-relative ones and uploads the slice.  Here a
slice passed as (block arrays, row_begin, row_end) must give what the same rows give as arrays of
their own with row_begin = 0 — bit for bit: the compiled minibatch, and the tables and predictions
after stepping it.  One block of 40 rows (0 .. 9 nonzeros a row, rows without nonzeros at both
edges of a slice, keys that repeat inside and across slices, values exact in fp32); the slices are
the whole block, one with a base, the last row, and one without rows."""
import ctypes as C
import functools
import os
import traceback

import numpy as np
import pytest

from tests import _sharded_modes_checker as M
from xflow_amd import capi

from .test_gpu_sharded_modes import _spawn
from .test_gpu_values import same
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu

SLICES = [(0, 40), (7, 29), (39, 40), (5, 5)]
FIELDS = 5


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()


@functools.lru_cache(None)
def _block():
    rng = np.random.RandomState(1729)
    lens = rng.randint(0, 10, size=40)
    lens[[7, 20, 28]] = 0                # rows without nonzeros: first and last row of [7, 29)
    lens[[0, 39]] = np.maximum(lens[[0, 39]], 1)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(rowptr[-1])
    keys = capi.hash_decimal_ids(rng.randint(0, 300, size=n).astype(np.uint64))
    fgid = rng.randint(0, FIELDS, size=n).astype(np.int32)
    vals = np.array([0.25, 0.5, 1.0, 2.0], np.float32)[rng.randint(0, 4, size=n)]
    labels = rng.randint(0, 2, size=40).astype(np.int32)
    return rowptr, keys, fgid, vals, labels


def _own(b, e):
    """rows [b, e) of the block as arrays of their own"""
    rowptr, keys, fgid, vals, labels = _block()
    lo, hi = int(rowptr[b]), int(rowptr[e])
    return rowptr[b:e + 1] - rowptr[b], keys[lo:hi], fgid[lo:hi], vals[lo:hi], labels[b:e]


def test_the_block_is_the_one_described():
    rowptr, keys, fgid, vals, labels = _block()
    lens = np.diff(rowptr.astype(np.int64))
    assert lens.min() == 0 and lens.max() <= 9 and (lens == 0).sum() >= 2
    assert lens[7] == 0 and lens[28] == 0 and lens[39] > 0
    inside = keys[int(rowptr[7]):int(rowptr[29])]
    assert len(np.unique(inside)) < len(inside)                       # repeats inside a slice
    assert np.intersect1d(inside, keys[:int(rowptr[7])]).size         # ... and across slices


# ---------------------------------------------------------------- the compiled minibatch
def _batch(arrs, b, e, kind, on_gpu):
    rowptr, keys, fgid, vals, labels = arrs
    kw = {"plain": {}, "valued": dict(values=vals), "fielded": dict(fields=FIELDS, fgid=fgid),
          "fielded_valued": dict(fields=FIELDS, fgid=fgid, values=vals)}[kind]
    return capi.Batch(rowptr, keys, labels, b, e, on_gpu=on_gpu, **kw)


def _same_batch(a, b):
    assert (a.R, a.NNZ, a.U, a.H) == (b.R, b.NNZ, b.U, b.H)
    ha, hb = a.host(), b.host()
    for n in ha:
        same(ha[n], hb[n])
    for x, y in zip(a.values() + a.field_arrays(), b.values() + b.field_arrays()):
        same(x, y)
    same(a.tiles(), b.tiles())
    same(a.heavy_chunks(), b.heavy_chunks())


@pytest.mark.parametrize("kind", ["plain", "valued", "fielded", "fielded_valued"])
@pytest.mark.parametrize("b,e", SLICES)
def test_a_slice_of_the_block_is_the_minibatch_of_its_rows(b, e, kind):
    rowptr = _block()[0]
    sl = _batch(_block(), b, e, kind, True)
    assert (sl.R, sl.NNZ) == (e - b, int(rowptr[e] - rowptr[b]))
    _same_batch(sl, _batch(_own(b, e), 0, e - b, kind, True))
    # the host build of the same slice: every array (tests/test_gpu_parity.py's _same_batch, the
    # value arrays of tests/test_gpu_values.py, the field arrays of tests/test_gpu_ffm.py)
    _same_batch(sl, _batch(_block(), b, e, kind, False))
    own = _own(b, e)
    if "valued" in kind:
        same(sl.values()[0], own[3])
    if "fielded" in kind and sl.NNZ:
        same(sl.field_arrays()[0], own[2].astype(np.uint32))


# ---------------------------------------------------------------- LocalBatch, xf_batch_compile_fm
def _same_exports(ta, tb):
    for x, y in zip(ta.export(), tb.export()):
        same(x, y)


def test_local_batches_of_slices_step_like_those_of_their_rows():
    ta, tb = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 12), capi.Table(capi.OPT_FTRL, 1,
                                                                         capacity=1 << 12)
    wa, wb = capi.Workspace(), capi.Workspace()
    for b, e in SLICES:
        rowptr, keys, _, _, labels = _block()
        orp, okeys, _, _, olab = _own(b, e)
        ba = capi.LocalBatch(ta, rowptr, keys, labels, b, e)
        bb = capi.LocalBatch(tb, orp, okeys, olab)
        assert (ba.R, ba.NNZ) == (bb.R, bb.NNZ) == (e - b, len(okeys))
        capi.lr_step(ta, ba, wa)
        capi.lr_step(tb, bb, wb)
        _same_exports(ta, tb)
        same(capi.lr_predict(ta, ba, wa), capi.lr_predict(tb, bb, wb))
    assert len(ta) == len(np.unique(_block()[1]))


def _fm_batch(tw, tv, rowptr, keys, labels, b, e):
    """xf_batch_compile_fm through the library: (the minibatch, *keyed)"""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if len(labels) == 0:
        labels = np.zeros(1, np.int32)
    bt = capi.Batch.__new__(capi.Batch)
    bt.h = capi.vp()
    bt.valued, bt.fields, bt.on_gpu = False, 0, True
    keyed = C.c_int(-1)
    capi.check(capi.lib().xf_batch_compile_fm(C.byref(bt.h), tw.h, tv.h, rowptr.ctypes.data,
                                              keys.ctypes.data, labels.ctypes.data, b, e, None,
                                              C.byref(keyed)))
    R, N, U, H = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    capi.check(capi.lib().xf_batch_dims(bt.h, C.byref(R), C.byref(N), C.byref(U), C.byref(H)))
    bt.R, bt.NNZ, bt.U, bt.H = R.value, N.value, U.value, H.value
    return bt, keyed.value


def test_fm_batches_of_slices_step_like_those_of_their_rows():
    k = 4
    pairs = []
    for _ in range(2):
        tw = capi.Table(capi.OPT_FTRL, 1, capacity=1 << 12)
        tv = capi.Table(capi.OPT_FTRL, k, capi.INIT_HASHNORM, 0.001, seed=7, capacity=1 << 12)
        for t in (tw, tv):                     # every key settled: the keyed build runs
            t.pull(np.unique(_block()[1]))
            t.defrag()
        pairs.append((tw, tv, capi.Workspace()))
    (wa, va, sa), (wb, vb, sb) = pairs
    seen = set()
    for b, e in SLICES:
        rowptr, keys, _, _, labels = _block()
        orp, okeys, _, _, olab = _own(b, e)
        ba, keyed_a = _fm_batch(wa, va, rowptr, keys, labels, b, e)
        bb, keyed_b = _fm_batch(wb, vb, orp, okeys, olab, 0, e - b)
        assert keyed_a == keyed_b and keyed_a in (0, 1)
        seen.add(keyed_a)
        assert (ba.R, ba.NNZ, ba.U) == (bb.R, bb.NNZ, bb.U) == (e - b, len(okeys),
                                                               len(np.unique(okeys)))
        capi.fm_step(wa, va, ba, sa)
        capi.fm_step(wb, vb, bb, sb)
        _same_exports(wa, wb)
        _same_exports(va, vb)
        same(capi.fm_predict(wa, va, ba, sa), capi.fm_predict(wb, vb, bb, sb))
    assert 1 in seen, "no slice took the keyed build"


# ---------------------------------------------------------------- the sharded trainer, one rank
_TRAINERS = {
    "lr": dict(model="lr"),
    "lr_host_keys": dict(model="lr", host_key_build=True),
    "fm": dict(model="fm", k=4),
    "canonical": dict(model="fm", k=4, fm_mode="canonical"),
    "field_aware": dict(model="fm", k=4, fm_mode="field_aware", fields=FIELDS),
}


def _sharded_compile(st, arrs, b, e, kind):
    rowptr, keys, fgid, vals, labels = arrs
    return st.compile(rowptr, keys, labels, b, e, values=vals if "valued" in kind else None,
                      fgid=fgid if "fielded" in kind else None)


def _step_slices(st, kind, own, slices=SLICES):
    """every slice in turn through one trainer: -> its predictions and its tables"""
    out = {}
    for i, (b, e) in enumerate(slices):
        mb = _sharded_compile(st, _own(b, e), 0, e - b, kind) if own else \
            _sharded_compile(st, _block(), b, e, kind)
        assert mb.R == e - b
        st.step(mb)
        st.check()
        out["pctr%d" % i] = st.predict(mb)
    st.check()
    for nm, t in (("w", st.w), ("v", st.v)):
        if t is not None:
            for f, a in zip("kwnz", t.export()):
                out[nm + "_" + f] = a
    return out


@pytest.mark.parametrize("trainer,kind", [
    ("lr", "plain"), ("lr_host_keys", "plain"), ("lr", "valued"), ("fm", "plain"),
    ("canonical", "plain"), ("canonical", "valued"), ("field_aware", "fielded"),
    ("field_aware", "fielded_valued")])
def test_one_rank_trainers_step_slices_like_their_rows(trainer, kind):
    outs = []
    for own in (False, True):
        st = capi.Sharded(None, capacity=1 << 12, seed=7, **_TRAINERS[trainer])
        outs.append(_step_slices(st, kind, own))
        st.close()
    assert sorted(outs[0]) == sorted(outs[1]) and len(outs[0]["w_k"]) == len(np.unique(_block()[1]))
    for f in outs[0]:
        same(outs[0][f], outs[1][f])


# ---------------------------------------------------------------- two ranks, schedule sequential
_TWO = [("lr", "plain"), ("field_aware", "fielded")]
_RANK_SLICE = [(7, 29), (5, 5)]          # rank 1 compiles a slice without rows


def _two_rank(rank, port, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(rank, 2, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        for trainer, kind in _TWO:
            st = capi.Sharded(g, capacity=1 << 12, seed=7, schedule="sequential",
                              **_TRAINERS[trainer])
            out = _step_slices(st, kind, False, [_RANK_SLICE[rank]])
            np.savez(os.path.join(outdir, "%s_rank%d.npz" % (trainer, rank)), **out)
            g.barrier()
            st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_two_ranks_one_without_rows_equal_the_one_rank_trainer(tmp_path):
    """rank 0 steps the slice [7, 29) of the block, rank 1 the slice [5, 5): the two shards are
    the one-rank trainer's table and rank 0's predictions its predictions, bit for bit as in
    tests/test_gpu_sharded_modes.py (test_a_rank_without_rows)"""
    port = free_port()
    _spawn(_two_rank, [(r, port, str(tmp_path)) for r in range(2)])
    for trainer, kind in _TWO:
        st = capi.Sharded(None, capacity=1 << 12, seed=7, **_TRAINERS[trainer])
        one = _step_slices(st, kind, False, [_RANK_SLICE[0]])
        st.close()
        parts = [np.load(str(tmp_path / ("%s_rank%d.npz" % (trainer, r)))) for r in range(2)]
        same(parts[0]["pctr0"], one["pctr0"])
        assert len(parts[1]["pctr0"]) == 0
        for nm in ("w", "v") if "v_k" in one else ("w",):
            for r, p in enumerate(parts):
                assert np.all(M.owner_of(p[nm + "_k"], 2) == r)
            order = np.argsort(np.concatenate([p[nm + "_k"] for p in parts]))
            ref = np.argsort(one[nm + "_k"])
            for f in "kwnz":
                got = np.concatenate([p[nm + "_" + f] for p in parts])[order]
                same(got, one[nm + "_" + f][ref].reshape(got.shape))

