"""The grouped AUC on the held-out rows (xf_gauc.hip, the validate tap, the worker's holdout_by=)
on a real MI355X, everything with == against the restatement (tests/_gauc_checker.py, pinned to a
plain pair count by tests/test_gauc_cpu.py): the reduction on crafted records aimed at its
workgroup and wavefront edges, the pack kernel, the tap of every validate path the holdout tests
cover (held to predict's own pctr), two ranks with a merged read, and the worker end to end."""
import math
import os
import re
import subprocess
import traceback

import numpy as np
import pytest

from xflow_amd import build, capi

from . import _ffm_checker as FF
from . import _gauc_checker as G
from . import _holdout_checker as H
from . import _progress_checker as P
from . import _sharded_modes_checker as M
from . import _valued_cases as Cs
from . import _zipf_text as Z
from . import test_gpu_fm_canonical as TC      # synth (the module, not its tests)
from . import test_gpu_progress as TP          # the step paths' tables (the module, not its tests)
from . import test_gpu_sharded_modes as SM     # _spawn, _trainer, _import_old
from .test_gpu_parity import synth
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(build.LIBDIR, "xflow_lr")
NONE = G.NONE
W = 64
eq = TP.eq
u64 = np.uint64


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


def want_of(ids, codes):
    return (G.figures if len(ids) <= 3000 else G.figures_fast)(ids, codes)


def check_entries(got, ids, codes, none=(0, 0), other=(0, 0), what=""):
    gid, fig, gnone, gother = got
    wid, wfig = want_of(ids, codes)
    eq(gid, wid, what + " ids")
    eq(fig, wfig, what + " figures")
    assert gnone.tolist() == list(none) and gother.tolist() == list(other), what
    # always: every row appended is somewhere
    assert int(fig[:, 0].sum() + fig[:, 1].sum()) == len(ids), what
    return fig


# ------------------------------------------------------------------ the reduction, crafted records
def _codes(rng, n, scores=40, p=0.3):
    return ((rng.integers(0, scores, size=n) << 1) | (rng.random(n) < p)).astype(np.uint32)


def _hashed(k):
    """distinct ids spread over the 64 bits, ascending in k only by accident"""
    return (np.arange(1, k + 1, dtype=u64) * u64(0x9E3779B97F4A7C15)) | u64(0)


def crafted():
    """[(name, ids, codes)]: the cases of the issue's list, in the order they go through ONE object"""
    B = capi.gauc_shape()["reduce_records"]
    rng = np.random.default_rng(17)
    out = [("one_record", np.array([5], u64), np.array([(7 << 1) | 1], np.uint32)),
           ("two_tied", np.array([5, 5], u64), np.array([(7 << 1) | 1, 7 << 1], np.uint32))]
    for n in (W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1):
        out.append(("one_group_%d" % n, np.full(n, 77, u64), _codes(rng, n)))
        out.append(("all_distinct_%d" % n, rng.permutation(_hashed(n)), _codes(rng, n)))
        # groups whose boundaries fall on, one before and one after every multiple of w and of B
        cuts = sorted({m * s + d for s in (W, B) for m in range(1, n // s + 2) for d in (-1, 0, 1)
                       if 0 < m * s + d < n})
        sizes = np.diff([0] + cuts + [n])
        gid = np.sort(_hashed(len(sizes)))         # (ascending: group k is the k-th in id order)
        ids = np.repeat(gid, sizes)
        perm = rng.permutation(n)
        out.append(("edge_groups_%d" % n, ids[perm], _codes(rng, n, scores=6)[perm]))
    # one group of about 5 B records: tie runs that straddle workgroup boundaries, one of them
    # covering a whole workgroup (records B - 10 .. 3 B + 10 are one score)
    runs = [B - 10, 2 * B + 20, 7, 1, W, B - 3, 5, B // 2 + 11]
    score = np.repeat(np.arange(len(runs)) * 3 + 1, runs)
    n = len(score)
    assert 4.5 * B < n < 5.5 * B and runs[0] < B and runs[0] + runs[1] > 3 * B
    perm = rng.permutation(n)
    out.append(("long_ties", np.full(n, 2 ** 63 + 5, u64),
                ((score << 1) | (rng.random(n) < 0.4)).astype(np.uint32)[perm]))
    n = B + 37
    out.append(("all_equal_scores", np.full(n, 9, u64),
                ((G.C << 1) | (rng.random(n) < 0.5)).astype(np.uint32)))
    ends = np.array([0, 1, (2 * G.C) << 1, G.CODE_MAX] * 25, np.uint32)
    out.append(("scores_0_and_2C", np.full(len(ends), 3, u64), rng.permutation(ends)))
    out.append(("positives_only", np.array([4] * 70 + [6] * 5, u64),
                (_codes(rng, 75) | np.uint32(1)).astype(np.uint32)))
    k = 123456789012345
    special = np.array([0, 1, 2 ** 63, 2 ** 64 - 2, k, k + 1], u64)
    ids = special[rng.integers(0, len(special), size=600)]
    out.append(("special_ids", ids, _codes(rng, 600, scores=5)))
    # beyond xf_sort_key_pos's in-LDS range: its merge path (Zipf ids: a hot head)
    n = 70000
    table = _hashed(2000)
    ids = table[np.minimum(rng.zipf(1.1, size=n), 2000) - 1]
    out.append(("zipf_70000", ids, _codes(rng, n, scores=2 * G.C + 1)))
    return out


@pytest.fixture(scope="module")
def obj():
    return capi.Gauc()


def test_no_records_no_launch(obj):
    gid, fig, none, other = obj.reduce(reset=True)
    assert len(gid) == 0 and fig.shape == (0, 4) and not none.any() and not other.any()
    assert obj.groups() == 0 and obj.count() == 0
    at = capi.gauc_launches()
    obj.append_dev(None, None, None, 0)              # R = 0: no launch
    obj.append([], [])
    assert capi.gauc_launches() == at and obj.count() == 0


def test_crafted_records_on_one_object(obj):
    B = capi.gauc_shape()["reduce_records"]
    for name, ids, codes in crafted():
        obj.append(ids, codes)
        assert obj.count() == len(ids), name
        fig = check_entries(obj.reduce(reset=True), ids, codes, what=name)
        assert obj.count() == 0, name
        if name == "all_equal_scores":
            assert len(fig) == 1 and int(fig[0, 2]) == int(fig[0, 0]) * int(fig[0, 1]) == int(fig[0, 3])
            assert fig[0, 0] > 0 and fig[0, 1] > 0
        if name == "positives_only":
            assert fig[:, 1:].tolist() == [[0, 0, 0], [0, 0, 0]] and fig[:, 0].tolist() == [70, 5]
        if name.startswith("all_distinct"):
            assert len(fig) == len(ids) and not fig[:, 2:].any()
        if name.startswith("edge_groups"):
            sizes = (fig[:, 0] + fig[:, 1]).astype(np.int64)
            ends = np.cumsum(sizes)
            for edge in (W, B):
                assert {c for c in (edge - 1, edge, edge + 1) if c < len(ids)} <= set(ends.tolist())
        if name == "long_ties":
            assert len(fig) == 1 and fig[0, 3] > B       # a tie mass no single workgroup holds
        if name == "special_ids":
            assert len(fig) == 6


def test_one_append_and_seven_shuffled_appends(obj):
    rng = np.random.default_rng(23)
    n = 5000
    ids = _hashed(300)[rng.integers(0, 300, size=n)]
    codes = _codes(rng, n)
    obj.append(ids, codes)
    one = obj.reduce(reset=True)
    perm = rng.permutation(n)
    for part in np.array_split(perm, 7):
        obj.append(ids[part], codes[part])
    seven = obj.reduce()
    for a, b in zip(one, seven):
        eq(a, b, "one append against seven")
    check_entries(seven, ids, codes)
    # reduce twice, then reset, then an empty reduce
    again = obj.reduce()
    for a, b in zip(seven, again):
        eq(a, b, "reduce twice")
    exported = obj.export()
    assert sorted(zip(exported[0].tolist(), exported[1].tolist())) == \
        sorted(zip(ids.tolist(), codes.tolist()))
    # an array too small: refused by name, the log intact
    groups = obj.groups()
    assert groups == len(one[0]) > 1
    with pytest.raises(capi.XFError, match=r"xf_gauc_reduce: %d groups do not fit an array of %d"
                       % (groups, groups - 1)):
        obj.reduce(reset=True, cap=groups - 1)
    assert obj.count() == n
    for a, b in zip(seven, obj.reduce(reset=True)):
        eq(a, b, "after the refusal")
    assert obj.count() == 0 and obj.groups() == 0 and len(obj.reduce()[0]) == 0
    n_ = capi.C.c_uint64()
    assert capi.lib().xf_gauc_reduce(obj.h, None, 0, capi.C.byref(n_), None, None, 1) != 0
    assert "cannot reset" in capi.lib().xf_last_error().decode()


def test_append_refuses_what_leaves_no_record(obj):
    with pytest.raises(capi.XFError, match="record 1 has the id XF_SLICE_NONE"):
        obj.append([3, NONE], [2, 2])
    with pytest.raises(capi.XFError, match="record 0 has code 4294967295"):
        obj.append([3], [G.OTHER])
    with pytest.raises(capi.XFError, match="record 2 has code %d" % (G.CODE_MAX + 1)):
        obj.append([3, 3, 3], [0, G.CODE_MAX, G.CODE_MAX + 1])
    assert obj.count() == 0
    with pytest.raises(capi.XFError, match="fewer than 2\\^30"):
        obj.reserve(2 ** 30)


# ------------------------------------------------------------------ the pack
def _edge_rows(rng, R):
    """losses that hit every branch: both classes' ordinary rows, NaN and q > 1 (other), ids from a
    small pool with NONE in it"""
    loss, labels = TP._random_losses(rng, R)
    labels[rng.random(R) < 0.05] = 7                         # a label other than 0 / 1
    special = np.array([np.nan, 1.5, -1.5, np.inf, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1e-45],
                       np.float32)
    at = rng.random(R) < 0.2
    loss[at] = special[rng.integers(0, len(special), size=int(at.sum()))]
    pool = np.array([11, 2 ** 64 - 2, NONE, 0, 12, NONE], u64)
    return loss.astype(np.float32), labels.astype(np.int32), pool[rng.integers(0, len(pool), size=R)]


def test_pack_every_branch_around_the_workgroup_rows():
    rows = capi.gauc_shape()["pack_rows"]
    g = capi.Gauc()
    rng = np.random.default_rng(31)
    all_ids, all_codes = [], []
    none, other = np.zeros(2, u64), np.zeros(2, u64)
    appended = 0
    for i, R in enumerate((1, W, rows - 1, rows, rows + 1, 2 * rows + 1)):
        loss, labels, ids = _edge_rows(rng, R)
        if i == 0:
            loss[0], ids[0] = 0.25, 11                       # (the single row leaves a record)
        ri, rc, rn, ro = G.records(loss, labels, ids)
        assert R < 100 or (rn.all() and ro.all() and len(ri) > 0)      # every branch, both classes
        tl, pl = _dev(loss, np.float32)
        tb, pb = _dev(labels, np.int32)
        ti, pi = _dev(ids, np.int64)
        at = capi.gauc_launches()
        if i == 3:
            g.reserve(appended + R)                          # sized ahead: the append waits for nothing
        g.append_dev(pl, pb, pi, R)
        assert capi.gauc_launches() == at + 1
        capi.stream_sync()
        all_ids.append(ri)
        all_codes.append(rc)
        none += rn
        other += ro
        appended += R
        want_ids, want_codes = np.concatenate(all_ids), np.concatenate(all_codes)
        gi, gc = g.export()                                  # the log grew and kept what it held
        assert sorted(zip(gi.tolist(), gc.tolist())) == sorted(zip(want_ids.tolist(), want_codes.tolist()))
        got = g.reduce()
        fig = check_entries(got, want_ids, want_codes, none.tolist(), other.tolist(), "R = %d" % R)
        assert int(fig[:, :2].sum()) + int(none.sum()) + int(other.sum()) == appended
    g.reduce(reset=True)
    got = g.reduce()
    assert len(got[0]) == 0 and not got[2].any() and not got[3].any()


# ------------------------------------------------------------------ the tap, one GPU
POOL = np.array([101, 202, 2 ** 64 - 2, 303, NONE, 0], u64)


def check_tap(ws, predict, validate, labels):
    """validate's records against the checker's, from predict's own pctr (every forward stores
    loss = pctr - (float)label in one fp32 subtraction)"""
    labels = np.asarray(labels, np.int32)
    R = len(labels)
    pctr = predict()
    assert len(np.unique(pctr)) > 1                          # (a trained model)
    loss = (pctr - labels.astype(np.float32)).astype(np.float32)
    rng = np.random.default_rng(R)
    g = capi.Gauc()
    ws.gauc(g)
    base = capi.Progress()
    ws.gauc(None)
    at = capi.gauc_launches()
    validate(base)                                           # nothing attached
    ws.gauc(g)
    validate(base)                                           # attached, no ids: appends nothing
    assert capi.gauc_launches() == at and g.count() == 0
    base_counts = base.read()
    assert (base_counts[0] % 2 == 0).all()
    for kind in ("pool", "single", "distinct"):
        ids = {"pool": POOL[rng.integers(0, len(POOL), size=R)],
               "single": np.full(R, 424242, u64),
               "distinct": _hashed(R)}[kind]
        t, ptr = _dev(ids, np.int64)
        p = capi.Progress()
        ws.gauc_ids(ptr, R)
        at, at_p = capi.gauc_launches(), capi.progress_launches()
        validate(p)
        assert capi.gauc_launches() == at + 1 and capi.progress_launches() == at_p + 1
        validate(p)                                          # the ids named ONE validate
        assert capi.gauc_launches() == at + 1
        counts = p.read()
        TP.same_counts((counts[0] // 2, counts[1] // 2), (base_counts[0] // 2, base_counts[1] // 2),
                       "the progress beside the grouped AUC")
        ri, rc, rn, ro = G.records(loss, labels, ids)
        got = g.reduce(reset=True)
        fig = check_entries(got, ri, rc, rn.tolist(), ro.tolist(), kind)
        m = capi.gauc_summary(got[0], got[1], got[2], got[3])[0]
        assert G.same(m, G.summary(got[0], got[1], got[2], got[3])[0])
        if kind == "pool":
            assert rn.any() and len(fig) == len(POOL) - 1
        if kind == "single":
            # one group of every row: its figures are those of the global AUC's counts
            half = (counts[0] // 2, counts[1] // 2)
            assert tuple(int(x) for x in fig[0]) == G.from_progress_counts(half[0])
            auc = capi.progress_summary(*half)["auc"]
            assert np.float64(m["gauc"]).view(u64) == np.float64(auc).view(u64) and 0 < auc < 1
            assert m["macro_auc"] == auc
        if kind == "distinct":
            assert m["groups"] == R and m["groups_scored"] == 0 and math.isnan(m["gauc"])
    eq(predict(), pctr, "predict after the validates")
    assert capi.gauc_launches() == at + 1                    # predict never appends
    t, ptr = _dev(np.zeros(R + 1, u64), np.int64)
    ws.gauc_ids(ptr, R + 1)
    with pytest.raises(capi.XFError, match="a validate of %d rows with the group ids of %d rows"
                       % (R, R + 1)):
        validate(capi.Progress())
    ws.gauc(None)
    with pytest.raises(capi.XFError, match="xf_workspace_gauc_ids"):
        ws.gauc_ids(ptr, R)                                  # ids without an object


def _lr(t, ws, b, labels):
    check_tap(ws, lambda: capi.lr_predict(t, b, ws), lambda p: capi.lr_validate(t, b, ws, p), labels)


def _fm(tw, tv, ws, b, labels):
    check_tap(ws, lambda: capi.fm_predict(tw, tv, b, ws),
              lambda p: capi.fm_validate(tw, tv, b, ws, p), labels)


def test_tap_lr_cells_and_local():
    ws = capi.Workspace()
    (t,), _ = TP._run_lr_cells(ws)
    held = synth(np.random.RandomState(77), 1000, 40, 45000, None, True)
    _lr(t, ws, capi.Batch(*held), held[2])
    _lr(t, ws, capi.LocalBatch(t, *held), held[2])


@pytest.mark.parametrize("path", ["generic", "local"])
def test_tap_valued_lr(path):
    ws = capi.Workspace()
    (t,), _ = TP._run_valued(ws, path)
    rp, ks, vs, lb = Cs.stream("ragged", seed=50)[0]
    b = capi.LocalBatch(t, rp, ks, lb, values=vs) if path == "local" else \
        capi.Batch(rp, ks, lb, on_gpu=True, values=vs)
    _lr(t, ws, b, lb)


def test_tap_canonical_fm():
    ws = capi.Workspace()
    (tw, tv), _ = TP._run_canonical(ws)
    held = TC.synth(np.random.RandomState(79), 300, 20, 6000, None)
    _fm(tw, tv, ws, capi.Batch(*held, on_gpu=True), held[2])


def test_tap_field_aware_fm():
    ws = capi.Workspace()
    (tw, tv), _ = TP._run_ffm(ws)
    Fd = 18
    rp, ks, fg, vs, lb = FF.stream("ragged", Fd)[-1]
    _fm(tw, tv, ws, capi.Batch(rp, ks, lb, on_gpu=True, values=vs, fields=Fd, fgid=fg), lb)


def test_trainer_one_rank_and_off_is_the_parent():
    """xf_sharded_gauc on the fused path: validate appends for minibatches that carry ids; with it
    off no pack is launched and the holdout's counts are what they were"""
    import torch
    raws = TP._lr_raws()
    held = synth(np.random.RandomState(77), 1000, 40, 45000, None, True)
    R = len(held[2])
    st = capi.Sharded(model="lr", capacity=1 << 17)
    with pytest.raises(capi.XFError, match="xf_sharded_gauc: the grouped AUC needs held-out"):
        st.set_gauc(True)
    st.set_gauc(False)                                       # (off is the default: accepted)
    st.set_holdout(True)
    with pytest.raises(capi.XFError, match="grouped AUC of the held rows is off"):
        st.gauc_read()
    hb, hb_plain = st.compile(*held), st.compile(*held)
    ids = POOL[np.random.default_rng(5).integers(0, len(POOL), size=R)]
    t = torch.from_numpy(ids.view(np.int64)).cuda()
    torch.cuda.synchronize()
    st.batch_slices(hb, t.data_ptr(), R)
    st.flush()
    del t
    for raw in raws:
        st.step(st.compile(*raw))
    pctr = st.predict(hb)
    at = capi.gauc_launches()
    st.validate(hb)                                          # off: no pack, ids or not
    off = st.holdout_read(reset=True)
    assert capi.gauc_launches() == at
    st.set_gauc(True)
    st.validate(hb)
    st.validate(hb_plain)                                    # no ids: appends nothing
    assert capi.gauc_launches() == at + 1
    on = st.holdout_read(reset=True)
    TP.same_counts((on[0] // 2, on[1] // 2), off, "the holdout's counts beside the grouped AUC")
    loss = (pctr - held[2].astype(np.float32)).astype(np.float32)
    ri, rc, rn, ro = G.records(loss, held[2], ids)
    check_entries(st.gauc_read(), ri, rc, rn.tolist(), ro.tolist(), "own")
    check_entries(st.gauc_read(reset=True, merged=True), ri, rc, rn.tolist(), ro.tolist(), "merged")
    assert len(st.gauc_read()[0]) == 0
    with pytest.raises(capi.XFError, match="xf_sharded_holdout: the grouped AUC"):
        st.set_holdout(False)
    st.set_gauc(False)
    st.set_holdout(False)
    eq(st.predict(hb), pctr)
    st.close()


# ------------------------------------------------------------------ the tap, two ranks
TWO = (("lr", 2, 0, 0, "ftrl", "sequential", "ragged", False),
       ("lr", 2, 0, 0, "ftrl", "stale1", "ragged", False))
POOL2 = np.array([7, 8, 9, NONE, 2 ** 64 - 2, 10, 11], u64)


def _gauc_rank(rank, world, port, spec, outdir, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        mode, _, F, k, opt, schedule, case, valued = spec
        strs = M.streams(mode, case, world, F)
        st = SM._trainer(g, spec)
        st.set_holdout(True)
        st.set_gauc(True)
        SM._import_old(st, spec, strs, rank, world)
        train, held = strs[rank]
        alive = []
        for mb in train:
            b = st.compile(mb[0], mb[1], mb[4])
            alive.append(b)
            st.step(b)
        hb = st.compile(held[0], held[1], held[4])
        R = len(held[4])
        pool = POOL2[:5 + rank]                              # (id 10 is rank 1's alone)
        ids = pool[np.random.default_rng(100 + rank).integers(0, len(pool), size=R)]
        t = torch.from_numpy(ids.view(np.int64)).cuda()
        torch.cuda.synchronize()
        st.batch_slices(hb, t.data_ptr(), R)
        st.flush()
        del t
        pctr = st.predict(hb)
        at = capi.gauc_launches()
        st.validate(hb)
        launches = capi.gauc_launches() - at
        own = st.gauc_read()
        mer = st.gauc_read(reset=True, merged=True)
        left = st.gauc_read()
        st.check()
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), own_i=own[0], own_f=own[1],
                 own_n=own[2], own_o=own[3], mer_i=mer[0], mer_f=mer[1], mer_n=mer[2], mer_o=mer[3],
                 left=np.array([len(left[0]) + int(left[2].sum()) + int(left[3].sum())]),
                 pctr=pctr, labels=np.asarray(held[4], np.int32), ids=ids,
                 launches=np.array([launches]), again=st.predict(hb))
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
    SM._spawn(_gauc_rank, [(r, world, port, spec, str(tmp_path)) for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    recs = []
    for r in range(world):
        p = parts[r]
        loss = (p["pctr"] - p["labels"].astype(np.float32)).astype(np.float32)
        ri, rc, rn, ro = G.records(loss, p["labels"], p["ids"])
        recs.append((ri, rc, rn, ro))
        check_entries((p["own_i"], p["own_f"], p["own_n"], p["own_o"]), ri, rc, rn.tolist(),
                      ro.tolist(), "rank %d's own" % r)
        assert p["left"][0] == 0 and p["launches"][0] == 1 and len(p["labels"]) > 0
        eq(p["again"], p["pctr"])
    # the merged read: both ranks' records reduced on rank 0 — the figures of a group whose rows
    # are spread over the ranks are not the sum of the parts'
    all_i = np.concatenate([r[0] for r in recs])
    all_c = np.concatenate([r[1] for r in recs])
    p = parts[0]
    check_entries((p["mer_i"], p["mer_f"], p["mer_n"], p["mer_o"]), all_i, all_c,
                  (recs[0][2] + recs[1][2]).tolist(), (recs[0][3] + recs[1][3]).tolist(), "merged")
    assert 10 in p["mer_i"] and 10 not in p["own_i"]
    shared = np.intersect1d(parts[0]["own_i"], parts[1]["own_i"])
    assert len(shared) >= 3
    p = parts[1]
    assert len(p["mer_i"]) == 0 and not p["mer_n"].any() and not p["mer_o"].any()


def _owner_refusal(port, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"       # a group of one on the exchange path
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        seen = []
        for sched in ("owner", "owner_stale1"):
            st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule=sched)
            st.set_gauc(False)                       # (off is the default: accepted)
            try:
                st.set_gauc(True)
            except capi.XFError as e:
                assert re.search(r"xf_sharded_gauc.*schedule %s\b" % sched, str(e)) \
                    and "sequential" in str(e), str(e)
                seen.append(sched)
            st.close()
        st = capi.Sharded(g, model="lr", optimizer="ftrl", capacity=1 << 12, schedule="stale1")
        try:
            st.set_gauc(True)                        # the holdout is off
        except capi.XFError as e:
            assert "xf_sharded_holdout" in str(e), str(e)
            seen.append("needs holdout")
        st.set_holdout(True)
        st.set_gauc(True)
        try:
            st.set_schedule("owner")
        except capi.XFError as e:
            assert "xf_sharded_set_schedule" in str(e), str(e)
            seen.append("then owner")
        try:
            st.set_holdout(False)
        except capi.XFError as e:
            assert "xf_sharded_gauc" in str(e), str(e)
            seen.append("holdout off under it")
        try:
            capi.Sharded(g, model="lr", capacity=1 << 12).gauc_read()
        except capi.XFError as e:
            assert "is off" in str(e), str(e)
            seen.append("read while off")
        st.close()
        g.close()
        q.put((0, ("ok", seen)))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_owner_schedules_refuse_the_grouped_auc():
    res = SM._spawn(_owner_refusal, [(free_port(),)])
    assert res[0][1] == ("ok", ["owner", "owner_stale1", "needs holdout", "then owner",
                                "holdout off under it", "read while off"]), res


# ------------------------------------------------------------------ the worker end to end
from . import _admit_checker as A              # noqa: E402
from . import _cross_checker as X              # noqa: E402
from . import _slices_checker as S             # noqa: E402

EPOCHS = 2
SHARE = 0.25
FIELD = 3
ADMIT = dict(admit_count=2, admit_log2_slots=14, admit_hashes=3)
CROSS = "2*3"
VARIANTS = {
    "plain": {},
    "neg_keep": dict(neg_keep=0.5),
    "admit": dict(ADMIT),
    "cross": dict(cross=CROSS),
    "nocache": dict(cache_batches=0),
}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """train-00000: generated click text of a few thousand rows (one block); held-00000: its held
    rows under the worker's seed, written by the holdout checker — also the test file"""
    d = tmp_path_factory.mktemp("gauc")
    with open(str(d / "train-00000"), "wb") as f:
        f.write(Z.zipf_text(41, 250000, positives=0.2))
    m = H.write_split(str(d / "train-00000"), str(d / "kept-00000"), str(d / "held-00000"), 0, 0,
                      SHARE)
    os.replace(str(d / "held-00000"), str(d / "test-00000"))
    blocks = list(capi.read_blocks(str(d / "train-00000"), 2 << 20))
    assert len(blocks) == 1 and len(blocks[0][3]) == len(m) > 2000
    assert 400 < int(m.sum()) < len(m) // 2
    return d


def run(data, tag, **params):
    pred = str(data / ("pred_%s.txt" % tag))
    x = capi.XFlow(str(data / "train"), str(data / "test"), capacity=1 << 15, pred_path=pred,
                   **params)
    x.train()
    return x, pred


def table_of(x):
    t = capi.Table.from_handle(x.tables()[0], 1, capi.OPT_FTRL)
    keys, w, n, z = t.export()[:4]
    return {int(k): (np.float32(a).tobytes(), np.float32(b).tobytes(), np.float32(c).tobytes())
            for k, a, b, c in zip(keys, w, n, z)}


def held_rows(data, variant, train="kept-00000", test="test-00000"):
    """the held rows: their labels, their group ids (named BEFORE the cross and admission) and
    the arrays validate scores — crossed, then filtered by the admission filter that has counted the
    (crossed) train part once: the restatements"""
    (rp, keys, fg, labels), = list(capi.read_blocks(str(data / test), 2 << 20))
    (trp, tkeys, tfg, _), = list(capi.read_blocks(str(data / train), 2 << 20))
    rp, trp = rp.astype(np.uint64), trp.astype(np.uint64)
    ids = S.ids_of(rp, keys, fg, FIELD)
    if variant == "cross":
        rp, keys, fg, _ = X.Cross(CROSS).apply(rp, keys, fg)
    if variant == "admit":
        flt = A.Filter(ADMIT["admit_log2_slots"], ADMIT["admit_count"], ADMIT["admit_hashes"], 0)
        flt.filter(trp, tkeys, update=True)
        rp, keys, _, _ = flt.filter(rp, keys, update=False)
    return rp.astype(np.uint64), keys, np.asarray(labels, np.int32), np.asarray(ids, u64)


def line_of(e, m):
    s = ("holdout groups epoch %d: field = %d groups = %d scored = %d rows = %d scored_rows = %d "
         "none_rows = %d gauc = %.6f (+- %.1e) macro_auc = %.6f"
         % (e, FIELD, m["groups"], m["groups_scored"], m["rows"], m["rows_scored"], m["none_rows"],
            m["gauc"], m["gauc_slack"], m["macro_auc"]))
    return s + (" other_rows = %d" % m["other_rows"] if m["other_rows"] else "")


def strip(out):
    return [ln for ln in out.split("\n")
            if not ln.startswith("examples/sec") and not ln.startswith("holdout groups epoch ")]


_refs = {}


def reference(data, variant, capfd, ingest="host"):
    """per epoch count e = 1 .. EPOCHS: a plain holdout run (no holdout_by) with the variant's
    parameters; its table scores the held rows -> predict's own pctr -> the checker's records,
    figures and summary that a holdout_by run must report after that epoch; and the last run's
    output, table and predictions"""
    if (variant, ingest) not in _refs:
        rp, keys, labels, ids = held_rows(data, variant)
        out = []
        for e in range(1, EPOCHS + 1):
            capfd.readouterr()
            x, pred = run(data, "%s_%s_ref%d" % (variant, ingest, e), epochs=e, holdout=SHARE,
                          ingest=ingest, **VARIANTS[variant])
            printed = capfd.readouterr().out
            t = capi.Table.from_handle(x.tables()[0], 1, capi.OPT_FTRL)
            pctr = capi.lr_predict(t, capi.Batch(rp, keys, labels), capi.Workspace())
            loss = (pctr - labels.astype(np.float32)).astype(np.float32)
            ri, rc, rn, ro = G.records(loss, labels, ids)
            gid, fig = G.figures_fast(ri, rc)
            m, auc, slack = G.summary(gid, fig, rn, ro)
            assert m["rows"] + m["none_rows"] + m["other_rows"] == len(labels)
            out.append(dict(m=m, gid=gid, fig=fig, auc=auc, slack=slack, printed=printed,
                            table=table_of(x), pred=open(pred, "rb").read(),
                            holdout_auc=x.metric("holdout_auc"),
                            logloss=x.metric("holdout_logloss")))
        m = out[-1]["m"]
        assert m["groups"] > 50 and m["groups_scored"] > 10 and m["none_rows"] > 0
        assert m["rows_one_class"] > 0 and 0.0 < m["gauc"] < 1.0
        _refs[(variant, ingest)] = out
    return _refs[(variant, ingest)]


def read_tsv(path):
    """{epoch: [(key, P, N, auc, slack)]} in file order"""
    out = {}
    for ln in open(path).read().strip().split("\n"):
        f = ln.split("\t")
        assert len(f) == 6, ln
        out.setdefault(int(f[0]), []).append((int(f[1], 16), int(f[2]), int(f[3]), float(f[4]),
                                              float(f[5])))
    return out


def check_run(x, pred, printed, tsv_path, ref):
    lines = [ln for ln in printed.split("\n") if ln.startswith("holdout groups epoch ")]
    assert lines == [line_of(e, ref[e]["m"]) for e in range(EPOCHS)], (lines, printed)
    all_lines = printed.split("\n")
    for e in range(EPOCHS):                                  # right after the holdout line
        at = all_lines.index(lines[e])
        assert all_lines[at - 1].startswith("holdout epoch %d: " % e)
    last = ref[-1]
    for name, key in (("holdout_gauc", "gauc"), ("holdout_gauc_slack", "gauc_slack"),
                      ("holdout_macro_auc", "macro_auc")):
        assert np.float64(x.metric(name)).view(u64) == np.float64(last["m"][key]).view(u64), name
    assert x.metric("holdout_groups") == last["m"]["groups"]
    assert x.metric("holdout_groups_scored") == last["m"]["groups_scored"]
    assert x.metric("holdout_gauc_rows") == last["m"]["rows_scored"]
    tsv = read_tsv(tsv_path)
    assert sorted(tsv) == list(range(EPOCHS))
    for e in range(EPOCHS):
        r = ref[e]
        assert [t[0] for t in tsv[e]] == r["gid"].tolist(), "one line a group, by key"
        assert [[t[1], t[2]] for t in tsv[e]] == r["fig"][:, :2].tolist()
        assert G.same_bits([t[3] for t in tsv[e]], r["auc"])
        assert G.same_bits([t[4] for t in tsv[e]], r["slack"])
    # everything else is the run without holdout_by: the other lines, the table, the predictions,
    # the holdout's own figures (the early-stop rule's input)
    assert strip(printed) == strip(last["printed"])
    assert table_of(x) == last["table"] and open(pred, "rb").read() == last["pred"]
    assert x.metric("holdout_auc") == last["holdout_auc"]
    assert x.metric("holdout_logloss") == last["logloss"]


@pytest.mark.parametrize("ingest", ["host", "gpu_fields"])
def test_worker_both_ingest_paths(data, capfd, ingest):
    ref = reference(data, "plain", capfd, ingest)
    tsv = str(data / ("groups_plain_%s.tsv" % ingest))
    capfd.readouterr()
    x, pred = run(data, "plain_%s" % ingest, epochs=EPOCHS, holdout=SHARE, holdout_by=FIELD,
                  holdout_groups_out=tsv, ingest=ingest)
    printed = capfd.readouterr().out
    assert x.metric("blocks_gpu") == (0 if ingest == "host" else 1)
    check_run(x, pred, printed, tsv, ref)


@pytest.mark.parametrize("variant", ["neg_keep", "admit", "cross", "nocache"])
def test_worker_with_the_other_stages(data, capfd, variant):
    ref = reference(data, variant, capfd)
    tsv = str(data / ("groups_%s.tsv" % variant))
    capfd.readouterr()
    x, pred = run(data, variant, epochs=EPOCHS, holdout=SHARE, holdout_by=FIELD,
                  holdout_groups_out=tsv, **VARIANTS[variant])
    check_run(x, pred, capfd.readouterr().out, tsv, ref)


def test_worker_off_creates_nothing(data, capfd):
    at = capi.gauc_launches()
    x, pred = run(data, "off", epochs=1, holdout=SHARE)
    assert capi.gauc_launches() == at
    assert "holdout groups" not in capfd.readouterr().out
    with pytest.raises(capi.XFError, match="holdout_gauc: no epoch has been reduced"):
        x.metric("holdout_gauc")
    x, pred = run(data, "on1", epochs=1, holdout=SHARE, holdout_by=FIELD)
    assert capi.gauc_launches() == at + 1                    # one held minibatch, one epoch


REFUSALS = [
    (dict(holdout_by=FIELD), "holdout_by=3 without holdout"),
    (dict(holdout_by=-1, holdout=SHARE), "holdout_by must be a field id in 0 .. 2147483647, not -1"),
    (dict(holdout_by=2 ** 31, holdout=SHARE), "holdout_by must be a field id in 0 .. 2147483647, not 2147483648"),
    (dict(holdout_by=FIELD, holdout=SHARE, ingest="gpu"), "holdout_by=3 together with ingest=gpu"),
    (dict(holdout_by=FIELD, holdout=SHARE, core_num=2), "holdout_by=3 needs core_num=1"),
    (dict(holdout_by=FIELD, holdout=SHARE, key_build="host"), "holdout_by=3 together with key_build=host"),
]


@pytest.mark.parametrize("params,message", REFUSALS, ids=[m.split(",")[0][:40] for _, m in REFUSALS])
def test_worker_refusals(data, params, message):
    with pytest.raises(capi.XFError) as e:
        run(data, "refused", epochs=1, **params)
    assert "XFStartTrain: " + message in str(e.value), str(e.value)
    with pytest.raises(capi.XFError, match="holdout_by must be a field id, not 'site'"):
        capi.XFlow(str(data / "train"), str(data / "test"), holdout_by="site")


def test_worker_field_2_31_minus_1_is_taken(data, capfd):
    """the largest field id: no row carries it — every held row is counted with none"""
    x, pred = run(data, "bigfield", epochs=1, holdout=SHARE, holdout_by=2 ** 31 - 1)
    line, = [ln for ln in capfd.readouterr().out.split("\n") if ln.startswith("holdout groups epoch")]
    rows = len(held_rows(data, "plain")[2])
    assert line == ("holdout groups epoch 0: field = 2147483647 groups = 0 scored = 0 rows = 0 "
                    "scored_rows = 0 none_rows = %d gauc = nan (+- nan) macro_auc = nan" % rows)
    assert math.isnan(x.metric("holdout_gauc")) and x.metric("holdout_groups") == 0


# ---- two workers: scripts/local.sh 2 2 xflow_lr ... holdout=0.25 holdout_by=3
def _local_sh(cwd, train, test, epochs, *args):
    env = dict(os.environ, DMLC_PS_ROOT_PORT=str(free_port()))
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "local.sh"), "2", "2", CLI,
                          train, test, "0", str(epochs), "transport=host", "capacity=32768",
                          "model_out=" + os.path.join(cwd, "model"),
                          "pred_path=" + os.path.join(cwd, "pred.txt"), *args],
                         capture_output=True, text=True, timeout=240, env=env, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    one = capi.Sharded(None, model="lr", optimizer="ftrl", capacity=1 << 16)
    one.load(os.path.join(cwd, "model"))                   # two shard files -> one table
    return out.stdout.split("\n"), one


def test_local_sh_two_workers(tmp_path):
    """each rank names the held rows of its own file; rank 0 reduces both ranks' records: the
    figures of a plain holdout run's table on both ranks' held rows"""
    d = tmp_path / "data"
    d.mkdir()
    held = []
    for r in range(2):
        with open(str(d / ("train-%05d" % r)), "wb") as f:
            f.write(Z.zipf_text(50 + r, 80000, positives=0.2))
        H.write_split(str(d / ("train-%05d" % r)), str(d / ("kept-%05d" % r)),
                      str(d / ("held-%05d" % r)), 0, r, SHARE)
        (blk,) = list(capi.read_blocks(str(d / ("held-%05d" % r)), 2 << 20))
        held.append((blk[0].astype(np.uint64), blk[1], np.asarray(blk[3], np.int32),
                     np.asarray(S.ids_of(blk[0], blk[1], blk[2], FIELD), u64)))
        assert len(blk[3]) > 100
    with open(str(d / "test-00000"), "wb") as f:
        f.write(Z.zipf_text(60, 4000))
    want, plain = [], None
    for e in (1, 2):
        cwd = tmp_path / ("ref%d" % e)
        cwd.mkdir()
        plain, one = _local_sh(str(cwd), str(d / "train"), str(d / "test"), e, "holdout=%r" % SHARE)
        recs = []
        for rp, keys, labels, ids in held:
            pctr = one.predict(one.compile(rp, keys, labels))
            recs.append(G.records((pctr - labels.astype(np.float32)).astype(np.float32), labels, ids))
        gid, fig = G.figures_fast(np.concatenate([r[0] for r in recs]),
                                  np.concatenate([r[1] for r in recs]))
        m = G.summary(gid, fig, recs[0][2] + recs[1][2], recs[0][3] + recs[1][3])[0]
        want.append((line_of(e - 1, m), gid, fig))
        one.close()
    cwd = tmp_path / "run"
    cwd.mkdir()
    lines, one = _local_sh(str(cwd), str(d / "train"), str(d / "test"), 2, "holdout=%r" % SHARE,
                           "holdout_by=%d" % FIELD, "holdout_groups_out=" + str(cwd / "g.tsv"))
    one.close()
    assert [ln for ln in lines if ln.startswith("holdout groups epoch ")] == [w[0] for w in want]
    # rank 0 alone prints the new line; every other line is the plain run's (the two workers write
    # to one pipe at the same time, so the order of their lines among each other is not defined)
    assert sorted(strip("\n".join(lines))) == sorted(strip("\n".join(plain)))
    tsv = read_tsv(str(cwd / "g.tsv"))
    for e in (0, 1):
        assert [t[0] for t in tsv[e]] == want[e][1].tolist()
        assert [[t[1], t[2]] for t in tsv[e]] == want[e][2][:, :2].tolist()
    shared = np.intersect1d(held[0][3], held[1][3])
    assert len(shared) > 10                                  # groups whose rows lie on both ranks
