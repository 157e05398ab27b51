"""Canonical FM, field-aware FM and feature values on SEVERAL ranks of the sharded trainer
(xf_sharded_*, schedules sequential and stale1), on real hardware.

The ranks are spawned processes that share one GPU, their exchanges staged through the group's
host transport, as in tests/test_gpu_sharded.py; at most three of them, the parent waits for each
with a timeout and fails on the first error, nothing is retried.  The reference is
tests/_sharded_modes_checker.py — the one-rank checkers' pieces in the order of N workers' Pulls
and Pushes — whose sums tests/test_sharded_modes_cpu.py shows to be exact on these very streams,
so every comparison is bit for bit: the ranks' shards (w, n, z of both tables) after three steps,
each rank's predictions of its held-out minibatch, and the ownership of every exported key."""
import ctypes as C
import multiprocessing as mp
import os
import re
import traceback

import numpy as np
import pytest

from tests import _sharded_modes_checker as M
from xflow_amd import capi

from .test_gpu_parity import same
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
_TIMEOUT = 150      # seconds the parent waits for a rank's report


# ---------------------------------------------------------------- what a rank does
def _trainer(g, spec, schedule=None, capacity=1 << 15, **hyper):
    mode, world, F, k, opt, sched, case, valued = spec
    kw = {"canonical": dict(fm_mode="canonical"),
          "field_aware": dict(fm_mode="field_aware", fields=F), "lr": {}}[mode]
    return capi.Sharded(g, model="lr" if mode == "lr" else "fm", optimizer=opt, k=k or 10,
                        capacity=capacity, schedule=schedule or sched, seed=7, **kw, **hyper)


def _import_old(st, spec, strs, rank, world):
    """the old state of every key of every rank's minibatches; this rank imports what it owns"""
    mode, _, F, k, opt, _, _, _ = spec
    keys = M.all_keys(strs)
    mine = M.owner_of(keys, world) == rank
    for t, state in zip((st.w, st.v), M.old_tables(mode, opt, k, F, keys)):
        if state is not None:
            t.import_(*[None if a is None else a[mine] for a in state])


def _compile(st, spec, mb):
    mode, valued = spec[0], spec[7]
    rowptr, keys, fg, vals, labels = mb
    return st.compile(rowptr, keys, labels, values=vals if valued else None,
                      fgid=fg if mode == "field_aware" else None)


def _export(st, out):
    for nm, t in (("w", st.w), ("v", st.v)):
        if t is not None:
            k, w, n, z = t.export()
            out.update({nm + "_k": k, nm + "_w": w, nm + "_n": n, nm + "_z": z})


def _steps(st, spec, strs, rank, defrag):
    train, held = strs[rank]
    alive = []   # freeing a minibatch whose Push is still outstanding would flush it early
    for s, mb in enumerate(train):
        b = _compile(st, spec, mb)
        alive.append(b)
        assert b.U == len(np.unique(mb[1]))
        st.step(b)
        if defrag and s == 1:
            st.defrag()          # row renumbering between steps must not change a bit
    st.check()
    out = {"pctr": st.predict(_compile(st, spec, held))}
    st.check()
    _export(st, out)
    return out


def _rank(rank, world, port, transport, spec, outdir, empty_ranks, save, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        ndev = C.c_int(0)
        capi.check(capi.lib().xf_device_count(C.byref(ndev)))
        g = capi.Group(rank, world, "127.0.0.1", port, transport,
                       device=0 if transport == capi.TRANSPORT_HOST else rank % ndev.value)
        mode, _, F, k, opt, schedule, case, valued = spec
        strs = M.streams(mode, case, world, F, empty_ranks)
        st = _trainer(g, spec)
        _import_old(st, spec, strs, rank, world)
        out = _steps(st, spec, strs, rank, defrag=schedule == "sequential")
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
        if save:
            st.save(os.path.join(outdir, "ckpt"))
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


def _spawn(target, argsets):
    """one process per argument set; the parent waits for each report with a timeout and fails on
    the first error (the others are ended: a rank whose peer has failed waits in a collective)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=target, args=a + (q,)) for a in argsets]
    for p in ps:
        p.start()
    try:
        res = []
        for _ in ps:
            r = q.get(timeout=_TIMEOUT)     # (rank, None or what it found | a traceback)
            assert not isinstance(r[1], str), r[1]
            res.append(r)
        for p in ps:
            p.join(timeout=60)
        return res
    finally:
        for p in ps:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)


def _run(spec, outdir, transport=capi.TRANSPORT_HOST, world=None, empty_ranks=(), save=False):
    world = world or spec[1]
    port = free_port()

    _spawn(_rank, [(r, world, port, transport, spec, str(outdir), tuple(empty_ranks), save)
                   for r in range(world)])
    return [np.load(os.path.join(str(outdir), "rank%d.npz" % r)) for r in range(world)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check_tables(parts, world, ws, vs, opt):
    """the ranks' shards, concatenated and sorted by key, are the checker's stores; every
    exported key belongs to its rank"""
    for nm, store in (("w", ws), ("v", vs)):
        if store is None:
            continue
        ks, wv, ns, zs = store.export()
        for r, p in enumerate(parts):
            assert np.all(M.owner_of(p[nm + "_k"], world) == r)
        k = np.concatenate([p[nm + "_k"] for p in parts])
        order = np.argsort(k)
        same(k[order], ks)
        for f, ref in (("_w", wv), ("_n", ns), ("_z", zs))[:3 if opt == "ftrl" else 1]:
            same(np.concatenate([p[nm + f] for p in parts])[order].reshape(ref.shape), ref)


# ---------------------------------------------------------------- 1. steps against the checker
@pytest.mark.parametrize("spec", M.CASES, ids=M.case_id)
def test_ranks_share_one_gpu_against_the_checker(tmp_path, spec):
    mode, world, F, k, opt, schedule, case, valued = spec
    ws, vs, pctr, log, strs, audit = M.run_case(spec)
    M.V.assert_exact(audit)
    parts = _run(spec, tmp_path)
    _check_tables(parts, world, ws, vs, opt)
    for r in range(world):
        same(parts[r]["pctr"], np.asarray(pctr[r], np.float32))
    if mode == "field_aware":
        # the (key, field) coordinates no rank touched hold the imported state, bit for bit
        keys = np.concatenate([p["v_k"] for p in parts])
        order = np.argsort(keys)
        keys = keys[order]
        free = np.repeat(M.never_touched(log, keys, F), k, axis=1)
        assert free.any()
        old = M.old_tables(mode, opt, k, F, keys)[1]
        for f, ref in (("v_w", old[1]), ("v_n", old[2]), ("v_z", old[3]))[:3 if opt == "ftrl" else 1]:
            got = np.concatenate([p[f] for p in parts])[order]
            assert np.array_equal(_bits(got)[free], _bits(ref)[free]), f


# ---------------------------------------------------------------- 2. general path = fused path
def _general_rank(port, spec, outdir, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        mode, _, F, k, opt, schedule, case, valued = spec
        strs = M.streams(mode, case, 1, F)
        for name, group in (("general", g), ("fused", None)):   # (no group: the fused step)
            st = _trainer(group, spec)
            _import_old(st, spec, strs, 0, 1)
            np.savez(os.path.join(outdir, name + ".npz"), **_steps(st, spec, strs, 0, defrag=True))
            st.close()
        g.close()
        q.put((0, None))
    except Exception:
        q.put((0, traceback.format_exc()))


@pytest.mark.parametrize("spec", M.GENERAL, ids=M.case_id)
def test_one_rank_on_the_exchange_path_is_the_fused_step(tmp_path, spec):
    """a group of one with XF_SHARDED_GENERAL=1 runs the exchange path with its self-copies — the
    emitting gradient kernels and the owner's (masked) push — and a plain one-rank trainer the
    fused step: the same three minibatches, the same tables and predictions"""
    _spawn(_general_rank, [(free_port(), spec, str(tmp_path))])
    a, b = np.load(str(tmp_path / "general.npz")), np.load(str(tmp_path / "fused.npz"))
    assert sorted(a.files) == sorted(b.files) and len(a["w_k"])
    for f in a.files:
        assert np.array_equal(_bits(a[f]), _bits(b[f])), f
    ws, vs, pctr, _, _, audit = M.run_case(spec)
    M.V.assert_exact(audit)
    _check_tables([a], 1, ws, vs, spec[4])
    same(a["pctr"], np.asarray(pctr[0], np.float32))


# ---------------------------------------------------------------- 3. a rank without rows
@pytest.mark.parametrize("spec,one", M.EMPTY_RANK, ids=[M.case_id(t) for t, _ in M.EMPTY_RANK])
def test_a_rank_without_rows(tmp_path, spec, one):
    """world 2, rank 1 compiles zero-row minibatches for every step and for predict: it serves
    rank 0's Pulls and Pushes, and the tables are the one-rank checker's (canonical valued, and
    the trainer's other two gradient branches: field-aware and valued LR)"""
    ws, vs, pctr, _, _, audit = M.run_case(one)
    M.V.assert_exact(audit)
    parts = _run(spec, tmp_path, empty_ranks=(1,))
    assert len(parts[1]["w_k"]) and len(parts[1]["pctr"]) == 0
    _check_tables(parts, 2, ws, vs, spec[4])
    same(parts[0]["pctr"], np.asarray(pctr[0], np.float32))


# ---------------------------------------------------------------- 4. checkpoint
def test_field_aware_checkpoint_saved_by_two_ranks_loaded_by_one(tmp_path):
    spec = M.CASES[6]
    assert spec[:4] == ("field_aware", 2, 3, 4)
    mode, world, F, k, opt, schedule, case, valued = spec
    ws, vs, pctr, _, strs, audit = M.run_case(spec)
    M.V.assert_exact(audit)
    _run(spec, tmp_path, save=True)
    one = _trainer(None, spec)
    one.load(str(tmp_path / "ckpt"))
    for got, ref in zip(one.v.export(), vs.export()):
        same(got, ref)
    for r in range(world):
        same(one.predict(_compile(one, spec, strs[r][1])), np.asarray(pctr[r], np.float32))


# ---------------------------------------------------------------- 5. refusals
def _owner_refusals(port, q):
    try:
        os.environ["XF_SHARDED_GENERAL"] = "1"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        g = capi.Group(0, 1, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        rowptr, keys, fg, vals, labels = M.rank_stream("field_aware", "ragged", 0, 3)[0][0]
        seen = []

        def refused(sched, what, call, st):
            try:
                call()
            except capi.XFError as e:
                assert re.search(r"schedule %s\b" % sched, str(e)) and "sequential" in str(e), str(e)
                for t in (st.w, st.v):
                    assert t is None or len(t.export()[0]) == 0
                seen.append((sched, what))
                return
            raise AssertionError("%s on schedule %s was not refused" % (what, sched))
        for sched in ("owner", "owner_stale1"):
            fm = capi.Sharded(g, model="fm", optimizer="ftrl", k=12, capacity=1 << 12,
                              schedule=sched, seed=7)
            refused(sched, "canonical", lambda: fm.set_fm_mode("canonical"), fm)
            capi.check(capi.lib().xf_sharded_set_fm_fields(fm.h, 3))
            refused(sched, "field_aware", lambda: fm.set_fm_mode("field_aware"), fm)
            refused(sched, "fielded minibatch",
                    lambda: fm.compile(rowptr, keys, labels, fgid=fg), fm)
            refused(sched, "valued FM minibatch",
                    lambda: fm.compile(rowptr, keys, labels, values=vals), fm)
            fm.close()
            lr = capi.Sharded(g, model="lr", optimizer="sgd", capacity=1 << 12, schedule=sched)
            refused(sched, "valued LR minibatch",
                    lambda: lr.compile(rowptr, keys, labels, values=vals), lr)
            lr.close()
        g.close()
        q.put((0, ("ok", seen)))
    except Exception:
        q.put((0, traceback.format_exc()))


def test_owner_schedules_refuse_the_modes_and_values():
    res = _spawn(_owner_refusals, [(free_port(),)])
    assert res[0][1][0] == "ok" and len(res[0][1][1]) == 10, res


def _bad_fgid_rank(rank, port, q):
    try:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ["XF_COLLECTIVE_TIMEOUT_S"] = "60"
        g = capi.Group(rank, 2, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        st = capi.Sharded(g, model="fm", optimizer="ftrl", k=4, capacity=1 << 12, seed=7,
                          fm_mode="field_aware", fields=3)
        rowptr, keys, fg, vals, labels = M.rank_stream("field_aware", "ragged", rank, 3)[0][0]
        fg = fg.copy()
        if rank == 1:
            fg[5] = 3            # outside [0, fields)
        msg = None
        try:
            st.compile(rowptr, keys, labels, values=vals, fgid=fg)
        except capi.XFError as e:
            msg = str(e)
        # ... and the ranks are still in step: a good minibatch compiles and steps on both
        good = M.rank_stream("field_aware", "ragged", rank, 3)[0][1]
        st.step(st.compile(good[0], good[1], good[4], values=good[3], fgid=good[2]))
        st.check()
        g.barrier()
        st.close()
        g.close()
        q.put((rank, ("refused", msg)))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_a_bad_fgid_on_one_rank_fails_the_compile_on_every_rank():
    port = free_port()
    res = dict(_spawn(_bad_fgid_rank, [(r, port) for r in range(2)]))
    assert res[0][0] == "refused" and res[1][0] == "refused"
    assert re.search(r"fgid 3.*fields = 3", res[1][1]), res[1][1]
    assert res[0][1] and re.search(r"rank 1 could not build", res[0][1]), res[0][1]


# ---------------------------------------------------------------- 6. RCCL
def test_canonical_valued_over_rccl(tmp_path):
    """one rank per GPU, the exchange over RCCL / xGMI"""
    n = C.c_int(0)
    capi.check(capi.lib().xf_device_count(C.byref(n)))
    if n.value < 2:
        pytest.skip("needs 2 GPUs, this box has %d" % n.value)
    spec = ("canonical", 2, 0, 16, "ftrl", "stale1", "zipf_chunks", True)
    ws, vs, pctr, _, _, audit = M.run_case(spec)
    M.V.assert_exact(audit)
    parts = _run(spec, tmp_path, transport=capi.TRANSPORT_RCCL)
    _check_tables(parts, 2, ws, vs, "ftrl")
    for r in range(2):
        same(parts[r]["pctr"], np.asarray(pctr[r], np.float32))
