"""Canonical FM, field-aware FM and feature values on SEVERAL ranks of the sharded trainer on
inputs in general position (tests/_general_cases.py: full mantissas, signs mixed inside a row,
magnitudes over many binades, exact zeros, an underflow minibatch), from FRESH tables — w from
zero, v hash-normal, nothing imported — on real hardware.

The ranks are spawned processes that share one GPU over the host transport, under the parent-side
discipline of tests/test_gpu_sharded_modes.py (its _spawn, _trainer and _compile).  A rank dumps
its shard of both tables after st.check() at every judged point — after every step for
sequential, after every second step for stale1 — and its held-out predictions at the end.  The
parent judges afterwards with tests/_sharded_general_checker.py, adopting each dump before it
judges the next: the keys and their owners, every coordinate one admissible state bit for bit,
what no rank moved the bits of the table before, pctr one of its candidates, and the Judge's caps
(which tests/test_sharded_general_cpu.py asserts for the checker alone on every case here)."""
import os
import traceback

import numpy as np
import pytest

from tests import _interval as I
from tests import _sharded_general_checker as S
from xflow_amd import capi

from . import test_gpu_sharded_modes as T
from .test_group_cpu import free_port

pytestmark = pytest.mark.gpu
bits = S.bits


# ---------------------------------------------------------------- what a rank does
def _rank(rank, spec, port, outdir, empty_ranks, general, hyper, q):
    try:
        if general:
            os.environ["XF_SHARDED_GENERAL"] = "1"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        world, schedule = spec[1], spec[5]
        g = capi.Group(rank, world, "127.0.0.1", port, capi.TRANSPORT_HOST, device=0)
        st = T._trainer(g, spec, **hyper)
        train, held = S.streams(spec, empty_ranks)[rank]
        last = [p[-1] for p in S.points(schedule, len(train))]
        out, alive = {}, []     # (a freed minibatch would flush its outstanding Push early)
        for s, mb in enumerate(train):
            b = T._compile(st, spec, mb)
            alive.append(b)
            st.step(b)
            if s in last:
                st.check()
                for nm, t in (("w", st.w), ("v", st.v)):
                    if t is not None:
                        for f, a in zip("kwnz", t.export()):
                            out["p%d_%s_%s" % (last.index(s), nm, f)] = a
        out["pctr"] = st.predict(T._compile(st, spec, held))
        st.check()
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
        g.barrier()
        st.close()
        g.close()
        q.put((rank, None))
    except Exception:
        q.put((rank, traceback.format_exc()))


# ---------------------------------------------------------------- the parent's judgement
def _table_is(parts, i, nm, adm, world, ftrl, what):
    """the ranks' shards of table nm at point i against an Admissible -> the table, sorted by key"""
    for r, p in enumerate(parts):
        assert np.all(S.owner_of(p["p%d_%s_k" % (i, nm)], world) == r), what + ": a foreign key"
    keys = np.concatenate([p["p%d_%s_k" % (i, nm)] for p in parts])
    order = np.argsort(keys)
    assert np.array_equal(keys[order], adm.keys), what + ": keys"
    shape = adm.pre[0].shape
    cols = [np.concatenate([p["p%d_%s_%s" % (i, nm, f)].reshape(-1, shape[1]) for p in parts])[order]
            for f in ("wnz" if ftrl else "w")]
    ok = adm.holds(*cols)
    if not ok.all():
        r, c = np.argwhere(~ok)[0]
        raise AssertionError(
            "%s: %d of %d coordinates hold no admissible state (%d of them pinned); first: key "
            "%d, coordinate %d of %d combinations, got %s, admissible %s, before %s" % (
                what, int((~ok).sum()), ok.size, int((~ok & adm.pinned()).sum()), adm.keys[r], c,
                adm.combos[r, c], [a[r, c] for a in cols],
                [[a[r, c] for a in t[:len(cols)]] for t in adm.tables], [a[r, c] for a in adm.pre]))
    for a, p in zip(cols, adm.pre):
        assert np.array_equal(bits(a)[~adm.stepped], bits(p)[~adm.stepped]), \
            what + ": a coordinate no rank moved has changed"
    return (adm.keys,) + tuple(cols)


def _judge(spec, tmp_path, empty_ranks=(), general=False, hyper=None):
    mode, world, F, k, opt, schedule, case, valued = spec
    port = free_port()
    T._spawn(_rank, [(r, spec, port, str(tmp_path), tuple(empty_ranks), general,
                      hyper.kw() if hyper else {}) for r in range(world)])
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    judge = I.Judge()
    strs = S.streams(spec, empty_ranks)
    run = S.Run(spec, strs, judge, S.init_seed(spec), hyper)
    ftrl = opt == "ftrl"
    for i, steps in enumerate(S.points(schedule, len(strs[0][0]))):
        p = run.point(steps)
        what = "%s, steps %s: " % (S.case_id(spec), steps)
        xw = _table_is(parts, i, "w", p.w, world, ftrl, what + "w")
        xv = None if p.v is None else _table_is(parts, i, "v", p.v, world, ftrl, what + "v")
        if mode == "field_aware" and F > 3:
            assert not p.v.stepped.all()             # untouched coordinates exist
        run.adopt(xw, xv)       # the next point starts from the GPU's state: nothing compounds
    for r in range(world):
        cands = run.predict(r)
        got = np.asarray(parts[r]["pctr"], np.float32)
        assert got.shape == cands.shape[:1], (r, got.shape, cands.shape)
        ok = (bits(got)[:, None] == bits(cands)).any(axis=1)
        assert ok.all(), "rank %d: %d of %d pctr are no candidate" % (r, int((~ok).sum()), ok.size)
    print(judge.format(S.case_id(spec)))
    judge.assert_cap()
    return parts


@pytest.mark.parametrize("spec", S.CASES + S.UNDERFLOW, ids=S.case_id)
def test_ranks_from_fresh_tables_in_general_position(tmp_path, spec):
    _judge(spec, tmp_path)


@pytest.mark.parametrize("spec", S.GENERAL, ids=S.case_id)
def test_one_rank_on_the_exchange_path_in_general_position(tmp_path, spec):
    """a group of one with XF_SHARDED_GENERAL=1: the emitting gradient kernels and the owner's
    (masked) push without other sources, judged by the same checker (not by bit equality with the
    fused step: arrival-order sums may differ between two runs)"""
    _judge(spec, tmp_path, general=True)


@pytest.mark.parametrize("spec", S.EMPTY_RANK, ids=S.case_id)
def test_a_rank_without_rows_in_general_position(tmp_path, spec):
    """world 2, rank 1 compiles zero-row minibatches: it serves Pulls that insert fresh rows it
    never computes on, and owns its share of the keys"""
    parts = _judge(spec, tmp_path, empty_ranks=(1,))
    assert len(parts[1]["p0_w_k"]) and len(parts[1]["p0_v_k"]) and len(parts[1]["pctr"]) == 0


@pytest.mark.parametrize("spec,hyper", S.HYPER, ids=S.hyper_id)
def test_ranks_away_from_the_default_hyper_parameters(tmp_path, spec, hyper):
    """capi.Sharded(alpha=, beta=, lambda1=, lambda2=, lr=): xf_sharded_create hands the five
    values to every rank's shard of both tables, the owners' steps use them"""
    _judge(spec, tmp_path, hyper=hyper)
