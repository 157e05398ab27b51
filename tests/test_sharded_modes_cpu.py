"""The several-rank checker (tests/_sharded_modes_checker.py) on its own, no GPU: every sum it
forms over the streams of tests/test_gpu_sharded_modes.py is exact (formed in both orders), the
streams hold what those tests need in order not to pass vacuously, and with one rank the
composition is the one-rank checkers' own step."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import _ffm_checker as FF
from tests import _fmc_checker as FC
from tests import _sharded_modes_checker as M
from tests import _valued_cases as Cs
from tests import _valued_checker as V

CASES, case_id, run_case = M.CASES, M.case_id, M.run_case
TILE_NNZ = 2048     # XF_TILE_NNZ: the occurrences of one chunk of a heavy key


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_store(a, b):
    for x, y in zip(a.export(), b.export()):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


# every stream x world in {2, 3} x mode the GPU tests use (both schedules: the tables a rank pulls
# from differ between them, and with them every addend)
_GRID = tuple((m, w, F, k, o, s, st, v) for (m, _, F, k, o, _, st, v) in CASES
              for w in (2, 3) for s in ("sequential", "stale1"))


@pytest.mark.parametrize("c", sorted(set(_GRID + M.GENERAL + tuple(one for _, one in M.EMPTY_RANK))), ids=case_id)
def test_every_sum_of_the_checker_is_exact(c):
    audit = run_case(c)[5]
    V.assert_exact(audit)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_streams_hold_what_the_gpu_tests_need(c):
    mode, world, F, k, opt, schedule, case, valued = c
    ws, vs, pctr, log, strs, audit = run_case(c)
    # a key present on two ranks in the same step: the owner's walk in source-rank order
    assert len(M.shared_key_steps(log)) == M.STEPS
    if mode == "field_aware":
        assert M.differing_mask_steps(log), "no key whose touched masks differ between two ranks"
        keys = vs.export()[0]
        free = M.never_touched(log, keys, F)
        assert free.any(), "every (key, field) is touched by some rank"
        # ... and those coordinates hold the imported state, bit for bit
        _, w0, n0, z0 = M.old_tables(mode, opt, k, F, keys)[1]
        cols = np.repeat(free, k, axis=1)
        _, w1, n1, z1 = vs.export()
        assert np.array_equal(_bits(w1)[cols], _bits(w0)[cols])
        if opt == "ftrl":
            assert np.array_equal(_bits(n1)[cols], _bits(n0)[cols])
            assert np.array_equal(_bits(z1)[cols], _bits(z0)[cols])
    if case == "zipf_chunks":
        most = max(Cs.heavy_profile(m)[1] for train, _ in strs for m in train)
        assert most > TILE_NNZ, "no heavy key of two chunks or more (%d occurrences)" % most
    if case.startswith("zipf"):
        assert all(Cs.heavy_profile(m)[0] >= 1 for train, _ in strs for m in train)
    if case == "ragged":
        for train, _ in strs:
            for rowptr, keys, _, _, _ in train:
                assert (np.diff(rowptr.astype(np.int64)) == 0).any()
                a = int(rowptr[1])
                assert keys[a] == keys[a + 2]


@pytest.mark.parametrize("mode,F,k,opt,case,valued", [
    ("canonical", 0, 4, "ftrl", "ragged", False), ("canonical", 0, 7, "sgd", "zipf_heavy", True),
    ("lr", 0, 0, "ftrl", "ragged", True), ("field_aware", 3, 4, "ftrl", "ragged", True),
    ("field_aware", 5, 4, "sgd", "zipf_heavy", False)])
def test_one_rank_is_the_one_rank_checkers_step(mode, F, k, opt, case, valued):
    """world 1, sequential: nothing lies between a step's Pull and its Push, so the composition
    must give the tables and predictions of _fmc_checker.step, _valued_checker.lr_step / fm_step
    and _ffm_checker.step on the same stream (stale1 pulls step t + 1 before Push(t) lands, at
    any world size: another function)"""
    schedule = "sequential"
    strs = M.streams(mode, case, 1, F)
    audit, audit1 = [], []
    with O.sum_mode(1):
        ws, vs, pctr, _ = M.run(mode, opt, k, F, valued, schedule, strs, audit)
        ws1, vs1 = M.stores(mode, opt, k, F, strs)
        train, held = strs[0]
        for rowptr, keys, fg, vals, labels in train:
            if mode == "lr":
                V.lr_step(ws1, rowptr, keys, vals, labels, audit1)
            elif mode == "field_aware":
                FF.step(ws1, vs1, F, rowptr, keys, fg, vals if valued else None, labels, audit1)
            elif valued:
                V.fm_step(ws1, vs1, rowptr, keys, vals, labels, audit1)
            else:
                FC.step(ws1, vs1, rowptr, keys, labels)
        rowptr, keys, fg, vals, labels = held
        if mode == "lr":
            p1 = V.lr_predict(ws1, rowptr, keys, vals, labels, audit1)
        elif mode == "field_aware":
            p1 = FF.predict(ws1, vs1, F, rowptr, keys, fg, vals if valued else None, labels, audit1)
        elif valued:
            p1 = V.fm_predict(ws1, vs1, rowptr, keys, vals, labels, audit1)
        else:
            p1 = FC.predict(ws1, vs1, rowptr, keys, labels)
    V.assert_exact(audit)
    same_store(ws, ws1)
    if vs is not None:
        same_store(vs, vs1)
    assert np.array_equal(_bits(pctr[0]), _bits(np.asarray(p1, np.float32)))


@pytest.mark.parametrize("two,one", M.EMPTY_RANK, ids=[case_id(t) for t, _ in M.EMPTY_RANK])
def test_a_rank_without_rows_changes_nothing(two, one):
    """world 2 with rank 1 empty = world 1 (the GPU test's reference)"""
    a, b = M.run_case(two, empty_ranks=(1,)), M.run_case(one)
    same_store(a[0], b[0])
    if a[1] is not None:
        same_store(a[1], b[1])
    assert np.array_equal(_bits(a[2][0]), _bits(b[2][0])) and len(a[2][1]) == 0
