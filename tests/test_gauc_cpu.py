"""The grouped AUC's host side (xf_gauc_host.cc) and its restatement (tests/_gauc_checker.py),
without a GPU: the code of a row's record against the restatement, the restatement's figures
against a plain O(m^2) pair count, the known answers, the summary as bits, the refusals that need
no device, and tools/gauc_host_check.cc under the host sanitizers."""
import math
import os
import subprocess

import numpy as np
import pytest

from xflow_amd import build, capi

from . import _gauc_checker as G
from . import _progress_checker as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
EINVAL = 1          # XF_EINVAL


def edge_losses():
    """the rank's edge values of q, as the loss of a negative (p = q) and of a positive
    (loss = p - 1 = -q'), and what leaves no record"""
    qs = [0.0, -0.0, 1e-45, 2.0 ** -126, 2.0 ** -24, 0.25,
          float(np.nextafter(f32(0.5), f32(0))), 0.5, float(np.nextafter(f32(0.5), f32(1))),
          1.0 - 2.0 ** -24, 1.0, float("nan"), float(np.nextafter(f32(1), f32(2))), 1.5,
          float("inf")]
    return np.array(qs + [-q for q in qs], f32)


def test_code_against_the_restatement():
    loss = edge_losses()
    for label in (0, 1, 7, -1):
        want = G.codes(loss, np.full(len(loss), label, np.int32))
        got = np.array([capi.gauc_code(x, label) for x in loss], np.uint32)
        assert np.array_equal(got, want), (label, got, want)
    # the edges by hand: a negative's score is the rank of q, a positive's 2C - rank
    assert capi.gauc_code(0.0, 0) == 0 and capi.gauc_code(-0.0, 0) == 0
    assert capi.gauc_code(1e-45, 0) == 0
    assert capi.gauc_code(0.5, 0) == G.C << 1 and capi.gauc_code(-0.5, 1) == (G.C << 1) | 1
    assert capi.gauc_code(1.0, 0) == (2 * G.C) << 1 and capi.gauc_code(-1.0, 1) == 1
    assert capi.gauc_code(0.0, 1) == G.CODE_MAX
    assert capi.gauc_code(1.0 - 2.0 ** -24, 0) >> 1 == 152576
    assert capi.gauc_code(-(2.0 ** -24), 1) >> 1 == 152576       # the same p, the other class
    for bad in (float("nan"), 1.5, -1.5, float("inf")):
        assert capi.gauc_code(bad, 0) == G.OTHER == capi.GAUC_OTHER and \
            capi.gauc_code(bad, 1) == G.OTHER
    # random losses, every class
    rng = np.random.RandomState(3)
    loss = (rng.rand(4000) * 2.2 - 1.1).astype(f32)
    labels = rng.randint(-1, 3, size=4000).astype(np.int32)
    got = np.array([capi.gauc_code(x, y) for x, y in zip(loss, labels)], np.uint32)
    assert np.array_equal(got, G.codes(loss, labels))
    assert (got == G.OTHER).any() and (got != G.OTHER).any() and got[got != G.OTHER].max() <= G.CODE_MAX


def test_checker_against_a_plain_pair_count():
    rng = np.random.RandomState(5)
    for trial in range(40):
        m = int(rng.randint(1, 60))
        groups = int(rng.randint(1, 6))
        ids = rng.randint(0, groups, size=m).astype(np.uint64) * np.uint64(2**61 + 3)
        score = rng.randint(0, [3, 8, 2 * G.C + 1][trial % 3], size=m)
        pos = (rng.rand(m) < [0.5, 0.1, 0.9][trial % 3]).astype(np.int64)
        codes = ((score << 1) | pos).astype(np.uint32)
        gid, fig = G.figures(ids, codes)
        fid, ffig = G.figures_fast(ids, codes)
        assert np.array_equal(gid, fid) and np.array_equal(fig, ffig)
        assert np.array_equal(gid, np.unique(ids))
        for g, (Pn, Nn, U2, T) in zip(gid, fig):
            sel = ids == g
            twice = G.pair_count(score[sel], pos[sel])
            assert int(U2) == twice                              # U2 / 2 is the count, exactly
            assert int(Pn) == int(pos[sel].sum()) and int(Pn) + int(Nn) == int(sel.sum())
            ties = sum(int(pos[sel][i]) * int(np.sum((score[sel] == score[sel][i]) & (pos[sel] == 0)))
                       for i in range(int(sel.sum())))
            assert int(T) == ties


def _one(ids, scores, pos):
    codes = (np.asarray(scores, np.int64) << 1 | np.asarray(pos, np.int64)).astype(np.uint32)
    gid, fig = G.figures(np.asarray(ids, np.uint64), codes)
    lib, auc, slack = capi.gauc_summary(gid, fig)
    chk, cauc, cslack = G.summary(gid, fig)
    assert G.same(lib, chk) and G.same_bits(auc, cauc) and G.same_bits(slack, cslack)
    return fig, lib, auc, slack


def test_known_answers():
    fig, m, auc, slack = _one([4, 4], [9, 3], [1, 0])             # a positive above a negative
    assert fig.tolist() == [[1, 1, 2, 0]] and auc[0] == 1.0 and m["gauc"] == 1.0 and \
        m["gauc_slack"] == 0.0
    fig, m, auc, slack = _one([4, 4], [3, 9], [1, 0])             # the reverse
    assert fig.tolist() == [[1, 1, 0, 0]] and auc[0] == 0.0 and m["gauc"] == 0.0
    fig, m, auc, slack = _one([4] * 5, [7] * 5, [1, 0, 0, 1, 0])  # all tied
    assert fig.tolist() == [[2, 3, 6, 6]] and auc[0] == 0.5 and slack[0] == 0.5 and \
        m["gauc"] == 0.5 and m["gauc_slack"] == 0.5 and m["macro_auc"] == 0.5
    fig, m, auc, slack = _one([4] * 3, [1, 2, 3], [1, 1, 1])      # one class: not scored
    assert fig.tolist() == [[3, 0, 0, 0]] and math.isnan(auc[0]) and math.isnan(m["gauc"]) and \
        m["groups"] == 1 and m["groups_scored"] == 0 and m["rows_one_class"] == 3
    # a weighted mean: a group of 2 rows at AUC 1 and one of 6 rows at AUC 0.5
    fig, m, auc, slack = _one([1, 1] + [2] * 6, [5, 1] + [3] * 6, [1, 0] + [1, 0, 0, 0, 1, 1])
    assert m["gauc"] == (2.0 * 1.0 + 6.0 * 0.5) / 8.0 and m["macro_auc"] == 0.75 and \
        m["rows"] == 8 and m["rows_scored"] == 8 and m["groups_scored"] == 2


def test_summary_against_the_restatement():
    rng = np.random.RandomState(8)
    for trial in range(30):
        m = int(rng.randint(0, 400))
        ids = rng.randint(0, max(1, m // [1, 4, 50][trial % 3]), size=m).astype(np.uint64)
        codes = ((rng.randint(0, 40, size=m) << 1) | (rng.rand(m) < 0.3)).astype(np.uint32)
        gid, fig = G.figures_fast(ids, codes)
        none, other = rng.randint(0, 9, size=2), rng.randint(0, 9, size=2)
        lib, auc, slack = capi.gauc_summary(gid, fig, none, other)
        chk, cauc, cslack = G.summary(gid, fig, none, other)
        assert G.same(lib, chk) and G.same_bits(auc, cauc) and G.same_bits(slack, cslack)
        assert lib["rows"] == m and lib["none_rows"] == int(none.sum())
    # no group; no scored group
    lib, auc, _ = capi.gauc_summary(np.zeros(0, np.uint64), np.zeros((0, 4), np.uint64), [1, 2], [3, 4])
    assert G.same(lib, G.summary([], [], [1, 2], [3, 4])[0]) and len(auc) == 0
    assert math.isnan(lib["gauc"]) and math.isnan(lib["gauc_slack"]) and math.isnan(lib["macro_auc"])
    assert lib["groups"] == 0 and lib["none_rows"] == 3 and lib["other_rows"] == 7
    fig = np.array([[3, 0, 0, 0], [0, 2, 0, 0]], np.uint64)
    lib, auc, _ = capi.gauc_summary([5, 2**64 - 2], fig)
    assert G.same(lib, G.summary([5, 2**64 - 2], fig)[0]) and math.isnan(lib["gauc"]) and \
        lib["groups"] == 2 and lib["groups_scored"] == 0 and lib["rows_one_class"] == 5
    # figures near the limits: fl(U2) and fl(2 P N) round
    Pn, Nn = 2**29 - 1, 2**29
    fig = np.array([[Pn, Nn, 2 * Pn * Nn - 12345, 999]], np.uint64)
    lib, auc, _ = capi.gauc_summary([0], fig)
    assert G.same(lib, G.summary([0], fig)[0])
    assert auc[0] == float(2 * Pn * Nn - 12345) / float(2 * Pn * Nn)


def test_refusals_without_a_device():
    ok = np.array([[1, 1, 1, 1]], np.uint64)
    with pytest.raises(capi.XFError, match="do not ascend"):
        capi.gauc_summary([3, 3], np.repeat(ok, 2, axis=0))
    with pytest.raises(capi.XFError, match="do not ascend"):
        capi.gauc_summary([4, 3], np.repeat(ok, 2, axis=0))
    for bad in ([0, 0, 0, 0], [1, 1, 3, 0], [1, 1, 2, 2], [2**30, 1, 0, 0], [2, 2, 1, 2]):
        with pytest.raises(capi.XFError, match="xf_gauc_summary: entry 0"):
            capi.gauc_summary([1], np.array([bad], np.uint64))
    m = capi.GaucMetrics()
    assert capi.lib().xf_gauc_summary(None, 1, None, None, capi.C.byref(m), None, None) == EINVAL
    assert capi.lib().xf_gauc_summary(None, 0, None, None, None, None, None) == EINVAL
    # calls that need an object refuse a null one before they touch a device
    L = capi.lib()
    n = capi.C.c_uint64()
    assert L.xf_gauc_reduce(None, None, 0, capi.C.byref(n), None, None, 0) == EINVAL
    assert L.xf_gauc_export(None, None, None, 0, capi.C.byref(n)) == EINVAL
    assert L.xf_gauc_append(None, None, None, 0) == EINVAL
    assert L.xf_gauc_append_dev(None, None, None, None, 0, None) == EINVAL
    assert L.xf_gauc_reserve(None, 1) == EINVAL
    assert L.xf_gauc_create(None) == EINVAL
    assert L.xf_gauc_destroy(None) == capi.XF_OK
    assert L.xf_workspace_gauc(None, None) == EINVAL
    assert L.xf_workspace_gauc_ids(None, None, 0) == EINVAL
    assert L.xf_sharded_gauc(None, 1) == EINVAL
    assert L.xf_sharded_gauc_read(None, None, 0, capi.C.byref(n), None, None, 0, 0) == EINVAL
    assert capi.gauc_shape() == {"pack_rows": 1024, "reduce_records": 1024}
    assert capi.gauc_launches() >= 0


def test_host_check_under_the_sanitizers(tmp_path):
    """tools/gauc_host_check.cc: the same host code from a main of its own, built with
    -fsanitize=address,undefined and run here"""
    exe = str(tmp_path / "gauc_host_check")
    csrc = os.path.join(ROOT, "xflow_amd", "csrc")
    cmd = [build._hipcc(), "-std=c++17", "-g", "-O1", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tools", "gauc_host_check.cc"), os.path.join(csrc, "xf_gauc_host.cc"),
           os.path.join(csrc, "xf_io.cc"), "-o", exe, "-lpthread"]
    made = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert made.returncode == 0, made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and ran.stdout.strip() == "gauc_host_check: ok", ran.stdout + ran.stderr
