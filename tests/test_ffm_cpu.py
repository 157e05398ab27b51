"""Field-aware FM (fm_mode=field_aware) without a GPU: the numpy checker of tests/_ffm_checker.py
against autograd and against the canonical form at fields = 1, the touched rule, the audit of
every stream the GPU tests use, the host builder's field arrays, and the parameters and refusals
of the C surface that need no device."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _ffm_checker as F
from . import _fmc_checker as FC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAIN, TEST = os.path.join(GOLDEN, "small_train-00000"), os.path.join(GOLDEN, "small_test-00000")


# ------------------------------------------------------------------ parameters and refusals
def _start(**params):
    """XFStartTrain through the C ABI itself (capi.XFlow.train asks for a GPU first): -> (rc,
    xf_last_error)"""
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode()


def test_parameters_of_the_worker():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test")
    x.set("fm_mode", "field_aware")
    x.set("fields", 18)
    x.set("fm_mode", "canonical")
    x.set("fm_mode", "reference")
    rc = capi.lib().XFSetParam(x.h, b"fm_mode", b"bogus")
    assert rc == capi.XF_OK + 1                        # XF_EINVAL
    msg = capi.lib().xf_last_error().decode()
    assert "reference" in msg and "canonical" in msg and "field_aware" in msg, msg
    assert capi.FM_FIELD_AWARE == 2 and capi.FM_MODES["field_aware"] == 2


@pytest.mark.parametrize("params,why", [
    (dict(fields=0), r"fields in 1 \.\. 64.*fields=0"),
    (dict(fields=65), r"fields in 1 \.\. 64.*fields=65"),
    (dict(), r"fields in 1 \.\. 64"),                                  # fields never set
    (dict(fields=64, k=65), r"64 x 65 exceeds 4096"),
    (dict(fields=18, model=0), r"model 1"),
    (dict(fields=18, world=2), r"one worker"),
    (dict(fields=18, parity="reference_order"), r"parity"),
    (dict(fields=18, ingest="gpu"), r"ingest=gpu.*fgid"),
    (dict(fields=18, feature_values="on", block_cache=1), r"feature_values.*block_cache"),
])
def test_start_train_refusals_are_named_without_a_gpu(params, why):
    import re
    t0 = time.time()
    p = dict(model=1, k=4)
    p.update(params)
    rc, msg = _start(fm_mode="field_aware", **p)
    assert rc == capi.XF_OK + 1, (rc, msg)
    assert re.search(why, msg), msg
    assert "field_aware" in msg or "feature_values" in msg, msg
    assert time.time() - t0 < 10


def test_workspace_refusals_without_a_gpu():
    ws = capi.Workspace()
    with pytest.raises(capi.XFError, match=r"xf_workspace_fm_fields"):
        ws.fm_mode("field_aware")                    # fields first
    for bad in (0, 65, -1):
        with pytest.raises(capi.XFError, match=r"1 \.\. 64"):
            ws.fm_fields(bad)
    ws.fm_fields(18)
    ws.fm_mode("field_aware")
    with pytest.raises(capi.XFError, match=r"field-aware.*capture"):
        capi.check(capi.lib().xf_workspace_capture(ws.h, 1))
    with pytest.raises(capi.XFError, match=r"reference-order"):
        ws.parity("reference_order")
    ws = capi.Workspace(capture=True)
    ws.fm_fields(3)
    with pytest.raises(capi.XFError, match=r"field-aware.*capture"):
        ws.fm_mode("field_aware")
    ws = capi.Workspace()
    ws.parity("reference_order")
    ws.fm_fields(3)
    with pytest.raises(capi.XFError, match=r"parity"):
        ws.fm_mode("field_aware")


# ------------------------------------------------------------------------ the function
def _batch(rng, R, max_len, U, F, k, valued):
    """repeated keys, keys under two fields, empty rows; row 0: one key twice (two fields), row 1:
    one key twice under ONE field"""
    lens = rng.randint(0, max_len + 1, size=R)
    lens[0], lens[1], lens[2] = 4, 3, 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(lens.sum())
    uidx = rng.randint(0, U, size=n).astype(np.int64)
    fg = rng.randint(0, F, size=n).astype(np.int64)
    uidx[2], fg[2] = uidx[0], (fg[0] + 1) % F
    uidx[6], fg[6] = uidx[4], fg[4]
    x = (rng.randint(1, 9, size=n) / 4.0).astype(np.float32) if valued else np.ones(n, np.float32)
    labels = rng.randint(0, 2, size=R).astype(np.int32)
    wu = (rng.randn(U) * 0.1).astype(np.float32)
    vu = (rng.randn(U, F * k) * 0.1).astype(np.float32)
    return rowptr, uidx, fg, x, labels, wu, vu


@pytest.mark.parametrize("F_,k,valued,seed", [(1, 3, False, 0), (3, 4, True, 1), (18, 4, True, 2),
                                              (5, 7, False, 3), (2, 1, True, 4)])
def test_gradients_equal_autograd(F_, k, valued, seed):
    torch = pytest.importorskip("torch")
    rng = np.random.RandomState(seed)
    rowptr, uidx, fg, x, labels, wu, vu = _batch(rng, 60, 9, 25, F_, k, valued)
    R, U = len(rowptr) - 1, len(wu)
    audit = []
    loss, _, _, pairs = F.forward(rowptr, uidx, fg, x, labels, wu, vu, F_, audit)
    gw, gv, touched = F.gradient(rowptr, uidx, fg, U, x, loss, F_, pairs, audit)

    w = torch.tensor(wu.astype(np.float64), requires_grad=True)
    v = torch.tensor(vu.astype(np.float64).reshape(U, F_, k), requires_grad=True)
    xt = torch.tensor(x.astype(np.float64))
    pi, pj, pr = (torch.tensor(a) for a in F.pairs_of(rowptr))
    ui, g = torch.tensor(uidx), torch.tensor(fg)
    t = ((v[ui[pi], g[pj]] * xt[pi][:, None]) * (v[ui[pj], g[pi]] * xt[pj][:, None])).sum(1)
    y2 = torch.zeros(R, dtype=torch.float64).index_add(0, pr, t)
    wx = torch.zeros(R, dtype=torch.float64).index_add(0, torch.tensor(F.rows_of(rowptr)),
                                                        w[ui] * xt)
    y = torch.tensor(labels.astype(np.float64))
    L = torch.nn.functional.binary_cross_entropy_with_logits(wx + y2, y, reduction="mean")
    L.backward()
    vg = v.grad.numpy().reshape(U, F_ * k)
    for got, want in ((gw, w.grad.numpy()), (gv, vg)):
        tol = 1e-5 * (np.abs(want) + np.sqrt(np.mean(want * want)))
        bad = np.abs(got.astype(np.float64) - want) > tol
        assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])
    # an untouched coordinate has no addend: its autograd gradient is an exact zero too
    assert np.all(vg[~np.repeat(touched, k, axis=1)] == 0.0)
    assert touched.any() and (F_ < 18 or not touched.all())


@pytest.mark.parametrize("k", [1, 4, 10])
def test_one_field_is_the_canonical_form(k):
    """fields = 1: sum_{i<j} <a_i, a_j>, which is the canonical 0.5 (T - Q).  Both in fp64, within
    rounding (the two forms round differently: no bit equality)"""
    rng = np.random.RandomState(k)
    rowptr, uidx, fg, x, labels, wu, vu = _batch(rng, 80, 12, 30, 1, k, False)
    wx, y2 = F.forward64(rowptr, uidx, fg, x, wu, vu, 1)
    _, _, _, T, Q = FC.forward(rowptr, uidx, labels, wu, vu)
    assert np.all(np.abs(y2 - 0.5 * (T - Q)) <= 1e-6 * (T + Q) + 1e-30)
    audit = []
    y2_32 = F.forward(rowptr, uidx, fg, x, labels, wu, vu, 1, audit)[2]
    assert np.all(np.abs(y2_32 - y2) <= 1e-5 * (T + Q) + 1e-30)


# ------------------------------------------------------------------------ the touched rule
def test_touched_rule_differs_from_stepping_every_coordinate_under_ftrl_only():
    Fd, k = 39, 4
    mbs = F.stream("ragged", Fd)
    out = {}
    for opt in ("sgd", "ftrl"):
        for rule in (True, False):
            ws, vs = F.stores(opt, Fd, k, 7)
            audit = []
            first = None
            for rowptr, keys, fg, vals, labels in mbs:
                r = F.step(ws, vs, Fd, rowptr, keys, fg, None, labels, audit, touched_only=rule)
                first = first or r
            out[opt, rule] = vs.export()
            if rule and opt == "ftrl":
                # after one step from fresh tables the untouched coordinates still hold the init
                ukeys, touched = first[0], first[5]
                assert 0.05 < 1.0 - touched.mean() < 0.99       # real test material
    for a, b in zip(out["sgd", True], out["sgd", False]):
        assert np.array_equal(a, b)                  # g = 0 moves nothing under SGD
    wt, wa = out["ftrl", True][1], out["ftrl", False][1]
    assert not np.array_equal(wt, wa)
    # every coordinate stepped: an untouched one lost its hash-normal init for good
    assert np.count_nonzero(wa == 0.0) > np.count_nonzero(wt == 0.0)


def test_untouched_coordinates_keep_their_state():
    Fd, k = 39, 4
    rowptr, keys, fg, vals, labels = F.stream("ragged", Fd)[0]
    mbs = [(rowptr, keys, fg, vals, labels)]
    for opt in ("ftrl", "sgd"):
        ws, vs = F.aged_stores(opt, Fd, k, mbs)
        before = vs.export()
        audit = []
        ukeys, _, _, _, gv, touched = F.step(ws, vs, Fd, rowptr, keys, fg, vals, labels, audit)
        F.assert_exact(audit)
        after = vs.export()
        at = np.searchsorted(before[0], ukeys)
        mask = np.repeat(touched, k, axis=1)
        for a, b in zip(before[1:], after[1:]):
            assert np.array_equal(a[at][~mask], b[at][~mask])
        assert not np.array_equal(before[1][at][mask], after[1][at][mask])


# ------------------------------------------------------------------------ the audit
@pytest.mark.parametrize("opt", ["sgd", "ftrl"])
@pytest.mark.parametrize("case,Fd,k", F.GRID)
def test_every_sum_of_the_gpu_streams_is_exact(case, Fd, k, opt):
    mbs = F.stream(case, Fd)
    for valued in (True, False):
        audit = []
        steps, _, _, _ = F.run_checker(opt, Fd, k, mbs, audit, valued=valued)
        F.assert_exact(audit)
        d = F.disagreements(audit)
        assert set(d) == {"wx", "y2", "gw", "gv"}
    if case == "long_rows":
        assert max(np.diff(mbs[0][0].astype(np.int64))) > 300
    if case == "zipf_chunks":
        cnt = np.unique(mbs[0][1], return_counts=True)[1]
        assert cnt.max() > 2 * 2048                  # several chunks of XF_TILE_NNZ
    touched = steps[0][5]
    assert Fd <= 3 or not touched.all()


@pytest.mark.parametrize("case,Fd,k,opt,valued,nsteps", F.FRESH)
def test_every_sum_of_the_fresh_table_streams_is_exact(case, Fd, k, opt, valued, nsteps):
    audit = []
    F.run_checker(opt, Fd, k, F.stream(case, Fd)[:nsteps], audit, valued=valued, aged=False)
    F.assert_exact(audit)


@pytest.mark.parametrize("valued", [False, True])
def test_golden_files_from_fresh_tables(valued):
    """fields = 18, k = 4, two epochs from fresh hash-normal tables: under SGD every sum is exact
    (what the worker test on the GPU relies on).  Under FTRL the y2 sums are not: 27 of 600
    (binary) and 40 of 600 (valued) depend on the order of their addends, so FTRL is not a case
    the worker test may judge under this audit (it judges it under the interval rule:
    tests/test_general_position_cpu.py::test_golden_files_under_ftrl_have_no_open_sum)."""
    audit = []
    F.run_checker_files("sgd", TRAIN, TEST, audit, valued)
    F.assert_exact(audit)
    d = F.disagreements(audit)
    assert d["y2"][0] == 600 and d["gv"][0] > 60000
    audit = []
    F.run_checker_files("ftrl", TRAIN, TEST, audit, valued)
    d = F.disagreements(audit)
    print("ftrl from fresh tables, valued=%s: %r" % (valued, d))
    assert d["y2"][1] > 0, "FTRL passes the audit now: add it to the worker test's optimizers"


# ------------------------------------------------------------------------ the host builder
def _check_arrays(rowptr, keys, fg, labels, Fd, vals=None):
    b = capi.Batch(rowptr, keys, labels, values=vals, fields=Fd, fgid=fg)
    xfg, pos = b.field_arrays()
    want_fg, want_pos = F.field_arrays(rowptr, keys, fg)
    assert np.array_equal(xfg, want_fg) and np.array_equal(pos, want_pos)
    h = b.host()
    # an occurrence's position names its row and its key
    row_of = F.rows_of(rowptr.astype(np.int64))
    assert np.array_equal(h["coo_row"], row_of[pos])
    assert np.array_equal(h["ukeys"][h["uidx"][pos]], np.repeat(h["ukeys"], np.diff(h["segptr"])))
    # the other arrays are those of a minibatch without fields
    plain = capi.Batch(rowptr, keys, labels, values=vals).host()
    for n in plain:
        assert np.array_equal(plain[n], h[n]), n
    if vals is not None:
        assert np.array_equal(b.values()[1], np.asarray(vals, np.float32)[pos])
    return b


def test_host_builder_field_arrays():
    for path, Fd in ((TRAIN, 18), (TEST, 18), (os.path.join(GOLDEN, "quirks-00000"), 40)):
        for rowptr, keys, fg, labels in O.read_blocks(path, 2 << 20):
            assert fg.max() < Fd
            _check_arrays(rowptr, keys, fg, labels, Fd)
    for case in ("zipf_chunks", "ragged"):
        rowptr, keys, fg, vals, labels = F.stream(case, 39)[0]
        b = _check_arrays(rowptr, keys, fg, labels, 39, vals)
        assert (b.H > 0) == (case == "zipf_chunks")
    # a minibatch without fields has none; an empty one with fields is fine
    assert capi.Batch(rowptr, keys, labels).field_arrays()[0].size == 0
    e = capi.Batch(np.zeros(3, np.uint64), np.zeros(0, np.uint64), np.zeros(2, np.int32),
                   fields=5, fgid=np.zeros(0, np.int32))
    assert (e.R, e.NNZ) == (2, 0)


def test_fgid_out_of_range_is_refused_by_name():
    path = os.path.join(GOLDEN, "quirks-00000")
    (rowptr, keys, fg, labels), = list(O.read_blocks(path, 2 << 20))
    assert fg.max() == 39                                # the quirks golden reaches 39
    with pytest.raises(capi.XFError, match=r"fgid 39.*fields = 39"):
        capi.Batch(rowptr, keys, labels, fields=39, fgid=fg)
    capi.Batch(rowptr, keys, labels, fields=40, fgid=fg)
    neg = fg.copy()
    neg[3] = -2
    with pytest.raises(capi.XFError, match=r"nonzero 3 has fgid -2.*fields = 64"):
        capi.Batch(rowptr, keys, labels, fields=64, fgid=neg)
    for bad in (0, 65):
        with pytest.raises(capi.XFError, match=r"fields must be in 1 \.\. 64"):
            capi.Batch(rowptr, keys, labels, fields=bad, fgid=fg)
