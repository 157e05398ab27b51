"""Feature values without a GPU: the reader's third field, the host builder's value arrays, the
feature_values parameter, and the numpy checker of tests/_valued_checker.py — against the
canonical checker with all values 1, and alone over every stream of the GPU tests, where each of
its fp64 sums must not depend on the order of its addends."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

from . import _fmc_checker as F
from . import _valued_cases as Cs
from . import _valued_checker as V

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _read(path, cap, values=True):
    blocks = list(capi.read_blocks(path, cap, values=values))
    return blocks


def _write(tmp_path, text, name="f-00000"):
    p = tmp_path / name
    p.write_bytes(text)
    return str(p)


# ------------------------------------------------------------------------------- reader
@pytest.mark.parametrize("cap", [1000, 4096, 2097152])
def test_golden_values_are_the_files_third_fields(cap):
    path = os.path.join(GOLD, "small_train-00000")
    blocks = _read(path, cap)
    vals = np.concatenate([b[4] for b in blocks])
    assert vals.dtype == np.float32
    assert all(len(b[4]) == len(b[1]) for b in blocks)
    assert {float(np.float32(0.3651)), 0.5} <= set(np.unique(vals).tolist())
    assert np.array_equal(vals, V.file_values(path))
    # the first row of the file: fifteen tokens of 0.3651, then two of 0.50000
    assert np.array_equal(vals[:17], np.float32([0.3651] * 15 + [0.5] * 2))


@pytest.mark.parametrize("name,caps", [("small_train-00000", (1000, 4096, 2097152)),
                                       ("small_test-00000", (1000, 4096, 2097152)),
                                       ("quirks-00000", (202, 777, 1048576))])
def test_values_change_nothing_else(name, caps):
    path = os.path.join(GOLD, name)
    for cap in caps:
        off, on = _read(path, cap, values=False), _read(path, cap)
        assert len(off) == len(on) > 0
        for a, b in zip(off, on):
            assert len(a) == 4 and len(b) == 5
            for x, y in zip(a, b[:4]):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            assert len(b[4]) == len(b[1])
    # one block holds the whole file: token order is the file's
    assert np.array_equal(np.concatenate([b[4] for b in _read(path, caps[-1])]),
                          V.file_values(path))


HAND = (b"1\t1:2:3 1:2:-0.25 1:2:1e-3\n"
        b"0\t1:2: 1:2:3:4 7:8:0.5  1:2:2\n"          # an empty field, further colons, an empty token
        b"1\t4:5:.5 4:5:1. 4:5:+2 4:5:-0 4:5:0x10 4:5:12abc\n"
        b"0\t9:9:0.1234567890123456789 9:9:123456789012345678 9:9:4e-46 9:9:16777217\n"
        b"1\t3:3:7 \n"                                 # a single blank before the newline: no token
        b"0\t6:6:0.75")                               # a value that ends the block (and the file)
HAND_WANT = [3, -0.25, 1e-3,
             0, 3, 0.5, 0.5, 2,
             0.5, 1, 2, -0.0, 16, 12,
             0.1234567890123456789, 123456789012345678, 0.0, 16777216,
             7,
             0.75]


def test_hand_written_tokens(tmp_path):
    path = _write(tmp_path, HAND)
    (rp, ks, fg, lb, vals), = _read(path, 1 << 20)
    want = np.array([np.float32(x) for x in HAND_WANT], np.float32)
    assert np.array_equal(rp, [0, 3, 8, 14, 18, 19, 20])
    assert np.array_equal(vals.view(np.uint32), want.view(np.uint32))   # (-0 is -0)
    assert ks[6] == ks[5] and fg[6] == fg[5]          # the empty token repeats key and value
    # cut into blocks at newlines: a value then ends a block, the values are the same (without
    # the line that ends in a blank: cut there, the blank would be a token before the terminator)
    lines = HAND.split(b"\n")
    path2 = _write(tmp_path, b"\n".join(lines[:4] + lines[5:]), "g-00000")
    (_, ks2, _, _, vals2), = _read(path2, 1 << 20)
    assert np.array_equal(vals2.view(np.uint32), np.delete(want, 18).view(np.uint32))
    small = _read(path2, 100)
    assert len(small) > 2
    assert np.array_equal(np.concatenate([b[4] for b in small]).view(np.uint32),
                          vals2.view(np.uint32))
    assert np.array_equal(np.concatenate([b[1] for b in small]), ks2)


def test_an_empty_token_before_the_block_terminator_repeats_the_value(tmp_path):
    path = _write(tmp_path, b"1\t1:2:0.25 3:4:1.5 ")   # no newline: the blank is a token
    (rp, ks, fg, lb, vals), = _read(path, 1 << 20)
    assert np.array_equal(rp, [0, 3]) and ks[2] == ks[1]
    assert np.array_equal(vals, np.float32([0.25, 1.5, 1.5]))


@pytest.mark.parametrize("field,why", [(b"nan", "not finite"), (b"inf", "not finite"),
                                       (b"-inf", "not finite"), (b"1e39", "not finite"),
                                       (b"0." + b"1" * 58, "too long")])
def test_rejected_values_name_the_cause(tmp_path, field, why):
    path = _write(tmp_path, b"1\t1:2:1 3:4:" + field + b" 5:6:1\n")
    with pytest.raises(capi.XFError) as e:
        _read(path, 1 << 20)
    assert "val" in str(e.value) and why in str(e.value)
    # values off: the field is never looked at
    (rp, ks, fg, lb), = _read(path, 1 << 20, values=False)
    assert len(ks) == 3


@pytest.mark.parametrize("seed", range(40))
def test_random_decimal_strings_convert_like_float(tmp_path, seed):
    rng = np.random.RandomState(seed)
    toks = []
    for _ in range(400):
        ni, nf = rng.randint(0, 12), rng.randint(0, 14)
        s = "".join(rng.choice(list("0123456789"), size=ni)) if ni else ""
        if nf or not s:
            s += "." + "".join(rng.choice(list("0123456789"), size=max(nf, 1)))
        if rng.rand() < 0.3:
            s = "-" + s
        if rng.rand() < 0.15:
            s += "e%d" % rng.randint(-30, 27)
        toks.append(s)
    want = np.array([np.float32(float(s)) for s in toks], np.float32)
    assert np.isfinite(want).all()
    lines = [b"1\t" + b" ".join(b"1:%d:%s" % (i, t.encode()) for i, t in enumerate(toks[a:a + 20]))
             for a in range(0, len(toks), 20)]
    path = _write(tmp_path, b"\n".join(lines) + b"\n")
    vals = np.concatenate([b[4] for b in _read(path, 700)])
    assert np.array_equal(vals.view(np.uint32), want.view(np.uint32))


def test_values_are_switched_on_before_the_first_block_and_not_over_a_cache(tmp_path):
    L = capi.lib()
    path = os.path.join(GOLD, "small_train-00000")
    r = capi.vp()
    capi.check(L.xf_reader_open(C.byref(r), path.encode(), 4096))
    try:
        rows = C.c_size_t()
        capi.check(L.xf_reader_next(r, C.byref(rows), None, None, None, None, None))
        assert L.xf_reader_set_values(r, 1) != 0
        assert "handed out a block" in L.xf_last_error().decode()
    finally:
        L.xf_reader_close(r)
    r, hit = capi.vp(), C.c_int()
    capi.check(L.xf_reader_open_cached(C.byref(r), path.encode(), 4096,
                                       str(tmp_path / "c.xfcsr").encode(), C.byref(hit)))
    try:
        assert L.xf_reader_set_values(r, 1) != 0
        assert "block cache" in L.xf_last_error().decode()
    finally:
        L.xf_reader_close(r)


# ------------------------------------------------------------------------- host builder
def test_host_builder_value_arrays_equal_numpy():
    rng = np.random.RandomState(3)
    for rowptr, keys, vals, labels in (Cs.ragged(0), Cs.zipf(1, 300, 12, 500)):
        b = capi.Batch(rowptr, keys, labels, values=vals)
        h = b.host()
        xval, coo_val = b.values()
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(xval.view(np.uint32), vals.view(np.uint32))
        assert np.array_equal(coo_val.view(np.uint32), vals[order].view(np.uint32))
        assert np.array_equal(h["coo_row"], F.rows_of(rowptr)[order])
        # everything else is the binary builder's
        hb = capi.Batch(rowptr, keys, labels).host()
        assert all(np.array_equal(h[n], hb[n]) for n in hb)
    # a row slice takes its slice of the values
    rowptr, keys, vals, labels = Cs.ragged(2)
    b = capi.Batch(rowptr, keys, labels, 10, 50, values=vals)
    a, e = int(rowptr[10]), int(rowptr[50])
    assert np.array_equal(b.values()[0], vals[a:e])
    assert np.array_equal(b.values()[1], vals[a:e][np.argsort(keys[a:e], kind="stable")])
    assert capi.Batch(rowptr, keys, labels).values()[0].size == 0   # a binary one has none
    del rng


# --------------------------------------------------------------------------- parameters
def test_feature_values_parameter_is_validated_without_a_gpu():
    L = capi.lib()
    h = capi.vp()
    assert L.XFCreate(C.byref(h), b"/nonexistent/train", b"/nonexistent/test") == 0
    try:
        for v in ("on", "off", "on"):
            assert L.XFSetParam(h, b"feature_values", v.encode()) == 0, L.xf_last_error()
        assert L.XFSetParam(h, b"feature_values", b"maybe") != 0
        msg = L.xf_last_error().decode()
        assert "feature_values" in msg and "maybe" in msg and "on or off" in msg
    finally:
        L.XFDestroy(h)


# ------------------------------------------------------------------------------ checker
@pytest.mark.parametrize("k,opt", [(1, "ftrl"), (7, "sgd"), (16, "ftrl"), (64, "sgd")])
def test_checker_with_all_values_one_is_the_canonical_checker(k, opt):
    mbs = Cs.stream("ragged", seed=5)
    o = O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD
    with O.sum_mode(1):
        ws, vs = Cs.stores("fm", opt, k)
        fw, fv = F.stores(o, k, 7)
        audit = []
        for rowptr, keys, vals, labels in mbs:
            got = V.fm_step(ws, vs, rowptr, keys, np.ones_like(vals), labels, audit)
            want = F.step(fw, fv, rowptr, keys, labels)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and np.array_equal(a, b)
        for a, b in zip(ws.export() + vs.export(), fw.export() + fv.export()):
            assert np.array_equal(a, b)
        rowptr, keys, vals, labels = mbs[0]
        assert np.array_equal(V.fm_predict(ws, vs, rowptr, keys, np.ones_like(vals), labels, audit),
                              F.predict(fw, fv, rowptr, keys, labels))


def test_lr_checker_with_all_values_one_is_the_oracles_update():
    mbs = Cs.stream("zipf_heavy", seed=9)
    with O.sum_mode(1):
        for opt in Cs.OPTS:
            ws, _ = Cs.stores("lr", opt, 1)
            s = O.Store(O.OPT_FTRL if opt == "ftrl" else O.OPT_SGD, 1)
            for rowptr, keys, vals, labels in mbs:
                V.lr_step(ws, rowptr, keys, np.ones_like(vals), labels, [])
                O.lr_update(s, O.Batch(rowptr, keys, labels))
            for a, b in zip(ws.export(), s.export()):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("case", Cs.CASES)
def test_the_streams_of_the_gpu_tests_are_what_they_claim(case):
    mbs = Cs.stream(case)
    for rowptr, keys, vals, labels in mbs:
        mag = np.abs(vals[vals != 0])
        assert (vals == 0).any() and (vals < 0).any() and (vals > 0).any()
        assert mag.min() >= 2.0 ** -4 and mag.max() < 4.0
        nheavy, top = Cs.heavy_profile((rowptr, keys))
        if case == "ragged":
            assert (np.diff(rowptr.astype(np.int64)) == 0).any()
            a = int(rowptr[1])
            assert keys[a] == keys[a + 2] and vals[a] != vals[a + 2]
        elif case == "zipf_heavy":
            assert nheavy >= 5 and capi.HEAVY_SEG < top <= 2048
        else:
            assert top > 3 * 2048


@pytest.mark.parametrize("case", Cs.CASES)
@pytest.mark.parametrize("model,opt,k", [("lr", o, 1) for o in Cs.OPTS] +
                         [("fm", o, k) for o in Cs.OPTS for k in Cs.KS])
def test_every_sum_of_the_checker_is_exact_on_the_gpu_tests_streams(case, model, opt, k):
    """the condition under which the checker may judge the GPU: ascending and descending order
    agree for EVERY sum it forms over these inputs"""
    audit = []
    with O.sum_mode(1):
        Cs.run_checker(model, opt, k, Cs.stream(case), audit)
    V.assert_exact(audit)
    fams = set(V.disagreements(audit))
    assert {"wx", "gw"} <= fams and (model == "lr" or {"S", "Q over j", "Q over f", "T", "gv"} <= fams)


@pytest.mark.parametrize("model,opt,k", Cs.E2E)
def test_every_sum_of_the_checker_is_exact_on_the_golden_files(model, opt, k):
    audit = []
    Cs.run_checker_files(model, opt, k, os.path.join(GOLD, "small_train-00000"),
                         os.path.join(GOLD, "small_test-00000"), audit)
    V.assert_exact(audit)
