"""Feature crosses without a GPU: the numpy restatement (tests/_cross_checker.py) against a loop in
plain Python ints, the library's key function against both and against the known answers, the
spec's parser with every refusal, and the worker's refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

from xflow_amd import capi

from . import _cross_checker as X

MASK = (1 << 64) - 1

KNOWN = [
    (0, 0, 0, 1, 0xb18a02f46d8d86c3),
    (1, 2, 3, 4, 0x9e115e4b8512df01),
    (2, 1, 3, 4, 0x2ab13db52cdaf5f3),
    (1, 2, 4, 3, 0x9ad29f2584d7d0f9),
    (MASK, MASK, 2147483647, 0, 0x6597064ef50b7085),
    (0x0123456789abcdef, 0xfedcba9876543210, 17, 16, 0x3d29a0d61dd42f35),
]


def _py_mix64(x):
    x = (x + 0x9e3779b97f4a7c15) & MASK
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def _py_cross_key(ka, kb, fa, fb):
    s = _py_mix64(((fa & 0xffffffff) << 32) | (fb & 0xffffffff))
    return _py_mix64((_py_mix64(ka ^ s) + kb) & MASK)


def _py_cross(pairs, base, rowptr, keys, fgid, vals):
    """the definition, nonzero by nonzero"""
    orp, ok, ofg, ov = [0], [], [], []
    for r in range(len(rowptr) - 1):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        for i in range(a, b):
            ok.append(int(keys[i]))
            ofg.append(int(fgid[i]))
            ov.append(np.float32(vals[i]))
        for p, (fa, fb) in enumerate(pairs):
            for i in range(a, b):
                if fgid[i] != fa:
                    continue
                for j in range(a, b):
                    if fgid[j] != fb:
                        continue
                    ok.append(_py_cross_key(int(keys[i]), int(keys[j]), fa, fb))
                    ofg.append(base + p)
                    ov.append(np.float32(vals[i]) * np.float32(vals[j]))
        orp.append(len(ok))
    return (np.array(orp, np.uint32), np.array(ok, np.uint64), np.array(ofg, np.int32),
            np.array(ov, np.float32))


# ------------------------------------------------------------------ the key
def test_known_answers():
    for ka, kb, fa, fb, want in KNOWN:
        assert _py_cross_key(ka, kb, fa, fb) == want
        assert int(X.cross_key(np.uint64(ka), np.uint64(kb), fa, fb)) == want
        assert capi.cross_key(ka, kb, fa, fb) == want, (ka, kb, fa, fb)


def test_key_function_equals_the_restatement():
    rng = np.random.RandomState(11)
    ka = rng.randint(0, 1 << 62, size=500).astype(np.uint64) * np.uint64(4) + np.uint64(1)
    kb = rng.randint(0, 1 << 62, size=500).astype(np.uint64) * np.uint64(4) + np.uint64(2)
    for fa, fb in ((0, 1), (1, 0), (2, 3), (2147483647, 5), (5, 2147483647), (16, 17)):
        want = X.cross_key(ka, kb, fa, fb)
        got = np.array([capi.cross_key(int(a), int(b), fa, fb) for a, b in zip(ka, kb)], np.uint64)
        assert np.array_equal(got, want), (fa, fb)
        assert got[0] == _py_cross_key(int(ka[0]), int(kb[0]), fa, fb)
    # the two field ids matter, and so does which key is on which side
    assert capi.cross_key(1, 2, 3, 4) != capi.cross_key(2, 1, 3, 4) != capi.cross_key(1, 2, 4, 3)


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_against_a_plain_loop(seed):
    rng = np.random.RandomState(seed)
    R = 40
    lens = rng.randint(0, 9, size=R)
    lens[[0, 7, R - 1]] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nnz = int(rowptr[-1])
    keys = rng.randint(0, 1 << 40, size=nnz).astype(np.uint64)
    fgid = rng.randint(0, 5, size=nnz).astype(np.int32)     # few fields: multi-valued ones
    vals = (rng.rand(nnz) * 4 - 2).astype(np.float32)
    pairs, base = [(0, 1), (1, 0), (2, 4), (0, 3), (7, 1)], 9
    chk = X.Cross(pairs, base)
    got = chk.apply(rowptr, keys, fgid, vals)
    want = _py_cross(pairs, base, rowptr, keys, fgid, vals)
    for g, w, name in zip(got, want, ("rowptr", "keys", "fgid", "values")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    rows, nin, ncross = chk.stats()
    assert (rows, nin) == (R, nnz) and ncross == len(got[1]) - nnz and ncross > nnz // 2
    multi = [r for r in range(R) if (fgid[int(rowptr[r]):int(rowptr[r + 1])] == 0).sum() > 1]
    assert multi, "a multi-valued field"
    # without values none come out; the rest is the same
    again = X.Cross(pairs, base).apply(rowptr, keys, fgid)
    assert again[3] is None and all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], got[:3]))


def test_restatement_identity_and_string_spec():
    rowptr = np.array([0, 2, 2, 5], np.uint64)
    keys = np.arange(5, dtype=np.uint64) + np.uint64(100)
    fgid = np.array([0, 1, 2, 0, 1], np.int32)
    vals = np.arange(5, dtype=np.float32)
    got = X.Cross("7*8,9*7").apply(rowptr, keys, fgid, vals)
    for g, w in zip(got, (rowptr.astype(np.uint32), keys, fgid, vals)):
        assert g.tobytes() == w.tobytes()
    assert X.parse("2*3,16*17") == [(2, 3), (16, 17)]


# ------------------------------------------------------------------ the parser
GOOD = ["2*3", "2*3,16*17", "0*2147483647", "3*2,2*3",
        ",".join("%d*%d" % (p, p + 1) for p in range(32))]


@pytest.mark.parametrize("spec", GOOD, ids=["one", "two", "ends", "both_orders", "32_pairs"])
def test_parse_and_params_round_trip(spec):
    pairs = capi.cross_parse(spec)
    assert pairs == X.parse(spec) and 1 <= len(pairs) <= 32
    for base in (0, 5):
        for arg in (spec, pairs):
            assert capi.Cross(arg, fgid_base=base).params() == (pairs, base)
    assert capi.Cross(spec).stats() == (0, 0, 0)


BAD = [
    ("", "empty"),
    ("2*2", "'2*2'"),
    ("2*3,2*3", "'2*3'"),
    (",".join("%d*%d" % (p, p + 1) for p in range(33)), "'32*33'"),
    ("2x3", "'2x3'"),
    ("2*", "'2*'"),
    ("-1*3", "'-1*3'"),
    ("2*2147483648", "'2*2147483648'"),
    ("2*3, 4*5", "' 4*5'"),
    ("2 *3", "'2 *3'"),
    ("2*3,", "''"),
    (",2*3", "''"),
    ("2*3*4", "'2*3*4'"),
    ("2*+3", "'2*+3'"),
]


@pytest.mark.parametrize("spec,piece", BAD, ids=[
    "empty", "self", "twice", "33_pairs", "x", "no_b", "negative", "2^31", "blank", "blank2",
    "trailing_comma", "leading_comma", "three", "sign"])
def test_parse_refuses_and_names_the_piece(spec, piece):
    with pytest.raises(capi.XFError) as e:
        capi.cross_parse(spec)
    assert "xf_cross_parse" in str(e.value) and piece in str(e.value), str(e.value)
    with pytest.raises(capi.XFError):
        capi.Cross(spec)


@pytest.mark.parametrize("pairs,base,word", [
    ([], 0, "1 .. 32 pairs"),
    ([(p, p + 1) for p in range(33)], 0, "1 .. 32 pairs"),
    ([(2, 2)], 0, "2*2"),
    ([(2, 3), (4, 5), (2, 3)], 0, "2*3"),
    ([(-1, 3)], 0, "-1*3"),
    ([(2, 3)], -1, "cross_fgid_base=-1"),
    ([(2, 3), (3, 2)], 2147483647, "cross_fgid_base=2147483647"),
], ids=["none", "33", "self", "twice", "negative", "base<0", "base_too_high"])
def test_create_refuses_a_bad_spec(pairs, base, word):
    with pytest.raises(capi.XFError) as e:
        capi.Cross(pairs, fgid_base=base)
    assert "xf_cross_create" in str(e.value) and word in str(e.value), str(e.value)


def test_create_takes_the_highest_base():
    assert capi.Cross([(2, 3)], fgid_base=2147483647).params() == ([(2, 3)], 2147483647)


# ------------------------------------------------------------------ the worker's refusals
def _start(**params):
    """XFStartTrain through the C ABI itself (capi.XFlow.train asks for a GPU first)"""
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode(), x


def test_the_parameters_and_the_metrics_are_accepted():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", cross="2*3,16*17",
                   cross_fgid_base=4)
    assert x.metric("cross_in") == 0 and x.metric("cross_out") == 0


@pytest.mark.parametrize("params,words", [
    (dict(cross="2*3", core_num=2), ["cross=2*3", "core_num=2"]),
    (dict(cross="2*3", key_build="host"), ["cross=2*3", "key_build=host"]),
    (dict(cross="2*3", parity="reference_order"), ["cross=2*3", "parity=reference_order"]),
    (dict(cross="2*3", ingest="gpu"), ["cross=2*3", "ingest=gpu", "ingest=gpu_fields"]),
    (dict(cross="2x3"), ["xf_cross_parse", "'2x3'"]),
    (dict(cross="2*3,2*3"), ["xf_cross_parse", "'2*3'", "twice"]),
    (dict(cross="2*3,16*17", cross_fgid_base=17, model=1, fm_mode="field_aware", fields=18),
     ["cross_fgid_base=17", "2 pairs", "fields >= 19", "fields=18"]),
], ids=["core_num", "key_build", "parity", "ingest", "malformed", "twice", "fields"])
def test_refusals_name_their_parameter(params, words):
    rc, msg, _ = _start(**params)
    assert rc != 0
    for w in words:
        assert w in msg, (w, msg)


def test_the_refusals_come_before_any_rendezvous():
    """world=2 with nobody to meet: a refusal returns at once instead of waiting for a peer"""
    rc, msg, _ = _start(cross="2*3", core_num=2, world=2, rank=0)
    assert rc != 0 and "core_num=2" in msg
