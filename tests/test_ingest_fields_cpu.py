"""ingest=gpu_fields without a GPU: the parameter, the refusals that stay with ingest=gpu, and the
two token classes of the GPU tokeniser's field modes (tests/_ingest_fields_cases.py) against the
host parser on this machine — for every token inside them the host parser yields
float32(+-m / 10^nf) and the decimal fgid, which is what the kernel computes."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

from xflow_amd import capi

from . import _ingest_fields_cases as cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _start(**params):
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test", **params)
    rc = capi.lib().XFStartTrain(C.byref(x.h))
    return rc, capi.lib().xf_last_error().decode()


def test_the_parameter_value_gpu_fields():
    x = capi.XFlow("/nonexistent/train", "/nonexistent/test")
    for v in ("gpu_fields", "gpu", "host", "gpu_fields"):
        x.set("ingest", v)
    rc = capi.lib().XFSetParam(x.h, b"ingest", b"bogus")
    assert rc == capi.XF_OK + 1                        # XF_EINVAL
    msg = capi.lib().xf_last_error().decode()
    assert re.search(r"\bgpu\b", msg) and "gpu_fields" in msg and "host" in msg, msg


@pytest.mark.parametrize("params", [
    dict(model=0, feature_values="on"),
    dict(model=1, k=4, fm_mode="canonical", feature_values="on"),
    dict(model=1, k=4, fm_mode="field_aware", fields=18),
    dict(model=1, k=4, fm_mode="field_aware", fields=18, feature_values="on"),
])
def test_gpu_fields_is_not_refused_where_gpu_is(params):
    t0 = time.time()
    rc, msg = _start(ingest="gpu_fields", **params)
    # (whatever a machine without a GPU, or without the file, says: it is not about the ingest)
    assert rc != capi.XF_OK and "ingest" not in msg, (rc, msg)
    rc, msg = _start(ingest="gpu", **params)
    assert rc == capi.XF_OK + 1, (rc, msg)
    assert re.search(r"ingest=gpu.*(fgid|values)", msg) and "gpu_fields" in msg, msg
    assert time.time() - t0 < 10


def test_capi_names_the_new_entry_points():
    L = capi.lib()
    assert L.xf_ingest_set_fields and L.xf_ingest_fields
    assert hasattr(capi.Ingest, "fields") and hasattr(capi.Ingest, "block_fields")


@pytest.fixture(scope="module")
def generated():
    return cases.gen_fields_text(3, 96 << 10)


def test_the_generator_covers_the_classes(generated):
    text, fg, vs = generated
    vals = [t.split(b":", 2)[2] for ln in text.split(b"\n")[:-1]
            for t in ln.rstrip(b"\r").split(b"\t")[1].split(b" ")]
    f0 = [t.split(b":")[0] for ln in text.split(b"\n")[:-1] for t in ln.split(b"\t")[1].split(b" ")]
    nd = {sum(c in b"0123456789" for c in v) for v in vals}
    nf = {len(v.split(b".")[1]) if b"." in v else 0 for v in vals}
    assert nd == set(range(0, 16)) and nf == set(range(0, 16))
    assert all(re.fullmatch(rb"(-?\d*\.?\d*)", v) and len(v) <= 17 for v in vals)
    for s in (b"-0", b".5", b"5.", b"000.100", b"999999999999999", b".000000000000001", b""):
        assert s in vals, s
    assert any(v.startswith(b"-") for v in vals)
    assert {len(f) for f in f0} == set(range(1, 10)) and all(f.isdigit() for f in f0)
    assert b"000000000" in f0 and b"999999999" in f0
    assert text.count(b"\r\n") > 10 and len(vals) == len(fg) == len(vs)


def test_host_parser_yields_the_class_values(generated):
    """the description of the two classes — float32(+-m / 10^nf), the decimal fgid — IS the host
    parser's result, bit for bit (-0.0 and +0.0 differ)"""
    text, fg, vs = generated
    rp, ks, hfg, lb, hvs = capi.parse_text_block(text, values=True)
    assert len(lb) == text.count(b"\n") and rp[-1] == len(ks) == len(fg)
    assert np.array_equal(hfg, fg)
    assert np.array_equal(hvs.view(np.uint32), vs.view(np.uint32))
    assert hvs.dtype == np.float32 and np.signbit(hvs[vs == 0]).any()
    # the default return is unchanged
    four = capi.parse_text_block(text)
    assert len(four) == 4 and all(np.array_equal(a, b) for a, b in zip(four, (rp, ks, hfg, lb)))
    # prefixes and the text without its last newline are the same tokens
    for cut in (text[:-1], text[:text.index(b"\n") + 1]):
        n = len(cut.replace(b"\t", b" ").split(b" ")) - 1
        out = capi.parse_text_block(cut, values=True)
        assert np.array_equal(out[4].view(np.uint32), vs[:len(out[4])].view(np.uint32))
        assert len(out[1]) == n


def test_defects_are_outside_and_the_host_still_reads_them():
    """every listed defect fails the class's pattern; the host parser takes each of them (atof,
    which refuses only nan and inf)"""
    for v in cases.VALUE_DEFECTS:
        digits = sum(c in b"0123456789" for c in v)
        assert not (re.fullmatch(rb"-?\d*\.?\d*", v) and 1 <= digits <= 15), v
        line = b"0\t1:22:" + v + b" 3:4:1\n"
        if v in (b"nan", b"inf"):                  # (a value that is not finite is a parse error)
            with pytest.raises(capi.XFError, match="not finite"):
                capi.parse_text_block(line, values=True)
        else:
            assert len(capi.parse_text_block(line, values=True)[1]) == 2
        assert len(capi.parse_text_block(line)[1]) == 2
    for f in cases.FIELD0_DEFECTS:
        assert not re.fullmatch(rb"\d{1,9}", f), f
        assert len(capi.parse_text_block(b"0\t" + f + b":22:0.5 3:4:1\n", values=True)[1]) == 2
    out = capi.parse_text_block(b"0\t1:2:" + cases.SIXTEEN_DIGITS + b"\n", values=True)
    assert out[4][0] == np.float32(1e-15)


@pytest.mark.parametrize("name,tokens", [("small_train-00000", 3508), ("small_test-00000", 3500)])
def test_the_sample_files_are_inside_both_classes(name, tokens):
    text = open(os.path.join(GOLD, name), "rb").read()
    lines = text.split(b"\n")
    lines = lines[:-1] if lines[-1] == b"" else lines
    toks = [t for ln in lines for t in ln.split(b"\t")[1].split(b" ")]
    assert len(lines) == 200 and len(toks) == tokens
    assert sum(ln.endswith(b"\r") for ln in lines) == 200
    f0 = [t.split(b":")[0] for t in toks]
    vals = [t.split(b":", 2)[2].rstrip(b"\r") for t in toks]
    assert all(re.fullmatch(rb"\d{1,9}", f) for f in f0) and max(int(f) for f in f0) == 17
    assert all(re.fullmatch(rb"-?\d*\.?\d*", v) and 1 <= sum(c in b"0123456789" for c in v) <= 15
               for v in vals)
    assert {len(v) for v in vals} <= {6, 7}


def test_pad_line_has_the_length_asked_for():
    for n in list(range(8, 120)) + [4000]:
        ln = cases.pad_line(n)
        assert len(ln) == n and len(capi.parse_text_block(ln)[3]) == 1
