"""Row normalisation without a GPU: the host definition (xf_rownorm_row, csrc/xf_rownorm.h as host
code) against the numpy restatement tests/_rownorm_checker.py with ==, the restatement against a
plain recursive loop, the special rows, unit length, the refusals that need no device, and the
power-of-two recipe the GPU tests build their exact minibatches with."""
import ctypes as C
import math

import numpy as np
import pytest

from xflow_amd import capi

from . import _rownorm_checker as Rn

LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 5000)


@pytest.fixture(scope="module", autouse=True)
def built():
    from xflow_amd import build
    build.build(verbose=False)


def general_rows():
    rng = np.random.RandomState(17)
    return [Rn.general_values(rng, m) for m in LENGTHS]


@pytest.mark.parametrize("x", general_rows(), ids=["m%d" % m for m in LENGTHS])
def test_host_definition_equals_the_restatement(x):
    y, s = capi.rownorm_row(x)
    ey, es, scaled = Rn.row(x)
    assert s == es and Rn.same_bits(y, ey)
    assert scaled == (len(x) > 0 and bool(np.any(x != 0)))
    assert y.dtype == np.float32 and len(y) == len(x)


def test_general_rows_are_in_general_position():
    """mixed signs, exact zeros, both rare scales — and sums the order of whose addends matters"""
    x = np.concatenate(general_rows())
    assert (x < 0).any() and (x > 0).any() and (x == 0).sum() > len(x) // 20
    assert (np.abs(x[x != 0]) < 1e-4).any() and (np.abs(x) > 40).any()
    row = general_rows()[-1].astype(np.float64)
    assert Rn.sumsq(row) != np.float64(np.cumsum(row * row)[-1])     # not the left-to-right sum


@pytest.mark.parametrize("name,x", Rn.special_rows(), ids=[n for n, _ in Rn.special_rows()])
def test_special_rows(name, x):
    y, s = capi.rownorm_row(x)
    ey, es, scaled = Rn.row(x)
    assert Rn.same_sums([s], [es]) and Rn.same_bits(y, ey), name
    if name in ("zeros", "nan", "inf", "nan_and_inf"):
        assert not scaled and Rn.same_bits(y, x), name               # unchanged, bit for bit
        assert (s == 0 and not np.signbit(s)) if name == "zeros" else not np.isfinite(s)
    elif name.startswith("one_"):
        assert scaled and y.tolist() == [1.0 if x[0] > 0 else -1.0]
    elif name == "subnormals":
        assert scaled and 0 < s < 1e-70 and np.all(np.abs(y) <= 1) and np.abs(y).max() > 0.1
        assert abs(math.fsum(float(v) ** 2 for v in y) - 1.0) <= 2.0 ** -22
    elif name == "flt_max":
        assert scaled and np.isfinite(s) and s > 1e77                # finite in fp64
        assert abs(float(np.abs(y).max()) - 5 ** -0.5) < 1e-7 and 0 < abs(y[4]) < 1e-38


def test_the_restatement_equals_a_plain_recursive_loop():
    rows = general_rows() + [x for _, x in Rn.special_rows()[:5]]
    for x in rows:
        sq = [float(v) * float(v) for v in np.asarray(x, np.float32)]
        assert Rn.sumsq(x) == Rn.tree_loop(sq), len(x)
    # ... and the tree's shape by hand: five addends pad to eight
    a, b, c, d, e = (float(np.float32(v)) ** 2 for v in (1.1, 2.3, 3.7, 0.9, 5.3))
    x = np.array([1.1, 2.3, 3.7, 0.9, 5.3], np.float32)
    assert Rn.sumsq(x) == ((a + b) + (c + d)) + ((e + 0.0) + (0.0 + 0.0))


def test_a_scaled_row_has_unit_length():
    """every y_i is one fp32 rounding (relative error <= 2^-24) of an fp64 value whose relative
    error is below 2^-50: sum y_i^2 is within (1 + 2^-24 + 2^-50)^2 - 1 < 2^-22 of 1"""
    checked = 0
    for x in general_rows():
        y, s = capi.rownorm_row(x)
        nz = y[y != 0]
        if not Rn.scales(s) or (np.abs(nz) < np.finfo(np.float32).tiny).any():
            continue
        assert abs(math.fsum(float(v) * float(v) for v in y) - 1.0) <= 2.0 ** -22, len(x)
        assert np.all(np.abs(y) <= 1)
        checked += 1
    assert checked >= 12


def test_the_power_of_two_recipe_is_exact():
    """a values +-1 and b values +-2 with a + 4 b in {4, 16, 64}: s is the target, exactly, and
    the normalised values are exactly +-2^-k"""
    rng = np.random.RandomState(23)
    for target, k in ((4, 1), (16, 2), (64, 3)):
        for b in range(target // 4 + 1):
            x = Rn.recipe_row(rng, target, b)
            assert len(x) == target - 3 * b
            y, s = capi.rownorm_row(x)
            assert s == float(target)
            assert Rn.same_bits(y, x * np.float32(2.0 ** -k))
            assert set(np.abs(y).tolist()) <= {2.0 ** -k, 2.0 ** (1 - k)}
            assert Rn.same_bits(Rn.row(x)[0], y)


def test_in_place_and_sumsq_optional():
    x = general_rows()[8].copy()
    want, _ = capi.rownorm_row(x)
    capi.check(capi.lib().xf_rownorm_row(capi._p(x, capi.f32p), len(x), capi._p(x, capi.f32p),
                                         None))
    assert Rn.same_bits(x, want)


def test_refusals_that_need_no_device(tmp_path):
    L = capi.lib()
    h = capi.vp()
    for kind in (0, 2, -1):
        with pytest.raises(capi.XFError, match=r"xf_rownorm_create: kind must be XF_ROWNORM_L2"):
            capi.check(L.xf_rownorm_create(C.byref(h), kind))
        assert not h.value
    with pytest.raises(capi.XFError, match=r"xf_rownorm_create: out is NULL"):
        capi.check(L.xf_rownorm_create(None, capi.ROWNORM_L2))
    x = np.ones(3, np.float32)
    with pytest.raises(capi.XFError, match=r"xf_rownorm_row: x is NULL"):
        capi.check(L.xf_rownorm_row(None, 3, capi._p(x, capi.f32p), None))
    with pytest.raises(capi.XFError, match=r"xf_rownorm_row: y is NULL"):
        capi.check(L.xf_rownorm_row(capi._p(x, capi.f32p), 3, None, None))
    capi.check(L.xf_rownorm_row(None, 0, None, None))                 # an empty row needs no arrays
    with pytest.raises(capi.XFError, match=r"xf_rownorm_stats: the stage is NULL"):
        capi.check(L.xf_rownorm_stats(None, None, None))
    out = capi.vp()
    with pytest.raises(capi.XFError, match=r"xf_rownorm_apply_dev: the stage is NULL"):
        capi.check(L.xf_rownorm_apply_dev(None, None, None, 0, 0, None, C.byref(out), None))
    st = capi.RowNorm()                                               # (allocates nothing)
    with pytest.raises(capi.XFError, match=r"xf_rownorm_apply_dev: d_vals_out is NULL"):
        capi.check(L.xf_rownorm_apply_dev(st.h, None, None, 0, 0, None, None, None))
    assert st.stats() == (0, 0) and capi.RowNorm.shape() == (16, 16)
    # the worker's parameter
    x = capi.XFlow(str(tmp_path / "train"), str(tmp_path / "test"))
    with pytest.raises(capi.XFError, match=r"XFSetParam: row_norm must be l2 or off, not 'bogus'"):
        x.set("row_norm", "bogus")
    for v in ("l2", "off", "l2"):
        x.set("row_norm", v)
