"""The rule that picks the forward's own row windows of a kept minibatch's key-sorted copy
(xf::cells_fwd_windows, xf_batch.cc; xf_cells.h, DESIGN.md 3 "forward windows"), by itself: a host
function, no GPU.  tests/test_gpu_fwd_windows.py runs the path."""
import pytest

from xflow_amd import capi

WIN_MAX = 17408
DEFAULT = 8          # xf::kFwdWinDefault: the measured choice (profiles/fwd_windows/README.md)
BENCH = dict(R=50000, NNZ=10 ** 7, M=10 ** 7)


def rule(R, NNZ, M, **kw):
    return capi.fwd_windows_rule(R, NNZ, M, **kw)


def off(r):
    return r["nwin_f"] == r["nwin"]


def test_the_bench_shape_takes_the_default():
    r = rule(**BENCH)
    assert (r["nwin"], r["nwin_f"], r["W_f"], r["G_f"]) == (3, DEFAULT, 6250, 32)
    # 10^7 / (8 x 4883 cells) = 256 entries per forward cell


def test_a_sparse_table_stays_off():
    # 10^8 keys: 48 829 chunks, 68 entries per gradient cell today
    assert off(rule(50000, 10 ** 7, 10 ** 8))
    # 3 x 10^7: 85 entries per forward cell at 8 windows, under the 128 the rule asks for
    assert off(rule(50000, 10 ** 7, 3 * 10 ** 7))
    # either side of 128 entries per forward cell: 8 windows x 100 chunks x 128
    assert not off(rule(50000, 8 * 100 * 128, 100 * 2048))
    assert off(rule(50000, 8 * 100 * 128 - 1, 100 * 2048))
    # R of at most four windows with sparse cells, every window count
    for R in (17408, 34816, 52224, 69632):
        assert off(rule(R, 200 * R, 10 ** 8))


def test_what_stays_off():
    assert off(rule(kept=False, **BENCH))      # no key-sorted copy
    assert off(rule(w_fixed=True, **BENCH))    # row-id cells: the owner dataflow
    assert off(rule(valued=True, **BENCH))     # valued cells
    assert off(rule(tune=1, **BENCH))          # switched off
    assert off(rule(50000, 0, 10 ** 7))        # nothing to regroup
    # five or more gradient windows
    assert rule(4 * WIN_MAX, 200 * 4 * WIN_MAX, 10 ** 7)["nwin_f"] == DEFAULT
    for R in (4 * WIN_MAX + 1, 87041, 10 * WIN_MAX):
        assert off(rule(R, 200 * R, 10 ** 7)), R
    # a small minibatch: forward windows of fewer than 1024 rows
    assert off(rule(1024 * DEFAULT - DEFAULT, 10 ** 7, 10 ** 6))
    assert not off(rule(1024 * DEFAULT - DEFAULT + 1, 10 ** 7, 10 ** 6))
    assert off(rule(512, 512 * 40, 5000))      # the smoke run's


def test_forced_windows():
    for n in (2, 5, 6, 8, 16, 32):
        r = rule(tune=n, **BENCH)
        if n == 2:
            assert off(r)                       # 25 000 rows do not fit a window
        else:
            assert (r["nwin_f"], r["W_f"], r["G_f"]) == (n, -(-50000 // n), 32 // n * 8), r
    # whatever the density; still off without a copy to regroup
    assert rule(7, 7, 10 ** 8, tune=16)["nwin_f"] == 16
    assert off(rule(7, 7, 10 ** 8, tune=16, kept=False))
    assert off(rule(7, 7, 10 ** 8, tune=16, valued=True))
    assert off(rule(7, 7, 10 ** 8, tune=16, w_fixed=True))
    assert off(rule(50000, 10 ** 7, 10 ** 7, tune=3))    # the gradient's own count
    with pytest.raises(capi.XFError):
        capi.tune("fwd_windows", 33)
    with pytest.raises(capi.XFError):
        capi.tune("fwd_windows", 2.5)
    assert capi.lib().xf_tune(b"fwd_windows", 0.0) == 0


def test_groups_over_a_sweep_of_rows():
    """G_f is a multiple of 8 (the XCD placement of k_lr_fwd_cells) and nwin_f x G_f <= 256 (one
    forward workgroup per CU), W_f rows fit a window and the windows cover the rows — under the
    rule and under every forced count"""
    for R in list(range(1, 70)) + list(range(1000, 90000, 997)) + [WIN_MAX * k + d for k in
                                                                   range(1, 6) for d in (-1, 0, 1)]:
        for tune in (0, 2, 3, 5, 6, 7, 8, 16, 31, 32):
            r = rule(R, 200 * R, 10 ** 6, tune=tune)
            assert r["G_f"] % 8 == 0 and r["G_f"] >= 8, (R, tune, r)
            assert r["nwin"] == -(-R // WIN_MAX)
            assert r["W_f"] == max(1, -(-R // r["nwin_f"])) and r["W_f"] <= WIN_MAX, (R, tune, r)
            assert r["nwin_f"] * r["W_f"] >= R
            if not off(r):
                assert r["nwin_f"] * r["G_f"] <= 256, (R, tune, r)
                assert r["nwin_f"] == (tune if tune >= 2 else DEFAULT)
