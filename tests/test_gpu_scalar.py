"""The scalar layer of every forward and step — sigmoid_ref, sqrtf, the fp32 division, div_by_rows
(xf_device.h) — on a real MI355X against the host, on EVERY float: the 65536 digests of a full 2^32
sweep by the functions as the kernels call them (xf_scalar_sweep) must equal the oracle's
(xo_scalar_sweep: Base::sigmoid, the host's sqrtf, the reference's fp64 `/= 1.0 * rows`), `==`,
every NaN counted as one value and nothing else forgiven.  A digest that differs is taken apart
by the elementwise probe, so that the failure names the inputs.  Then the two-operand division on
2^24 pairs, the 22 floats at which the sigmoid hangs on the last two bits of pow
(tests/golden/sigmoid_fragile.npz; tests/test_scalar_cpu.py shows there are no others) one by one,
and the same 22 as row sums through the LR and FM forward kernels."""
import os

import numpy as np
import pytest

from oracle import pyoracle as O
from xflow_amd import capi

pytestmark = pytest.mark.gpu

NBLOCKS = 1 << 16
NAMES = {capi.SCALAR_SIGMOID: "sigmoid_ref", capi.SCALAR_SQRT: "sqrtf", capi.SCALAR_DIV: "a / b",
         capi.SCALAR_DIV_ROWS: "div_by_rows"}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.require_gpu()
    assert (capi.SCALAR_SIGMOID, capi.SCALAR_SQRT, capi.SCALAR_DIV, capi.SCALAR_DIV_ROWS) == \
        (O.SCALAR_SIGMOID, O.SCALAR_SQRT, O.SCALAR_DIV, O.SCALAR_DIV_ROWS)


def is_nan_bits(u):
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def differing(got, want):
    """indices at which two float32 arrays differ in their bits, a NaN equal to any NaN"""
    g, w = got.view(np.uint32), want.view(np.uint32)
    return np.flatnonzero((g != w) & ~(is_nan_bits(g) & is_nan_bits(w)))


def report(op, param, a, b, got, want, idx, limit=12):
    lines = []
    for i in idx[:limit]:
        arg = "%08x" % a.view(np.uint32)[i] + (", %08x" % b.view(np.uint32)[i] if b is not None
                                               else "")
        lines.append("%s(%s): device %08x, host %08x" % (
            NAMES[op], arg, got.view(np.uint32)[i], want.view(np.uint32)[i]))
    return "%s%s: %d inputs differ\n  %s" % (
        NAMES[op], " by %d rows" % param if op == capi.SCALAR_DIV_ROWS else "", len(idx),
        "\n  ".join(lines))


def sweep_equals_host(op, param=0):
    """all 2^32 inputs: one launch, one host sweep, 65536 digests each"""
    dev = capi.scalar_sweep(op, param)
    host = O.scalar_sweep(op, param, 0, NBLOCKS, O.sweep_threads())
    bad = np.flatnonzero(dev != host)
    if bad.size == 0:
        return
    found = []
    for blk in bad[:8]:     # name the inputs: the elementwise probe on the first differing blocks
        a = (np.arange(65536, dtype=np.uint32) + np.uint32(int(blk) << 16)).view(np.float32)
        got, want = capi.scalar_probe(op, a, None, param), O.scalar_ref(op, a, None, param)
        idx = differing(got, want)
        found.append(report(op, param, a, None, got, want, idx) if idx.size else
                     "block %#06x: the digests differ, the elementwise probe does not" % blk)
    pytest.fail("%d of %d blocks differ (the first: %s)\n%s" % (
        bad.size, NBLOCKS, ", ".join("%#06x" % b for b in bad[:8]), "\n".join(found)))


def test_sweep_plumbing_a_few_blocks_against_the_elementwise_probe():
    """the device's digest of a block is the digest of the device's elementwise answers (the host
    side of the same statement: tests/test_scalar_cpu.py), for a run of blocks that does not start
    at 0 — and the sweep refuses blocks that do not exist and the op it has no sweep for"""
    from .test_scalar_cpu import block_inputs, digest
    for op, param in ((capi.SCALAR_SIGMOID, 0), (capi.SCALAR_SQRT, 0),
                      (capi.SCALAR_DIV_ROWS, (1 << 24) + 1)):
        run = capi.scalar_sweep(op, param, 0x7FFE, 4)        # 0x7ffe .. 0x8001
        for j, blk in enumerate(range(0x7FFE, 0x8002)):
            bits = block_inputs(blk)
            out = capi.scalar_probe(op, bits.view(np.float32), None, param)
            assert int(run[j]) == digest(bits, out.view(np.uint32)), (op, hex(blk))
    assert capi.scalar_sweep(capi.SCALAR_SQRT, 0, NBLOCKS, 0).size == 0
    for args in ((capi.SCALAR_SQRT, 0, NBLOCKS - 1, 2), (capi.SCALAR_DIV, 0, 0, 1),
                 (capi.SCALAR_DIV_ROWS, 0, 0, 1), (7, 0, 0, 1)):
        with pytest.raises(capi.XFError):
            capi.scalar_sweep(*args)


def test_sigmoid_of_every_float():
    """sigmoid_ref against Base::sigmoid as the host computes it: the device library's double pow
    under one fp64 division and one rounding, the clamps at -30 and 30 and the floats either side
    of them, +-0, +-inf, NaN"""
    sweep_equals_host(capi.SCALAR_SIGMOID)


def test_sqrt_of_every_float():
    """sqrtf as the FTRL step calls it: correctly rounded, subnormal inputs and results kept,
    -0 -> -0, negative -> NaN"""
    sweep_equals_host(capi.SCALAR_SQRT)


@pytest.mark.parametrize("rows", [1, 3, 50000, (1 << 24) - 1, 1 << 24, (1 << 24) + 1,
                                  (1 << 32) - 1])
def test_every_float_divided_by_a_row_count(rows):
    """div_by_rows against the reference's `float /= 1.0 * rows`: the fp32 division below 2^24
    rows, the fp64 one from there on (2^24 + 1 is not a float)"""
    sweep_equals_host(capi.SCALAR_DIV_ROWS, rows)


def division_pairs(n=1 << 24):
    """n (dividend, divisor) pairs: any bit patterns; quotients from 2^-151 to 2^-124 — subnormal,
    or within a binade of FLT_MIN; quotients that are exact midpoints of two subnormals; every pair
    of +-0, +-inf, NaN, the smallest and largest subnormal and normal numbers and 1"""
    rng = np.random.RandomState(20261020)

    def bits(m):
        return rng.randint(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    sp = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 1, 0x80000001,
                   0x007FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000,
                   0xBF800000], np.uint32)
    a4, b4 = [g.ravel() for g in np.meshgrid(sp, sp)]
    # exact midpoints: d an even integer below 2^24, x = (2 j + 1) (d / 2) 2^-149 < 2^-125
    m3 = 1 << 20
    half = rng.randint(1, 1 << 22, m3).astype(np.int64)
    odd = 2 * (rng.randint(0, 1 << 23, m3).astype(np.int64) % ((1 << 23) // half)) + 1
    a3 = (odd * half).astype(np.uint32)         # the integer N < 2^24 is the bits of N 2^-149
    b3 = (2 * half).astype(np.float32).view(np.uint32)
    sign3 = bits(m3)
    a3 |= sign3 & np.uint32(0x80000000)
    b3 |= (sign3 << np.uint32(1)) & np.uint32(0x80000000)
    a3[0], b3[0] = 25000, np.float32(50000).view(np.uint32)
    # small quotients: full mantissas, exponents 125 .. 150 apart
    m2 = 1 << 22
    ea = rng.randint(1, 101, m2).astype(np.uint32)
    eb = ea + rng.randint(125, 151, m2).astype(np.uint32)
    a2 = (bits(m2) & np.uint32(0x807FFFFF)) | (ea << np.uint32(23))
    b2 = (bits(m2) & np.uint32(0x807FFFFF)) | (eb << np.uint32(23))
    m1 = n - m2 - m3 - a4.size
    a = np.concatenate([bits(m1), a2, a3, a4]).view(np.float32)
    b = np.concatenate([bits(m1), b2, b3, b4]).view(np.float32)
    assert a.size == b.size == n
    return a, b


def test_fp32_division_on_2_to_the_24_pairs():
    """a / b in a kernel against a / b on the host"""
    a, b = division_pairs()
    want = O.scalar_ref(O.SCALAR_DIV, a, b)
    w = np.abs(want[(1 << 24) - (1 << 22) - (1 << 20) - 225:])
    small, mid = w[:1 << 22], w[1 << 22:(1 << 22) + (1 << 20)]
    assert small.max() < 2.0 ** -124 and (small < 2.0 ** -126).mean() > 0.5   # the strata are
    assert mid.max() < 2.0 ** -125 and want[-225 - (1 << 20)] == 0.0          # what they say:
    #                                                      25000 2^-149 / 50000 ties to even, 0
    got = capi.scalar_probe(capi.SCALAR_DIV, a, b)
    idx = differing(got, want)
    assert idx.size == 0, report(capi.SCALAR_DIV, 0, a, b, got, want, idx)


@pytest.fixture(scope="module")
def fragile(golden_dir):
    g = np.load(os.path.join(golden_dir, "sigmoid_fragile.npz"))
    return g["inputs"].view(np.float32).ravel(), g["host"].ravel()


def test_sigmoid_at_the_inputs_that_hang_on_the_last_bits_of_pow(fragile):
    """the 22 floats at which a pow one or two units off in its last place gives another float,
    and the floats next to them, against the recorded answers of the real Base::sigmoid"""
    x, want = fragile
    got = capi.scalar_probe(capi.SCALAR_SIGMOID, x)
    idx = differing(got, want)
    assert idx.size == 0, report(capi.SCALAR_SIGMOID, 0, x, None, got, want, idx, limit=66)


def test_fragile_row_sums_through_the_forward_kernels(fragile):
    """where the product would show it: each of the 66 floats is the weight of a key of its own
    and the only key of a row, so it is that row's sum; the pctr of xf_lr_predict on a generic and
    on a local (cells) minibatch and of xf_fm_predict with k = 1 and a zero v is the host's
    sigmoid of it, bit for bit"""
    x, want = fragile
    assert np.array_equal(np.array([O.sigmoid(v) for v in x], np.float32).view(np.uint32),
                          want.view(np.uint32))
    keys = np.array([capi.hash_str("fragile %d" % i) for i in range(x.size)], np.uint64)
    rowptr = np.arange(x.size + 1, dtype=np.uint64)
    labels = np.zeros(x.size, np.int32)
    tw = capi.Table(capi.OPT_SGD, 1, capacity=1 << 12)
    tv = capi.Table(capi.OPT_SGD, 1, capi.INIT_ZERO, capacity=1 << 12)
    tw.import_(keys, x)
    ws = capi.Workspace()
    paths = [("xf_lr_predict, generic", lambda: capi.lr_predict(
                 tw, capi.Batch(rowptr, keys, labels), ws)),
             ("xf_lr_predict, local", lambda: capi.lr_predict(
                 tw, capi.LocalBatch(tw, rowptr, keys, labels), ws)),
             ("xf_fm_predict, k = 1", lambda: capi.fm_predict(
                 tw, tv, capi.Batch(rowptr, keys, labels), ws))]
    for name, run in paths:
        got = run()
        idx = differing(got, want)
        assert idx.size == 0, name + ": " + report(capi.SCALAR_SIGMOID, 0, x, None, got, want,
                                                   idx, limit=66)
    assert not tv.export()[1].view(np.uint32).any()     # the v the FM forward read: +0
