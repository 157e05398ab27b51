"""The host side of the scalar-layer sweeps (tests/test_gpu_scalar.py compares the GPU's
sigmoid_ref, sqrtf, fp32 division and div_by_rows with the oracle on every float): that the oracle's
digests are what they claim to be, that the list of floats at which the sigmoid hangs on the last
bits of pow (tests/golden/sigmoid_fragile.npz) is complete, that glibc's pow is correctly rounded at
those — which is what makes the host the side to follow there —, and div_by_rows' argument on the
host: below 2^24 rows the fp32 quotient IS the reference's fp64 quotient rounded back, for every
float."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O


def mix64(x):
    """splitmix64's finaliser on a uint64 array (xf_device.h: mix64)"""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def block_inputs(block):
    """the 65536 floats of a sweep block, as bit patterns"""
    return np.arange(65536, dtype=np.uint32) + np.uint32(block << 16)


def is_nan_bits(u):
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def digest(bits, out_bits):
    """one block's digest from its inputs' and outputs' bit patterns"""
    r = np.where(is_nan_bits(out_bits), np.uint32(0x7FC00000), out_bits)
    with np.errstate(over="ignore"):
        return int(mix64(bits.astype(np.uint64) << np.uint64(32) | r.astype(np.uint64))
                   .sum(dtype=np.uint64))


# blocks that hold +0 and the positive subnormals, the last subnormals and the first normals, 0.5,
# 30 and the first float above it, inf and the NaNs after it, quiet NaNs, and the same below zero
BLOCKS = [0x0000, 0x007F, 0x0080, 0x3F00, 0x41F0, 0x7F80, 0x7FC0, 0x7FFF,
          0x8000, 0x807F, 0xBF00, 0xC1F0, 0xFF80, 0xFFC0, 0xFFFF]
CASES = [(O.SCALAR_SIGMOID, 0), (O.SCALAR_SQRT, 0), (O.SCALAR_DIV_ROWS, 3),
         (O.SCALAR_DIV_ROWS, (1 << 24) + 1)]


@pytest.mark.parametrize("op,param", CASES)
def test_sweep_digests_are_the_sum_over_the_block_of_the_elementwise_answers(op, param):
    """xo_scalar_sweep against a numpy recomputation from xo_scalar_ref, on several threads and on
    one, whole runs of blocks and single ones"""
    want = []
    for blk in BLOCKS:
        bits = block_inputs(blk)
        out = O.scalar_ref(op, bits.view(np.float32), None, param)
        want.append(digest(bits, out.view(np.uint32)))
        assert int(O.scalar_sweep(op, param, blk, 1, 3)[0]) == want[-1], hex(blk)
    run = O.scalar_sweep(op, param, 0x7F80, 0x81, 4)    # 0x7f80 .. 0x8000, across the sign
    assert int(run[0]) == want[BLOCKS.index(0x7F80)]
    assert int(run[0x40]) == want[BLOCKS.index(0x7FC0)]
    assert int(run[0x7F]) == want[BLOCKS.index(0x7FFF)]
    assert int(run[0x80]) == want[BLOCKS.index(0x8000)]
    assert np.array_equal(run, O.scalar_sweep(op, param, 0x7F80, 0x81, 1))
    assert len(set(want)) == len(want)


def test_nan_sign_and_payload_do_not_reach_a_digest_and_nothing_else_is_forgiven():
    bits = block_inputs(0xFFC0)
    out = O.scalar_ref(O.SCALAR_SQRT, bits.view(np.float32)).view(np.uint32)
    assert is_nan_bits(out).all()
    d = digest(bits, out)
    assert digest(bits, out ^ np.uint32(0x80000000)) == d
    assert digest(bits, np.full_like(out, 0x7F800001)) == d
    bits = block_inputs(0x3F00)
    out = O.scalar_ref(O.SCALAR_SQRT, bits.view(np.float32)).view(np.uint32)
    one_off = out.copy()
    one_off[12345] ^= np.uint32(1)
    assert digest(bits, one_off) != digest(bits, out)
    zero_sign = O.scalar_ref(O.SCALAR_SQRT, np.array([-0.0, 0.0], np.float32)).view(np.uint32)
    assert zero_sign.tolist() == [0x80000000, 0]


def test_elementwise_answers_are_the_plain_host_operations():
    """xo_scalar_ref against numpy's correctly rounded float32 sqrt and division, the fp64
    division rounded back, and xo_sigmoid"""
    rng = np.random.RandomState(5)
    a = np.concatenate([rng.randint(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32),
                        block_inputs(0x0000)[:64], block_inputs(0x8000)[:64],
                        np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x00800000, 0x007FFFFF],
                                 np.uint32)]).view(np.float32)
    b = rng.randint(0, 1 << 32, a.size, dtype=np.uint64).astype(np.uint32).view(np.float32)

    def same(got, want):
        g, w = got.view(np.uint32), want.view(np.uint32)
        assert np.array_equal(g[~is_nan_bits(w)], w[~is_nan_bits(w)])
        assert is_nan_bits(g[is_nan_bits(w)]).all()
    with np.errstate(all="ignore"):
        same(O.scalar_ref(O.SCALAR_SQRT, a), np.sqrt(a))
        same(O.scalar_ref(O.SCALAR_DIV, a, b), a / b)
        for R in (1, 3, 50000, (1 << 24) + 1, (1 << 32) - 1):
            same(O.scalar_ref(O.SCALAR_DIV_ROWS, a, None, R),
                 (a.astype(np.float64) / np.float64(R)).astype(np.float32))
    x = a[:2000]
    same(O.scalar_ref(O.SCALAR_SIGMOID, x), np.array([O.sigmoid(v) for v in x], np.float32))
    edge = np.array([30.0, -30.0], np.float32).view(np.uint32)
    edge = np.concatenate([edge - np.uint32(1), edge, edge + np.uint32(1)]).view(np.float32)
    assert O.scalar_ref(O.SCALAR_SIGMOID, edge).view(np.uint32).tolist() == \
        [np.float32(O.sigmoid(v)).view(np.uint32) for v in edge]
    assert O.scalar_ref(O.SCALAR_SIGMOID, edge)[2] == 1.0             # first float above 30
    assert O.scalar_ref(O.SCALAR_SIGMOID, edge)[5] == np.float32(1e-6)  # first float below -30


@pytest.fixture(scope="module")
def fragile(golden_dir):
    g = np.load(os.path.join(golden_dir, "sigmoid_fragile.npz"))
    return {k: g[k] for k in ("bits", "inputs", "host", "fragile1")}


def test_fragile_fixture_holds_the_hosts_answers(fragile):
    """22 inputs, 12 of them flagged, each with the float below and above; the recorded answers
    are the oracle's, and the real Base::sigmoid's where oracle/_ref is built"""
    bits, inputs, host = fragile["bits"], fragile["inputs"], fragile["host"]
    assert bits.shape == (22,) and inputs.shape == host.shape == (22, 3)
    assert fragile["fragile1"].sum() == 12 and len(set(bits.tolist())) == 22
    assert np.array_equal(inputs[:, 1], bits)
    assert np.array_equal(inputs[:, 0] + np.uint32(1), bits)
    assert np.array_equal(inputs[:, 2] - np.uint32(1), bits)
    assert np.all(np.abs(bits.view(np.float32)) < 3.3e-6)
    got = O.scalar_ref(O.SCALAR_SIGMOID, inputs.view(np.float32).ravel()).reshape(host.shape)
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))
    if O.ref_available():
        import ctypes
        live = np.array([O.ref().ref_sigmoid(ctypes.c_float(x))
                         for x in inputs.view(np.float32).ravel()], np.float32)
        assert np.array_equal(live.view(np.uint32), host.view(np.uint32).ravel())


def test_fragile_set_is_complete(fragile):
    """every float with |x| <= 30, pow's result moved by 1 and by 2 units in the last place either
    way: the sigmoid changes at the fixture's 22 inputs and nowhere else, and under a move of one
    unit at its 12 flagged ones"""
    bits, ulp = O.sigmoid_fragile(2, O.sweep_threads())
    assert sorted(bits.tolist()) == sorted(fragile["bits"].tolist()), \
        [hex(b) for b in bits]
    assert sorted(bits[ulp == 1].tolist()) == \
        sorted(fragile["bits"][fragile["fragile1"]].tolist())
    assert set(ulp.tolist()) == {1, 2}


def test_host_pow_is_correctly_rounded_at_the_fragile_inputs(fragile):
    """glibc's pow(2.718281828, x) at the 22 inputs against a 200-bit evaluation rounded to double:
    a device pow good to one unit in the last place may round these the other way, a correctly
    rounded host may not — so where the two differ the host is right"""
    mp = pytest.importorskip("mpmath")
    with mp.workprec(200):
        for b in fragile["bits"]:
            x = float(np.array([b], np.uint32).view(np.float32)[0])
            exact = mp.power(mp.mpf(2.718281828), mp.mpf(x))
            assert math.pow(2.718281828, x) == float(exact), hex(int(b))


DIV_ROWS_SRC = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char **argv) {
  unsigned long long bad_total = 0;
  for (int ai = 1; ai < argc; ++ai) {
    const uint32_t R = (uint32_t)strtoul(argv[ai], NULL, 10);
    unsigned long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (long long i = 0; i < (1LL << 32); ++i) {
      uint32_t u = (uint32_t)i, a, b;
      float x;
      memcpy(&x, &u, 4);
      volatile float q1 = x / (float)R;                 /* xf_device.h: div_by_rows, R < 2^24 */
      float s = q1, t = x;
      t /= 1.0 * R;                                     /* lr_worker.cc:117 */
      memcpy(&a, &s, 4);
      memcpy(&b, &t, 4);
      if ((a & 0x7FFFFFFFu) > 0x7F800000u && (b & 0x7FFFFFFFu) > 0x7F800000u) continue;
      bad += a != b;
    }
    printf("R %u: %llu\n", R, bad);
    bad_total += bad;
  }
  return bad_total != 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_fp32_quotient_by_a_row_count_is_the_fp64_quotient_rounded_back_for_every_float(tmp_path):
    """div_by_rows below 2^24 rows: x / (float)R == (float)((double)x / (1.0 * R)) for all 2^32 x
    (NaN for NaN), at R = 3, 50000 and 2^24 - 1 — subnormal quotients and their exact midpoints
    included (x = 25000 * 2^-149 over 50000)"""
    c = tmp_path / "d.c"
    c.write_text(DIV_ROWS_SRC)
    exe = tmp_path / "d"
    r = subprocess.run(["gcc", "-O2", "-fopenmp", "-ffp-contract=off", str(c), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0:     # (no libgomp on this machine, say: nothing to check with)
        pytest.skip("cannot build the checker: " + r.stderr[-300:])
    rows = ["3", "50000", str((1 << 24) - 1)]
    out = subprocess.run([str(exe)] + rows, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, OMP_NUM_THREADS=str(O.sweep_threads())))
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["R", "3:", "0", "R", "50000:", "0", "R", "16777215:", "0"], \
        out.stdout
