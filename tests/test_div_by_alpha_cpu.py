"""ftrl_step divides by alpha twice per step (ftrl.h:63,70) and every gradient is a sum divided by
the minibatch's row count (lr_worker.cc:117, fm_worker.cc:150-156).  The kernels compute x / d for
such a call-invariant divisor as the double product with the reciprocal, rounded to float, and do
the division itself only where the result is in or next to the subnormal range (xf_device.h:
div_by_const) — three instructions instead of an IEEE fp32 division's eleven in VALU-bound
kernels.  This must be the SAME float for every x: checked here exhaustively, all 2^32 bit
patterns of x, for the reference's default alpha, divisors with exact midpoints among their
subnormal quotients (50000, the bench's row count: the guard's reason) and other row counts, on
the host (IEEE double multiply and double -> float rounding are what the GPU's v_mul_f64 /
v_cvt_f32_f64 do).  Without the guard the unguarded product differs for d = 50000 at 1308 values
of x, all with subnormal quotients (exact rounding midpoints exist there: x = 25000 * 2^-149):
checked too.

The GPU side: the bit-exact parity tests run at alpha = 0.05 (and 0.1, 0.3, 0.01), which the
table finds exact divisors, so they run the unguarded product only.  The function itself with its
guard, at d = 50000 on the list inexact_list() makes here, and the table's verdict kernel, run on
the device in tests/test_gpu_hyper.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest


def inexact_list(d, chunk=1 << 24):
    """the bit patterns (uint32) of every x with |x| < 2^-120 d at which the bare product
    (float)((double)x * (1.0 / d)) is not the float x / d, the positive ones ascending, then their
    negatives (the two operations are odd functions of x).  All x above the bound have quotients
    of at least 2^-120, where the two agree for every d (xf_device.h: div_by_const)."""
    d = np.float32(d)
    inv = 1.0 / np.float64(d)
    stop = int(np.float32(np.float32(2.0 ** -120) * d).view(np.uint32))
    found = []
    with np.errstate(under="ignore"):
        for a in range(1, stop, chunk):
            u = np.arange(a, min(a + chunk, stop), dtype=np.uint32)
            x = u.view(np.float32)
            bare = (x.astype(np.float64) * inv).astype(np.float32)
            found.append(u[(x / d).view(np.uint32) != bare.view(np.uint32)])
    pos = np.concatenate(found)
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def test_the_host_list_of_inexact_quotients_of_50000():
    """the 1308 of the exhaustive run below, found again in seconds: 654 positive x, every one
    with a subnormal quotient, 0x02432b61 among them"""
    bad = inexact_list(50000.0)
    assert len(bad) == 1308 and len(np.unique(bad)) == 1308
    assert 0x02432B61 in bad[:654]
    with np.errstate(under="ignore"):
        q = np.abs(bad.view(np.float32) / np.float32(50000.0))
    assert np.all(q < np.finfo(np.float32).tiny)
    for d in (0.05, 0.1):
        assert len(inexact_list(d)) == 0

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static inline float div_by_const(float x, float d, double inv_d) {  /* xf_device.h */
  const float q = (float)((double)x * inv_d);
  if (fabsf(q) >= 0x1p-125f || x == 0.0f) return q;
  return x / d;
}
int main(int argc, char **argv) {
  unsigned long long bad_total = 0;
  for (int ai = 1; ai < argc; ++ai) {
    const float d = strtof(argv[ai], NULL);
    const double inv = 1.0 / (double)d;
    unsigned long long bad = 0, bad_plain = 0;
#pragma omp parallel for reduction(+ : bad, bad_plain) schedule(static)
    for (long long i = 0; i < (1LL << 32); ++i) {
      uint32_t u = (uint32_t)i, a, b, c;
      float x;
      memcpy(&x, &u, 4);
      if (!isfinite(x)) continue;
      volatile float q1 = x / d;
      float t = q1, q2 = div_by_const(x, d, inv), q3 = (float)((double)x * inv);
      memcpy(&a, &t, 4);
      memcpy(&b, &q2, 4);
      memcpy(&c, &q3, 4);
      bad += a != b;
      bad_plain += a != c;
    }
    printf("d %.9g: %llu (unguarded %llu)\n", d, bad, bad_plain);
    bad_total += bad;
  }
  return bad_total != 0;
}
"""


def _compile(tmp_path, src, name):
    c = tmp_path / (name + ".c")
    c.write_text(src)
    exe = tmp_path / name
    r = subprocess.run(["gcc", "-O2", "-fopenmp", "-ffp-contract=off", str(c), "-o", str(exe),
                        "-lm"], capture_output=True, text=True)
    if r.returncode != 0:     # (no libgomp on this machine, say: nothing to check with)
        pytest.skip("cannot build the checker: " + r.stderr[-300:])
    return exe


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_double_product_with_the_reciprocal_is_the_fp32_quotient_for_every_float(tmp_path):
    """2 x 10^10 divisions: minutes on a machine with few cores (the time limit is the test's own)"""
    exe = _compile(tmp_path, SRC, "t")
    divisors = ["0.05", "10", "50000", "16667", "16777215"]
    out = subprocess.run([str(exe)] + divisors, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, OMP_NUM_THREADS="8"))
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(divisors) and all(": 0 (" in ln for ln in lines), out.stdout
    # the guard is there for a reason: the bare product mis-rounds subnormal quotients of 50000
    assert not lines[2].endswith("(unguarded 0)"), out.stdout
    # ... and the reference's alpha is a divisor that does not need it: what the table's own
    # check on the GPU (xf_table.hip: div_exact_for) finds for it, every x, before it lets the
    # step drop the guard
    assert lines[0].endswith("(unguarded 0)"), out.stdout


RANDOM_SRC = SRC.split("int main")[0] + r"""
static uint64_t s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
int main(void) {   /* alpha is the user's to set: random divisors, random and subnormal-range x */
  unsigned long long bad = 0;
  for (int di = 0; di < 20000; ++di) {
    uint32_t ud = rnd() & 0x7FFFFFFFu;
    float d;
    memcpy(&d, &ud, 4);
    if (!isfinite(d) || d == 0.0f) continue;
    const double inv = 1.0 / (double)d;
    for (int xi = 0; xi < 2000; ++xi) {
      uint32_t ux = rnd();
      if (xi & 1) ux = (ux & 0x80FFFFFFu) | ((rnd() % 40) << 23);   /* tiny x: subnormal quotients */
      float x;
      memcpy(&x, &ux, 4);
      if (!isfinite(x)) continue;
      volatile float q1 = x / d;
      float t = q1, q2 = div_by_const(x, d, inv);
      uint32_t a, b;
      memcpy(&a, &t, 4);
      memcpy(&b, &q2, 4);
      if (isnan(t) && isnan(q2)) continue;
      bad += a != b;
    }
  }
  printf("%llu\n", bad);
  return bad != 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_guarded_product_is_the_quotient_for_random_divisors(tmp_path):
    """the general claim behind div_by_const (alpha is user-settable): 4 x 10^7 random (x, d)
    pairs, half of them with x in the range whose quotients are subnormal or next to it"""
    exe = _compile(tmp_path, RANDOM_SRC, "r")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr
