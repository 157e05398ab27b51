// slices_host_check.cc — the host side of sliced progressive validation (xflow_amd/csrc/
// xf_slices_host.cc: the home slot, the table of fixed-point row terms, the summary, the parameter
// check; with xf_progress_host.cc's row term behind the table) driven from a main of its own, for
// a run under the host sanitizers.  No GPU, no Python:
//
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//     -Iinclude -Ixflow_amd/csrc tools/slices_host_check.cc xflow_amd/csrc/xf_slices_host.cc \
//     xflow_amd/csrc/xf_progress_host.cc xflow_amd/csrc/xf_io.cc -o /tmp/slices_host_check \
//     -lpthread && /tmp/slices_host_check
//
// Covers: the home slot against two public splitmix64 outputs at b = 2, 16, 26, its range over a
// sweep of keys and 0 outside 2 .. 26; the probe limit; the fixed-point q at 0, -0, a denormal,
// 0.5, 1; every word of the table of terms against the progress summary's own logloss of one row
// of that rank (the one definition), its edges (0, ln 2, 25 ln 2) and its 31-bit range; the summary
// on no rows, one class only, `other` only, w = 1 and w = 4, counters near 2^63 (n1 2^31 needs
// more than 64 bits) and the refusals (null, w < 1, NaN, qsum1 beyond n1 rows, field and b outside
// their ranges).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "xf_common.h"
#include "xf_slices.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, xf_last_error());
  }
}

int main() {
  const uint32_t C = XF_PROGRESS_CENTER, RANKS = XF_PROGRESS_RANKS;
  const uint64_t mix0 = 0xE220A8397B1DCDAFull, mixg = 0x6E789E6AA1B965F4ull;  // splitmix64(0): 1st, 2nd
  for (int b : {2, 16, 26}) {
    expect(xf_slices_home(0, b) == mix0 >> (64 - b), "home(0, b): splitmix64's first output");
    expect(xf_slices_home(0x9e3779b97f4a7c15ull, b) == mixg >> (64 - b),
           "home(golden, b): splitmix64's second output");
  }
  for (int b = 2; b <= 26; ++b)
    for (uint64_t k = 0; k < 2000; ++k)
      expect(xf_slices_home(k * 0x2545F4914F6CDD1Dull + b, b) < (1ull << b), "home in range");
  for (int b : {-1, 0, 1, 27, 32, 64, 65})
    expect(xf_slices_home(12345, b) == 0, "home outside 2 .. 26 is 0");
  expect(xf::slices_probes(2) == 4 && xf::slices_probes(6) == 64 && xf::slices_probes(7) == 128 &&
             xf::slices_probes(26) == 128,
         "the probe limit: min(2^b, 128)");
  expect(xf::slices_qfix(0.0f) == 0 && xf::slices_qfix(-0.0f) == 0 && xf::slices_qfix(1e-45f) == 0 &&
             xf::slices_qfix(0.5f) == (1u << 30) && xf::slices_qfix(-0.5f) == (1u << 30) &&
             xf::slices_qfix(1.0f) == (1u << 31) && xf::slices_qfix(-1.0f) == (1u << 31) &&
             xf::slices_qfix(0.75f) == 3u << 29,
         "the fixed-point q");

  std::vector<uint32_t> terms(RANKS);
  expect(xf_slices_terms(terms.data()) == XF_OK, "the table of terms");
  expect(xf_slices_terms(nullptr) == XF_EINVAL, "null table refused");
  expect(terms[0] == 0 && terms[C] == (uint32_t)llrint(ldexp(log(2.0), 24)) &&
             terms[2 * C] == (uint32_t)llrint(ldexp(25.0 * log(2.0), 24)),
         "the terms' edges");
  // one row of rank r at a time through the progress summary: its logloss IS the term
  std::vector<uint64_t> counts(2 * (size_t)RANKS, 0);
  uint64_t other[2] = {0, 0};
  xf_progress_metrics pm;
  uint32_t biggest = 0;
  for (uint32_t r = 0; r < RANKS; r += (r < 8 || r + 8 > RANKS || (r > C - 4 && r < C + 4)) ? 1 : 1301) {
    counts[r] = 1;
    expect(xf_progress_summary(counts.data(), other, 1.0f, &pm) == XF_OK &&
               terms[r] == (uint32_t)llrint(ldexp(pm.logloss, 24)),
           "a term is the progress summary's logloss of one row of that rank");
    counts[r] = 0;
  }
  for (uint32_t r = 0; r < RANKS; ++r) biggest = terms[r] > biggest ? terms[r] : biggest;
  expect(biggest < (1u << 31), "the terms fit 31 bits");

  xf_slice_metrics m;
  uint64_t w7[XF_SLICE_WORDS] = {0, 0, 0, 0, 0, 0, 0};
  expect(xf_slices_summary(w7, 1.0f, &m) == XF_OK && m.rows == 0 && isnan(m.ctr) && isnan(m.pctr) &&
             isnan(m.logloss) && m.other == 0 && m.pctr_bound == ldexp(1.0, -31) &&
             m.logloss_bound > 4.88e-4 && m.logloss_bound < 4.89e-4,
         "no rows: every mean NaN");
  w7[6] = 41;
  expect(xf_slices_summary(w7, 4.0f, &m) == XF_OK && m.rows == 0 && isnan(m.ctr) && m.other == 41,
         "other only");
  w7[6] = 0;
  w7[1] = 3;               // positives only: q sums to 2^31 over 3 rows
  w7[3] = 1ull << 31;
  w7[5] = 3 * 11629080ull;
  expect(xf_slices_summary(w7, 4.0f, &m) == XF_OK && m.rows == 3 && m.ctr == 1.0 &&
             m.pctr == (double)(2ull << 31) / 2147483648.0 / 3.0 &&
             m.logloss == (double)(3 * 11629080ull) / 16777216.0 / 3.0,
         "positives only: w plays no part");
  const uint64_t both[XF_SLICE_WORDS] = {10, 5, 3ull << 30, (1ull << 31) + 12345, (7ull << 24) + 1,
                                         9ull << 23, 2};
  for (float w : {1.0f, 4.0f}) {
    const double dw = w, rows = 5.0 + dw * 10.0;
    expect(xf_slices_summary(both, w, &m) == XF_OK && m.rows == rows && m.ctr == 5.0 / rows &&
               m.other == 2 &&
               m.pctr == ((double)((5ull << 31) - both[3]) + dw * (double)both[2]) / 2147483648.0 / rows &&
               m.logloss == ((double)both[5] + dw * (double)both[4]) / 16777216.0 / rows,
           "both classes, w = 1 and w = 4");
  }
  // n1 2^31 beyond 64 bits: n1 = 2^39 + 1, qsum1 = 2^63 + 12345
  const uint64_t big[XF_SLICE_WORDS] = {(1ull << 40) + 3, (1ull << 39) + 1, ((1ull << 40) + 3) * (1ull << 23) - 5,
                                        (1ull << 63) + 12345, (1ull << 62) + 7, (1ull << 61) + 9, 1ull << 33};
  const unsigned __int128 p1 = ((unsigned __int128)big[1] << 31) - big[3];
  expect((((unsigned __int128)big[1] << 31) >> 64) != 0, "the case needs more than 64 bits");
  expect(xf_slices_summary(big, 1.0f, &m) == XF_OK &&
             m.pctr == ((double)p1 + (double)big[2]) / 2147483648.0 / m.rows && m.pctr > 0 && m.pctr < 1,
         "counters near 2^63");
  expect(xf_slices_summary(nullptr, 1.0f, &m) == XF_EINVAL, "null words refused");
  expect(xf_slices_summary(both, 1.0f, nullptr) == XF_EINVAL, "null metrics refused");
  expect(xf_slices_summary(both, 0.5f, &m) == XF_EINVAL, "w < 1 refused");
  expect(xf_slices_summary(both, NAN, &m) == XF_EINVAL, "w NaN refused");
  const uint64_t bad[XF_SLICE_WORDS] = {0, 1, 0, (1ull << 31) + 1, 0, 0, 0};
  expect(xf_slices_summary(bad, 1.0f, &m) == XF_EINVAL, "qsum1 beyond n1 rows refused");
  expect(xf_slices_check(0, 2) == XF_OK && xf_slices_check(0x7fffffff, 26) == XF_OK, "the ranges' ends");
  expect(xf_slices_check(-1, 16) == XF_EINVAL && xf_slices_check(1ll << 31, 16) == XF_EINVAL &&
             xf_slices_check(3, 1) == XF_EINVAL && xf_slices_check(3, 27) == XF_EINVAL,
         "field and b outside their ranges refused");
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("slices_host_check: ok\n");
  return 0;
}
