// progress_host_check.cc — the host side of progressive validation (xflow_amd/csrc/
// xf_progress_host.cc: the exported rank and the summary of the counts) driven from a main of its
// own, for a run under the host sanitizers.  No GPU, no Python:
//
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//     -Iinclude -Ixflow_amd/csrc tools/progress_host_check.cc xflow_amd/csrc/xf_progress_host.cc \
//     xflow_amd/csrc/xf_io.cc -o /tmp/progress_host_check -lpthread && /tmp/progress_host_check
//
// Covers: the rank at the edge values (0, -0, a denormal, 2^-126, 2^-24, 0.25, both neighbours of
// 0.5, 0.5, 1 - 2^-24, 1), NaN and |loss| > 1, monotonicity over a sweep of bit patterns and the
// mirror identity; the summary on empty counts, one class only, every row at C (logloss == ln 2,
// auc == 0.5), counts near 2^40 (U2 needs more than 64 bits: checked against a closed form),
// w != 1 (w cancels in auc, scales rows_neg) and the refusals (null, w < 1, NaN).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "xf_common.h"
#include "xf_progress.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, xf_last_error());
  }
}

int main() {
  const uint32_t C = XF_PROGRESS_CENTER, RANKS = XF_PROGRESS_RANKS;
  expect(C == 0x1F800 && RANKS == 258049, "the constants");
  const struct {
    float q;
    uint32_t rank;
  } edges[] = {{0.0f, 0},           {-0.0f, 0},           {1e-45f, 0},
               {ldexpf(1, -126), 1024}, {ldexpf(1, -24), 105472}, {0.25f, 128000},
               {nextafterf(0.5f, 0.0f), 129023}, {0.5f, 129024}, {nextafterf(0.5f, 1.0f), 129025},
               {1.0f - ldexpf(1, -24), 152576}, {1.0f, 258048}};
  for (const auto &e : edges) {
    expect(xf_progress_rank(e.q) == e.rank, "an edge value of xf_progress_rank");
    expect(xf_progress_rank(-e.q) == e.rank, "an edge value of xf_progress_rank, negated");
  }
  for (float bad : {NAN, 1.0000001f, -1.0000001f, 2.0f, INFINITY, -INFINITY})
    expect(xf_progress_rank(bad) == RANKS, "a loss that takes no part");
  uint32_t prev = 0;
  for (uint32_t bits = 0; bits <= 0x3f800000u; bits += 997) {
    float q;
    memcpy(&q, &bits, 4);
    const uint32_t r = xf_progress_rank(q);
    expect(r >= prev && r <= 2 * C, "monotone, in range");
    prev = r;
    const float m = 1.0f - q;
    // (1 - q is exact: both differences agree in fp64, which a tiny q rounded away fails)
    if ((double)m == 1.0 - (double)q && (double)q == 1.0 - (double)m)
      expect(xf_progress_rank(m) == 2 * C - r, "the mirror identity");
  }

  std::vector<uint64_t> counts(2 * (size_t)RANKS, 0);
  uint64_t other[2] = {0, 0};
  uint64_t *neg = counts.data(), *pos = counts.data() + RANKS;
  xf_progress_metrics m;
  expect(xf_progress_summary(counts.data(), other, 1.0f, &m) == XF_OK, "empty counts succeed");
  expect(isnan(m.logloss) && isnan(m.auc) && isnan(m.ctr) && isnan(m.pctr) && m.rows_pos == 0 &&
             m.rows_neg == 0 && m.logloss_bound > 4.88e-4 && m.logloss_bound < 4.89e-4,
         "empty counts: every mean NaN");
  pos[5] = 3;
  pos[2 * C] = 2;
  other[1] = 7;
  expect(xf_progress_summary(counts.data(), other, 4.0f, &m) == XF_OK && isnan(m.auc) &&
             !isnan(m.logloss) && !isnan(m.auc_slack) && m.ctr == 1.0 && m.rows_pos == 5 &&
             m.saturated == 2 && m.other == 7,
         "positives only: auc alone is NaN");
  pos[5] = pos[2 * C] = 0;
  other[1] = 0;
  neg[C] = 40;
  pos[C] = 24;
  expect(xf_progress_summary(counts.data(), other, 1.0f, &m) == XF_OK && m.logloss == log(2.0) &&
             m.auc == 0.5 && m.auc_slack == 0.5 && m.pctr == 0.5 && m.ctr == 24.0 / 64.0,
         "every row at C: ln 2 and 0.5");
  neg[C] = pos[C] = 0;
  // negatives at score ranks 100 and 200000, positives at score ranks 150 and 200000:
  // U2 = a (2 A) + b (2 (A + 0) ... ) — closed form below, beyond 2^64
  const uint64_t A = 1ull << 40, B = (1ull << 40) + 12345, a = (1ull << 40) + 7, b = 1ull << 39;
  neg[100] = A;
  neg[200000] = B;
  pos[2 * C - 150] = a;
  pos[2 * C - 200000] = b;
  const unsigned __int128 U2 = (unsigned __int128)a * (2 * (unsigned __int128)A) +
                               (unsigned __int128)b * (2 * (unsigned __int128)A + B);
  const unsigned __int128 D = 2 * (unsigned __int128)(a + b) * (unsigned __int128)(A + B);
  expect((U2 >> 64) != 0, "the case needs more than 64 bits");
  expect(xf_progress_summary(counts.data(), other, 1.0f, &m) == XF_OK &&
             m.auc == (double)U2 / (double)D &&
             m.auc_slack == (double)((unsigned __int128)b * B) / (double)D,
         "counts near 2^40: U2 in 128 bits");
  const double auc1 = m.auc, rows_neg1 = m.rows_neg, ll1 = m.logloss;
  const float w = 1.0f / 0.3f;
  expect(xf_progress_summary(counts.data(), other, w, &m) == XF_OK && m.auc == auc1 &&
             m.rows_neg == (double)w * rows_neg1 && m.logloss != ll1 &&
             m.ctr == m.rows_pos / (m.rows_pos + m.rows_neg),
         "w != 1: cancels in auc, weighs the negatives");
  expect(xf_progress_summary(nullptr, other, 1.0f, &m) == XF_EINVAL, "null counts refused");
  expect(xf_progress_summary(counts.data(), other, 0.5f, &m) == XF_EINVAL, "w < 1 refused");
  expect(xf_progress_summary(counts.data(), other, NAN, &m) == XF_EINVAL, "w NaN refused");
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("progress_host_check: ok\n");
  return 0;
}
