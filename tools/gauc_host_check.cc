// gauc_host_check.cc — the host side of the grouped AUC (xflow_amd/csrc/xf_gauc_host.cc: the code
// of a row's record, the summary of the group figures) driven from a main of its own, for a run
// under the host sanitizers.  No GPU, no Python:
//
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//     -Iinclude -Ixflow_amd/csrc tools/gauc_host_check.cc xflow_amd/csrc/xf_gauc_host.cc \
//     xflow_amd/csrc/xf_io.cc -o /tmp/gauc_host_check -lpthread && /tmp/gauc_host_check
//
// Covers: the code at the rank's edge losses for both classes and a label other than 0 / 1 (a
// positive's score is 2C - rank, a negative's is rank; equal p means equal score), NaN and q > 1;
// the summary on no group, one-class groups only, the known answers (AUC 1, 0, all tied), two
// scored groups with their weights, arrays of exactly n values, counts near the limits, and the
// refusals (null, ids that do not ascend, figures no group can have).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "xf_common.h"
#include "xf_gauc.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, xf_last_error());
  }
}

int main() {
  const uint32_t C = XF_PROGRESS_CENTER;
  // loss = p - label: a negative's loss is p, a positive's p - 1
  expect(xf_gauc_code(0.0f, 0) == 0 && xf_gauc_code(-0.0f, 0) == 0, "p = 0, negative: score 0");
  expect(xf_gauc_code(1e-45f, 0) == 0, "the smallest subnormal ranks with 0");
  expect(xf_gauc_code(0.5f, 0) == (C << 1) && xf_gauc_code(-0.5f, 1) == ((C << 1) | 1u),
         "p = 0.5: score C for both classes");
  expect(xf_gauc_code(-0.5f, 7) == ((C << 1) | 1u) && xf_gauc_code(-0.5f, -1) == ((C << 1) | 1u),
         "a label other than 0 / 1 is a positive");
  expect(xf_gauc_code(1.0f, 0) == ((2 * C) << 1), "p = 1, negative: score 2C");
  expect(xf_gauc_code(-0.0f, 1) == (((2 * C) << 1) | 1u), "p = 1, positive: score 2C");
  expect(xf_gauc_code(-1.0f, 1) == 1u, "p = 0, positive: score 0");
  expect(xf_gauc_code(1.0f - ldexpf(1.0f, -24), 0) >> 1 ==
             (xf_gauc_code(-ldexpf(1.0f, -24), 1) >> 1),
         "p = 1 - 2^-24: one score for both classes");
  expect(xf_gauc_code(0.25f, 0) >> 1 == (xf_gauc_code(-0.75f, 1) >> 1),
         "p = 0.25: one score for both classes");
  expect(xf_gauc_code(NAN, 0) == XF_GAUC_OTHER && xf_gauc_code(NAN, 1) == XF_GAUC_OTHER &&
             xf_gauc_code(1.5f, 0) == XF_GAUC_OTHER && xf_gauc_code(-1.5f, 1) == XF_GAUC_OTHER &&
             xf_gauc_code(INFINITY, 0) == XF_GAUC_OTHER,
         "NaN and q > 1 leave no record");
  uint32_t last = 0;
  bool monotone = true;
  for (int i = 0; i <= 4096; ++i) {  // p ascending: the score never descends
    const uint32_t s = xf_gauc_code((float)i / 4096.0f, 0) >> 1;
    monotone = monotone && s >= last && s <= 2 * C;
    last = s;
  }
  expect(monotone && xf::kGaucCodeMax == (((2 * C) << 1) | 1u), "the score is monotone in p");

  xf_gauc_metrics m;
  const uint64_t none[2] = {3, 4}, other[2] = {5, 6};
  expect(xf_gauc_summary(nullptr, 0, none, other, &m, nullptr, nullptr) == XF_OK && m.groups == 0 &&
             m.groups_scored == 0 && m.rows == 0 && isnan(m.gauc) && isnan(m.gauc_slack) &&
             isnan(m.macro_auc) && m.none_rows == 7 && m.other_rows == 11,
         "no group: the means are NaN");
  {
    const std::vector<uint64_t> e = {1, 3, 0, 0, 0, 9, 0, 2, 0, 0};  // (exactly n entries)
    std::vector<double> auc(2), slack(2);
    expect(xf_gauc_summary(e.data(), 2, nullptr, nullptr, &m, auc.data(), slack.data()) == XF_OK &&
               m.groups == 2 && m.groups_scored == 0 && m.rows == 5 && m.rows_one_class == 5 &&
               m.rows_scored == 0 && isnan(m.gauc) && isnan(auc[0]) && isnan(slack[1]) &&
               m.none_rows == 0,
           "one-class groups are not scored");
  }
  {
    // id 2: one positive above one negative (U2 = 2); id 5: the reverse (U2 = 0); id 9: all tied,
    // P = 2, N = 3 (U2 = P N = 6, T = 6); id 11: positives only
    const std::vector<uint64_t> e = {2, 1, 1, 2, 0, 5, 1, 1, 0, 0, 9, 2, 3, 6, 6, 11, 4, 0, 0, 0};
    std::vector<double> auc(4), slack(4);
    expect(xf_gauc_summary(e.data(), 4, none, other, &m, auc.data(), slack.data()) == XF_OK &&
               auc[0] == 1.0 && slack[0] == 0.0 && auc[1] == 0.0 && auc[2] == 0.5 &&
               slack[2] == 0.5 && isnan(auc[3]),
           "the known answers");
    const double w2 = 2.0 / 9.0, w5 = 5.0 / 9.0;  // a group's weight: its share of the scored rows
    expect(m.groups == 4 && m.groups_scored == 3 && m.rows == 13 && m.rows_scored == 9 &&
               m.rows_one_class == 4 && m.gauc == ((0.0 + w2 * 1.0) + w2 * 0.0) + w5 * 0.5 &&
               m.gauc_slack == ((0.0 + w2 * 0.0) + w2 * 0.0) + w5 * 0.5 &&
               m.macro_auc == ((0.0 + 1.0) + 0.0 + 0.5) / 3.0,
           "the means: the groups' rows as weight, and unweighted");
  }
  {
    const uint64_t P = (1ull << 29) - 1, N = 1ull << 29;  // near the limit: 2 P N < 2^60
    const std::vector<uint64_t> e = {0xFFFFFFFFFFFFFFFEull, P, N, 2 * P * N - 1, 12345};
    expect(xf_gauc_summary(e.data(), 1, nullptr, nullptr, &m, nullptr, nullptr) == XF_OK &&
               m.gauc == (double)(2 * P * N - 1) / (double)(2 * P * N) && m.macro_auc == m.gauc &&
               m.rows == P + N,
           "counts near 2^30");
  }
  const std::vector<uint64_t> ok = {1, 1, 1, 1, 1};
  expect(xf_gauc_summary(ok.data(), 1, nullptr, nullptr, nullptr, nullptr, nullptr) == XF_EINVAL,
         "null metrics refused");
  expect(xf_gauc_summary(nullptr, 1, nullptr, nullptr, &m, nullptr, nullptr) == XF_EINVAL,
         "null entries refused");
  {
    const std::vector<uint64_t> e = {4, 1, 1, 1, 1, 4, 1, 1, 1, 1};
    expect(xf_gauc_summary(e.data(), 2, nullptr, nullptr, &m, nullptr, nullptr) == XF_EINVAL,
           "an id twice refused");
    const std::vector<uint64_t> d = {4, 1, 1, 1, 1, 3, 1, 1, 1, 1};
    expect(xf_gauc_summary(d.data(), 2, nullptr, nullptr, &m, nullptr, nullptr) == XF_EINVAL,
           "ids that descend refused");
  }
  for (const std::vector<uint64_t> &bad :
       {std::vector<uint64_t>{1, 0, 0, 0, 0}, std::vector<uint64_t>{1, 1, 1, 3, 0},
        std::vector<uint64_t>{1, 1, 1, 2, 2}, std::vector<uint64_t>{1, 1ull << 30, 1, 0, 0},
        std::vector<uint64_t>{1, 2, 2, 1, 2}})
    expect(xf_gauc_summary(bad.data(), 1, nullptr, nullptr, &m, nullptr, nullptr) == XF_EINVAL,
           "figures no group can have refused");
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("gauc_host_check: ok\n");
  return 0;
}
