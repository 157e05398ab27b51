// xf_gauc_host.cc — the host side of the grouped AUC that needs no GPU: the exported code of a
// row's record and the summary of the group figures (xf_gauc.h).  Plain C++: it also builds into a
// stand-alone program under the host sanitizers (tools/gauc_host_check.cc).
//
// The device only produces integers (xf_gauc.hip); every floating-point figure is formed here, in
// fp64, in one fixed order: the groups by ascending id.
#include <math.h>
#include <string.h>

#include "xf_common.h"
#include "xf_gauc.h"

extern "C" uint32_t xf_gauc_code(float loss, int32_t label) { return xf::gauc_code(loss, label); }

extern "C" int xf_gauc_summary(const uint64_t *entries, uint64_t n, const uint64_t *none,
                               const uint64_t *other, xf_gauc_metrics *out, double *auc,
                               double *slack) {
  XF_REQUIRE(out && (entries || n == 0), "xf_gauc_summary: null argument");
  constexpr size_t E = XF_GAUC_WORDS + 1;
  memset(out, 0, sizeof(*out));
  double gauc = 0.0, gauc_slack = 0.0, sum_auc = 0.0;
  uint64_t rows = 0, rows_scored = 0, scored = 0;
  for (uint64_t g = 0; g < n; ++g) {  // (the scored groups' rows first: the weights' divisor)
    const uint64_t P = entries[g * E + 1], N = entries[g * E + 2];
    if (P > 0 && N > 0 && P < xf::kGaucMaxRecords && N < xf::kGaucMaxRecords) rows_scored += P + N;
  }
  for (uint64_t g = 0; g < n; ++g) {
    const uint64_t *e = entries + g * E;
    const uint64_t P = e[1], N = e[2], U2 = e[3], T = e[4];
    XF_REQUIRE(g == 0 || e[0] > entries[(g - 1) * E],
               "xf_gauc_summary: entry %llu: the ids do not ascend", (unsigned long long)g);
    XF_REQUIRE(P < xf::kGaucMaxRecords && N < xf::kGaucMaxRecords && P + N > 0 &&
                   rows + P + N < xf::kGaucMaxRecords,
               "xf_gauc_summary: entry %llu: P = %llu, N = %llu are not a group's counts of fewer "
               "than 2^30 records", (unsigned long long)g, (unsigned long long)P,
               (unsigned long long)N);
    const uint64_t pn2 = 2 * P * N;  // (< 2^61)
    XF_REQUIRE(U2 <= pn2 && T <= pn2 / 2 && T <= U2,
               "xf_gauc_summary: entry %llu: U2 = %llu, T = %llu exceed what P = %llu, N = %llu "
               "allow", (unsigned long long)g, (unsigned long long)U2, (unsigned long long)T,
               (unsigned long long)P, (unsigned long long)N);
    rows += P + N;
    double a = NAN, s = NAN;
    if (P > 0 && N > 0) {
      a = (double)U2 / (double)pn2;
      s = (double)T / (double)pn2;
      // a group's weight is its share of the scored rows — one group alone weighs exactly 1, so
      // its gauc is its auc bit for bit
      const double w = (double)(P + N) / (double)rows_scored;
      gauc += w * a;
      gauc_slack += w * s;
      sum_auc += a;
      ++scored;
    }
    if (auc) auc[g] = a;
    if (slack) slack[g] = s;
  }
  out->groups = n;
  out->groups_scored = scored;
  out->rows = rows;
  out->rows_scored = rows_scored;
  out->rows_one_class = rows - rows_scored;
  out->none_rows = none ? none[0] + none[1] : 0;
  out->other_rows = other ? other[0] + other[1] : 0;
  out->gauc = scored ? gauc : NAN;
  out->gauc_slack = scored ? gauc_slack : NAN;
  out->macro_auc = scored ? sum_auc / (double)scored : NAN;
  return XF_OK;
}
