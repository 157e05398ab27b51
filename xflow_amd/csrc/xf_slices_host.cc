// xf_slices_host.cc — the host side of sliced progressive validation that needs no GPU: the
// exported home slot, the parameter check, the table of fixed-point row terms and the summary of a
// slice's seven words (xf_slices.h).  Plain C++: it also builds into a stand-alone program under
// the host sanitizers (tools/slices_host_check.cc).
//
// The device only adds integers (xf_slices.hip); every floating-point figure is formed here, in
// fp64, in one fixed order.
#include <math.h>
#include <string.h>

#include "xf_common.h"
#include "xf_slices.h"

int xf::slices_check_params(const char *who, long long F, long long b) {
  XF_REQUIRE(F >= 0 && F <= 0x7fffffffll, "%s: a field id is 0 .. 2147483647, not %lld", who, F);
  XF_REQUIRE(b >= kSlicesMinLog2 && b <= kSlicesMaxLog2,
             "%s: the slice table has 2^b entries, b in %d .. %d, not %lld", who, kSlicesMinLog2,
             kSlicesMaxLog2, b);
  return XF_OK;
}

void xf::slices_terms(uint32_t *out) {
  // (no bucket's term exceeds -ln of the smallest denormal, < 104: 104 * 2^24 < 2^31)
  for (uint32_t r = 0; r < XF_PROGRESS_RANKS; ++r)
    out[r] = (uint32_t)llrint(ldexp(xf::progress_term(r), 24));
}

extern "C" uint64_t xf_slices_home(uint64_t key, int log2_slots) {
  if (log2_slots < xf::kSlicesMinLog2 || log2_slots > xf::kSlicesMaxLog2) return 0;
  return xf::slices_home(key, log2_slots);
}

extern "C" int xf_slices_terms(uint32_t *out) {
  XF_REQUIRE(out, "xf_slices_terms: null argument");
  xf::slices_terms(out);
  return XF_OK;
}

extern "C" int xf_slices_check(int64_t field, int64_t log2_slots) {
  return xf::slices_check_params("xf_slices_check", field, log2_slots);
}

extern "C" int xf_slices_summary(const uint64_t *words, float neg_weight, xf_slice_metrics *out) {
  XF_REQUIRE(words && out, "xf_slices_summary: null argument");
  XF_REQUIRE(isfinite(neg_weight) && neg_weight >= 1.0f,
             "xf_slices_summary: the weight of a kept negative is 1 / neg_keep >= 1 and finite, "
             "not %g", (double)neg_weight);
  const double w = (double)neg_weight;
  const uint64_t n0 = words[xf::kSlN0], n1 = words[xf::kSlN1];
  const unsigned __int128 full = (unsigned __int128)n1 << 31;
  XF_REQUIRE(words[xf::kSlQ1] <= full,
             "xf_slices_summary: qsum[1] = %llu exceeds 2^31 a row over n[1] = %llu rows: not a "
             "slice's counters", (unsigned long long)words[xf::kSlQ1], (unsigned long long)n1);
  const double rows = (double)n1 + w * (double)n0;
  // a positive's p is 1 - q: n1 2^31 - qsum1 in exact integers
  const unsigned __int128 p1 = full - words[xf::kSlQ1];
  memset(out, 0, sizeof(*out));
  out->rows = rows;
  out->other = (double)words[xf::kSlOther];
  out->logloss_bound = -log(1.0 - ldexp(1.0, -(XF_PROGRESS_MANT + 1))) + ldexp(1.0, -25);
  out->pctr_bound = ldexp(1.0, -31);
  const bool any = n0 != 0 || n1 != 0;
  out->ctr = any ? (double)n1 / rows : NAN;
  out->pctr = any ? ((double)p1 + w * (double)words[xf::kSlQ0]) / 2147483648.0 / rows : NAN;
  out->logloss =
      any ? ((double)words[xf::kSlLl1] + w * (double)words[xf::kSlLl0]) / 16777216.0 / rows : NAN;
  return XF_OK;
}
