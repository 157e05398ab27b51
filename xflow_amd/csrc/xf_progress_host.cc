// xf_progress_host.cc — the host side of progressive validation that needs no GPU: the exported
// rank and the summary of the counts (xf_progress.h).  Plain C++: it also builds into a stand-alone
// program under the host sanitizers (tools/progress_host_check.cc).
//
// The device only counts (xf_progress.hip); every floating-point figure is formed here, in fp64,
// in one fixed order: a class's buckets by ascending rank, sum += (double)count * term.
#include <math.h>
#include <string.h>

#include "xf_common.h"
#include "xf_progress.h"

namespace {

constexpr uint32_t C = XF_PROGRESS_CENTER, RANKS = XF_PROGRESS_RANKS;

double edge(uint32_t r) {  // the fp32 value whose bits are r << SH, as a double
  const uint32_t bits = r << XF_PROGRESS_SHIFT;
  float f;
  memcpy(&f, &bits, 4);
  return (double)f;
}

// the representative m of a bucket — the midpoint of its fp32 bounds — of q below C, of 1 - q
// above; 0.5 at C (the bucket holds nothing else), 2^-25 for the saturated bucket (q == 1: the
// sigmoid rounded to 1, or returned it above 30)
double bucket_m(uint32_t rank) {
  if (rank == C) return 0.5;
  if (rank == 2 * C) return ldexp(1.0, -25);
  const uint32_t r = rank < C ? rank : 2 * C - rank;
  return 0.5 * (edge(r) + edge(r + 1));
}

}  // namespace

// the row term of a bucket: -log1p(-m) below C, -ln(m) from C on (m: the bucket's representative)
double xf::progress_term(uint32_t rank) {
  const double m = bucket_m(rank);
  return rank < C ? -log1p(-m) : -log(m);
}

extern "C" uint32_t xf_progress_rank(float loss) { return xf::progress_rank(loss); }

extern "C" int xf_progress_summary(const uint64_t *counts, const uint64_t *other, float neg_weight,
                                   xf_progress_metrics *out) {
  XF_REQUIRE(counts && other && out, "xf_progress_summary: null argument");
  XF_REQUIRE(isfinite(neg_weight) && neg_weight >= 1.0f,
             "xf_progress_summary: the weight of a kept negative is 1 / neg_keep >= 1 and finite, "
             "not %g", (double)neg_weight);
  const uint64_t *neg = counts, *pos = counts + RANKS;
  const double w = (double)neg_weight;
  unsigned __int128 P = 0, N = 0;
  double loss_pos = 0.0, loss_neg = 0.0, p_pos = 0.0, p_neg = 0.0;
  for (uint32_t r = 0; r < RANKS; ++r) {
    if (!pos[r] && !neg[r]) continue;
    const double m = bucket_m(r);
    const double term = xf::progress_term(r);
    const double q = r < C ? m : 1.0 - m;  // the error mass; p = q for a negative, 1 - q for a positive
    const double pq = r < C ? 1.0 - m : m;
    P += pos[r];
    N += neg[r];
    loss_pos += (double)pos[r] * term;
    loss_neg += (double)neg[r] * term;
    p_pos += (double)pos[r] * pq;
    p_neg += (double)neg[r] * q;
  }
  // AUC over score ranks: a negative's is rank(q), a positive's 2C - rank(q).  Exact integers.
  unsigned __int128 U2 = 0, T2 = 0, below = 0;
  for (uint32_t s = 0; s < RANKS; ++s) {
    const unsigned __int128 ps = pos[2 * C - s], ns = neg[s];
    U2 += ps * (2 * below + ns);
    T2 += ps * ns;
    below += ns;
  }
  const double dP = (double)P, dN = (double)N, rows = dP + w * dN;
  memset(out, 0, sizeof(*out));
  out->rows_pos = dP;
  out->rows_neg = w * dN;
  out->saturated = (double)pos[2 * C] + w * (double)neg[2 * C];
  out->other = (double)other[1] + w * (double)other[0];
  out->logloss_bound = -log(1.0 - ldexp(1.0, -(XF_PROGRESS_MANT + 1)));
  const bool any = P != 0 || N != 0, both = P != 0 && N != 0;
  out->logloss = any ? (loss_pos + w * loss_neg) / rows : NAN;
  out->ctr = any ? dP / rows : NAN;
  out->pctr = any ? (p_pos + w * p_neg) / rows : NAN;
  const double den = (double)(2 * P * N);
  out->auc = both ? (double)U2 / den : NAN;
  out->auc_slack = both ? (double)T2 / den : any ? 0.0 : NAN;  // (one class only: auc alone is NaN)
  return XF_OK;
}
