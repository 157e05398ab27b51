// xf_gauc.h — grouped AUC on the held-out rows (xf_gauc.hip, xf_gauc_host.cc): what the host and
// the device side share — the code of a held row's record — and the tap of the validate passes.
#ifndef XF_GAUC_H_
#define XF_GAUC_H_

#include <stdint.h>

#include "xf_admit.h"     // XF_ADMIT_HD
#include "xf_progress.h"  // progress_rank, XF_PROGRESS_CENTER
#include "xflow_amd.h"    // XF_GAUC_WORDS, XF_SLICE_NONE

#define XF_GAUC_OTHER 0xFFFFFFFFu /* the code of a row that takes no part (NaN, q > 1) */

namespace xf {

// the largest code: score 2C, positive
constexpr uint32_t kGaucCodeMax = ((2u * XF_PROGRESS_CENTER) << 1) | 1u;
// records a reduce takes: fewer than 2^30 (U2 < 2^60, positions in 32 bits)
constexpr uint64_t kGaucMaxRecords = 1ull << 30;

// The code of a row's record: score = the score rank the global AUC uses (a positive's is
// 2C - rank, a negative's is rank: monotone in p, equal p means equal score), the class in bit 0.
// Sorting by code puts a score's negatives in front of its positives.
XF_ADMIT_HD uint32_t gauc_code(float loss, int32_t label) {
  const uint32_t rank = progress_rank(loss), pos = label != 0 ? 1u : 0u;
  if (rank == XF_PROGRESS_RANKS) return XF_GAUC_OTHER;
  const uint32_t score = pos ? 2u * XF_PROGRESS_CENTER - rank : rank;
  return (score << 1) | pos;
}

}  // namespace xf

struct xf_gauc;

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace xf {
// the records of rows [0, R) appended on `s` (k_ga_pack); R == 0: no launch
int gauc_append(xf_gauc *g, const float *loss, const int32_t *labels, const uint64_t *id,
                uint32_t R, hipStream_t s);
}  // namespace xf
#endif

#endif  // XF_GAUC_H_
