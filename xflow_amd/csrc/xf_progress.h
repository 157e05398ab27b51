// xf_progress.h — progressive validation (xf_progress.hip, xf_progress_host.cc): what the host and
// the device side share — the rank of a row's loss — and the tap of the training steps.
#ifndef XF_PROGRESS_H_
#define XF_PROGRESS_H_

#include <stdint.h>

#include "xf_admit.h"  // XF_ADMIT_HD
#include "xflow_amd.h"  // XF_PROGRESS_MANT (mantissa bits a rank keeps), XF_PROGRESS_RANKS

#define XF_PROGRESS_SHIFT (23 - XF_PROGRESS_MANT)    /* SH */
#define XF_PROGRESS_CENTER (0x3f000000u >> XF_PROGRESS_SHIFT) /* C = bits(0.5f) >> SH */
static_assert(XF_PROGRESS_RANKS == 2u * XF_PROGRESS_CENTER + 1u, "ranks per class: 0 .. 2C");

namespace xf {

XF_ADMIT_HD uint32_t progress_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// The rank of a row's loss (loss = sigmoid - label): q = |loss| is the probability the model put on
// the wrong class.  0 .. 2C, monotone in q, rank(1 - q) = 2C - rank(q) wherever 1 - q is exact;
// XF_PROGRESS_RANKS for a row that takes no part (NaN, q > 1).
//   q <  0.5: bits(q) >> SH                    (-0.0 -> 0)
//   q >= 0.5: 2C - (bits(1 - q) >> SH)         (1 - q is exact: Sterbenz; q = 1 -> 2C)
XF_ADMIT_HD uint32_t progress_rank(float loss) {
  const float q = loss < 0.0f ? -loss : loss;
  if (!(q <= 1.0f)) return XF_PROGRESS_RANKS;
  if (q < 0.5f) return progress_bits(q) << 1 >> 1 >> XF_PROGRESS_SHIFT;
  const float m = 1.0f - q;
  return 2u * XF_PROGRESS_CENTER - (progress_bits(m) >> XF_PROGRESS_SHIFT);
}

// where a row is counted in the device's one array of 2 * RANKS + 2 words: counts[cls][rank] at
// cls * RANKS + rank, other[cls] behind them
XF_ADMIT_HD uint32_t progress_word(float loss, int32_t label) {
  const uint32_t cls = label != 0 ? 1u : 0u, rank = progress_rank(loss);
  return rank == XF_PROGRESS_RANKS ? 2u * XF_PROGRESS_RANKS + cls : cls * XF_PROGRESS_RANKS + rank;
}
constexpr uint32_t kProgressWords = 2u * XF_PROGRESS_RANKS + 2u;

// host only (xf_progress_host.cc): the row term the summary gives a row of that rank, rank in
// 0 .. 2C — the one definition, also behind the sliced counters' fixed-point terms (xf_slices.h)
double progress_term(uint32_t rank);

}  // namespace xf

struct xf_progress;

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace xf {
// counts += the ranks of loss[0 .. R) on `s` (k_pg_accumulate); R == 0: no launch.  In a training
// step: after the forward has written the losses, before the negatives' weight touches them.
int progress_accumulate(xf_progress *p, const float *loss, const int32_t *labels, uint32_t R,
                        hipStream_t s);
}  // namespace xf
#endif

#endif  // XF_PROGRESS_H_
