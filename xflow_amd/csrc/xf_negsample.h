// xf_negsample.h — negative subsampling (xf_negsample.hip): what the host and the device side
// share — the keep decision of a row — and the launch of the weight kernel for the training steps.
#ifndef XF_NEGSAMPLE_H_
#define XF_NEGSAMPLE_H_

#include <stdint.h>

#include "xf_admit.h"  // admit_mix64: xf_device.h's mix64 for both sides

namespace xf {

// T = floor(keep * 2^32) as the 64-bit threshold of the decision; keep in (0, 1]: 1 .. 2^32
XF_ADMIT_HD uint64_t negsample_threshold(double keep) {
  return (uint64_t)(keep * 4294967296.0);  // (the product is exact: a power-of-two scale)
}

// mix64(seed ^ stream): once per apply
XF_ADMIT_HD uint64_t negsample_base(uint64_t seed, uint64_t stream) {
  return admit_mix64(seed ^ stream);
}

// a NEGATIVE row of this ordinal is kept iff the top 32 bits of mix64(base + ordinal) are below T
XF_ADMIT_HD bool negsample_keep_row(uint64_t base, uint64_t ordinal, uint64_t T) {
  return (admit_mix64(base + ordinal) >> 32) < T;
}

}  // namespace xf

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace xf {
// loss[r] = labels[r] != 0 ? loss[r] : fp32(w * loss[r]) over R rows on `s` (k_weigh_negatives);
// w == 1 or R == 0: no launch.  Between a training step's forward and whatever reads its losses.
// (The LR cells steps do not come here: k_lr_finalize_cells stores the weighted loss itself.
// xf_weigh_negatives_launches counts the launches made, for the tests that hold them to that.)
int weigh_negatives(float *loss, const int32_t *labels, uint32_t R, float w, hipStream_t s);
}  // namespace xf
#endif

#endif  // XF_NEGSAMPLE_H_
