// xf_holdout.h — held-out validation (xf_holdout.hip, xf_holdout_host.cc): what the host and the
// device side share — the decision whether a row is held out of training.
#ifndef XF_HOLDOUT_H_
#define XF_HOLDOUT_H_

#include <stdint.h>

#include "xf_admit.h"   // admit_mix64: xf_device.h's mix64 for both sides
#include "xflow_amd.h"  // XF_HOLDOUT_SALT

namespace xf {

// T = floor(share * 2^32) as the 64-bit threshold of the decision; share in [0, 1): 0 .. 2^32 - 1
XF_ADMIT_HD uint64_t holdout_threshold(double share) {
  return (uint64_t)(share * 4294967296.0);  // (the product is exact: a power-of-two scale)
}

// mix64(seed ^ stream ^ SALT): once per split.  The salt makes the decision independent of
// negsample_keep_row on the same seed and stream.
XF_ADMIT_HD uint64_t holdout_base(uint64_t seed, uint64_t stream) {
  return admit_mix64(seed ^ stream ^ XF_HOLDOUT_SALT);
}

// a row of this ordinal is held iff the top 32 bits of mix64(base + ordinal) are below T
XF_ADMIT_HD bool holdout_held_row(uint64_t base, uint64_t ordinal, uint64_t T) {
  return (admit_mix64(base + ordinal) >> 32) < T;
}

}  // namespace xf

#endif  // XF_HOLDOUT_H_
