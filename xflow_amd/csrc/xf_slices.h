// xf_slices.h — sliced progressive validation (xf_slices.hip, xf_slices_host.cc): what the host
// and the device side share — the home slot of a slice's key and what one row adds to its slice —
// and the host-only pieces (the parameter check, the table of row terms) that need no GPU.
#ifndef XF_SLICES_H_
#define XF_SLICES_H_

#include <stdint.h>

#include "xf_admit.h"     // XF_ADMIT_HD, admit_mix64
#include "xf_progress.h"  // progress_rank
#include "xflow_amd.h"    // XF_SLICE_NONE, XF_SLICE_WORDS

namespace xf {

// the seven words of a slice, in this order
enum : uint32_t { kSlN0 = 0, kSlN1, kSlQ0, kSlQ1, kSlLl0, kSlLl1, kSlOther };
static_assert(XF_SLICE_WORDS == kSlOther + 1, "n[2], qsum[2], llsum[2], other");

constexpr int kSlicesMinLog2 = 2, kSlicesMaxLog2 = 26;
constexpr uint32_t kSlicesProbeMax = 128;

// home(key, b) = mix64(key) >> (64 - b), b in 2 .. 26
XF_ADMIT_HD uint64_t slices_home(uint64_t key, int b) { return admit_mix64(key) >> (64 - b); }
// probes of the global table: min(2^b, 128)
XF_ADMIT_HD uint32_t slices_probes(int b) {
  return (1ull << b) < kSlicesProbeMax ? (uint32_t)(1ull << b) : kSlicesProbeMax;
}

// q * 2^31 truncated: q = |loss| <= 1, so the product is exact (a power of two) and fits 32 bits
XF_ADMIT_HD uint32_t slices_qfix(float loss) {
  const float q = loss < 0.0f ? -loss : loss;
  return (uint32_t)(q * 2147483648.0f);
}

// ---- host only (xf_slices_host.cc)
// F in 0 .. 2^31 - 1, b in 2 .. 26: XF_EINVAL naming `who` and the offender
int slices_check_params(const char *who, long long F, long long b);
// out[rank] = (uint32) llrint(progress_term(rank) * 2^24), XF_PROGRESS_RANKS words
void slices_terms(uint32_t *out);

}  // namespace xf

struct xf_slices;

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace xf {
// the slices' counters += rows [0, R) on `s` (k_sl_accumulate); R == 0 or no ids: no launch
int slices_accumulate(xf_slices *sl, const float *loss, const int32_t *labels, const uint64_t *id,
                      uint32_t R, hipStream_t s);
}  // namespace xf
#endif

#endif  // XF_SLICES_H_
