// xf_cross.h — feature crosses (xf_cross.hip): what the host and the device side share — the key of
// a crossed nonzero — and the host-only pieces (the spec's parser and check, xf_cross_host.cc) that
// need no GPU.
#ifndef XF_CROSS_H_
#define XF_CROSS_H_

#include <stdint.h>

#include "xf_admit.h"  // admit_mix64: xf_device.h's mix64 for both sides

namespace xf {

constexpr int kCrossMaxPairs = 32;

// salt(fa, fb) = mix64(fa << 32 | fb): once per pair, not per nonzero
XF_ADMIT_HD uint64_t cross_salt(int32_t fa, int32_t fb) {
  return admit_mix64((uint64_t)(uint32_t)fa << 32 | (uint32_t)fb);
}

// cross_key = mix64(mix64(ka ^ salt) + kb), 64-bit wrapping
XF_ADMIT_HD uint64_t cross_key_salted(uint64_t ka, uint64_t kb, uint64_t salt) {
  return admit_mix64(admit_mix64(ka ^ salt) + kb);
}
XF_ADMIT_HD uint64_t cross_key(uint64_t ka, uint64_t kb, int32_t fa, int32_t fb) {
  return cross_key_salted(ka, kb, cross_salt(fa, fb));
}

// a + b, or 2^64 - 1 where the sum leaves 64 bits (the stage's totals: associative, so a scan may
// use it)
XF_ADMIT_HD uint64_t cross_sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? ~0ull : s;
}

// ---- host only (xf_cross_host.cc)
// 1 .. 32 pairs, fa != fb, both in 0 .. 2^31 - 1, no pair twice: XF_EINVAL naming `who` and the
// offending pair
int cross_check_spec(const char *who, const int32_t *fa, const int32_t *fb, long npairs);
// fgid_base >= 0 and fgid_base + npairs <= 2^31: the crossed nonzeros' fgids are int32
int cross_check_base(const char *who, long fgid_base, long npairs);
// the row-shape knobs of the emit (xf_tune cross_short_max, cross_lds_chunks)
uint32_t cross_short_max();
uint32_t cross_lds_chunks();
int cross_set_knob(const char *name, double value);  // XF_OK, or -1: not a knob of this stage

}  // namespace xf
#endif  // XF_CROSS_H_
