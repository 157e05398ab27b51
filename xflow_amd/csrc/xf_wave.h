// xf_wave.h — small device and launch helpers shared by the FM / LR model kernels
// (xf_model.hip, xf_fm_canonical.hip).
#ifndef XF_WAVE_H_
#define XF_WAVE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xf {

// butterfly sum over groups of G lanes (every lane of a group returns the group's sum)
template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}

// the heavy key that owns chunk c: the largest h with hch[h] <= c (hch ascends, H + 1 entries)
__device__ __forceinline__ uint32_t heavy_of_chunk(const uint32_t *__restrict__ hch, uint32_t H,
                                                   uint32_t c) {
  uint32_t lo = 0, hi = H;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (hch[mid] <= c) lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// workgroups for n_items items of items_per_block each, at least one, at most 8192 (grid-stride)
inline int blocks_for_groups(uint32_t n_items, int items_per_block) {
  size_t g = ((size_t)n_items + items_per_block - 1) / items_per_block;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace xf
#endif  // XF_WAVE_H_
