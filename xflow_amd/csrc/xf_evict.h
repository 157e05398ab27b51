// xf_evict.h — the eviction kernels' launches (xf_evict.hip), called by xf_table_evict.
#ifndef XF_EVICT_H_
#define XF_EVICT_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xf {

// blocks of rows / 64-bit mask words the passes over n rows use (the mask's allocation)
size_t evict_blocks(size_t n);
size_t evict_mask_words(size_t n);
// rows [0, n) judged: mask[evict_mask_words(n)] = the keep bits, cnt[evict_blocks(n) + 1] = the
// exclusive scan of the blocks' survivor counts, the total last.  In stream order.
int evict_mark_scan(const float *w, const float2 *nz, size_t n, float n_below,
                    unsigned long long *mask, uint32_t *cnt, hipStream_t s);
// the survivors' keys, w and nz at their ranks in out_keys / w2 / nz2
int evict_compact(const uint64_t *keys, const float *w, const float2 *nz, size_t n,
                  const unsigned long long *mask, const uint32_t *base, uint64_t *out_keys,
                  float *w2, float2 *nz2, hipStream_t s);

}  // namespace xf
#endif  // XF_EVICT_H_
