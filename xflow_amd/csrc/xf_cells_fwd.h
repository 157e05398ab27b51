// xf_cells_fwd.h — device helpers of the forward kernels over cells (internal; included by
// xf_cells_fwd.hip and xf_cells_valued.hip).
#ifndef XF_CELLS_FWD_H_
#define XF_CELLS_FWD_H_

#include "xf_cells_impl.h"

namespace {
// the cell of entry j, known to lie in [lo, hi]: the largest c with cellptr[c] <= j
__device__ __forceinline__ uint32_t cell_of(const uint32_t *__restrict__ cellptr, uint32_t lo,
                                            uint32_t hi, uint32_t j) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (cellptr[mid] <= j) lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

constexpr int kFwdE = (int)(kBlk / 64);

struct FwdBlock {
  uint32_t ent[kFwdE];
  uint32_t lo, hi;
};

__device__ __forceinline__ void fwd_load(FwdBlock &B, const uint32_t *__restrict__ entries,
                                         const uint32_t *__restrict__ blk_cell, uint32_t b,
                                         uint32_t pb, uint32_t pe, uint32_t lane) {
  B.lo = blk_cell[b];
  B.hi = blk_cell[b + 1];
#pragma unroll
  for (int q = 0; q < kFwdE; ++q) {
    const uint32_t j = b * kBlk + q * 64 + lane;
    B.ent[q] = (j >= pb && j < pe) ? entries[j] : 0xFFFFFFFFu;
  }
}

}  // namespace

namespace xf {
// loss / pctr of every row from the window workgroups' partial sums (k_lr_finalize_cells);
// neg_weight: as cells_lr_forward's
int cells_lr_finalize(const xf_cells *c, const double *d_partial, const int32_t *d_labels,
                      float *d_loss, float *d_pctr, hipStream_t s, float neg_weight = 1.0f);
}  // namespace xf

#endif  // XF_CELLS_FWD_H_
