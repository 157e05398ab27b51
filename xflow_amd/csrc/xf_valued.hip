// xf_valued.hip — feature values (feature_values = on, gfx950), LR: a nonzero contributes x = val
// instead of 1, on the generic compiled minibatch, whose two value arrays run beside its two
// views: xval[NNZ] beside uidx (CSR order), coo_val[NNZ] beside coo_row (grouped by key).
//
//   wx_r    = fp32(sum_j fp32(w[u_j] x_j))          gw[u] = fp32(fp32(sum_occ fp32(loss_r x_occ)) / R)
// Every fp64 sum adds fp32 values, as in xf_fm_canonical.hip, whose kernels are the valued
// canonical FM (VAL = true).  The values are streamed with the index they belong to (coalesced,
// next to uidx / coo_row), never gathered.
//
// On the GENERIC minibatch a valued LR step is the w half of the canonical step — Pull of the
// key list, a wavefront per row over the CSR, the gradient tiles with the optimizer step in place,
// heavy keys through the canonical pair of kernels with k = 0.  (The valued form of LR's cell
// kernels, on a local minibatch whose cells carry the values: xf_cells_valued.hip.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "xf_common.h"
#include "xf_device.h"
#include "xf_fm_canonical.h"
#include "xf_wave.h"

namespace xf {
const TableDev &table_dev(const xf_table *t);
}

namespace {

constexpr int kBlock = 256;
using xf::blocks_for_groups;
using xf::group_sum;

// ---------------------------------------------------------------------------- forward, LR
// a wavefront per row, a lane per nonzero, four gathers of w in flight per lane
__global__ void __launch_bounds__(kBlock)
k_val_lr_forward(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ uidx,
                 const float *__restrict__ xval, const float *__restrict__ wu,
                 const int32_t *__restrict__ labels, uint32_t R, float *__restrict__ loss,
                 float *__restrict__ pctr) {
#pragma clang fp contract(off)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nwaves = gridDim.x * (kBlock / 64);
  for (uint32_t r = blockIdx.x * (kBlock / 64) + threadIdx.x / 64; r < R; r += nwaves) {
    const uint32_t b = rowptr[r], n = rowptr[r + 1] - b;
    double wx = 0.0;
    for (uint32_t j0 = lane; j0 < n; j0 += 4 * 64) {
      uint32_t ui[4];
      float xv[4], ww[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool in = j0 + i * 64 < n;
        ui[i] = in ? uidx[b + j0 + i * 64] : 0xFFFFFFFFu;
        xv[i] = in ? xval[b + j0 + i * 64] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) ww[i] = ui[i] != 0xFFFFFFFFu ? wu[ui[i]] : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) wx += (double)(ww[i] * xv[i]);
    }
    wx = group_sum<64>(wx);
    if (lane == 0) {
      const float p = xf::sigmoid_ref((float)wx);
      if (pctr) pctr[r] = p;
      loss[r] = p - (float)labels[r];
    }
  }
}

// ------------------------------------------------------------- gradient + Push, LR
// the w half of k_fmc_grad_tiled<OPT, K, true>: a tile's loss x in LDS, a lane per key
// (OPT = xf::kOptEmit: gw[u] written and nothing stepped — TW, wu and rows_w are not read)
template <int OPT>
__global__ void __launch_bounds__(kBlock)
k_val_lr_grad_tiled(xf::TableDev TW, const uint32_t *__restrict__ tile_ptr, uint32_t ntiles,
                    const uint32_t *__restrict__ segptr, const uint32_t *__restrict__ coo_row,
                    const float *__restrict__ coo_val, const float *__restrict__ loss,
                    const float *__restrict__ wu, const uint32_t *__restrict__ rows_w, uint32_t R,
                    float *__restrict__ gw) {
#pragma clang fp contract(off)
  __shared__ float lx[XF_GRAD_TILE_NNZ];
  __shared__ uint32_t sp[XF_GRAD_TILE_KEYS + 1];
  const uint32_t tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t ua = tile_ptr[tile], ub = tile_ptr[tile + 1], nk = ub - ua;
    const uint32_t j0 = segptr[ua], j1 = segptr[ub];
    if (nk == 1 && j1 - j0 > XF_HEAVY_SEG) continue;
    for (uint32_t q = tid; q <= nk; q += kBlock) sp[q] = segptr[ua + q] - j0;
    for (uint32_t j = j0 + tid; j < j1; j += kBlock) lx[j - j0] = loss[coo_row[j]] * coo_val[j];
    __syncthreads();
    for (uint32_t q = tid; q < nk; q += kBlock) {
      double aw = 0.0;
      for (uint32_t j = sp[q]; j < sp[q + 1]; ++j) aw += (double)lx[j];
      const float g1 = xf::div_by_rows((float)aw, R);
      gw[ua + q] = g1;
      if constexpr (OPT != xf::kOptEmit) xf::step_coord<OPT>(TW, rows_w[ua + q], wu[ua + q], g1);
    }
    __syncthreads();
  }
}

}  // namespace

namespace xf {

// loss[R], pctr[R] (may be null) from the pulled w and the values in CSR order
int val_lr_forward(const xf_dev_batch *b, const float *d_xval, const float *d_wu, float *d_loss,
                   float *d_pctr, hipStream_t s) {
  XF_REQUIRE(b && d_wu && d_loss && (d_xval || b->NNZ == 0), "valued lr forward: bad argument");
  if (b->R == 0) return XF_OK;
  hipLaunchKernelGGL(k_val_lr_forward, dim3(blocks_for_groups(b->R, kBlock / 64)), dim3(kBlock), 0,
                     s, b->rowptr, b->uidx, d_xval, d_wu, b->labels, b->R, d_loss, d_pctr);
  XF_HIP(hipGetLastError());
  return XF_OK;
}

// the tile kernel and the heavy keys' two for one OPT (an optimizer, or kOptEmit)
static int val_lr_grad_launch(int opt, const TableDev &TW, const xf_dev_batch *b,
                              const float *d_coo_val, const uint32_t *d_rows_w, const float *d_wu,
                              const float *d_loss, float *d_gw, double *d_hpart, hipStream_t s) {
  XF_REQUIRE(b->ntiles && b->tile_ptr, "valued lr gradient: the minibatch has no gradient tiles");
  XF_REQUIRE(!b->H || (b->heavy_chunk_ptr && d_hpart),
             "valued lr gradient: heavy keys without their chunks or scratch");
  const dim3 gt((unsigned)std::min<uint32_t>(b->ntiles, 1u << 16)), blk(kBlock);
  if (opt == kOptEmit)
    hipLaunchKernelGGL(k_val_lr_grad_tiled<kOptEmit>, gt, blk, 0, s, TW, b->tile_ptr, b->ntiles,
                       b->segptr, b->coo_row, d_coo_val, d_loss, d_wu, d_rows_w, b->R, d_gw);
  else if (opt == XF_OPT_FTRL)
    hipLaunchKernelGGL(k_val_lr_grad_tiled<XF_OPT_FTRL>, gt, blk, 0, s, TW, b->tile_ptr, b->ntiles,
                       b->segptr, b->coo_row, d_coo_val, d_loss, d_wu, d_rows_w, b->R, d_gw);
  else
    hipLaunchKernelGGL(k_val_lr_grad_tiled<XF_OPT_SGD>, gt, blk, 0, s, TW, b->tile_ptr, b->ntiles,
                       b->segptr, b->coo_row, d_coo_val, d_loss, d_wu, d_rows_w, b->R, d_gw);
  XF_HIP(hipGetLastError());
  if (b->H) {
    fmc_heavy_update(opt, TW, TW, 0, b, d_rows_w, d_rows_w, d_wu, d_wu, nullptr, d_loss, d_gw,
                     nullptr, d_hpart, d_coo_val, s);
    XF_HIP(hipGetLastError());
  }
  return XF_OK;
}

// gradient + Push of w with the values in key-grouped order.  d_hpart: n_heavy_chunks doubles
// (fmc_heavy_doubles(b, 0)).
int val_lr_grad_update(xf_table *tw, const xf_dev_batch *b, const float *d_coo_val,
                       const uint32_t *d_rows_w, const float *d_wu, const float *d_loss,
                       float *d_gw, double *d_hpart, hipStream_t s) {
  XF_REQUIRE(tw && b && d_coo_val && d_rows_w && d_wu && d_loss && d_gw,
             "valued lr gradient: null argument");
  if (b->U == 0) return XF_OK;
  const xf::TableDev &TW = xf::table_dev(tw);
  return val_lr_grad_launch(TW.nz != nullptr ? XF_OPT_FTRL : XF_OPT_SGD, TW, b, d_coo_val, d_rows_w,
                            d_wu, d_loss, d_gw, d_hpart, s);
}

// The gradient alone, for a worker whose keys live on other ranks (as fmc_grad_emit): gw[U],
// every entry written; no table, state row or pulled w is read.
int val_lr_grad_emit(const xf_dev_batch *b, const float *d_coo_val, const float *d_loss,
                     float *d_gw, double *d_hpart, hipStream_t s) {
  XF_REQUIRE(b, "valued lr gradient (emit): null argument");
  if (b->U == 0) return XF_OK;  // (no key: nothing to write, and the arrays may be empty)
  XF_REQUIRE(d_coo_val && d_loss && d_gw, "valued lr gradient (emit): null argument");
  const TableDev none{};
  return val_lr_grad_launch(kOptEmit, none, b, d_coo_val, nullptr, nullptr, d_loss, d_gw, d_hpart,
                            s);
}

}  // namespace xf
