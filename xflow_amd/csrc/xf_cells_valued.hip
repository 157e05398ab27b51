// xf_cells_valued.hip — feature values (feature_values = on) on the cells path, LR (gfx950): the
// valued forms of the forward and of the gradient + Push kernels over cells whose nonzeros carry
// a value each (xf_cells.h: vals[NNZ], in the order of `entries`).
//
//   wx_r  = fp32(sum_j fp32(w[row_j] x_j))                   gw = fp32(fp32(sum_occ fp32(loss_r x_occ)) / R)
// — the function of xf_valued.hip, sum for sum: every product is rounded to fp32 first, every
// sum is an fp64 sum (LDS atomics) of those fp32 values, rounded to fp32 once.  All values 1:
// the binary kernels' results bit for bit (w * 1 and loss * 1 are exact).
//
// Replaces (paths relative to the reference tree), with x in place of the reference's implicit 1:
//   LRWorker::calculate_loss           src/model/lr/lr_worker.cc:121-143  (k_lr_fwd_cells_valued)
//   LRWorker::calculate_gradient       src/model/lr/lr_worker.cc:100-119  (k_lr_grad_cells_valued)
//   KVWorker::Push -> FTRL / SGD       src/optimizer/ftrl.h:54-74, sgd.h:52 (fused in the same)
//
// Both kernels have the structure of their binary models (k_lr_fwd_cells, xf_cells_fwd.hip; the
// one-source MODE 0 shape of k_lr_grad_cells, xf_cells_grad.hip), which stay as they are: a
// binary minibatch runs the code it ran.  The value of an entry is loaded WITH the entry —
// coalesced, from the same offset of a parallel array — and never gathered.  Valued cells are one
// segment without holes (the sort-based local build, xf_cells_build.hip).  HBM-bound, no MFMA.
#include <rocprim/device/device_radix_sort.hpp>

#include "xf_cells_fwd.h"
#include "xf_cells_grad.h"

namespace {
// -------------------------------------------------------------------------------- build
// Valued cells: a nonzero's value rides through the sort with its entry as ONE 64-bit payload
// (value bits << 32 | entry), packed here from the two arrays k_cell_keys* and the caller left in
// the same order, and taken apart again behind the sort.
__global__ void __launch_bounds__(kBlock)
k_cell_pack_val(const uint32_t *__restrict__ ent, const float *__restrict__ xval, size_t n,
                uint64_t *__restrict__ pay) {
  XF_GRID_STRIDE(j, n)
  pay[j] = ((uint64_t)__float_as_uint(xval[j]) << 32) | ent[j];
}

__global__ void __launch_bounds__(kBlock)
k_cell_split_val(const uint64_t *__restrict__ pay, size_t n, uint32_t *__restrict__ entries,
                 float *__restrict__ vals) {
  XF_GRID_STRIDE(j, n) {
    const uint64_t p = pay[j];
    entries[j] = (uint32_t)p;
    vals[j] = __uint_as_float((uint32_t)(p >> 32));
  }
}

// ------------------------------------------------------------------------------ forward
// k_lr_fwd_cells with a value per entry: a block buffer grows by kFwdE floats, the fp32 product
// w * x is formed where the binary kernel forms wv[q].
struct FwdBlockV {
  FwdBlock E;
  float x[kFwdE];
};

__device__ __forceinline__ void fwd_load_v(FwdBlockV &B, const uint32_t *__restrict__ entries,
                                           const float *__restrict__ vals,
                                           const uint32_t *__restrict__ blk_cell, uint32_t b,
                                           uint32_t pb, uint32_t pe, uint32_t lane) {
  fwd_load(B.E, entries, blk_cell, b, pb, pe, lane);
#pragma unroll
  for (int q = 0; q < kFwdE; ++q) {
    const uint32_t j = b * kBlk + q * 64 + lane;
    B.x[q] = (j >= pb && j < pe) ? vals[j] : 0.0f;
  }
}

__device__ __forceinline__ void fwd_process_v(const FwdBlockV &B, uint32_t b, uint32_t c0,
                                              uint32_t nchunk, uint32_t lane,
                                              const uint32_t *__restrict__ cellptr,
                                              const float *__restrict__ w, double *wx) {
#pragma clang fp contract(off)
  // the block may begin in the window before and end in the one after
  const uint32_t lo = B.E.lo < c0 ? c0 : B.E.lo;
  const uint32_t hi = B.E.hi >= c0 + nchunk ? c0 + nchunk - 1 : B.E.hi;
  const bool near = hi - lo <= kTagMask;  // wave-uniform
  float wv[kFwdE];
#pragma unroll
  for (int q = 0; q < kFwdE; ++q) {
    const uint32_t e = B.E.ent[q];
    if (e == 0xFFFFFFFFu) continue;
    const uint32_t cell = near ? lo + (((e >> kTagShift) - (lo - c0)) & kTagMask)
                               : cell_of(cellptr, lo, hi, b * kBlk + q * 64 + lane);
    wv[q] = w[(size_t)(cell - c0) * kChunk + (e & (kChunk - 1))] * B.x[q];  // fp32(w x)
  }
#pragma unroll
  for (int q = 0; q < kFwdE; ++q) {
    const uint32_t e = B.E.ent[q];
    if (e != 0xFFFFFFFFu) atomicAdd(&wx[(e >> kChunkBits) & kRowMask], (double)wv[q]);
  }
}

// (16 wavefronts per workgroup: 128 VGPRs per lane; two buffers of 16 entries + 16 values + 2)
__global__ void __launch_bounds__(kFwdBlock)
k_lr_fwd_cells_valued(const uint32_t *__restrict__ entries, const float *__restrict__ vals,
                      const uint32_t *__restrict__ cellptr, const uint32_t *__restrict__ blk_cell,
                      uint32_t nchunk, uint32_t W, uint32_t G, const float *__restrict__ w,
                      double *__restrict__ partial) {
  __shared__ double wx[kWinMax];
  __shared__ uint32_t next_blk;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  // (group g of window v is block ((g / 8) * nwin + v) * 8 + g % 8: see k_lr_fwd_cells)
  const uint32_t nwin = gridDim.x / G;
  const uint32_t slot = blockIdx.x >> 3, v = slot % nwin, g = (slot / nwin) * 8 + (blockIdx.x & 7u);
  double *out = partial + ((size_t)v * G + g) * W;
  for (uint32_t r = tid; r < W; r += kFwdBlock) wx[r] = 0.0;
  const uint32_t c0 = v * nchunk;
  const uint32_t wb = cellptr[c0], we = cellptr[c0 + nchunk];
  const uint64_t n = we - wb;
  uint32_t pb = g == 0 ? wb : (uint32_t)((wb + n * g / G) & ~(uint64_t)(kBlk - 1));
  uint32_t pe = g == G - 1 ? we : (uint32_t)((wb + n * (g + 1) / G) & ~(uint64_t)(kBlk - 1));
  if (pb < wb) pb = wb;
  if (pe < pb) pe = pb;
  const uint32_t b_first = pb / kBlk, b_end = pb < pe ? (pe - 1) / kBlk + 1 : b_first;
  if (tid == 0) next_blk = b_first;
  __syncthreads();
  auto grab = [&]() -> uint32_t {  // the wavefront's next block
    uint32_t b = 0;
    if (lane == 0) b = atomicAdd(&next_blk, 1u);
    return (uint32_t)__shfl((int)b, 0);
  };
  // two block buffers that swap roles (no register copies), as in k_lr_fwd_cells
  FwdBlockV A, B;
  uint32_t ba = grab(), bb = 0;
  if (ba < b_end) fwd_load_v(A, entries, vals, blk_cell, ba, pb, pe, lane);
  while (ba < b_end) {
    bb = grab();
    if (bb < b_end) fwd_load_v(B, entries, vals, blk_cell, bb, pb, pe, lane);
    fwd_process_v(A, ba, c0, nchunk, lane, cellptr, w, wx);
    if (bb >= b_end) break;
    ba = grab();
    if (ba < b_end) fwd_load_v(A, entries, vals, blk_cell, ba, pb, pe, lane);
    fwd_process_v(B, bb, c0, nchunk, lane, cellptr, w, wx);
  }
  __syncthreads();
  for (uint32_t r = tid; r < W; r += kFwdBlock) out[r] = wx[r];
}

// ------------------------------------------------------------------- gradient + Push
// The one-source, MODE 0 shape of k_lr_grad_cells with a value per entry: one work item is one
// (chunk, slice), kGradE entries per lane and round, the value loaded with the entry, and
// l[q] = fp32(loss[row] * x) before add_keys_folded.  From there on nothing knows about values:
// the sparse-list and the sweep update phases step the touched keys in place (apply through
// w_of_nz as the binary kernel), the slices of a split chunk add into gsum / gtouched and
// k_lr_grad_split_finish does the rest.  A key whose values are all zero is touched and stepped
// with g = +0 (a sum starts from +0; -0 addends leave it there), as on the generic path.
template <int OPT>
__global__ void __launch_bounds__(kBlock, 6)
k_lr_grad_cells_valued(xf::TableDev T, const uint32_t *__restrict__ entries,
                       const float *__restrict__ vals, const uint32_t *__restrict__ cellptr,
                       uint32_t nchunk, uint32_t nwin, uint32_t W,
                       const uint32_t *__restrict__ item_chunk,
                       const uint32_t *__restrict__ item_slice,
                       const uint32_t *__restrict__ item_dump, const float *__restrict__ loss,
                       uint32_t R, uint32_t M, double *__restrict__ gsum,
                       uint8_t *__restrict__ gtouched, uint32_t chunk0) {
#pragma clang fp contract(off)
  __shared__ double acc[kChunk];
  __shared__ uint8_t touched[kChunk];
  __shared__ uint32_t cum[kGradWin + 1], sbase[kGradWin];
  __shared__ uint32_t nlist;
  const uint32_t tid = threadIdx.x;
  // the old weight of a step derived from the row's (n, z) instead of read (TableDev::w_of_nz)
  const bool wnz = OPT == XF_OPT_FTRL && T.w_of_nz;
  if (tid == 0) nlist = 0;
  const uint32_t c = item_chunk[blockIdx.x];
  const uint32_t sl = item_slice[blockIdx.x], s = sl & 0xFFFFu, S = sl >> 16;
  for (uint32_t k = tid; k < kChunk; k += kBlock) {
    acc[k] = 0.0;
    touched[k] = 0;
  }
  // the item's share of the chunk's cells as ONE index space, kGradWin windows at a time
  for (uint32_t v0 = 0; v0 < nwin; v0 += kGradWin) {
    const uint32_t nv = min(nwin - v0, kGradWin);
    __syncthreads();
    if (tid < nv) {
      const size_t cell = (size_t)(v0 + tid) * nchunk + c;
      const uint32_t b = cellptr[cell], e = cellptr[cell + 1];
      const uint64_t n = e - b;
      sbase[tid] = b + (uint32_t)(n * s / S);
      cum[tid + 1] = (uint32_t)(n * (s + 1) / S) - (uint32_t)(n * s / S);
    }
    __syncthreads();
    if (tid == 0) {
      cum[0] = 0;
      for (uint32_t v = 0; v < nv; ++v) cum[v + 1] += cum[v];
    }
    __syncthreads();
    const uint32_t total = cum[nv];
    for (uint32_t p0 = 0; p0 < total; p0 += kBlock * kGradE) {  // workgroup-uniform trip count
      uint32_t ent[kGradE], vq[kGradE];
      float l[kGradE];  // the entry's value, then fp32(loss x)
      uint32_t v = 0;   // (p ascends with q: v never goes back)
#pragma unroll
      for (int q = 0; q < kGradE; ++q) {
        const uint32_t p = p0 + q * kBlock + tid;
        ent[q] = 0xFFFFFFFFu;
        vq[q] = 0;
        l[q] = 0.0f;
        if (p < total) {
          while (p >= cum[v + 1]) ++v;
          vq[q] = v;
          const uint32_t j = sbase[v] + (p - cum[v]);
          ent[q] = entries[j];
          l[q] = vals[j];
        }
      }
#pragma unroll
      for (int q = 0; q < kGradE; ++q)
        l[q] = ent[q] != 0xFFFFFFFFu
                   ? loss[(size_t)(v0 + vq[q]) * W + ((ent[q] >> kChunkBits) & kRowMask)] * l[q]
                   : 0.0f;
      add_keys_folded<kGradE>(acc, touched, ent, l);
    }
  }
  __syncthreads();
  if (S > 1) {  // a slice of a split chunk: into the chunk's accumulators in HBM
    const size_t slot = item_dump[blockIdx.x];
    for (uint32_t k = tid; k < kChunk; k += kBlock)
      if (touched[k]) {
        unsafeAtomicAdd(&gsum[slot * kChunk + k], acc[k]);
        gtouched[slot * kChunk + k] = 1;
      }
    return;
  }
  const size_t row0 = (size_t)(chunk0 + c) * kChunk;
  // few touched keys: listed (in the bytes of `touched`) and stepped with all lanes busy
  if constexpr (kChunk == kBlock * 8) {
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (touched[i * kBlock + tid] && row0 + i * kBlock + tid < M) mine |= 1u << i;
    const uint32_t cnt = (uint32_t)__popc(mine), lane = tid & 63u;
    uint32_t inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o);
      if ((int)lane >= o) inc += u;
    }
    uint32_t base = 0;
    if (lane == 63) base = atomicAdd(&nlist, inc);
    base = (uint32_t)__shfl((int)base, 63);
    __syncthreads();
    const uint32_t n = nlist;
    if (n <= kSparseKeys) {  // workgroup-uniform
      uint16_t *list = (uint16_t *)touched;
      uint32_t pos = base + inc - cnt;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (mine >> i & 1u) list[pos++] = (uint16_t)(i * kBlock + tid);
      __syncthreads();
      constexpr int kS = (int)(kSparseKeys / kBlock);
      uint32_t k[kS];
      float g[kS], sw[kS], sn[kS], sz[kS];
#pragma unroll
      for (int i = 0; i < kS; ++i) {
        const uint32_t j = i * kBlock + tid;
        k[i] = j < n ? list[j] : 0xFFFFFFFFu;
        const size_t r = row0 + (j < n ? k[i] : 0u);
        g[i] = j < n ? xf::div_by_rows((float)acc[k[i]], R) : 0.0f;  // lr_worker.cc:117
        sw[i] = 0.0f;
        if (!wnz) sw[i] = T.w[r];
        sn[i] = sz[i] = 0.0f;
        if (OPT == XF_OPT_FTRL) xf::load_nz(T, r, sn[i], sz[i]);
      }
#pragma unroll
      for (int i = 0; i < kS; ++i) {
        if (k[i] == 0xFFFFFFFFu) continue;
        if (wnz) sw[i] = xf::ftrl_w_of(T.alpha, T.inv_alpha, T.beta, T.lambda1, T.lambda2, sn[i], sz[i]);
        if (OPT == XF_OPT_FTRL)
          xf::ftrl_step(T.alpha, T.inv_alpha, T.beta, T.lambda1, T.lambda2, g[i], sw[i], sn[i], sz[i]);
        else
          sw[i] = xf::sgd_step(T.lr, g[i], sw[i]);
      }
#pragma unroll
      for (int i = 0; i < kS; ++i) {
        if (k[i] == 0xFFFFFFFFu) continue;
        T.w[row0 + k[i]] = sw[i];
        if (OPT == XF_OPT_FTRL) xf::store_nz(T, row0 + k[i], sn[i], sz[i]);
      }
      return;
    }
  }
  // eight keys per thread at a time in three sweeps: every state row requested, stepped, stored
  for (uint32_t kb = 0; kb < kChunk; kb += kBlock * 8) {
    bool t[8];
    float g[8], sw[8], sn[8], sz[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t k = kb + i * kBlock + tid;
      t[i] = k < kChunk && touched[k] != 0;
      g[i] = 0.0f;
      if (t[i]) {
        g[i] = xf::div_by_rows((float)acc[k], R);  // lr_worker.cc:117
        t[i] = row0 + k < M;
      }
      // (an idle slot loads the chunk's first row: no load under a branch)
      const size_t r = t[i] ? row0 + k : row0;
      sw[i] = 0.0f;
      if (!wnz) sw[i] = T.w[r];
      sn[i] = sz[i] = 0.0f;
      if (OPT == XF_OPT_FTRL) xf::load_nz(T, r, sn[i], sz[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (!t[i]) continue;
      if (wnz) sw[i] = xf::ftrl_w_of(T.alpha, T.inv_alpha, T.beta, T.lambda1, T.lambda2, sn[i], sz[i]);
      if (OPT == XF_OPT_FTRL)
        xf::ftrl_step(T.alpha, T.inv_alpha, T.beta, T.lambda1, T.lambda2, g[i], sw[i], sn[i], sz[i]);
      else
        sw[i] = xf::sgd_step(T.lr, g[i], sw[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (!t[i]) continue;
      T.w[row0 + kb + i * kBlock + tid] = sw[i];
      if (OPT == XF_OPT_FTRL) xf::store_nz(T, row0 + kb + i * kBlock + tid, sn[i], sz[i]);
    }
  }
}
}  // namespace

namespace xf {

// the sort of cells_build (xf_cells_build.hip) for valued cells, in this file so that the binary
// build's instantiation of the library sort stays the only one in its own
int cells_sort_valued(const uint32_t *cid, uint32_t *cid_s, const uint32_t *ent,
                      const float *xval, uint32_t n, int bits, uint32_t *entries, float *vals,
                      hipStream_t s) {
  Scratch sc;
  uint64_t *pay = nullptr, *pay_s = nullptr;
  XF_TRY(sc.get(&pay, n));
  XF_TRY(sc.get(&pay_s, n));
  hipLaunchKernelGGL(k_cell_pack_val, dim3(grid_for((size_t)n)), dim3(kBlock), 0, s, ent, xval,
                     (size_t)n, pay);
  size_t tb = 0;
  XF_HIP(rocprim::radix_sort_pairs(nullptr, tb, cid, cid_s, pay, pay_s, (size_t)n, 0, bits, s));
  void *tmp = nullptr;
  XF_TRY(sc.get((char **)&tmp, tb));
  XF_HIP(rocprim::radix_sort_pairs(tmp, tb, cid, cid_s, pay, pay_s, (size_t)n, 0, bits, s));
  hipLaunchKernelGGL(k_cell_split_val, dim3(grid_for((size_t)n)), dim3(kBlock), 0, s, pay_s,
                     (size_t)n, entries, vals);
  XF_HIP(hipGetLastError());
  return XF_OK;
}

int cells_lr_forward_valued(const xf_cells *c, const float *d_w, const int32_t *d_labels,
                            double *d_partial, float *d_loss, float *d_pctr, hipStream_t s,
                            float neg_weight) {
  XF_REQUIRE(c && d_w && d_partial && (d_loss || d_pctr),
             "cells_lr_forward_valued: null argument");
  XF_REQUIRE(!c->next && c->chunk0 == 0 && c->entries_k == c->entries && (c->vals || c->NNZ == 0),
             "cells_lr_forward_valued: valued cells are one segment with their values and no "
             "key-sorted copy");
  if (c->R == 0) return XF_OK;
  hipLaunchKernelGGL(k_lr_fwd_cells_valued, dim3(c->nwin * c->G), dim3(kFwdBlock), 0, s, c->entries,
                     c->vals, c->cellptr, c->blk_cell, c->nchunk, c->W, c->G, d_w, d_partial);
  XF_HIP(hipGetLastError());
  return cells_lr_finalize(c, d_partial, d_labels, d_loss, d_pctr, s, neg_weight);
}

int cells_lr_grad_update_valued(const xf_cells *c, const xf_table *t, const float *d_loss,
                                hipStream_t s) {
  XF_REQUIRE(c && t && d_loss, "cells_lr_grad_update_valued: null argument");
  XF_REQUIRE(c->mode == kCellsTableRows, "cells_lr_grad_update_valued: cells are not table rows");
  XF_REQUIRE(!c->next && c->chunk0 == 0 && (c->vals || c->NNZ == 0),
             "cells_lr_grad_update_valued: valued cells are one segment with their values");
  TableDev T = table_dev(t);
  XF_REQUIRE(T.dim == 1, "cells_lr_grad_update_valued: dim must be 1");
  table_note_write(const_cast<xf_table *>(t));
  if (c->nitems == 0) return XF_OK;
  if (path_switch(kPathOldWeight) == 1) T.w_of_nz = false;  // (old_weight = read, xf_common.h)
  if (c->nsplit_chunks) {
    if (c->split_dirty) XF_HIP(hipMemsetAsync(c->gsum, 0, c->split_bytes, s));
    c->split_dirty = true;  // (until the finish kernel that cleans them is in the stream)
  }
  const int opt = T.nz != nullptr ? XF_OPT_FTRL : XF_OPT_SGD;
  if (opt == XF_OPT_FTRL)
    hipLaunchKernelGGL(k_lr_grad_cells_valued<XF_OPT_FTRL>, dim3(c->nitems), dim3(kBlock), 0, s, T,
                       c->entries, c->vals, c->cellptr, c->nchunk, c->nwin, c->W, c->item_chunk,
                       c->item_slice, c->item_dump, d_loss, c->R, c->M, c->gsum, c->gtouched,
                       c->chunk0);
  else
    hipLaunchKernelGGL(k_lr_grad_cells_valued<XF_OPT_SGD>, dim3(c->nitems), dim3(kBlock), 0, s, T,
                       c->entries, c->vals, c->cellptr, c->nchunk, c->nwin, c->W, c->item_chunk,
                       c->item_slice, c->item_dump, d_loss, c->R, c->M, c->gsum, c->gtouched,
                       c->chunk0);
  XF_HIP(hipGetLastError());
  XF_TRY(cells_launch_split_finish(opt, c, T, s));
  c->split_dirty = false;
  return XF_OK;
}

}  // namespace xf
