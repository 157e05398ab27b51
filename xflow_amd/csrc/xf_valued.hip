// xf_valued.hip — feature values (feature_values = on, gfx950): a nonzero contributes x = val
// instead of 1.  LR and canonical FM on the generic compiled minibatch, whose two value arrays
// run beside its two views: xval[NNZ] beside uidx (CSR order), coo_val[NNZ] beside coo_row
// (grouped by key).
//
//   wx_r    = fp32(sum_j fp32(w[u_j] x_j))          gw[u] = fp32(fp32(sum_occ fp32(loss_r x_occ)) / R)
//   a_jf    = fp32(v[u_j,f] x_j)                    S[r,f] = fp32(sum_j a_jf)
//   y2_r    = fp32(0.5 (sum_f fp32(S[r,f]^2) - sum_f sum_j fp32(a_jf^2)))
//   gv[u,f] = fp32(fp32(sum_occ fp32(fp32(loss_r x_occ) fp32(S[r,f] - a_occ,f))) / R)
// Every fp64 sum adds fp32 values, as in xf_fm_canonical.hip; with every x = 1 each product above
// is exact and the results are, bit for bit, those of the binary kernels (canonical FM; LR's cells
// path).  The kernels are those of xf_fm_canonical.hip with the value where the function puts it —
// a second set: the binary instantiations stay the code they are.  The values are streamed with
// the index they belong to (coalesced, next to uidx / coo_row), never gathered.
//
// LR has no valued form of its cell kernels: a valued LR step is the w half of the canonical
// step — Pull of the key list, a wavefront per row over the CSR, the gradient tiles with the
// optimizer step in place, heavy keys in chunks (the finish kernel is the canonical one, k = 0).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "xf_common.h"
#include "xf_device.h"
#include "xf_wave.h"

namespace xf {
const TableDev &table_dev(const xf_table *t);
void fmc_heavy_finish(const TableDev &TW, const TableDev &TV, int k, const xf_dev_batch *b,
                      const double *d_hpart, const uint32_t *d_rows_w, const uint32_t *d_rows_v,
                      const float *d_wu, const float *d_vu, float *d_gw, hipStream_t s);
}  // namespace xf

namespace {

constexpr int kBlock = 256;
using xf::blocks_for_groups;
using xf::group_sum;
using xf::heavy_of_chunk;

// ---------------------------------------------------------------------------- forward, FM
// k_fmc_forward with a = v x in place of v and w x in place of w; a lane's value loads sit at
// the addresses of its index loads
template <int P, bool EXACT>
__global__ void __launch_bounds__(kBlock)
k_val_fm_forward(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ uidx,
                 const float *__restrict__ xval, const float *__restrict__ wu,
                 const float *__restrict__ vu, int k_rt, const int32_t *__restrict__ labels,
                 uint32_t R, float *__restrict__ loss, float *__restrict__ pctr,
                 float *__restrict__ S) {
#pragma clang fp contract(off)
  static_assert(P >= 1 && P <= 64 && (P & (P - 1)) == 0, "P: a power of two <= 64");
  const uint32_t k = EXACT ? (uint32_t)P : (uint32_t)k_rt;
  constexpr uint32_t kG = 64u / P;
  const uint32_t lane = threadIdx.x & 63u, f = lane % P, sub = lane / P;
  const uint32_t nwaves = gridDim.x * (kBlock / 64);
  for (uint32_t r = blockIdx.x * (kBlock / 64) + threadIdx.x / 64; r < R; r += nwaves) {
    const uint32_t b = rowptr[r], n = rowptr[r + 1] - b;
    double wx = 0.0, t = 0.0, q = 0.0;
    for (uint32_t f0 = 0; f0 < k; f0 += P) {
      const uint32_t fk = f0 + f;
      const bool on = fk < k;
      double s = 0.0;
      for (uint32_t j0 = sub; j0 < n; j0 += 4 * kG) {
        uint32_t ui[4];
        float xv[4], vv[4], ww[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool in = j0 + i * kG < n;
          ui[i] = in ? uidx[b + j0 + i * kG] : 0xFFFFFFFFu;
          xv[i] = in ? xval[b + j0 + i * kG] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          vv[i] = (on && ui[i] != 0xFFFFFFFFu) ? vu[(size_t)ui[i] * k + fk] : 0.0f;
          ww[i] = (f0 == 0 && f == 0 && ui[i] != 0xFFFFFFFFu) ? wu[ui[i]] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float a = vv[i] * xv[i];  // fp32 products, here and below
          s += (double)a;
          q += (double)(a * a);
          wx += (double)(ww[i] * xv[i]);
        }
      }
#pragma unroll
      for (uint32_t off = P; off < 64; off <<= 1) s += __shfl_xor(s, (int)off);
      const float sf = (float)s;
      if (sub == 0 && on) {
        S[(size_t)r * k + fk] = sf;
        t += (double)(sf * sf);
      }
    }
    t = group_sum<64>(t);
    q = group_sum<64>(q);
    wx = group_sum<64>(wx);
    if (lane == 0) {
      const float y2 = (float)(0.5 * (t - q));
      const float p = xf::sigmoid_ref((float)wx + y2);
      if (pctr) pctr[r] = p;
      loss[r] = p - (float)labels[r];
    }
  }
}

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

// the optimizer step of one key's w (the last lines of k_fmc_grad_tiled)
template <int OPT>
__device__ __forceinline__ void step_w(const xf::TableDev &TW, uint32_t rw, float w_old, float g) {
  if (OPT == XF_OPT_FTRL) {
    float w = w_old, nn, z;
    xf::load_nz(TW, rw, nn, z);
    xf::ftrl_step(TW.alpha, TW.inv_alpha, TW.beta, TW.lambda1, TW.lambda2, g, w, nn, z);
    TW.w[rw] = w;
    xf::store_nz(TW, rw, nn, z);
  } else {
    TW.w[rw] = xf::sgd_step(TW.lr, g, w_old);
  }
}

// ------------------------------------------------------- gradient + the two Pushes, FM
// k_fmc_grad_tiled with the occurrences' values staged beside their rows: lx = loss x (what the
// w gradient sums), xs = x (for a = v x)
template <int OPT, int K>
__global__ void __launch_bounds__(kBlock)
k_val_fm_grad_tiled(xf::TableDev TW, xf::TableDev TV, const uint32_t *__restrict__ tile_ptr,
                    uint32_t ntiles, const uint32_t *__restrict__ segptr,
                    const uint32_t *__restrict__ coo_row, const float *__restrict__ coo_val,
                    const float *__restrict__ loss, const float *__restrict__ S,
                    const float *__restrict__ wu, const float *__restrict__ vu,
                    const uint32_t *__restrict__ rows_w, const uint32_t *__restrict__ rows_v,
                    uint32_t R, int k_rt, float *__restrict__ gw) {
#pragma clang fp contract(off)
  __shared__ float lx[XF_GRAD_TILE_NNZ];
  __shared__ float xs[XF_GRAD_TILE_NNZ];
  __shared__ uint32_t ss[XF_GRAD_TILE_NNZ];
  __shared__ uint32_t sp[XF_GRAD_TILE_KEYS + 1];
  const uint32_t k = K > 0 ? (uint32_t)K : (uint32_t)k_rt;
  const uint32_t tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t ua = tile_ptr[tile], ub = tile_ptr[tile + 1], nk = ub - ua;
    const uint32_t j0 = segptr[ua], j1 = segptr[ub];
    if (nk == 1 && j1 - j0 > XF_HEAVY_SEG) continue;  // heavy key: the chunked kernels
    for (uint32_t q = tid; q <= nk; q += kBlock) sp[q] = segptr[ua + q] - j0;
    for (uint32_t j = j0 + tid; j < j1; j += kBlock) {
      const uint32_t sid = coo_row[j];
      const float x = coo_val[j];
      ss[j - j0] = sid;
      xs[j - j0] = x;
      lx[j - j0] = loss[sid] * x;
    }
    __syncthreads();
    const uint32_t nel = nk * k;
    constexpr int kUn = 4;
    for (uint32_t el0 = tid; el0 < nel; el0 += kBlock * kUn) {
      uint32_t kq[kUn], kk[kUn];
      float v[kUn], vn[kUn], vz[kUn];
      size_t to[kUn];
      bool on[kUn];
#pragma unroll
      for (int i = 0; i < kUn; ++i) {
        const uint32_t el = el0 + i * kBlock;
        on[i] = el < nel;
        kq[i] = on[i] ? el / k : 0;
        kk[i] = on[i] ? el - kq[i] * k : 0;
      }
#pragma unroll
      for (int i = 0; i < kUn; ++i) {
        v[i] = on[i] ? vu[(size_t)(ua + kq[i]) * k + kk[i]] : 0.0f;
        to[i] = on[i] ? (size_t)rows_v[ua + kq[i]] * k + kk[i] : 0;
      }
      if (OPT == XF_OPT_FTRL) {
#pragma unroll
        for (int i = 0; i < kUn; ++i) {
          vn[i] = vz[i] = 0.0f;
          if (on[i]) xf::load_nz(TV, to[i], vn[i], vz[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < kUn; ++i) {
        if (!on[i]) continue;
        const uint32_t a = sp[kq[i]], e = sp[kq[i] + 1];
        double acc = 0.0;
        uint32_t j = a;
        for (; j + 3 < e; j += 4) {  // four S gathers in flight
          float sv[4];
#pragma unroll
          for (int m = 0; m < 4; ++m) sv[m] = S[(size_t)ss[j + m] * k + kk[i]];
#pragma unroll
          for (int m = 0; m < 4; ++m) acc += (double)(lx[j + m] * (sv[m] - v[i] * xs[j + m]));
        }
        for (; j < e; ++j) acc += (double)(lx[j] * (S[(size_t)ss[j] * k + kk[i]] - v[i] * xs[j]));
        const float g = xf::div_by_rows((float)acc, R);
        if (OPT == XF_OPT_FTRL) {
          float w = v[i], nn = vn[i], z = vz[i];
          xf::ftrl_step(TV.alpha, TV.inv_alpha, TV.beta, TV.lambda1, TV.lambda2, g, w, nn, z);
          TV.w[to[i]] = w;
          xf::store_nz(TV, to[i], nn, z);
        } else {
          TV.w[to[i]] = xf::sgd_step(TV.lr, g, v[i]);
        }
      }
    }
    for (uint32_t q = tid; q < nk; q += kBlock) {
      double aw = 0.0;
      for (uint32_t j = sp[q]; j < sp[q + 1]; ++j) aw += (double)lx[j];
      const float g1 = xf::div_by_rows((float)aw, R);
      gw[ua + q] = g1;
      step_w<OPT>(TW, rows_w[ua + q], wu[ua + q], g1);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------- gradient + Push, LR
// the w half of the kernel above: a tile's loss x in LDS, a lane per key
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
      step_w<OPT>(TW, rows_w[ua + q], wu[ua + q], g1);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------- heavy keys
// k_fmc_heavy_partial with the chunk's values staged; k = 0 (LR) leaves the loss x column alone.
// The second kernel is the canonical one (xf::fmc_heavy_finish): it reads sums, not values.
__global__ void __launch_bounds__(kBlock)
k_val_heavy_partial(const uint32_t *__restrict__ heavy, const uint32_t *__restrict__ hch,
                    uint32_t H, const uint32_t *__restrict__ segptr,
                    const uint32_t *__restrict__ coo_row, const float *__restrict__ coo_val,
                    const float *__restrict__ loss, const float *__restrict__ S,
                    const float *__restrict__ vu, int k_rt, double *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float lx[XF_TILE_NNZ];
  __shared__ float xs[XF_TILE_NNZ];
  __shared__ uint32_t ss[XF_TILE_NNZ];
  __shared__ double red[kBlock];
  const uint32_t tid = threadIdx.x, c = blockIdx.x, k = (uint32_t)k_rt;
  const uint32_t h = heavy_of_chunk(hch, H, c);
  const uint32_t u = heavy[h];
  const uint32_t b = segptr[u] + (c - hch[h]) * XF_TILE_NNZ;
  const uint32_t e = min(segptr[u + 1], b + XF_TILE_NNZ);
  const uint32_t n = e > b ? e - b : 0u;
  for (uint32_t j = tid; j < n; j += kBlock) {
    const uint32_t sid = coo_row[b + j];
    const float x = coo_val[b + j];
    ss[j] = sid;
    xs[j] = x;
    lx[j] = loss[sid] * x;
  }
  __syncthreads();
  const uint32_t ncol = k + 1u, cpp = min(ncol, (uint32_t)kBlock), nsl = kBlock / cpp;
  const uint32_t cl = tid % cpp, sl = tid / cpp;
  for (uint32_t c0 = 0; c0 < ncol; c0 += cpp) {
    const uint32_t col = c0 + cl;
    const bool act = sl < nsl && col < ncol, fac = col < k;
    const float v = (act && fac) ? vu[(size_t)u * k + col] : 0.0f;
    double acc = 0.0;
    if (act) {
      if (fac) {
        double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        uint32_t j = sl;
        for (; j + 7 * nsl < n; j += 8 * nsl) {  // eight S gathers in flight
          float sv[8];
#pragma unroll
          for (int m = 0; m < 8; ++m) sv[m] = S[(size_t)ss[j + m * nsl] * k + col];
#pragma unroll
          for (int m = 0; m < 8; ++m)
            a[m] += (double)(lx[j + m * nsl] * (sv[m] - v * xs[j + m * nsl]));
        }
        for (; j < n; j += nsl)
          a[0] += (double)(lx[j] * (S[(size_t)ss[j] * k + col] - v * xs[j]));
        acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
      } else {
        for (uint32_t j = sl; j < n; j += nsl) acc += (double)lx[j];
      }
    }
    red[tid] = acc;
    __syncthreads();
    if (sl == 0 && col < ncol) {
      for (uint32_t q = 1; q < nsl; ++q) acc += red[q * cpp + cl];
      partial[(size_t)c * ncol + col] = acc;
    }
    __syncthreads();
  }
}

}  // namespace

namespace xf {

// loss[R], pctr[R] (may be null), S[R x k] from the pulled rows and the values in CSR order
int val_fm_forward(const xf_dev_batch *b, const float *d_xval, int k, const float *d_wu,
                   const float *d_vu, float *d_S, float *d_loss, float *d_pctr, hipStream_t s) {
  XF_REQUIRE(b && d_wu && d_vu && d_S && d_loss && k >= 1 && (d_xval || b->NNZ == 0),
             "valued fm forward: bad argument");
  if (b->R == 0) return XF_OK;
  const dim3 g(blocks_for_groups(b->R, kBlock / 64)), blk(kBlock);
#define XF_VAL_FWD(PP, EX)                                                                     \
  hipLaunchKernelGGL((k_val_fm_forward<PP, EX>), g, blk, 0, s, b->rowptr, b->uidx, d_xval, d_wu, \
                     d_vu, k, b->labels, b->R, d_loss, d_pctr, d_S)
  switch (k) {
    case 4: XF_VAL_FWD(4, true); break;
    case 8: XF_VAL_FWD(8, true); break;
    case 16: XF_VAL_FWD(16, true); break;
    case 32: XF_VAL_FWD(32, true); break;
    case 64: XF_VAL_FWD(64, true); break;
    default:
      if (k <= 1) XF_VAL_FWD(1, false);
      else if (k <= 2) XF_VAL_FWD(2, false);
      else if (k <= 4) XF_VAL_FWD(4, false);
      else if (k <= 8) XF_VAL_FWD(8, false);
      else if (k <= 16) XF_VAL_FWD(16, false);
      else if (k <= 32) XF_VAL_FWD(32, false);
      else XF_VAL_FWD(64, false);
      break;
  }
#undef XF_VAL_FWD
  XF_HIP(hipGetLastError());
  return XF_OK;
}

int val_lr_forward(const xf_dev_batch *b, const float *d_xval, const float *d_wu, float *d_loss,
                   float *d_pctr, hipStream_t s) {
  XF_REQUIRE(b && d_wu && d_loss && (d_xval || b->NNZ == 0), "valued lr forward: bad argument");
  if (b->R == 0) return XF_OK;
  hipLaunchKernelGGL(k_val_lr_forward, dim3(blocks_for_groups(b->R, kBlock / 64)), dim3(kBlock), 0,
                     s, b->rowptr, b->uidx, d_xval, d_wu, b->labels, b->R, d_loss, d_pctr);
  XF_HIP(hipGetLastError());
  return XF_OK;
}

// gradient + both Pushes (fmc_grad_update's contract) with the values in key-grouped order
int val_fm_grad_update(xf_table *tw, xf_table *tv, const xf_dev_batch *b, const float *d_coo_val,
                       const uint32_t *d_rows_w, const uint32_t *d_rows_v, const float *d_wu,
                       const float *d_vu, const float *d_S, const float *d_loss, float *d_gw,
                       double *d_hpart, hipStream_t s) {
  XF_REQUIRE(tw && tv && b && d_coo_val && d_rows_w && d_rows_v && d_wu && d_vu && d_S && d_loss &&
                 d_gw, "valued fm gradient: null argument");
  if (b->U == 0) return XF_OK;
  const xf::TableDev &TW = xf::table_dev(tw), &TV = xf::table_dev(tv);
  const int k = TV.dim;
  const bool ftrl = TV.nz != nullptr;
  XF_REQUIRE((TW.nz != nullptr) == ftrl, "valued fm gradient: w and v use different optimizers");
  XF_REQUIRE(b->ntiles && b->tile_ptr, "valued fm gradient: the minibatch has no gradient tiles");
  XF_REQUIRE(!b->H || (b->heavy_chunk_ptr && d_hpart),
             "valued fm gradient: heavy keys without their chunks or scratch");
  const dim3 gt((unsigned)std::min<uint32_t>(b->ntiles, 1u << 16)), blk(kBlock);
#define XF_VAL_GU(OPTV, KK)                                                                       \
  hipLaunchKernelGGL((k_val_fm_grad_tiled<OPTV, KK>), gt, blk, 0, s, TW, TV, b->tile_ptr,         \
                     b->ntiles, b->segptr, b->coo_row, d_coo_val, d_loss, d_S, d_wu, d_vu, d_rows_w, \
                     d_rows_v, b->R, k, d_gw)
#define XF_VAL_GU_K(OPTV)                 \
  switch (k) {                            \
    case 4: XF_VAL_GU(OPTV, 4); break;    \
    case 8: XF_VAL_GU(OPTV, 8); break;    \
    case 16: XF_VAL_GU(OPTV, 16); break;  \
    case 32: XF_VAL_GU(OPTV, 32); break;  \
    case 64: XF_VAL_GU(OPTV, 64); break;  \
    default: XF_VAL_GU(OPTV, 0); break;   \
  }
  if (ftrl) {
    XF_VAL_GU_K(XF_OPT_FTRL)
  } else {
    XF_VAL_GU_K(XF_OPT_SGD)
  }
#undef XF_VAL_GU_K
#undef XF_VAL_GU
  XF_HIP(hipGetLastError());
  if (b->H) {
    hipLaunchKernelGGL(k_val_heavy_partial, dim3(b->n_heavy_chunks), blk, 0, s, b->heavy,
                       b->heavy_chunk_ptr, b->H, b->segptr, b->coo_row, d_coo_val, d_loss, d_S,
                       d_vu, k, d_hpart);
    fmc_heavy_finish(TW, TV, k, b, d_hpart, d_rows_w, d_rows_v, d_wu, d_vu, d_gw, s);
    XF_HIP(hipGetLastError());
  }
  return XF_OK;
}

// LR: gradient + Push of w.  d_hpart: n_heavy_chunks doubles (fmc_heavy_doubles(b, 0)).
int val_lr_grad_update(xf_table *tw, const xf_dev_batch *b, const float *d_coo_val,
                       const uint32_t *d_rows_w, const float *d_wu, const float *d_loss,
                       float *d_gw, double *d_hpart, hipStream_t s) {
  XF_REQUIRE(tw && b && d_coo_val && d_rows_w && d_wu && d_loss && d_gw,
             "valued lr gradient: null argument");
  if (b->U == 0) return XF_OK;
  const xf::TableDev &TW = xf::table_dev(tw);
  XF_REQUIRE(b->ntiles && b->tile_ptr, "valued lr gradient: the minibatch has no gradient tiles");
  XF_REQUIRE(!b->H || (b->heavy_chunk_ptr && d_hpart),
             "valued lr gradient: heavy keys without their chunks or scratch");
  const dim3 gt((unsigned)std::min<uint32_t>(b->ntiles, 1u << 16)), blk(kBlock);
  if (TW.nz != nullptr)
    hipLaunchKernelGGL(k_val_lr_grad_tiled<XF_OPT_FTRL>, gt, blk, 0, s, TW, b->tile_ptr, b->ntiles,
                       b->segptr, b->coo_row, d_coo_val, d_loss, d_wu, d_rows_w, b->R, d_gw);
  else
    hipLaunchKernelGGL(k_val_lr_grad_tiled<XF_OPT_SGD>, gt, blk, 0, s, TW, b->tile_ptr, b->ntiles,
                       b->segptr, b->coo_row, d_coo_val, d_loss, d_wu, d_rows_w, b->R, d_gw);
  XF_HIP(hipGetLastError());
  if (b->H) {
    hipLaunchKernelGGL(k_val_heavy_partial, dim3(b->n_heavy_chunks), blk, 0, s, b->heavy,
                       b->heavy_chunk_ptr, b->H, b->segptr, b->coo_row, d_coo_val, d_loss,
                       (const float *)nullptr, (const float *)nullptr, 0, d_hpart);
    fmc_heavy_finish(TW, TW, 0, b, d_hpart, d_rows_w, d_rows_w, d_wu, d_wu, d_gw, s);
    XF_HIP(hipGetLastError());
  }
  return XF_OK;
}

}  // namespace xf
