// xf_ffm.hip — field-aware factorization machine (fm_mode = field_aware, gfx950).
//
// A key keeps one k-vector per field: the v table is F k wide, coordinate (h, f) at h k + f.  A
// pair of nonzeros interacts through the vectors each holds for the OTHER's field (Juan et al.).
// Nonzero j of row r: key index u_j, field g_j, x_j (its value with feature_values = on, else 1);
// fp32(.) marks every rounding to fp32:
//   a_j[h,f]  = fp32(v[u_j,h,f] x_j)
//   wx_r      = fp32(sum_j fp32(w[u_j] x_j))
//   y2_r      = fp32(sum_{i<j in row r} sum_f fp32(a_i[g_j,f] a_j[g_i,f]))
//   gw[u]     = fp32(fp32(sum_occ fp32(loss_r x_occ)) / R)
//   gv[u,h,f] = fp32(fp32(sum_{occ i of u} sum_{j in row(i), j != i, g_j = h}
//                         fp32(fp32(loss_r x_i) a_j[g_i,f])) / R)
// Pairs are pairs of positions: a key twice in a row, or under two fields, is two nonzeros.
// Every fp64 sum adds fp32 values, so it is exact and does not depend on lane assignment or on
// the order the LDS atomics arrive in.  Only TOUCHED coordinates of v are stepped: (u, h) is
// touched when some occurrence i of u has a j != i in its row with g_j = h.  An FTRL step with
// g = 0 would set a fresh hash-normal weight to 0, and two zero vectors never leave zero: stepping
// every coordinate of a pushed key would erase the init of every field it has not met yet.
//
// One set of kernels, VAL their last template parameter (as xf_fm_canonical.hip): the values are
// read from xval beside uidx / xfg in CSR order; VAL = false never reads the pointer.
//
// Forward: one wavefront per row.  The row's (u, g, x) go to LDS (rows longer than kStage are
// read in place), a lane is a (pair slot, factor): P factors, 64 / P slots, four pairs in flight
// per lane; a pair reads two contiguous k x 4-byte pieces of the pulled U x F k block.
// Gradient + the two Pushes: the minibatch's key tiles (xf_tiling.h).  A workgroup holds
// kAcc = 4096 fp64 accumulators in LDS (32 KiB: one key at the table's widest row, 56 keys at
// F k = 72) and walks a tile's keys in groups of kAcc / (F k); a wavefront takes a key, walks the
// rows of its occurrences and adds fp32(lx_i a_j[g_i,:]) into the key's (g_j,:) with LDS fp64
// atomics, collecting the touched mask in a register.  With the masks (2 KiB) a workgroup uses
// 34 KiB of LDS: four workgroups, 16 wavefronts, per CU of 160 KiB.  Heavy keys
// (> XF_HEAVY_SEG occurrences): a workgroup per chunk leaves F k + 1 fp64 columns and the mask,
// a second kernel adds a key's chunks and steps.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "xf_common.h"
#include "xf_device.h"
#include "xf_ffm.h"
#include "xf_wave.h"

namespace xf {
const TableDev &table_dev(const xf_table *t);
}

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kStage = 128;  // nonzeros of a row staged per wavefront (forward)
constexpr uint32_t kAcc = 4096;   // fp64 accumulators per workgroup (gradient): the widest v row
using xf::blocks_for_groups;      // xf_wave.h
using xf::group_sum;
using xf::heavy_of_chunk;

// pair number p -> (i, j), i < j, pairs in the order (0,1), (0,2), (1,2), (0,3), ...
__device__ __forceinline__ void pair_of(uint64_t p, uint32_t &i, uint32_t &j) {
  uint64_t jj = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
  while (jj * (jj - 1) / 2 > p) --jj;
  while ((jj + 1) * jj / 2 <= p) ++jj;
  j = (uint32_t)jj;
  i = (uint32_t)(p - jj * (jj - 1) / 2);
}

__device__ __forceinline__ uint64_t wave_or(uint64_t m) {
  uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo |= __shfl_xor(lo, off);
    hi |= __shfl_xor(hi, off);
  }
  return ((uint64_t)hi << 32) | lo;
}

// ------------------------------------------------------------------------------ forward
// P: factor lanes per pair (a power of two <= 64); EXACT: k == P (a compile-time factor count).
template <int P, bool EXACT, bool VAL>
__global__ void __launch_bounds__(kBlock)
k_ffm_forward(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ uidx,
              const uint32_t *__restrict__ xfg, const float *__restrict__ wu,
              const float *__restrict__ vu, int k_rt, uint32_t dim,
              const int32_t *__restrict__ labels, uint32_t R, float *__restrict__ loss,
              float *__restrict__ pctr, const float *__restrict__ xval) {
#pragma clang fp contract(off)
  static_assert(P >= 1 && P <= 64 && (P & (P - 1)) == 0, "P: a power of two <= 64");
  __shared__ uint32_t su[kWaves][kStage];
  __shared__ uint32_t sg[kWaves][kStage];
  __shared__ float sx[VAL ? kWaves : 1][VAL ? kStage : 1];
  const uint32_t k = EXACT ? (uint32_t)P : (uint32_t)k_rt;
  constexpr uint32_t kG = 64u / P;  // pair slots
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x / 64u, f = lane % P, sub = lane / P;
  // (every wavefront of a workgroup makes the same number of trips: the barriers are uniform)
  for (uint32_t r0 = blockIdx.x * kWaves; r0 < R; r0 += gridDim.x * kWaves) {
    const uint32_t r = r0 + wv;
    const bool row = r < R;
    const uint32_t b = row ? rowptr[r] : 0u, n = row ? rowptr[r + 1] - b : 0u;
    const bool st = n <= kStage;
    if (st) {
      for (uint32_t j = lane; j < n; j += 64) {
        su[wv][j] = uidx[b + j];
        sg[wv][j] = xfg[b + j];
        if constexpr (VAL) sx[wv][j] = xval[b + j];
      }
    }
    __syncthreads();
    double wx = 0.0, y2 = 0.0;
    for (uint32_t j = lane; j < n; j += 64) {
      const uint32_t u = st ? su[wv][j] : uidx[b + j];
      const float x = VAL ? (st ? sx[wv][j] : xval[b + j]) : 1.0f;
      wx += (double)(VAL ? wu[u] * x : wu[u]);  // fp32 products, here and below
    }
    const uint64_t np = (uint64_t)n * (n > 0 ? n - 1 : 0) / 2;
    for (uint64_t p0 = sub; p0 < np; p0 += 4 * kG) {
      size_t oi[4], oj[4];
      float xi[4], xj[4];
      bool in[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint64_t p = p0 + (uint64_t)m * kG;
        in[m] = p < np;
        uint32_t i = 0, j = 0;
        if (in[m]) pair_of(p, i, j);
        const uint32_t ui = in[m] ? (st ? su[wv][i] : uidx[b + i]) : 0u;
        const uint32_t uj = in[m] ? (st ? su[wv][j] : uidx[b + j]) : 0u;
        const uint32_t gi = in[m] ? (st ? sg[wv][i] : xfg[b + i]) : 0u;
        const uint32_t gj = in[m] ? (st ? sg[wv][j] : xfg[b + j]) : 0u;
        xi[m] = (VAL && in[m]) ? (st ? sx[VAL ? wv : 0][VAL ? i : 0] : xval[b + i]) : 1.0f;
        xj[m] = (VAL && in[m]) ? (st ? sx[VAL ? wv : 0][VAL ? j : 0] : xval[b + j]) : 1.0f;
        oi[m] = (size_t)ui * dim + (size_t)gj * k;
        oj[m] = (size_t)uj * dim + (size_t)gi * k;
      }
      for (uint32_t fk = f; fk < k; fk += P) {  // one trip unless k > 64
        float a[4], c[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          a[m] = in[m] ? vu[oi[m] + fk] : 0.0f;
          c[m] = in[m] ? vu[oj[m] + fk] : 0.0f;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float ai = VAL ? a[m] * xi[m] : a[m];
          const float aj = VAL ? c[m] * xj[m] : c[m];
          y2 += (double)(ai * aj);
        }
      }
    }
    wx = group_sum<64>(wx);
    y2 = group_sum<64>(y2);
    if (row && lane == 0) {
      const float p = xf::sigmoid_ref((float)wx + (float)y2);
      if (pctr) pctr[r] = p;
      loss[r] = p - (float)labels[r];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------ gradient + the two Pushes
// One occurrence (key-grouped position j) by one wavefront: the walk of its row.  A group of kp
// lanes takes a nonzero jj != the occurrence's own position and adds fp32(lx a_jj[g_i, f]) into
// acc[g_jj k + f]; returns this lane's part of the touched mask.
template <bool VAL>
__device__ __forceinline__ uint64_t ffm_occ(uint32_t j, uint32_t lane, uint32_t k, uint32_t kp,
                                            uint32_t dim, const uint32_t *__restrict__ coo_row,
                                            const uint32_t *__restrict__ coo_pos,
                                            const uint32_t *__restrict__ rowptr,
                                            const uint32_t *__restrict__ uidx,
                                            const uint32_t *__restrict__ xfg,
                                            const float *__restrict__ xval,
                                            const float *__restrict__ loss,
                                            const float *__restrict__ vu, double *acc) {
#pragma clang fp contract(off)
  const uint32_t pos = coo_pos[j], r = coo_row[j];
  const uint32_t gi = xfg[pos];
  const float lx = VAL ? loss[r] * xval[pos] : loss[r];
  const uint32_t b = rowptr[r], e = rowptr[r + 1];
  const uint32_t f = lane & (kp - 1u), slot = lane / kp, nsl = 64u / kp;
  uint64_t m = 0;
  for (uint32_t jj = b + slot; jj < e; jj += nsl) {
    if (jj == pos) continue;
    const uint32_t h = xfg[jj];
    const float x2 = VAL ? xval[jj] : 1.0f;
    const float *src = vu + (size_t)uidx[jj] * dim + (size_t)gi * k;
    double *dst = acc + (size_t)h * k;
    for (uint32_t fk = f; fk < k; fk += kp) {
      const float a = VAL ? src[fk] * x2 : src[fk];
      atomicAdd(&dst[fk], (double)(lx * a));
    }
    m |= 1ull << h;
  }
  return m;
}

// fp32(loss x) of occurrence j
template <bool VAL>
__device__ __forceinline__ float ffm_lx(uint32_t j, const uint32_t *__restrict__ coo_row,
                                        const uint32_t *__restrict__ coo_pos,
                                        const float *__restrict__ xval,
                                        const float *__restrict__ loss) {
#pragma clang fp contract(off)
  const float l = loss[coo_row[j]];
  return VAL ? l * xval[coo_pos[j]] : l;
}

// A workgroup per gradient tile (keys [tile_ptr[t], tile_ptr[t+1]), <= XF_GRAD_TILE_NNZ
// occurrences).  w: one lane per key, as k_fmc_grad_tiled.  v: the tile's keys in groups of
// kAcc / dim; a wavefront per key walks its occurrences (ffm_occ), then a lane per (key,
// coordinate) steps the touched ones in place (the pulled value is the current weight).
// OPT = xf::kOptEmit: nothing is stepped — gv[u dim + c] leaves with the gradient of a touched
// coordinate and 0 for an untouched one, mask[u] with the key's touched mask, beside gw[u]; the
// state rows, the tables and wu are not read (the worker of a sharded trainer: the owner steps).
template <int OPT, int K /* compile-time factor count, 0 = k_rt */, bool VAL>
__global__ void __launch_bounds__(kBlock)
k_ffm_grad_tiled(xf::TableDev TW, xf::TableDev TV, const uint32_t *__restrict__ tile_ptr,
                 uint32_t ntiles, const uint32_t *__restrict__ segptr,
                 const uint32_t *__restrict__ coo_row, const uint32_t *__restrict__ coo_pos,
                 const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ uidx,
                 const uint32_t *__restrict__ xfg, const float *__restrict__ loss,
                 const float *__restrict__ wu, const float *__restrict__ vu,
                 const uint32_t *__restrict__ rows_w, const uint32_t *__restrict__ rows_v,
                 uint32_t R, int k_rt, int kp_rt, uint32_t dim, float *__restrict__ gw,
                 const float *__restrict__ xval, float *__restrict__ gv,
                 unsigned long long *__restrict__ mask) {
#pragma clang fp contract(off)
  constexpr bool kEmit = OPT == xf::kOptEmit;
  __shared__ double acc[kAcc];
  __shared__ unsigned long long msk[XF_GRAD_TILE_KEYS];
  const uint32_t k = K > 0 ? (uint32_t)K : (uint32_t)k_rt;
  const uint32_t kp = K > 0 ? (uint32_t)K : (uint32_t)kp_rt;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid / 64u;
  const uint32_t kpg = max(1u, kAcc / dim);  // keys per group (dim <= kAcc)
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t ua = tile_ptr[tile], ub = tile_ptr[tile + 1], nk = ub - ua;
    if (nk == 1 && segptr[ub] - segptr[ua] > XF_HEAVY_SEG) continue;  // heavy: the chunked kernels
    // the keys' w: the true gradient (sum of the occurrences' fp32(loss x)) / R
    for (uint32_t q = tid; q < nk; q += kBlock) {
      double aw = 0.0;
      for (uint32_t j = segptr[ua + q]; j < segptr[ua + q + 1]; ++j)
        aw += (double)ffm_lx<VAL>(j, coo_row, coo_pos, xval, loss);
      const float g1 = xf::div_by_rows((float)aw, R);
      gw[ua + q] = g1;
      if constexpr (!kEmit) xf::step_coord<OPT>(TW, rows_w[ua + q], wu[ua + q], g1);
    }
    for (uint32_t q0 = 0; q0 < nk; q0 += kpg) {
      const uint32_t nq = min(kpg, nk - q0), nel = nq * dim;
      for (uint32_t el = tid; el < nel; el += kBlock) acc[el] = 0.0;
      __syncthreads();
      for (uint32_t q = wv; q < nq; q += kWaves) {
        const uint32_t u = ua + q0 + q;
        uint64_t m = 0;
        for (uint32_t j = segptr[u]; j < segptr[u + 1]; ++j)
          m |= ffm_occ<VAL>(j, lane, k, kp, dim, coo_row, coo_pos, rowptr, uidx, xfg, xval, loss,
                            vu, acc + (size_t)q * dim);
        m = wave_or(m);
        if (lane == 0) {
          msk[q] = m;
          if constexpr (kEmit) mask[u] = m;
        }
      }
      __syncthreads();
      for (uint32_t el = tid; el < nel; el += kBlock) {
        const uint32_t q = el / dim, c = el - q * dim;
        if constexpr (kEmit) {  // an untouched coordinate leaves as 0: the buffer is fully defined
          gv[(size_t)(ua + q0 + q) * dim + c] =
              ((msk[q] >> (c / k)) & 1ull) ? xf::div_by_rows((float)acc[el], R) : 0.0f;
        } else {
          if (!((msk[q] >> (c / k)) & 1ull)) continue;  // untouched: w, n, z stay as they are
          const uint32_t u = ua + q0 + q;
          const float g = xf::div_by_rows((float)acc[el], R);
          xf::step_coord<OPT>(TV, (size_t)rows_v[u] * dim + c, vu[(size_t)u * dim + c], g);
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------- heavy keys
// A heavy key's occurrences in chunks of XF_TILE_NNZ (the batch's heavy_chunk_ptr), one
// workgroup per chunk: partial[chunk][col] for the dim coordinates, the sum of fp32(loss x)
// (column dim) and the touched mask (column dim + 1, its 64 bits as they are).
template <bool VAL>
__global__ void __launch_bounds__(kBlock)
k_ffm_heavy_partial(const uint32_t *__restrict__ heavy, const uint32_t *__restrict__ hch,
                    uint32_t H, const uint32_t *__restrict__ segptr,
                    const uint32_t *__restrict__ coo_row, const uint32_t *__restrict__ coo_pos,
                    const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ uidx,
                    const uint32_t *__restrict__ xfg, const float *__restrict__ loss,
                    const float *__restrict__ vu, int k_rt, int kp_rt, uint32_t dim,
                    double *__restrict__ partial, const float *__restrict__ xval) {
#pragma clang fp contract(off)
  __shared__ double acc[kAcc + 1];
  __shared__ unsigned long long msk;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid / 64u, c = blockIdx.x;
  const uint32_t k = (uint32_t)k_rt, kp = (uint32_t)kp_rt;
  const uint32_t h = heavy_of_chunk(hch, H, c);
  const uint32_t u = heavy[h];
  const uint32_t b = segptr[u] + (c - hch[h]) * XF_TILE_NNZ;
  const uint32_t e = min(segptr[u + 1], b + XF_TILE_NNZ);
  for (uint32_t el = tid; el <= dim; el += kBlock) acc[el] = 0.0;
  if (tid == 0) msk = 0ull;
  __syncthreads();
  uint64_t m = 0;
  for (uint32_t j = b + wv; j < e; j += kWaves)
    m |= ffm_occ<VAL>(j, lane, k, kp, dim, coo_row, coo_pos, rowptr, uidx, xfg, xval, loss, vu,
                      acc);
  double aw = 0.0;
  for (uint32_t j = b + tid; j < e; j += kBlock)
    aw += (double)ffm_lx<VAL>(j, coo_row, coo_pos, xval, loss);
  aw = group_sum<64>(aw);
  m = wave_or(m);
  if (lane == 0) {
    atomicAdd(&acc[dim], aw);
    atomicOr(&msk, (unsigned long long)m);
  }
  __syncthreads();
  const size_t ncol = (size_t)dim + 2;
  for (uint32_t el = tid; el <= dim; el += kBlock) partial[(size_t)c * ncol + el] = acc[el];
  if (tid == 0) ((unsigned long long *)partial)[(size_t)c * ncol + dim + 1] = msk;
}

// one workgroup per heavy key: its chunks' sums added per column and their masks joined, then
// the optimizer steps of its touched coordinates and of its w (OPT = xf::kOptEmit: gv, mask[u] and
// gw[u] written as k_ffm_grad_tiled does, nothing stepped)
template <int OPT>
__global__ void __launch_bounds__(kBlock)
k_ffm_heavy_finish(xf::TableDev TW, xf::TableDev TV, const uint32_t *__restrict__ heavy,
                   const uint32_t *__restrict__ hch, const double *__restrict__ partial,
                   const uint32_t *__restrict__ rows_w, const uint32_t *__restrict__ rows_v,
                   const float *__restrict__ wu, const float *__restrict__ vu, uint32_t R,
                   int k_rt, uint32_t dim, float *__restrict__ gw, float *__restrict__ gv,
                   unsigned long long *__restrict__ mask) {
#pragma clang fp contract(off)
  constexpr bool kEmit = OPT == xf::kOptEmit;
  __shared__ unsigned long long msk;
  const uint32_t tid = threadIdx.x, h = blockIdx.x, k = (uint32_t)k_rt;
  const uint32_t u = heavy[h], c0 = hch[h], c1 = hch[h + 1];
  const size_t ncol = (size_t)dim + 2;
  if (tid == 0) {
    unsigned long long m = 0ull;
    for (uint32_t c = c0; c < c1; ++c)
      m |= ((const unsigned long long *)partial)[(size_t)c * ncol + dim + 1];
    msk = m;
    if constexpr (kEmit) mask[u] = m;
  }
  __syncthreads();
  for (uint32_t col = tid; col <= dim; col += kBlock) {
    double a = 0.0;
    for (uint32_t c = c0; c < c1; ++c) a += partial[(size_t)c * ncol + col];
    const float g = xf::div_by_rows((float)a, R);
    if (col < dim) {
      if constexpr (kEmit) {
        gv[(size_t)u * dim + col] = ((msk >> (col / k)) & 1ull) ? g : 0.0f;
      } else {
        if ((msk >> (col / k)) & 1ull)
          xf::step_coord<OPT>(TV, (size_t)rows_v[u] * dim + col, vu[(size_t)u * dim + col], g);
      }
    } else {
      gw[u] = g;
      if constexpr (!kEmit) xf::step_coord<OPT>(TW, rows_w[u], wu[u], g);
    }
  }
}

// lanes per (occurrence, nonzero) item of the walk for a runtime k: the next power of two, <= 64
int lanes_for(int k) {
  int p = 1;
  while (p < k && p < 64) p <<= 1;
  return p;
}

}  // namespace

namespace xf {

// scratch of the heavy keys' chunk sums: doubles (dim + 1 columns and the mask per chunk)
size_t ffm_heavy_doubles(const xf_dev_batch *b, int dim) {
  return b->H ? (size_t)b->n_heavy_chunks * ((size_t)dim + 2) : 0;
}

// loss[R], pctr[R] (may be null) from the pulled rows w_u[U], v_u[U x F k]
int ffm_forward(const xf_dev_batch *b, int k, int F, const float *d_wu, const float *d_vu,
                const uint32_t *d_xfg, float *d_loss, float *d_pctr, const float *d_xval,
                hipStream_t s) {
  XF_REQUIRE(b && d_wu && d_vu && d_loss && k >= 1 && F >= 1 && F <= 64 && (b->NNZ == 0 || d_xfg),
             "field-aware FM forward: bad argument");
  if (b->R == 0) return XF_OK;
  const dim3 g(blocks_for_groups(b->R, kWaves)), blk(kBlock);
  const uint32_t dim = (uint32_t)F * (uint32_t)k;
#define XF_FFM_FWD_V(PP, EX, VAL)                                                                \
  hipLaunchKernelGGL((k_ffm_forward<PP, EX, VAL>), g, blk, 0, s, b->rowptr, b->uidx, d_xfg, d_wu, \
                     d_vu, k, dim, b->labels, b->R, d_loss, d_pctr, d_xval)
#define XF_FFM_FWD(PP, EX)                  \
  do {                                      \
    if (d_xval) XF_FFM_FWD_V(PP, EX, true); \
    else XF_FFM_FWD_V(PP, EX, false);       \
  } while (0)
  switch (k) {
    case 4: XF_FFM_FWD(4, true); break;
    case 8: XF_FFM_FWD(8, true); break;
    case 16: XF_FFM_FWD(16, true); break;
    default:
      if (k <= 1) XF_FFM_FWD(1, false);
      else if (k <= 2) XF_FFM_FWD(2, false);
      else if (k <= 4) XF_FFM_FWD(4, false);
      else if (k <= 8) XF_FFM_FWD(8, false);
      else if (k <= 16) XF_FFM_FWD(16, false);
      else if (k <= 32) XF_FFM_FWD(32, false);
      else XF_FFM_FWD(64, false);
      break;
  }
#undef XF_FFM_FWD
#undef XF_FFM_FWD_V
  XF_HIP(hipGetLastError());
  return XF_OK;
}

// the tile kernel and the heavy keys' two for one OPT (an optimizer, or kOptEmit with d_gv, d_mask)
static int ffm_grad_launch(int opt, const TableDev &TW, const TableDev &TV, uint32_t dim,
                           const xf_dev_batch *b, int F, const uint32_t *d_rows_w,
                           const uint32_t *d_rows_v, const float *d_wu, const float *d_vu,
                           const uint32_t *d_xfg, const uint32_t *d_coo_pos, const float *d_loss,
                           float *d_gw, float *d_gv, unsigned long long *d_mask, double *d_hpart,
                           const float *d_xval, hipStream_t s) {
  XF_REQUIRE(F >= 1 && F <= 64 && dim >= 1 && dim <= kAcc && dim % (uint32_t)F == 0,
             "field-aware FM gradient: the v table's dim (%u) is not fields (%d) x k, or exceeds "
             "%u", dim, F, kAcc);
  const int k = (int)(dim / (uint32_t)F), kp = lanes_for(k);
  XF_REQUIRE(b->ntiles && b->tile_ptr, "field-aware FM gradient: the minibatch has no gradient tiles");
  XF_REQUIRE(!b->H || (b->heavy_chunk_ptr && d_hpart),
             "field-aware FM gradient: heavy keys without their chunks or scratch");
  const dim3 gt((unsigned)std::min<uint32_t>(b->ntiles, 1u << 16)), blk(kBlock);
#define XF_FFM_GU_V(OPTV, KK, VAL)                                                              \
  hipLaunchKernelGGL((k_ffm_grad_tiled<OPTV, KK, VAL>), gt, blk, 0, s, TW, TV, b->tile_ptr,     \
                     b->ntiles, b->segptr, b->coo_row, d_coo_pos, b->rowptr, b->uidx, d_xfg,    \
                     d_loss, d_wu, d_vu, d_rows_w, d_rows_v, b->R, k, kp, dim, d_gw, d_xval,    \
                     d_gv, d_mask)
#define XF_FFM_GU(OPTV, KK)                      \
  do {                                           \
    if (d_xval) XF_FFM_GU_V(OPTV, KK, true);     \
    else XF_FFM_GU_V(OPTV, KK, false);           \
  } while (0)
#define XF_FFM_GU_K(OPTV)                 \
  switch (k) {                            \
    case 4: XF_FFM_GU(OPTV, 4); break;    \
    case 8: XF_FFM_GU(OPTV, 8); break;    \
    case 16: XF_FFM_GU(OPTV, 16); break;  \
    default: XF_FFM_GU(OPTV, 0); break;   \
  }
  if (opt == kOptEmit) {
    XF_FFM_GU_K(kOptEmit)
  } else if (opt == XF_OPT_FTRL) {
    XF_FFM_GU_K(XF_OPT_FTRL)
  } else {
    XF_FFM_GU_K(XF_OPT_SGD)
  }
#undef XF_FFM_GU_K
#undef XF_FFM_GU
#undef XF_FFM_GU_V
  XF_HIP(hipGetLastError());
  if (b->H) {
    const dim3 gp(b->n_heavy_chunks), gf(b->H);
#define XF_FFM_HP(VAL)                                                                           \
  hipLaunchKernelGGL(k_ffm_heavy_partial<VAL>, gp, blk, 0, s, b->heavy, b->heavy_chunk_ptr, b->H, \
                     b->segptr, b->coo_row, d_coo_pos, b->rowptr, b->uidx, d_xfg, d_loss, d_vu, k, \
                     kp, dim, d_hpart, d_xval)
#define XF_FFM_HF(OPTV)                                                                          \
  hipLaunchKernelGGL(k_ffm_heavy_finish<OPTV>, gf, blk, 0, s, TW, TV, b->heavy, b->heavy_chunk_ptr, \
                     d_hpart, d_rows_w, d_rows_v, d_wu, d_vu, b->R, k, dim, d_gw, d_gv, d_mask)
    if (d_xval) XF_FFM_HP(true);
    else XF_FFM_HP(false);
    if (opt == kOptEmit) XF_FFM_HF(kOptEmit);
    else if (opt == XF_OPT_FTRL) XF_FFM_HF(XF_OPT_FTRL);
    else XF_FFM_HF(XF_OPT_SGD);
#undef XF_FFM_HF
#undef XF_FFM_HP
    XF_HIP(hipGetLastError());
  }
  return XF_OK;
}

// gradient + both Pushes for the tables on this GPU.  rows_w / rows_v: the keys' state rows,
// d_wu / d_vu: the rows the Pull returned (current: the step has not written them yet).  gw[U]
// is written for every key; d_hpart: ffm_heavy_doubles(b, F k) doubles.
int ffm_grad_update(xf_table *tw, xf_table *tv, const xf_dev_batch *b, int F,
                    const uint32_t *d_rows_w, const uint32_t *d_rows_v, const float *d_wu,
                    const float *d_vu, const uint32_t *d_xfg, const uint32_t *d_coo_pos,
                    const float *d_loss, float *d_gw, double *d_hpart, const float *d_xval,
                    hipStream_t s) {
  XF_REQUIRE(tw && tv && b && d_rows_w && d_rows_v && d_wu && d_vu && d_xfg && d_coo_pos &&
                 d_loss && d_gw, "field-aware FM gradient: null argument");
  if (b->U == 0) return XF_OK;
  const xf::TableDev &TW = xf::table_dev(tw), &TV = xf::table_dev(tv);
  const bool ftrl = TV.nz != nullptr;
  XF_REQUIRE((TW.nz != nullptr) == ftrl, "field-aware FM gradient: w and v use different optimizers");
  return ffm_grad_launch(ftrl ? XF_OPT_FTRL : XF_OPT_SGD, TW, TV, (uint32_t)TV.dim, b, F, d_rows_w,
                         d_rows_v, d_wu, d_vu, d_xfg, d_coo_pos, d_loss, d_gw, nullptr, nullptr,
                         d_hpart, d_xval, s);
}

// The gradient alone, for a worker whose keys live on other ranks: gw[U], gv[U x F k] and
// mask[U] (bit h: the minibatch touched field h of the key) from the pulled d_vu[U x F k] and the
// forward's d_loss.  Every entry of the three is written, an untouched coordinate of gv as 0; no
// table, state row or pulled w is read.  The keys' owners step what the Push brings them, v
// through the masks (table_update_heads_masked).  d_hpart: ffm_heavy_doubles(b, F k) doubles.
int ffm_grad_emit(const xf_dev_batch *b, int k, int F, const float *d_vu, const uint32_t *d_xfg,
                  const uint32_t *d_coo_pos, const float *d_loss, float *d_gw, float *d_gv,
                  uint64_t *d_mask, double *d_hpart, const float *d_xval, hipStream_t s) {
  XF_REQUIRE(b && k >= 1, "field-aware FM gradient (emit): bad argument");
  if (b->U == 0) return XF_OK;  // (no key: nothing to write, and the arrays may be empty)
  XF_REQUIRE(d_vu && d_xfg && d_coo_pos && d_loss && d_gw && d_gv && d_mask,
             "field-aware FM gradient (emit): bad argument");
  const TableDev none{};
  return ffm_grad_launch(kOptEmit, none, none, (uint32_t)F * (uint32_t)k, b, F, nullptr, nullptr,
                         nullptr, d_vu, d_xfg, d_coo_pos, d_loss, d_gw, d_gv,
                         (unsigned long long *)d_mask, d_hpart, d_xval, s);
}

}  // namespace xf
