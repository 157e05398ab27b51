// xf_fm_canonical.hip — canonical factorization machine (fm_mode = canonical, gfx950).
//
// Rendle's second-order term with per-factor sums and the 1/2, a nonzero contributing x (its
// value with feature_values = on, else 1); fp32(.) marks every rounding to fp32:
//   wx_r    = fp32(sum_j fp32(w[u_j] x_j))          gw[u] = fp32(fp32(sum_occ fp32(loss_r x_occ)) / R)
//   a_jf    = fp32(v[u_j,f] x_j)                    S[r,f] = fp32(sum_j a_jf)   (R x k, kept for the gradient)
//   y2_r    = fp32(0.5 (sum_f fp32(S[r,f]^2) - sum_f sum_j fp32(a_jf^2))) = sum_{i<j} <a_i, a_j>
//   gv[u,f] = fp32(fp32(sum_occ fp32(fp32(loss_r x_occ) fp32(S[r,f] - a_occ,f))) / R)
// The reference form (xf_model.hip, fm_worker.cc:159-202) pools its sums over all k factors,
// which collapses the k factors into one scalar per key; this form does not.  Every fp64 sum
// adds fp32 values (products are rounded to fp32 first), so it is exact and the result does
// not depend on lane assignment or order.  With x = 1 every product with x is exact: that gives
// the binary form exactly, bit for bit.
//
// One set of kernels, VAL their last template parameter.  VAL = true streams the values with the
// index they belong to (xval beside uidx in CSR order, coo_val beside coo_row grouped by key:
// coalesced, never gathered); VAL = false is the binary form with x folded away at compile time —
// no value load, no value staging, the value pointer (the last kernel argument) unread.
//
// Forward: one wavefront per row.  A lane is a (nonzero slot, factor) pair — P factors, 64 / P
// slots, four nonzeros in flight per lane; the per-factor fp64 sums are joined across the slots
// with shuffles, the S row leaves as one coalesced store.  P = k for k in {4, 8, 16, 32, 64};
// other k run with P = the next power of two (lanes beyond k idle), k > 64 in passes of 64.
// Gradient + the two Pushes: the minibatch's key tiles (xf_tiling.h) as in k_fm_grad_tiled,
// a tile's occurrence rows and losses staged in LDS, a lane per (key, factor) reading
// S[sid, f] of the key's occurrences from L2.  Heavy keys (> XF_HEAVY_SEG occurrences) are
// reduced in chunks over the whole chip and stepped by a second kernel.
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
using xf::blocks_for_groups;  // xf_wave.h
using xf::group_sum;
using xf::heavy_of_chunk;

// ------------------------------------------------------------------------------ forward
// P: factors per pass (a power of two <= 64); EXACT: k == P (a compile-time factor count).
// VAL: a = v x in place of v and w x in place of w, a lane's value loads at the addresses of its
// index loads
template <int P, bool EXACT, bool VAL>
__global__ void __launch_bounds__(kBlock)
k_fmc_forward(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ uidx,
              const float *__restrict__ wu, const float *__restrict__ vu, int k_rt,
              const int32_t *__restrict__ labels, uint32_t R, float *__restrict__ loss,
              float *__restrict__ pctr, float *__restrict__ S,
              const float *__restrict__ xval) {
#pragma clang fp contract(off)
  static_assert(P >= 1 && P <= 64 && (P & (P - 1)) == 0, "P: a power of two <= 64");
  const uint32_t k = EXACT ? (uint32_t)P : (uint32_t)k_rt;
  constexpr uint32_t kG = 64u / P;  // nonzero slots per pass
  const uint32_t lane = threadIdx.x & 63u, f = lane % P, sub = lane / P;
  const uint32_t nwaves = gridDim.x * (kBlock / 64);
  for (uint32_t r = blockIdx.x * (kBlock / 64) + threadIdx.x / 64; r < R; r += nwaves) {
    const uint32_t b = rowptr[r], n = rowptr[r + 1] - b;
    double wx = 0.0, t = 0.0, q = 0.0;
    for (uint32_t f0 = 0; f0 < k; f0 += P) {  // one pass unless k > 64
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
          xv[i] = (VAL && in) ? xval[b + j0 + i * kG] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          vv[i] = (on && ui[i] != 0xFFFFFFFFu) ? vu[(size_t)ui[i] * k + fk] : 0.0f;
          ww[i] = (f0 == 0 && f == 0 && ui[i] != 0xFFFFFFFFu) ? wu[ui[i]] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float a = VAL ? vv[i] * xv[i] : vv[i];  // fp32 products, here and below
          s += (double)a;
          q += (double)(a * a);
          wx += (double)(VAL ? ww[i] * xv[i] : ww[i]);
        }
      }
#pragma unroll
      for (uint32_t off = P; off < 64; off <<= 1) s += __shfl_xor(s, (int)off);
      const float sf = (float)s;
      if (sub == 0 && on) {
        S[(size_t)r * k + fk] = sf;
        t += (double)(sf * sf);  // fp32 square
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

// ------------------------------------------------------------ gradient + the two Pushes
// A workgroup per gradient tile (keys [tile_ptr[t], tile_ptr[t+1]), <= XF_GRAD_TILE_NNZ
// occurrences): the occurrences' rows and losses go to LDS once, then a lane per (key, factor)
// item sums loss * (S[sid, f] - v[u, f]) over the key's occurrences — the S values of one
// occurrence are read by neighbouring lanes from one contiguous k x 4-byte row — and applies
// the optimizer step to that coordinate of the key's v row (the pulled value is the current
// weight: nothing touched the row since the Pull).  One lane per key does the same for w.
// VAL: the occurrences' values staged beside their rows — lx = loss x (what the w gradient sums),
// xs = x (for a = v x); binary: lx is the plain loss and xs is not there.
// OPT = xf::kOptEmit: the gradient goes out instead — gv[u k + f] beside gw[u] — and neither the
// state rows nor the tables nor wu are read (the worker of a sharded trainer: the owner steps).
template <int OPT, int K /* compile-time factor count, 0 = k_rt */, bool VAL>
__global__ void __launch_bounds__(kBlock)
k_fmc_grad_tiled(xf::TableDev TW, xf::TableDev TV, const uint32_t *__restrict__ tile_ptr,
                 uint32_t ntiles, const uint32_t *__restrict__ segptr,
                 const uint32_t *__restrict__ coo_row, const float *__restrict__ loss,
                 const float *__restrict__ S, const float *__restrict__ wu,
                 const float *__restrict__ vu, const uint32_t *__restrict__ rows_w,
                 const uint32_t *__restrict__ rows_v, uint32_t R, int k_rt,
                 float *__restrict__ gw, const float *__restrict__ coo_val,
                 float *__restrict__ gv) {
#pragma clang fp contract(off)
  constexpr bool kEmit = OPT == xf::kOptEmit;
  __shared__ float lx[XF_GRAD_TILE_NNZ];
  __shared__ float xs[VAL ? XF_GRAD_TILE_NNZ : 1];
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
      const float x = VAL ? coo_val[j] : 1.0f;
      ss[j - j0] = sid;
      if constexpr (VAL) xs[j - j0] = x;
      lx[j - j0] = VAL ? loss[sid] * x : loss[sid];
    }
    __syncthreads();
    const uint32_t nel = nk * k;
    constexpr int kUn = 4;  // items in flight per lane: factors and state requested together
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
        if constexpr (kEmit) to[i] = (size_t)(ua + kq[i]) * k + kk[i];  // (its place in gv)
        else
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
          for (int m = 0; m < 4; ++m)
            acc += (double)(lx[j + m] * (sv[m] - (VAL ? v[i] * xs[j + m] : v[i])));
        }
        for (; j < e; ++j)
          acc += (double)(lx[j] * (S[(size_t)ss[j] * k + kk[i]] - (VAL ? v[i] * xs[j] : v[i])));
        const float g = xf::div_by_rows((float)acc, R);
        constexpr bool kNZ = OPT == XF_OPT_FTRL;  // (vn, vz: requested above, FTRL only)
        if constexpr (kEmit) gv[to[i]] = g;
        else
          xf::step_coord<OPT>(TV, to[i], v[i], g, kNZ ? vn[i] : 0.0f, kNZ ? vz[i] : 0.0f);
      }
    }
    // the keys' w: the true gradient (sum of the occurrences' losses) / R, one lane per key
    for (uint32_t q = tid; q < nk; q += kBlock) {
      double aw = 0.0;
      for (uint32_t j = sp[q]; j < sp[q + 1]; ++j) aw += (double)lx[j];
      const float g1 = xf::div_by_rows((float)aw, R);
      gw[ua + q] = g1;
      if constexpr (!kEmit) xf::step_coord<OPT>(TW, rows_w[ua + q], wu[ua + q], g1);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------- heavy keys
// A heavy key's occurrences in chunks of XF_TILE_NNZ (the batch's heavy_chunk_ptr), one
// workgroup per chunk: partial[chunk][col] for the k factor columns and the loss sum (column k).
// A thread is (slice of the chunk's occurrences, column); columns beyond one workgroup's width
// (k >= 256) take further passes.  VAL: the chunk's values staged as in k_fmc_grad_tiled.  k = 0
// (LR, xf_valued.hip) leaves the loss column alone: S and vu are not read.
template <bool VAL>
__global__ void __launch_bounds__(kBlock)
k_fmc_heavy_partial(const uint32_t *__restrict__ heavy, const uint32_t *__restrict__ hch,
                    uint32_t H, const uint32_t *__restrict__ segptr,
                    const uint32_t *__restrict__ coo_row, const float *__restrict__ loss,
                    const float *__restrict__ S, const float *__restrict__ vu, int k_rt,
                    double *__restrict__ partial, const float *__restrict__ coo_val) {
#pragma clang fp contract(off)
  __shared__ float lx[XF_TILE_NNZ];
  __shared__ float xs[VAL ? XF_TILE_NNZ : 1];
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
    const float x = VAL ? coo_val[b + j] : 1.0f;
    ss[j] = sid;
    if constexpr (VAL) xs[j] = x;
    lx[j] = VAL ? loss[sid] * x : loss[sid];
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
        // a slice is ~n / nsl occurrences long (k = 64: ~680): eight S gathers in flight per
        // thread, eight independent sums (exact: joined in any order)
        double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        uint32_t j = sl;
        for (; j + 7 * nsl < n; j += 8 * nsl) {
          float sv[8];
#pragma unroll
          for (int m = 0; m < 8; ++m) sv[m] = S[(size_t)ss[j + m * nsl] * k + col];
#pragma unroll
          for (int m = 0; m < 8; ++m)
            a[m] += (double)(lx[j + m * nsl] * (sv[m] - (VAL ? v * xs[j + m * nsl] : v)));
        }
        for (; j < n; j += nsl)
          a[0] += (double)(lx[j] * (S[(size_t)ss[j] * k + col] - (VAL ? v * xs[j] : v)));
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

// one workgroup per heavy key: its chunks' partial sums added per column, then the optimizer
// steps of its k factors and of its w (OPT = xf::kOptEmit: gv[u k + col] and gw[u] written, no step)
template <int OPT>
__global__ void __launch_bounds__(kBlock)
k_fmc_heavy_finish(xf::TableDev TW, xf::TableDev TV, const uint32_t *__restrict__ heavy,
                   const uint32_t *__restrict__ hch, const double *__restrict__ partial,
                   const uint32_t *__restrict__ rows_w, const uint32_t *__restrict__ rows_v,
                   const float *__restrict__ wu, const float *__restrict__ vu, uint32_t R,
                   int k_rt, float *__restrict__ gw, float *__restrict__ gv) {
#pragma clang fp contract(off)
  constexpr bool kEmit = OPT == xf::kOptEmit;
  __shared__ double red[kBlock];
  const uint32_t tid = threadIdx.x, h = blockIdx.x, k = (uint32_t)k_rt;
  const uint32_t u = heavy[h], c0h = hch[h], c1h = hch[h + 1];
  const uint32_t ncol = k + 1u, cpp = min(ncol, (uint32_t)kBlock), nsl = kBlock / cpp;
  const uint32_t cl = tid % cpp, sl = tid / cpp;
  for (uint32_t p0 = 0; p0 < ncol; p0 += cpp) {
    const uint32_t col = p0 + cl;
    double acc = 0.0;
    if (sl < nsl && col < ncol)
      for (uint32_t c = c0h + sl; c < c1h; c += nsl) acc += partial[(size_t)c * ncol + col];
    red[tid] = acc;
    __syncthreads();
    if (sl == 0 && col < ncol) {
      for (uint32_t q = 1; q < nsl; ++q) acc += red[q * cpp + cl];
      const float g = xf::div_by_rows((float)acc, R);
      if (col < k) {
        if constexpr (kEmit) gv[(size_t)u * k + col] = g;
        else
          xf::step_coord<OPT>(TV, (size_t)rows_v[u] * k + col, vu[(size_t)u * k + col], g);
      } else {
        gw[u] = g;
        if constexpr (!kEmit) xf::step_coord<OPT>(TW, rows_w[u], wu[u], g);
      }
    }
    __syncthreads();
  }
}

}  // namespace

namespace xf {

// scratch of the heavy keys' chunk sums: doubles
size_t fmc_heavy_doubles(const xf_dev_batch *b, int k) {
  return b->H ? (size_t)b->n_heavy_chunks * ((size_t)k + 1) : 0;
}

// loss[R], pctr[R] (may be null), S[R x k] from the pulled rows w_u[U], v_u[U x k].  d_xval: the
// values in CSR order, null for a binary minibatch (the caller holds a valued one to its array).
int fmc_forward(const xf_dev_batch *b, int k, const float *d_wu, const float *d_vu, float *d_S,
                float *d_loss, float *d_pctr, const float *d_xval, hipStream_t s) {
  XF_REQUIRE(b && d_wu && d_vu && d_S && d_loss && k >= 1, "fm canonical forward: bad argument");
  if (b->R == 0) return XF_OK;
  const dim3 g(blocks_for_groups(b->R, kBlock / 64)), blk(kBlock);
#define XF_FMC_FWD_V(PP, EX, VAL)                                                                  \
  hipLaunchKernelGGL((k_fmc_forward<PP, EX, VAL>), g, blk, 0, s, b->rowptr, b->uidx, d_wu, d_vu, k, \
                     b->labels, b->R, d_loss, d_pctr, d_S, d_xval)
#define XF_FMC_FWD(PP, EX)                  \
  do {                                      \
    if (d_xval) XF_FMC_FWD_V(PP, EX, true); \
    else XF_FMC_FWD_V(PP, EX, false);       \
  } while (0)
  switch (k) {
    case 4: XF_FMC_FWD(4, true); break;
    case 8: XF_FMC_FWD(8, true); break;
    case 16: XF_FMC_FWD(16, true); break;
    case 32: XF_FMC_FWD(32, true); break;
    case 64: XF_FMC_FWD(64, true); break;
    default:
      if (k <= 1) XF_FMC_FWD(1, false);
      else if (k <= 2) XF_FMC_FWD(2, false);
      else if (k <= 4) XF_FMC_FWD(4, false);
      else if (k <= 8) XF_FMC_FWD(8, false);
      else if (k <= 16) XF_FMC_FWD(16, false);
      else if (k <= 32) XF_FMC_FWD(32, false);
      else XF_FMC_FWD(64, false);
      break;
  }
#undef XF_FMC_FWD
#undef XF_FMC_FWD_V
  XF_HIP(hipGetLastError());
  return XF_OK;
}

// the heavy keys' two kernels: the chunk sums, then a key's chunks added and its k + 1 coordinates
// stepped.  k = 0 steps w alone (valued LR, xf_valued.hip: d_S, d_vu, d_rows_v and TV are not
// read).  d_coo_val: null for a binary minibatch.  d_hpart: fmc_heavy_doubles(b, k) doubles.
// opt: XF_OPT_* — the tables' optimizer — or kOptEmit: d_gw[u] and d_gv[u k + col] written and
// nothing stepped (the tables, the state rows and d_wu are not read).
void fmc_heavy_update(int opt, const TableDev &TW, const TableDev &TV, int k, const xf_dev_batch *b,
                      const uint32_t *d_rows_w, const uint32_t *d_rows_v, const float *d_wu,
                      const float *d_vu, const float *d_S, const float *d_loss, float *d_gw,
                      float *d_gv, double *d_hpart, const float *d_coo_val, hipStream_t s) {
  const dim3 gp(b->n_heavy_chunks), gf(b->H), blk(kBlock);
#define XF_FMC_HP(VAL)                                                                         \
  hipLaunchKernelGGL(k_fmc_heavy_partial<VAL>, gp, blk, 0, s, b->heavy, b->heavy_chunk_ptr, b->H, \
                     b->segptr, b->coo_row, d_loss, d_S, d_vu, k, d_hpart, d_coo_val)
#define XF_FMC_HF(OPTV)                                                                         \
  hipLaunchKernelGGL(k_fmc_heavy_finish<OPTV>, gf, blk, 0, s, TW, TV, b->heavy, b->heavy_chunk_ptr, \
                     d_hpart, d_rows_w, d_rows_v, d_wu, d_vu, b->R, k, d_gw, d_gv)
  if (d_coo_val) XF_FMC_HP(true);
  else XF_FMC_HP(false);
  if (opt == kOptEmit) XF_FMC_HF(kOptEmit);
  else if (opt == XF_OPT_FTRL) XF_FMC_HF(XF_OPT_FTRL);
  else XF_FMC_HF(XF_OPT_SGD);
#undef XF_FMC_HF
#undef XF_FMC_HP
}

// the tile kernel and the heavy keys' two for one OPT (an optimizer, or kOptEmit with d_gv)
static int fmc_grad_launch(int opt, const TableDev &TW, const TableDev &TV, int k,
                           const xf_dev_batch *b, const uint32_t *d_rows_w,
                           const uint32_t *d_rows_v, const float *d_wu, const float *d_vu,
                           const float *d_S, const float *d_loss, float *d_gw, float *d_gv,
                           double *d_hpart, const float *d_coo_val, hipStream_t s) {
  XF_REQUIRE(b->ntiles && b->tile_ptr, "fm canonical gradient: the minibatch has no gradient tiles");
  XF_REQUIRE(!b->H || (b->heavy_chunk_ptr && d_hpart),
             "fm canonical gradient: heavy keys without their chunks or scratch");
  const dim3 gt((unsigned)std::min<uint32_t>(b->ntiles, 1u << 16)), blk(kBlock);
#define XF_FMC_GU_V(OPTV, KK, VAL)                                                               \
  hipLaunchKernelGGL((k_fmc_grad_tiled<OPTV, KK, VAL>), gt, blk, 0, s, TW, TV, b->tile_ptr,      \
                     b->ntiles, b->segptr, b->coo_row, d_loss, d_S, d_wu, d_vu, d_rows_w, d_rows_v, \
                     b->R, k, d_gw, d_coo_val, d_gv)
#define XF_FMC_GU(OPTV, KK)                        \
  do {                                             \
    if (d_coo_val) XF_FMC_GU_V(OPTV, KK, true);    \
    else XF_FMC_GU_V(OPTV, KK, false);             \
  } while (0)
#define XF_FMC_GU_K(OPTV)                 \
  switch (k) {                            \
    case 4: XF_FMC_GU(OPTV, 4); break;    \
    case 8: XF_FMC_GU(OPTV, 8); break;    \
    case 16: XF_FMC_GU(OPTV, 16); break;  \
    case 32: XF_FMC_GU(OPTV, 32); break;  \
    case 64: XF_FMC_GU(OPTV, 64); break;  \
    default: XF_FMC_GU(OPTV, 0); break;   \
  }
  if (opt == kOptEmit) {
    XF_FMC_GU_K(kOptEmit)
  } else if (opt == XF_OPT_FTRL) {
    XF_FMC_GU_K(XF_OPT_FTRL)
  } else {
    XF_FMC_GU_K(XF_OPT_SGD)
  }
#undef XF_FMC_GU_K
#undef XF_FMC_GU
#undef XF_FMC_GU_V
  XF_HIP(hipGetLastError());
  if (b->H) {
    fmc_heavy_update(opt, TW, TV, k, b, d_rows_w, d_rows_v, d_wu, d_vu, d_S, d_loss, d_gw, d_gv,
                     d_hpart, d_coo_val, s);
    XF_HIP(hipGetLastError());
  }
  return XF_OK;
}

// gradient + both Pushes for the tables on this GPU.  rows_w / rows_v: the keys' state rows,
// d_wu / d_vu: the rows the Pull returned (current: the step has not written them yet).  gw[U]
// is written for every key (the capture hook); d_hpart: fmc_heavy_doubles(b, k) doubles.
// d_coo_val: the values in key-grouped order, null for a binary minibatch.
int fmc_grad_update(xf_table *tw, xf_table *tv, const xf_dev_batch *b, const uint32_t *d_rows_w,
                    const uint32_t *d_rows_v, const float *d_wu, const float *d_vu,
                    const float *d_S, const float *d_loss, float *d_gw, double *d_hpart,
                    const float *d_coo_val, hipStream_t s) {
  XF_REQUIRE(tw && tv && b && d_rows_w && d_rows_v && d_wu && d_vu && d_S && d_loss && d_gw,
             "fm canonical gradient: null argument");
  if (b->U == 0) return XF_OK;
  const xf::TableDev &TW = xf::table_dev(tw), &TV = xf::table_dev(tv);
  const bool ftrl = TV.nz != nullptr;
  XF_REQUIRE((TW.nz != nullptr) == ftrl, "fm canonical gradient: w and v use different optimizers");
  return fmc_grad_launch(ftrl ? XF_OPT_FTRL : XF_OPT_SGD, TW, TV, TV.dim, b, d_rows_w, d_rows_v,
                         d_wu, d_vu, d_S, d_loss, d_gw, nullptr, d_hpart, d_coo_val, s);
}

// The gradient alone, for a worker whose keys live on other ranks: gw[U] and gv[U x k] from the
// pulled d_vu[U x k], the forward's d_S and d_loss; every entry of both is written.  No table,
// no state row and no pulled w is read: the keys' owners step what the Push brings them
// (table_update_heads).  d_hpart, d_coo_val: as fmc_grad_update's.
int fmc_grad_emit(const xf_dev_batch *b, int k, const float *d_vu, const float *d_S,
                  const float *d_loss, float *d_gw, float *d_gv, double *d_hpart,
                  const float *d_coo_val, hipStream_t s) {
  XF_REQUIRE(b && k >= 1, "fm canonical gradient (emit): bad argument");
  if (b->U == 0) return XF_OK;  // (no key: nothing to write, and the arrays may be empty)
  XF_REQUIRE(d_vu && d_S && d_loss && d_gw && d_gv, "fm canonical gradient (emit): bad argument");
  const TableDev none{};
  return fmc_grad_launch(kOptEmit, none, none, k, b, nullptr, nullptr, nullptr, d_vu, d_S, d_loss,
                         d_gw, d_gv, d_hpart, d_coo_val, s);
}

}  // namespace xf
