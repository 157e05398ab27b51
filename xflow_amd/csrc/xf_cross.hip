// xf_cross.hip — feature crosses: a GPU stage ahead of the key build.
//
// LR on click data is as good as its crossed features, and the input carries what a cross needs:
// every token is fgid:fid:val.  For each listed pair of fields (fa, fb) a row gains one nonzero per
// (member of fa, member of fb), keyed by a hash of the two keys and the two field ids (xf_cross.h,
// one definition for the host and the kernels).  Not in the reference.
//
// Like admission (xf_admit.hip) and negative subsampling (xf_negsample.hip) the stage is a filter
// on a minibatch's CSR arrays ahead of any key build; it keeps no state and ADDS nonzeros: a row's
// output is its input followed by the crossed nonzeros of pair 0, 1, ...; inside a pair the member
// of fa is the slow index.  Every position is arithmetic on counts — no atomic decides one — so the
// result does not depend on the launch shape.
//
// Kernels (a workgroup is 4 waves and owns kCxTile consecutive rows; a wave takes every fourth):
//   k_cx_count      a wave per row: the row's fgids in the lanes (64 at a time), a pair's members two
//                   __ballot masks, its crossed nonzeros the product of their popcounts; the row's
//                   output length (saturated to 32 bits; the sums are 64-bit and saturate too), per
//                   tile the total, and — statistics, not positions — the input nonzeros and the
//                   longest row.  (rocPRIM's exclusive scan turns the tile totals into offsets.)
//   k_cx_emit       the same tiles: a scan of the tile's output lengths gives rowptr_out; then a
//                   wave per row of at most 64 nonzeros (every click row): the lanes hold the row,
//                   copy it, and lane c of each 64 crossed positions finds its pair by the running
//                   sum of the products and its (i, j) as the n-th set bits of the pair's two masks;
//                   the two keys and values come by __shfl.
//   k_cx_emit_long  launched only when the count saw a longer row: the workgroup takes each long row
//                   of its tile in turn; per pair the member masks of the row's 64-nonzero chunks and
//                   their running popcounts are the member lists (24 bytes per chunk: in LDS up to
//                   2048 chunks = 131072 nonzeros, beyond that in a global scratch), a crossed
//                   position maps to (i, j) by a binary search of the running counts and the n-th
//                   set bit of the chunk's mask.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <vector>

#include "xf_common.h"
#include "xf_cross.h"
#include "xflow_amd.h"

namespace {

constexpr int kCxThreads = 256;
constexpr uint32_t kCxWaves = kCxThreads / 64;
constexpr uint32_t kCxTile = 64;          // rows of one workgroup of the count and the emit passes
constexpr uint32_t kCxMaxChunks = 2048;   // chunks of a long row whose member lists sit in LDS
static_assert(kCxTile == 64, "one wave scans a tile's output lengths");

struct CxSpec {
  int32_t fa[xf::kCrossMaxPairs], fb[xf::kCrossMaxPairs];
  uint64_t salt[xf::kCrossMaxPairs];
  int32_t P, fgid_base;
};

struct SatPlus {
  __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
    return xf::cross_sat_add(a, b);
  }
};

// the row's first nonzero and its length; a row whose offsets descend or leave the arrays has
// length 0
__device__ inline uint32_t cx_row(const uint32_t *__restrict__ rowptr, uint32_t r, uint32_t NNZ,
                                  uint32_t *a) {
  const uint32_t x = rowptr[r], y = rowptr[r + 1];
  *a = x;
  return (y >= x && y <= NNZ) ? y - x : 0u;
}

// the position of the n-th (from 0) set bit of m; n below the popcount
__device__ inline uint32_t cx_nth_bit(uint64_t m, uint32_t n) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t w = 32; w; w >>= 1) {
    const uint32_t c = (uint32_t)__popcll((m >> pos) & ((1ull << w) - 1));
    if (n >= c) {
      n -= c;
      pos += w;
    }
  }
  return pos & 63;
}

// the crossed nonzeros of one row, sum over the pairs of |A| x |B| (every lane of the wave calls;
// the result is wave-uniform)
__device__ inline uint64_t cx_count_row(const int32_t *__restrict__ fgid, uint32_t a, uint32_t len,
                                        uint32_t lane, const CxSpec &sp) {
  uint64_t n = 0;
  if (len <= 64) {
    const bool in = lane < len;
    const int32_t fg = in ? fgid[a + lane] : 0;
    for (int p = 0; p < sp.P; ++p) {
      const uint32_t na = (uint32_t)__popcll(__ballot(in && fg == sp.fa[p]));
      const uint32_t nb = (uint32_t)__popcll(__ballot(in && fg == sp.fb[p]));
      n += (uint64_t)na * nb;
    }
    return n;
  }
  for (int p = 0; p < sp.P; ++p) {
    uint32_t na = 0, nb = 0;  // (na + nb <= len < 2^32: the product stays below 2^62)
    for (uint32_t c = 0; c < len; c += 64) {
      const bool in = lane < len - c;
      const int32_t fg = in ? fgid[a + c + lane] : 0;
      na += (uint32_t)__popcll(__ballot(in && fg == sp.fa[p]));
      nb += (uint32_t)__popcll(__ballot(in && fg == sp.fb[p]));
      if (len - c <= 64) break;  // (c + 64 may not wrap)
    }
    n = xf::cross_sat_add(n, (uint64_t)na * nb);
  }
  return n;
}

// row_cnt[r] = min(2^32 - 1, the row's output length); tile_cnt[tile] = the tile's output nonzeros
// (saturating), tile_cnt[ntiles] = 0 (its exclusive sum: the total); stat[0] += input nonzeros,
// stat[1] = max(longest row), stat[2] += rows whose offsets descend or leave the arrays (zero on
// entry)
__global__ __launch_bounds__(kCxThreads) void k_cx_count(
    const int32_t *__restrict__ fgid, const uint32_t *__restrict__ rowptr, uint32_t R,
    uint32_t NNZ, const CxSpec sp, uint32_t *__restrict__ row_cnt,
    uint64_t *__restrict__ tile_cnt, uint32_t ntiles, unsigned long long *stat) {
  __shared__ uint64_t s_out[kCxWaves], s_in[kCxWaves];
  __shared__ uint32_t s_max[kCxWaves], s_bad[kCxWaves];
  const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint64_t out = 0, in = 0;
  uint32_t longest = 0, bad = 0;
  for (uint32_t k = wave; k < kCxTile; k += kCxWaves) {
    const uint32_t r = tile * kCxTile + k;
    if (r >= R) break;
    uint32_t a;
    const uint32_t len = cx_row(rowptr, r, NNZ, &a);
    const uint64_t n = xf::cross_sat_add(len, cx_count_row(fgid, a, len, lane, sp));
    if (lane == 0) row_cnt[r] = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
    out = xf::cross_sat_add(out, n);
    in += len;
    longest = max(longest, len);
    if (rowptr[r + 1] < a || rowptr[r + 1] > NNZ) ++bad;
  }
  if (lane == 0) {
    s_out[wave] = out;
    s_in[wave] = in;
    s_max[wave] = longest;
    s_bad[wave] = bad;
  }
  __syncthreads();
  if (t == 0) {
    out = in = 0;
    longest = bad = 0;
    for (uint32_t w = 0; w < kCxWaves; ++w) {
      out = xf::cross_sat_add(out, s_out[w]);
      in += s_in[w];
      longest = max(longest, s_max[w]);
      bad += s_bad[w];
    }
    tile_cnt[tile] = out;
    if (tile == 0) tile_cnt[ntiles] = 0;
    if (in) atomicAdd(&stat[0], (unsigned long long)in);
    if (longest) atomicMax(&stat[1], (unsigned long long)longest);
    if (bad) atomicAdd(&stat[2], (unsigned long long)bad);
  }
}

// s_at[k] = the output offset of row tile * kCxTile + k, s_cnt[k] its output length (wave 0 scans;
// the caller synchronises); rowptr_out for the tile's rows, the last tile closes it
__device__ inline void cx_place_tile(const uint32_t *__restrict__ row_cnt,
                                     const uint64_t *__restrict__ tile_off, uint32_t ntiles,
                                     uint32_t R, uint32_t tile, uint32_t t, uint32_t *s_at,
                                     uint32_t *s_cnt, uint32_t *__restrict__ rowptr_out) {
  if (t >= 64) return;
  const uint32_t r = tile * kCxTile + t;
  const uint32_t c = r < R ? row_cnt[r] : 0u;
  uint32_t incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(incl, off, 64);
    if (t >= (uint32_t)off) incl += u;
  }
  const uint32_t at = (uint32_t)tile_off[tile] + incl - c;
  s_at[t] = at;
  s_cnt[t] = c;
  if (rowptr_out) {
    if (r < R) rowptr_out[r] = at;
    if (tile == ntiles - 1 && t == 0) rowptr_out[R] = (uint32_t)tile_off[ntiles];
  }
}

__global__ __launch_bounds__(kCxThreads) void k_cx_emit(
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ fgid,
    const float *__restrict__ vals, const uint32_t *__restrict__ rowptr, uint32_t R, uint32_t NNZ,
    const CxSpec sp, const uint32_t *__restrict__ row_cnt, const uint64_t *__restrict__ tile_off,
    uint32_t ntiles, uint32_t short_max, uint64_t *__restrict__ keys_out,
    int32_t *__restrict__ fgid_out, float *__restrict__ vals_out,
    uint32_t *__restrict__ rowptr_out) {
  __shared__ uint32_t s_at[kCxTile], s_cnt[kCxTile];
  const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint64_t total = tile_off[ntiles];
  if (total >= 0xFFFFFFFFull) return;  // (uniform; the host has refused the call from this total)
  const uint32_t nnz_out = (uint32_t)total;
  cx_place_tile(row_cnt, tile_off, ntiles, R, tile, t, s_at, s_cnt, rowptr_out);
  __syncthreads();
  for (uint32_t k = wave; k < kCxTile; k += kCxWaves) {
    const uint32_t r = tile * kCxTile + k;
    if (r >= R) break;
    uint32_t a;
    const uint32_t len = cx_row(rowptr, r, NNZ, &a);
    if (len == 0 || len > short_max) continue;  // (longer rows: k_cx_emit_long)
    const uint32_t out = s_at[k], ncross = s_cnt[k] - len;
    const bool in = lane < len;
    const uint64_t key = in ? keys[a + lane] : 0ull;
    const int32_t fg = in ? fgid[a + lane] : 0;
    const float v = in && vals ? vals[a + lane] : 0.0f;
    if (in && out + lane < nnz_out) {
      keys_out[out + lane] = key;
      if (fgid_out) fgid_out[out + lane] = fg;
      if (vals_out) vals_out[out + lane] = v;
    }
    for (uint32_t c0 = 0; c0 < ncross; c0 += 64) {
      const uint32_t c = c0 + lane;
      uint64_t my_ma = 0, my_mb = 0, my_salt = 0;
      uint32_t my_q = 0, my_nb = 1, base = 0;
      int32_t my_p = 0;
      for (int p = 0; p < sp.P; ++p) {
        const uint64_t ma = __ballot(in && fg == sp.fa[p]), mb = __ballot(in && fg == sp.fb[p]);
        const uint32_t nb = (uint32_t)__popcll(mb), cnt = (uint32_t)__popcll(ma) * nb;
        if (c >= base && c - base < cnt) {
          my_ma = ma;
          my_mb = mb;
          my_salt = sp.salt[p];
          my_q = c - base;
          my_nb = nb;
          my_p = p;
        }
        base += cnt;
      }
      const uint32_t ia = my_q / my_nb, jb = my_q - ia * my_nb;
      const uint32_t i = cx_nth_bit(my_ma, ia), j = cx_nth_bit(my_mb, jb);
      const uint64_t ki = __shfl(key, (int)i, 64), kj = __shfl(key, (int)j, 64);
      const float vi = __shfl(v, (int)i, 64), vj = __shfl(v, (int)j, 64);
      const uint32_t pos = out + len + c;
      if (c < ncross && my_ma && pos < nnz_out) {
        keys_out[pos] = xf::cross_key_salted(ki, kj, my_salt);
        if (fgid_out) fgid_out[pos] = sp.fgid_base + my_p;
        if (vals_out) vals_out[pos] = vi * vj;
      }
    }
  }
}

// the n-th (from 0) member of one side of a pair in a long row, as its index in the row: the chunk
// is the last one whose running count is at most n
template <typename M, typename Q>
__device__ inline uint32_t cx_member(const M *mask, const Q *pre, uint32_t nch, uint32_t n) {
  uint32_t lo = 0, hi = nch - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (pre[mid] <= n) lo = mid;
    else
      hi = mid - 1;
  }
  return lo * 64 + cx_nth_bit(mask[lo], n - pre[lo]);
}

// one long row by the whole workgroup; m0 / m1, p0 / p1: room for nch masks and running counts of
// the two sides (LDS or global), tot: two words of LDS
template <typename M, typename Q>
__device__ inline void cx_long_row(const uint64_t *__restrict__ keys,
                                   const int32_t *__restrict__ fgid,
                                   const float *__restrict__ vals, uint32_t a, uint32_t len,
                                   uint32_t out, uint32_t nnz_out, const CxSpec &sp, M *m0, M *m1,
                                   Q *p0, Q *p1, uint32_t *tot, uint64_t *__restrict__ keys_out,
                                   int32_t *__restrict__ fgid_out, float *__restrict__ vals_out) {
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t nch = (len - 1) / 64 + 1;
  for (uint32_t i = t; i < len; i += kCxThreads)
    if (out + i < nnz_out) {
      keys_out[out + i] = keys[a + i];
      if (fgid_out) fgid_out[out + i] = fgid[a + i];
      if (vals_out) vals_out[out + i] = vals[a + i];
    }
  uint64_t base = len;  // the row-relative position of the pair's first crossed nonzero
  for (int p = 0; p < sp.P; ++p) {
    for (uint32_t c = wave; c < nch; c += kCxWaves) {
      const bool in = lane < len - c * 64;
      const int32_t fg = in ? fgid[a + c * 64 + lane] : 0;
      const uint64_t ma = __ballot(in && fg == sp.fa[p]), mb = __ballot(in && fg == sp.fb[p]);
      if (lane == 0) {
        m0[c] = ma;
        m1[c] = mb;
      }
    }
    __syncthreads();
    if (wave < 2) {  // the running counts: wave 0 the fa side, wave 1 the fb side
      const M *m = wave ? m1 : m0;
      Q *pr = wave ? p1 : p0;
      uint32_t carry = 0;
      for (uint32_t c0 = 0; c0 < nch; c0 += 64) {
        const uint32_t c = c0 + lane;
        const uint32_t x = c < nch ? (uint32_t)__popcll(m[c]) : 0u;
        uint32_t incl = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t u = __shfl_up(incl, off, 64);
          if (lane >= (uint32_t)off) incl += u;
        }
        if (c < nch) pr[c] = carry + incl - x;
        carry += __shfl(incl, 63, 64);
      }
      if (lane == 0) tot[wave] = carry;
    }
    __syncthreads();
    const uint32_t nb = tot[1];
    const uint64_t cnt = (uint64_t)tot[0] * nb;
    const uint64_t salt = sp.salt[p];
    for (uint64_t q = t; q < cnt; q += kCxThreads) {
      const uint64_t pos = (uint64_t)out + base + q;
      if (pos >= nnz_out) break;
      const uint32_t ia = (uint32_t)(q / nb), jb = (uint32_t)(q - (uint64_t)ia * nb);
      const uint32_t i = cx_member(m0, p0, nch, ia), j = cx_member(m1, p1, nch, jb);
      if (i >= len || j >= len) continue;  // (never: the masks cover the row)
      keys_out[pos] = xf::cross_key_salted(keys[a + i], keys[a + j], salt);
      if (fgid_out) fgid_out[pos] = sp.fgid_base + p;
      if (vals_out) vals_out[pos] = vals[a + i] * vals[a + j];
    }
    base += cnt;
    __syncthreads();  // (the next pair rewrites the lists)
  }
}

// g_mask / g_pre: 2 * g_cap entries each, for the rows whose lists do not fit lds_chunks; such a
// row's region starts at entry 2 * (a / 64 + r) — disjoint where every row's offsets ascend (the
// host takes such a row only then: the count's third statistic)
__global__ __launch_bounds__(kCxThreads) void k_cx_emit_long(
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ fgid,
    const float *__restrict__ vals, const uint32_t *__restrict__ rowptr, uint32_t R, uint32_t NNZ,
    const CxSpec sp, const uint64_t *__restrict__ tile_off, uint32_t ntiles,
    const uint32_t *__restrict__ rowptr_out, uint32_t short_max, uint32_t lds_chunks,
    uint64_t *g_mask, uint32_t *g_pre, uint64_t g_cap, uint64_t *__restrict__ keys_out,
    int32_t *__restrict__ fgid_out, float *__restrict__ vals_out) {
  __shared__ uint64_t s_mask[2][kCxMaxChunks];
  __shared__ uint32_t s_pre[2][kCxMaxChunks];
  __shared__ uint32_t s_tot[2];
  const uint32_t tile = blockIdx.x;
  const uint64_t total = tile_off[ntiles];
  if (total >= 0xFFFFFFFFull) return;  // (uniform)
  for (uint32_t k = 0; k < kCxTile; ++k) {
    const uint32_t r = tile * kCxTile + k;
    if (r >= R) break;
    uint32_t a;
    const uint32_t len = cx_row(rowptr, r, NNZ, &a);
    if (len == 0 || len <= short_max) continue;  // (uniform: the whole workgroup takes the row)
    const uint32_t nch = (len - 1) / 64 + 1, out = rowptr_out[r];
    if (nch <= lds_chunks && nch <= kCxMaxChunks) {
      cx_long_row(keys, fgid, vals, a, len, out, (uint32_t)total, sp, s_mask[0], s_mask[1],
                  s_pre[0], s_pre[1], s_tot, keys_out, fgid_out, vals_out);
    } else {
      const uint64_t off = (uint64_t)(a / 64) + r;
      if (!g_mask || off + nch > g_cap) continue;  // (never: the host sized the scratch)
      cx_long_row(keys, fgid, vals, a, len, out, (uint32_t)total, sp, g_mask + 2 * off,
                  g_mask + 2 * off + nch, g_pre + 2 * off, g_pre + 2 * off + nch, s_tot, keys_out,
                  fgid_out, vals_out);
    }
  }
}

template <typename T>
int grow(T **p, size_t *cap, size_t need) {
  if (need <= *cap && *p) return XF_OK;
  if (*p) XF_HIP(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  const size_t n = need + need / 4 + 64;
  XF_HIP(hipMalloc((void **)p, n * sizeof(T)));
  *cap = n;
  return XF_OK;
}

}  // namespace

struct xf_cross {
  CxSpec spec;
  uint64_t rows_seen = 0, nonzeros_in = 0, nonzeros_crossed = 0;
  // the crossed minibatch (valid until the next apply)
  uint64_t *o_keys = nullptr;
  int32_t *o_fgid = nullptr;
  float *o_vals = nullptr;
  uint32_t *o_rowptr = nullptr;
  size_t cap_keys = 0, cap_fgid = 0, cap_vals = 0, cap_rowptr = 0;
  // scratch of the passes
  uint32_t *row_cnt = nullptr;
  uint64_t *tile_cnt = nullptr, *tile_off = nullptr;
  size_t cap_rcnt = 0, cap_tcnt = 0, cap_toff = 0;
  char *scan_tmp = nullptr;
  size_t cap_scan = 0;
  uint64_t *g_mask = nullptr;  // the member lists of rows too long for LDS
  uint32_t *g_pre = nullptr;
  size_t cap_gmask = 0, cap_gpre = 0;
  unsigned long long *d_stat = nullptr;  // input nonzeros, longest row, bad rows of the running apply
  uint64_t *h_back = nullptr;            // pinned: the total and the three stats
  // xf_cross_apply's copies of the host arrays
  uint64_t *u_keys = nullptr;
  int32_t *u_fgid = nullptr, *u_labels = nullptr;
  float *u_vals = nullptr;
  uint32_t *u_rowptr = nullptr;
  size_t ucap_keys = 0, ucap_fgid = 0, ucap_labels = 0, ucap_vals = 0, ucap_rowptr = 0;
  std::vector<uint32_t> h_rowptr;
};

extern "C" int xf_cross_destroy(xf_cross *x) {
  if (!x) return XF_OK;
  if ((x->d_stat || x->o_rowptr || x->u_rowptr) && !xf::device_poisoned()) {  // (an apply has run)
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)x->o_keys, (void *)x->o_fgid, (void *)x->o_vals, (void *)x->o_rowptr,
                    (void *)x->row_cnt, (void *)x->tile_cnt, (void *)x->tile_off,
                    (void *)x->scan_tmp, (void *)x->g_mask, (void *)x->g_pre, (void *)x->d_stat,
                    (void *)x->u_keys, (void *)x->u_fgid, (void *)x->u_labels, (void *)x->u_vals,
                    (void *)x->u_rowptr})
      if (p) (void)hipFree(p);
    if (x->h_back) (void)hipHostFree(x->h_back);
  }
  delete x;
  return XF_OK;
}

extern "C" int xf_cross_create(xf_cross **out, const int32_t *fa, const int32_t *fb, int npairs,
                               int32_t fgid_base) {
  XF_REQUIRE(out, "xf_cross_create: null argument");
  *out = nullptr;
  XF_TRY(xf::cross_check_spec("xf_cross_create", fa, fb, npairs));
  XF_TRY(xf::cross_check_base("xf_cross_create", fgid_base, npairs));
  xf_cross *x = new xf_cross;
  x->spec.P = npairs;
  x->spec.fgid_base = fgid_base;
  for (int p = 0; p < xf::kCrossMaxPairs; ++p) {
    x->spec.fa[p] = p < npairs ? fa[p] : 0;
    x->spec.fb[p] = p < npairs ? fb[p] : 0;
    x->spec.salt[p] = p < npairs ? xf::cross_salt(fa[p], fb[p]) : 0;
  }
  // (nothing on the device yet: the first apply allocates)
  *out = x;
  return XF_OK;
}

extern "C" int xf_cross_params(const xf_cross *x, int32_t *fa, int32_t *fb, int cap, int *npairs,
                               int32_t *fgid_base) {
  XF_REQUIRE(x, "xf_cross_params: null argument");
  XF_REQUIRE(!(fa || fb) || cap >= x->spec.P, "xf_cross_params: %d pairs do not fit arrays of %d",
             x->spec.P, cap);
  for (int p = 0; p < x->spec.P; ++p) {
    if (fa) fa[p] = x->spec.fa[p];
    if (fb) fb[p] = x->spec.fb[p];
  }
  if (npairs) *npairs = x->spec.P;
  if (fgid_base) *fgid_base = x->spec.fgid_base;
  return XF_OK;
}

extern "C" int xf_cross_stats(const xf_cross *x, uint64_t *rows_seen, uint64_t *nonzeros_in,
                              uint64_t *nonzeros_crossed) {
  XF_REQUIRE(x, "xf_cross_stats: null argument");
  if (rows_seen) *rows_seen = x->rows_seen;
  if (nonzeros_in) *nonzeros_in = x->nonzeros_in;
  if (nonzeros_crossed) *nonzeros_crossed = x->nonzeros_crossed;
  return XF_OK;
}

extern "C" int xf_cross_apply_dev(xf_cross *x, const uint64_t *d_keys, const int32_t *d_fgid,
                                  const float *d_vals, const uint32_t *d_rowptr, uint32_t R,
                                  uint32_t NNZ, void *stream, int want_fgid_out,
                                  const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                                  const float **d_vals_out, const uint32_t **d_rowptr_out,
                                  uint32_t *NNZ_out) {
  XF_REQUIRE(x && d_keys_out && d_rowptr_out && NNZ_out, "xf_cross_apply_dev: null argument");
  XF_REQUIRE(d_fgid, "xf_cross_apply_dev: the stage needs the nonzeros' field ids (d_fgid is NULL)");
  XF_REQUIRE(!want_fgid_out || d_fgid_out, "xf_cross_apply_dev: want_fgid_out without d_fgid_out");
  XF_REQUIRE(NNZ == 0 || (d_keys && R > 0),
             "xf_cross_apply_dev: %u nonzeros need keys and rows (R = %u)", NNZ, R);
  XF_REQUIRE(R == 0 || d_rowptr, "xf_cross_apply_dev: %u rows without row offsets", R);
  XF_REQUIRE(NNZ < 0xFFFFE000u && R < 0xFFFFFF00u,
             "xf_cross_apply_dev: a minibatch of %u rows, %u nonzeros is too large", R, NNZ);
  hipStream_t st = (hipStream_t)stream;
  *NNZ_out = 0;
  if (R == 0) {  // no row: the one zero offset (asynchronous, nothing to read back)
    XF_TRY(grow(&x->o_keys, &x->cap_keys, 0));
    if (want_fgid_out) XF_TRY(grow(&x->o_fgid, &x->cap_fgid, 0));
    if (d_vals) XF_TRY(grow(&x->o_vals, &x->cap_vals, 0));
    XF_TRY(grow(&x->o_rowptr, &x->cap_rowptr, 1));
    XF_HIP(hipMemsetAsync(x->o_rowptr, 0, 4, st));
    *d_keys_out = x->o_keys;
    if (d_fgid_out) *d_fgid_out = want_fgid_out ? x->o_fgid : nullptr;
    if (d_vals_out) *d_vals_out = d_vals ? x->o_vals : nullptr;
    *d_rowptr_out = x->o_rowptr;
    return XF_OK;
  }
  const uint32_t ntiles = (R + kCxTile - 1) / kCxTile;
  if (!x->d_stat) XF_HIP(hipMalloc((void **)&x->d_stat, 3 * sizeof(unsigned long long)));
  if (!x->h_back) XF_HIP(hipHostMalloc((void **)&x->h_back, 4 * sizeof(uint64_t)));
  XF_TRY(grow(&x->row_cnt, &x->cap_rcnt, R));
  XF_TRY(grow(&x->tile_cnt, &x->cap_tcnt, (size_t)ntiles + 1));
  XF_TRY(grow(&x->tile_off, &x->cap_toff, (size_t)ntiles + 1));
  size_t tb = 0;
  XF_HIP(rocprim::exclusive_scan((void *)nullptr, tb, x->tile_cnt, x->tile_off, (uint64_t)0,
                                 (size_t)ntiles + 1, SatPlus(), st));
  XF_TRY(grow(&x->scan_tmp, &x->cap_scan, tb));
  XF_HIP(hipMemsetAsync(x->d_stat, 0, 3 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_cx_count, dim3(ntiles), dim3(kCxThreads), 0, st, d_fgid, d_rowptr, R, NNZ,
                     x->spec, x->row_cnt, x->tile_cnt, ntiles, x->d_stat);
  XF_HIP(hipGetLastError());
  XF_HIP(rocprim::exclusive_scan((void *)x->scan_tmp, tb, x->tile_cnt, x->tile_off, (uint64_t)0,
                                 (size_t)ntiles + 1, SatPlus(), st));
  XF_HIP(hipMemcpyAsync(x->h_back, x->tile_off + ntiles, 8, hipMemcpyDeviceToHost, st));
  XF_HIP(hipMemcpyAsync(x->h_back + 1, x->d_stat, 24, hipMemcpyDeviceToHost, st));
  XF_HIP(hipStreamSynchronize(st));  // the one wait: the total (and the three stats)
  const uint64_t total = x->h_back[0], in_total = x->h_back[1];
  const uint32_t longest = (uint32_t)x->h_back[2];
  XF_REQUIRE(in_total <= NNZ,
             "xf_cross_apply_dev: the rows hold %llu nonzeros of %u: the row offsets overlap",
             (unsigned long long)in_total, NNZ);
  XF_REQUIRE(total < 0xFFFFFFFFull,
             "xf_cross_apply_dev: the crossed minibatch would hold %llu nonzeros (%llu of them "
             "crossed); a minibatch holds fewer than 4294967295",
             (unsigned long long)total, (unsigned long long)(total - in_total));
  // the emit: this is where the output grows
  const uint32_t short_max = xf::cross_short_max(), lds_chunks = xf::cross_lds_chunks();
  const bool any_long = longest > short_max;
  XF_TRY(grow(&x->o_keys, &x->cap_keys, (size_t)total));
  if (want_fgid_out) XF_TRY(grow(&x->o_fgid, &x->cap_fgid, (size_t)total));
  if (d_vals) XF_TRY(grow(&x->o_vals, &x->cap_vals, (size_t)total));
  XF_TRY(grow(&x->o_rowptr, &x->cap_rowptr, (size_t)R + 1));
  uint64_t g_cap = 0;
  if (any_long && (longest - 1) / 64 + 1 > std::min(lds_chunks, kCxMaxChunks)) {
    XF_REQUIRE(x->h_back[3] == 0,
               "xf_cross_apply_dev: a row of %u nonzeros (its member lists go to the global "
               "scratch) in a minibatch with %llu rows whose offsets descend or leave the arrays",
               longest, (unsigned long long)x->h_back[3]);
    g_cap = (uint64_t)NNZ / 64 + R + 2;
    XF_TRY(grow(&x->g_mask, &x->cap_gmask, (size_t)(2 * g_cap)));
    XF_TRY(grow(&x->g_pre, &x->cap_gpre, (size_t)(2 * g_cap)));
  }
  hipLaunchKernelGGL(k_cx_emit, dim3(ntiles), dim3(kCxThreads), 0, st, d_keys, d_fgid, d_vals,
                     d_rowptr, R, NNZ, x->spec, (const uint32_t *)x->row_cnt,
                     (const uint64_t *)x->tile_off, ntiles, short_max, x->o_keys,
                     want_fgid_out ? x->o_fgid : nullptr, d_vals ? x->o_vals : nullptr,
                     x->o_rowptr);
  if (any_long)
    hipLaunchKernelGGL(k_cx_emit_long, dim3(ntiles), dim3(kCxThreads), 0, st, d_keys, d_fgid,
                       d_vals, d_rowptr, R, NNZ, x->spec, (const uint64_t *)x->tile_off, ntiles,
                       (const uint32_t *)x->o_rowptr, short_max, lds_chunks,
                       g_cap ? x->g_mask : nullptr, g_cap ? x->g_pre : nullptr, g_cap, x->o_keys,
                       want_fgid_out ? x->o_fgid : nullptr, d_vals ? x->o_vals : nullptr);
  XF_HIP(hipGetLastError());
  *d_keys_out = x->o_keys;
  if (d_fgid_out) *d_fgid_out = want_fgid_out ? x->o_fgid : nullptr;
  if (d_vals_out) *d_vals_out = d_vals ? x->o_vals : nullptr;
  *d_rowptr_out = x->o_rowptr;
  *NNZ_out = (uint32_t)total;
  x->rows_seen += R;
  x->nonzeros_in += in_total;
  x->nonzeros_crossed += total - in_total;
  return XF_OK;
}

// xf_cross_apply's upload of a row slice of the reader's host arrays (rowptr rebased to u32), as
// negative subsampling's upload_slice
static int upload_slice(xf_cross *x, const uint64_t *rowptr, const uint64_t *keys,
                        const int32_t *fgid, const float *vals, const int32_t *labels,
                        size_t row_begin, size_t row_end, hipStream_t st, uint32_t *R_up,
                        uint32_t *NNZ_up) {
  XF_REQUIRE(x && rowptr && row_begin <= row_end, "xf_cross_apply: bad argument");
  XF_REQUIRE(fgid, "xf_cross_apply: the stage needs the nonzeros' field ids (fgid is NULL)");
  const size_t R = row_end - row_begin;
  const uint64_t base = rowptr[row_begin];
  XF_REQUIRE(rowptr[row_end] >= base, "xf_cross_apply: row offsets descend");
  const uint64_t nnz = rowptr[row_end] - base;
  XF_REQUIRE(R < 0xFFFFFF00ull && nnz < 0xFFFFE000ull,
             "xf_cross_apply: a minibatch of %zu rows, %llu nonzeros is too large", R,
             (unsigned long long)nnz);
  XF_REQUIRE(nnz == 0 || keys, "xf_cross_apply: %llu nonzeros without keys",
             (unsigned long long)nnz);
  x->h_rowptr.resize(R + 1);
  for (size_t r = 0; r <= R; ++r) {
    const uint64_t at = rowptr[row_begin + r];
    XF_REQUIRE(at >= base && at - base <= nnz && (r == 0 || at - base >= x->h_rowptr[r - 1]),
               "xf_cross_apply: row offsets descend at row %zu", row_begin + r);
    x->h_rowptr[r] = (uint32_t)(at - base);
  }
  XF_TRY(grow(&x->u_rowptr, &x->ucap_rowptr, R + 1));
  XF_HIP(hipMemcpyAsync(x->u_rowptr, x->h_rowptr.data(), (R + 1) * 4, hipMemcpyHostToDevice, st));
  XF_TRY(grow(&x->u_keys, &x->ucap_keys, (size_t)nnz));
  XF_TRY(grow(&x->u_fgid, &x->ucap_fgid, (size_t)nnz));
  if (vals) XF_TRY(grow(&x->u_vals, &x->ucap_vals, (size_t)nnz));
  if (nnz) {
    XF_HIP(hipMemcpyAsync(x->u_keys, keys + base, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    XF_HIP(hipMemcpyAsync(x->u_fgid, fgid + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    if (vals)
      XF_HIP(hipMemcpyAsync(x->u_vals, vals + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  XF_TRY(grow(&x->u_labels, &x->ucap_labels, R));
  if (R && labels)
    XF_HIP(hipMemcpyAsync(x->u_labels, labels + row_begin, R * 4, hipMemcpyHostToDevice, st));
  *R_up = (uint32_t)R;
  *NNZ_up = (uint32_t)nnz;
  return XF_OK;
}

extern "C" int xf_cross_apply(xf_cross *x, const uint64_t *rowptr, const uint64_t *keys,
                              const int32_t *fgid, const float *vals, const int32_t *labels,
                              size_t row_begin, size_t row_end, void *stream, int want_fgid_out,
                              const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                              const float **d_vals_out, const uint32_t **d_rowptr_out,
                              const int32_t **d_labels_out, uint32_t *R_out, uint32_t *NNZ_out) {
  XF_REQUIRE(R_out, "xf_cross_apply: null argument");
  uint32_t R = 0, nnz = 0;
  XF_TRY(upload_slice(x, rowptr, keys, fgid, vals, labels, row_begin, row_end,
                      (hipStream_t)stream, &R, &nnz));
  // (the host arrays may be pageable: the copies above have read them when they return; the
  // vector of rebased offsets lives until the next call.  R = 0: nothing waits, so wait here)
  if (R == 0) XF_HIP(hipStreamSynchronize((hipStream_t)stream));
  *R_out = R;
  if (d_labels_out) *d_labels_out = labels ? x->u_labels : nullptr;
  return xf_cross_apply_dev(x, x->u_keys, x->u_fgid, vals ? x->u_vals : nullptr, x->u_rowptr, R,
                            nnz, stream, want_fgid_out, d_keys_out, d_fgid_out, d_vals_out,
                            d_rowptr_out, NNZ_out);
}
