// xf_holdout.hip — held-out validation: a hashed row split of a minibatch.
//
// A multi-epoch run needs a loss on rows the model never trains on, in every epoch the SAME rows.
// The split takes a fixed, hash-chosen share of a minibatch's rows out: the decision is a hash of
// (seed, stream, the row's ordinal) — xf_holdout.h, one definition for the host and the kernels —
// and nothing else.  It has the shape of the negative sampler (xf_negsample.hip), but it is a
// stable two-way partition: the rows go, in order, into a TRAIN and a HELD minibatch, each with
// its own row-relative rowptr, its labels, keys and fgid / vals.
//
// Both parts live in ONE set of output arrays — the train part at the front, the held part behind
// it at the next multiple of kHoAlign elements — so every nonzero is written once and the arrays
// are as large as the input, whatever the share.
//
// Kernels:
//   k_ho_flag    a thread per row, kHoTile rows per workgroup: the decision and the row's length;
//                per tile the held rows and held nonzeros, packed into one 64-bit count (rows in
//                the high half), and beside it the tile's nonzeros of BOTH parts — rows whose
//                offsets descend or leave the arrays count as empty, so the train part's offsets
//                cannot be read off rowptr.  One rocPRIM exclusive scan over the pairs turns the
//                tile counts into the offsets of both parts (train = all - held).
//   k_ho_place   the same tiles: a scan inside the workgroup gives every row its index and its
//                offset in its part (stable); rowptr_out, labels_out and the row's SOURCE offset
//   k_ho_copy    a workgroup per kHoChunk OUTPUT nonzeros of ONE part, lanes on consecutive ones:
//                the row of an output position is a binary search in that part's rowptr_out over
//                the rows the chunk touches (found once per workgroup).  The grid covers the INPUT
//                nonzeros plus one chunk (an upper bound of both parts' chunks that needs no host
//                wait); chunks beyond the parts return at once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <math.h>

#include <vector>

#include "xf_common.h"
#include "xf_holdout.h"
#include "xflow_amd.h"

namespace {

constexpr int kHoThreads = 256;
constexpr uint32_t kHoTile = 256;    // rows of one workgroup of the flag and the place pass
static_assert(kHoTile == kHoThreads, "a row per thread");
constexpr uint32_t kHoChunk = 2048;  // output nonzeros of one workgroup of the copy
constexpr int kHoPerThread = kHoChunk / kHoThreads;
constexpr uint32_t kHoAlign = 64;    // the held part starts at a multiple of this many elements

// a tile's counts, and their exclusive sums: held = held rows << 32 | held nonzeros; all = the
// nonzeros of both parts (64-bit: rows that overlap can sum past 2^32, which is refused)
struct __attribute__((aligned(16))) HoCnt {
  uint64_t held, all;
};
struct HoPlus {
  __host__ __device__ HoCnt operator()(const HoCnt &a, const HoCnt &b) const {
    return HoCnt{a.held + b.held, a.all + b.all};
  }
};

__host__ __device__ inline uint32_t ho_align(uint32_t n) {
  return (n + kHoAlign - 1) / kHoAlign * kHoAlign;
}

// the totals of a split, from the scan's last word; ok: the counts stay inside the arrays (a
// caller's rows that overlap do not: nothing is placed or copied, and the host refuses the call)
struct HoTotal {
  uint32_t R_train, R_held, N_train, N_held;
  bool ok;
};
__host__ __device__ inline HoTotal ho_total(HoCnt total, uint32_t R, uint32_t NNZ) {
  HoTotal o;
  const uint64_t rows = total.held >> 32, nz = total.held & 0xFFFFFFFFull;
  o.ok = total.all <= NNZ && nz <= total.all && rows <= R;
  o.R_held = (uint32_t)rows;
  o.N_held = (uint32_t)nz;
  o.R_train = o.ok ? R - o.R_held : 0u;
  o.N_train = o.ok ? (uint32_t)total.all - o.N_held : 0u;
  return o;
}

// the row's decision and length; a row whose offsets descend or leave the arrays has length 0
__device__ inline bool ho_row(const uint32_t *__restrict__ rowptr, uint32_t r, uint32_t NNZ,
                              uint64_t base, uint64_t first_ordinal, uint64_t T, uint32_t *len) {
  const uint32_t a = rowptr[r], b = rowptr[r + 1];
  *len = (b >= a && b <= NNZ) ? b - a : 0u;
  return xf::holdout_held_row(base, first_ordinal + (uint64_t)r, T);
}

// tile_cnt[tile] = {held rows << 32 | held nonzeros, nonzeros}; tile_cnt[ntiles] = 0 (its
// exclusive sum: the totals)
__global__ __launch_bounds__(kHoThreads) void k_ho_flag(
    const uint32_t *__restrict__ rowptr, uint32_t R, uint32_t NNZ, uint64_t base,
    uint64_t first_ordinal, uint64_t T, HoCnt *__restrict__ tile_cnt, uint32_t ntiles) {
  __shared__ uint32_t wave_rows[kHoThreads / 64];
  __shared__ uint64_t wide[2][kHoThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x, r = tile * kHoTile + t;
  uint32_t rows = 0, nz = 0, all = 0;
  if (r < R) {
    uint32_t len;
    const bool held = ho_row(rowptr, r, NNZ, base, first_ordinal, T, &len);
    rows = held ? 1u : 0u;
    nz = held ? len : 0u;
    all = len;
  }
  // (a tile's 256 lengths can sum past 2^32 when the caller's rows overlap: the nonzeros are
  // summed in 64 bits from the waves' sums on)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) rows += __shfl_xor(rows, off, 64);
  uint64_t nz64 = nz, all64 = all;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nz64 += __shfl_xor(nz64, off, 64);
    all64 += __shfl_xor(all64, off, 64);
  }
  if ((t & 63) == 0) {
    wave_rows[t >> 6] = rows;
    wide[0][t >> 6] = nz64;
    wide[1][t >> 6] = all64;
  }
  __syncthreads();
  if (t == 0) {
    uint64_t h_rows = 0, h_nz = 0, a_nz = 0;
    for (int w = 0; w < kHoThreads / 64; ++w) {
      h_rows += wave_rows[w];
      h_nz += wide[0][w];
      a_nz += wide[1][w];
    }
    // (h_nz <= a_nz; past 2^32 it carries into the row half, and a_nz > NNZ refuses the call)
    tile_cnt[tile] = HoCnt{(h_rows << 32) + h_nz, a_nz};
    if (tile == 0) tile_cnt[ntiles] = HoCnt{0, 0};
  }
}

// row -> (part, index j in the part, offset in the part): rowptr_out, labels_out, src_off; the
// last tile closes both rowptr_out.  Indices: j < the part's rows <= R, offsets <= the part's
// nonzeros <= NNZ — from counts that ho_total found inside the arrays.
__global__ __launch_bounds__(kHoThreads) void k_ho_place(
    const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ labels, uint32_t R,
    uint32_t NNZ, uint64_t base, uint64_t first_ordinal, uint64_t T,
    const HoCnt *__restrict__ tile_off, uint32_t ntiles, uint32_t *__restrict__ rowptr_out,
    int32_t *__restrict__ labels_out, uint32_t *__restrict__ src_off) {
  __shared__ uint32_t wave_rows[kHoThreads / 64], wave_nz[kHoThreads / 64],
      wave_all[kHoThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t r = tile * kHoTile + t;
  const HoTotal tot = ho_total(tile_off[ntiles], R, NNZ);  // (uniform: the same word for all)
  if (!tot.ok) return;
  bool held = false;
  uint32_t len = 0;
  if (r < R) held = ho_row(rowptr, r, NNZ, base, first_ordinal, T, &len);
  const uint32_t c_rows = held ? 1u : 0u, c_nz = held ? len : 0u, c_all = len;
  uint32_t i_rows = c_rows, i_nz = c_nz, i_all = c_all;  // inclusive scans of the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ur = __shfl_up(i_rows, off, 64), un = __shfl_up(i_nz, off, 64),
                   ua = __shfl_up(i_all, off, 64);
    if (lane >= (uint32_t)off) {
      i_rows += ur;
      i_nz += un;
      i_all += ua;
    }
  }
  if (lane == 63) {
    wave_rows[wave] = i_rows;
    wave_nz[wave] = i_nz;
    wave_all[wave] = i_all;
  }
  __syncthreads();
  const HoCnt off0 = tile_off[tile];  // (tot.ok: every sum below stays under 2^32)
  uint32_t h_rows = (uint32_t)(off0.held >> 32) + i_rows - c_rows;  // held rows before this one
  uint32_t h_nz = (uint32_t)off0.held + i_nz - c_nz;                // their nonzeros
  uint32_t a_nz = (uint32_t)off0.all + i_all - c_all;               // nonzeros of all rows before
  for (uint32_t w = 0; w < wave; ++w) {
    h_rows += wave_rows[w];
    h_nz += wave_nz[w];
    a_nz += wave_all[w];
  }
  const uint32_t row0 = ho_align(tot.R_train), ptr0 = ho_align(tot.R_train + 1);
  if (r < R) {
    if (held) {
      rowptr_out[ptr0 + h_rows] = h_nz;
      labels_out[row0 + h_rows] = labels[r];
      src_off[row0 + h_rows] = rowptr[r];
    } else {
      const uint32_t j = r - h_rows;
      rowptr_out[j] = a_nz - h_nz;
      labels_out[j] = labels[r];
      src_off[j] = rowptr[r];
    }
  }
  if (tile == ntiles - 1 && t == 0) {
    rowptr_out[tot.R_train] = tot.N_train;
    rowptr_out[ptr0 + tot.R_held] = tot.N_held;
  }
}

// the last row j in [lo, hi] with rowptr_out[j] <= i (rowptr_out[lo] <= i holds on entry)
__device__ inline uint32_t ho_row_of(const uint32_t *__restrict__ rowptr_out, uint32_t lo,
                                     uint32_t hi, uint32_t i) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (rowptr_out[mid] <= i) lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kHoThreads) void k_ho_copy(
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ fgid,
    const float *__restrict__ vals, uint32_t R, uint32_t NNZ,
    const HoCnt *__restrict__ tile_off, uint32_t ntiles, const uint32_t *__restrict__ rowptr_out,
    const uint32_t *__restrict__ src_off, uint64_t *__restrict__ keys_out,
    int32_t *__restrict__ fgid_out, float *__restrict__ vals_out) {
  __shared__ uint32_t range[2];
  const HoTotal tot = ho_total(tile_off[ntiles], R, NNZ);
  if (!tot.ok) return;  // (uniform)
  // the train part's chunks first, then the held part's
  const uint32_t train_chunks = (tot.N_train + kHoChunk - 1) / kHoChunk;
  const bool held = blockIdx.x >= train_chunks;
  const uint32_t chunk = held ? blockIdx.x - train_chunks : blockIdx.x;
  const uint32_t n = held ? tot.N_held : tot.N_train, rows = held ? tot.R_held : tot.R_train;
  const uint32_t c0 = chunk * kHoChunk, t = threadIdx.x;  // (chunk <= NNZ / kHoChunk + 1)
  if (c0 >= n) return;                                    // (uniform)
  const uint32_t c1 = min(c0 + kHoChunk, n);
  const uint32_t *__restrict__ rp = rowptr_out + (held ? ho_align(tot.R_train + 1) : 0u);
  const uint32_t *__restrict__ so = src_off + (held ? ho_align(tot.R_train) : 0u);
  const uint32_t out0 = held ? ho_align(tot.N_train) : 0u;
  // (rows >= 1 here: the part has nonzeros; rp[0] = 0 <= every position)
  if (t < 2) range[t] = ho_row_of(rp, 0, rows - 1, t == 0 ? c0 : c1 - 1);
  __syncthreads();
  const uint32_t lo = range[0], hi = range[1];
#pragma unroll
  for (int q = 0; q < kHoPerThread; ++q) {
    const uint32_t i = c0 + q * kHoThreads + t;
    if (i < c1) {
      const uint32_t j = ho_row_of(rp, lo, hi, i);
      const uint32_t src = so[j] + (i - rp[j]);
      if (src < NNZ) {  // (always, for row offsets that ascend)
        keys_out[out0 + i] = keys[src];
        if (fgid) fgid_out[out0 + i] = fgid[src];
        if (vals) vals_out[out0 + i] = vals[src];
      }
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

int check_share(const char *who, float share) {
  XF_REQUIRE(isfinite(share) && share >= 0.0f && share < 1.0f,
             "%s: holdout must be in [0, 1), not %g", who, (double)share);
  return XF_OK;
}

}  // namespace

struct xf_holdout {
  float share = 0.0f;
  uint64_t seed = 0, T = 0;
  uint64_t rows_seen = 0, rows_held = 0, nnz_held = 0;
  // both parts of the split minibatch (valid until the next split)
  uint64_t *o_keys = nullptr;
  int32_t *o_fgid = nullptr, *o_labels = nullptr;
  float *o_vals = nullptr;
  uint32_t *o_rowptr = nullptr;
  size_t cap_keys = 0, cap_fgid = 0, cap_labels = 0, cap_vals = 0, cap_rowptr = 0;
  // scratch of the passes
  uint32_t *src_off = nullptr;
  HoCnt *tile_cnt = nullptr, *tile_off = nullptr;
  size_t cap_src = 0, cap_tcnt = 0, cap_toff = 0;
  char *scan_tmp = nullptr;
  size_t cap_scan = 0;
  HoCnt *h_back = nullptr;  // pinned: the totals
  // xf_holdout_split's copies of the host arrays
  uint64_t *u_keys = nullptr;
  int32_t *u_fgid = nullptr, *u_labels = nullptr;
  float *u_vals = nullptr;
  uint32_t *u_rowptr = nullptr;
  size_t ucap_keys = 0, ucap_fgid = 0, ucap_labels = 0, ucap_vals = 0, ucap_rowptr = 0;
  std::vector<uint32_t> h_rowptr;
};

extern "C" int xf_holdout_destroy(xf_holdout *s) {
  if (!s) return XF_OK;
  if (s->h_back && !xf::device_poisoned()) {  // (h_back: a split has run)
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)s->o_keys, (void *)s->o_fgid, (void *)s->o_labels, (void *)s->o_vals,
                    (void *)s->o_rowptr, (void *)s->src_off, (void *)s->tile_cnt,
                    (void *)s->tile_off, (void *)s->scan_tmp, (void *)s->u_keys,
                    (void *)s->u_fgid, (void *)s->u_labels, (void *)s->u_vals,
                    (void *)s->u_rowptr})
      if (p) (void)hipFree(p);
    (void)hipHostFree(s->h_back);
  }
  delete s;
  return XF_OK;
}

extern "C" int xf_holdout_create(xf_holdout **out, float share, uint64_t seed) {
  XF_REQUIRE(out, "xf_holdout_create: null argument");
  *out = nullptr;
  XF_TRY(check_share("xf_holdout_create", share));
  xf_holdout *s = new xf_holdout;
  s->share = share;
  s->seed = seed;
  s->T = xf::holdout_threshold((double)share);
  // (nothing on the device yet: the first split allocates)
  *out = s;
  return XF_OK;
}

extern "C" int xf_holdout_params(const xf_holdout *s, float *share, uint64_t *seed) {
  XF_REQUIRE(s, "xf_holdout_params: null argument");
  if (share) *share = s->share;
  if (seed) *seed = s->seed;
  return XF_OK;
}

extern "C" int xf_holdout_stats(const xf_holdout *s, uint64_t *rows_seen, uint64_t *rows_held,
                                uint64_t *nnz_held) {
  XF_REQUIRE(s, "xf_holdout_stats: null argument");
  if (rows_seen) *rows_seen = s->rows_seen;
  if (rows_held) *rows_held = s->rows_held;
  if (nnz_held) *nnz_held = s->nnz_held;
  return XF_OK;
}

extern "C" void xf_holdout_shape(uint32_t out[3]) {
  out[0] = kHoTile;
  out[1] = kHoChunk;
  out[2] = kHoAlign;
}

static void set_part(xf_holdout_part *p, const xf_holdout *s, bool fgid, bool vals, uint32_t nz0,
                     uint32_t row0, uint32_t ptr0, uint32_t R, uint32_t NNZ) {
  p->d_keys = s->o_keys + nz0;
  p->d_fgid = fgid ? s->o_fgid + nz0 : nullptr;
  p->d_vals = vals ? s->o_vals + nz0 : nullptr;
  p->d_rowptr = s->o_rowptr + ptr0;
  p->d_labels = s->o_labels + row0;
  p->R = R;
  p->NNZ = NNZ;
}

extern "C" int xf_holdout_split_dev(xf_holdout *s, uint64_t stream_id, uint64_t first_ordinal,
                                    const uint64_t *d_keys, const int32_t *d_fgid,
                                    const float *d_vals, const uint32_t *d_rowptr,
                                    const int32_t *d_labels, uint32_t R, uint32_t NNZ,
                                    void *stream, xf_holdout_part *train, xf_holdout_part *held) {
  XF_REQUIRE(s && train && held, "xf_holdout_split_dev: null argument");
  XF_REQUIRE(NNZ == 0 || (d_keys && R > 0),
             "xf_holdout_split_dev: %u nonzeros need keys and rows (R = %u)", NNZ, R);
  XF_REQUIRE(R == 0 || (d_rowptr && d_labels),
             "xf_holdout_split_dev: %u rows without row offsets or labels", R);
  XF_REQUIRE(NNZ < 0xFFFFFFFFu - 4 * kHoChunk && R < 0xFFFFFFFFu - 4 * kHoTile,
             "xf_holdout_split_dev: a minibatch of %u rows, %u nonzeros is too large", R, NNZ);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t ntiles = (R + kHoTile - 1) / kHoTile;
  if (!s->h_back) XF_HIP(hipHostMalloc((void **)&s->h_back, sizeof(HoCnt)));
  // (the held part starts at a multiple of kHoAlign behind the train part: one gap per array)
  XF_TRY(grow(&s->o_keys, &s->cap_keys, (size_t)NNZ + kHoAlign));
  if (d_fgid) XF_TRY(grow(&s->o_fgid, &s->cap_fgid, (size_t)NNZ + kHoAlign));
  if (d_vals) XF_TRY(grow(&s->o_vals, &s->cap_vals, (size_t)NNZ + kHoAlign));
  XF_TRY(grow(&s->o_rowptr, &s->cap_rowptr, (size_t)R + 2 + kHoAlign));
  XF_TRY(grow(&s->o_labels, &s->cap_labels, (size_t)R + kHoAlign));
  if (R == 0) {  // no row to decide on: two zero offsets (asynchronous, nothing to read back)
    XF_HIP(hipMemsetAsync(s->o_rowptr, 0, (size_t)(ho_align(1) + 1) * 4, st));
    set_part(train, s, d_fgid, d_vals, 0, 0, 0, 0, 0);
    set_part(held, s, d_fgid, d_vals, ho_align(0), ho_align(0), ho_align(1), 0, 0);
    return XF_OK;
  }
  XF_TRY(grow(&s->src_off, &s->cap_src, (size_t)R + kHoAlign));
  XF_TRY(grow(&s->tile_cnt, &s->cap_tcnt, (size_t)ntiles + 1));
  XF_TRY(grow(&s->tile_off, &s->cap_toff, (size_t)ntiles + 1));
  size_t tb = 0;
  XF_HIP(rocprim::exclusive_scan((void *)nullptr, tb, s->tile_cnt, s->tile_off, HoCnt{0, 0},
                                 (size_t)ntiles + 1, HoPlus(), st));
  XF_TRY(grow(&s->scan_tmp, &s->cap_scan, tb));
  const uint64_t base = xf::holdout_base(s->seed, stream_id);
  hipLaunchKernelGGL(k_ho_flag, dim3(ntiles), dim3(kHoThreads), 0, st, d_rowptr, R, NNZ, base,
                     first_ordinal, s->T, s->tile_cnt, ntiles);
  XF_HIP(hipGetLastError());
  XF_HIP(rocprim::exclusive_scan((void *)s->scan_tmp, tb, s->tile_cnt, s->tile_off, HoCnt{0, 0},
                                 (size_t)ntiles + 1, HoPlus(), st));
  hipLaunchKernelGGL(k_ho_place, dim3(ntiles), dim3(kHoThreads), 0, st, d_rowptr, d_labels, R, NNZ,
                     base, first_ordinal, s->T, (const HoCnt *)s->tile_off, ntiles, s->o_rowptr,
                     s->o_labels, s->src_off);
  if (NNZ)
    hipLaunchKernelGGL(k_ho_copy, dim3((NNZ + kHoChunk - 1) / kHoChunk + 1), dim3(kHoThreads), 0,
                       st, d_keys, d_fgid, d_vals, R, NNZ, (const HoCnt *)s->tile_off, ntiles,
                       (const uint32_t *)s->o_rowptr, (const uint32_t *)s->src_off, s->o_keys,
                       s->o_fgid, s->o_vals);
  XF_HIP(hipGetLastError());
  XF_HIP(hipMemcpyAsync(s->h_back, s->tile_off + ntiles, sizeof(HoCnt), hipMemcpyDeviceToHost, st));
  XF_HIP(hipStreamSynchronize(st));  // the one wait: the counts
  const HoTotal tot = ho_total(*s->h_back, R, NNZ);
  XF_REQUIRE(tot.ok,
             "xf_holdout_split_dev: the rows hold %llu nonzeros of %u: the row offsets overlap",
             (unsigned long long)s->h_back->all, NNZ);
  set_part(train, s, d_fgid, d_vals, 0, 0, 0, tot.R_train, tot.N_train);
  set_part(held, s, d_fgid, d_vals, ho_align(tot.N_train), ho_align(tot.R_train),
           ho_align(tot.R_train + 1), tot.R_held, tot.N_held);
  s->rows_seen += R;
  s->rows_held += tot.R_held;
  s->nnz_held += tot.N_held;
  return XF_OK;
}

// xf_holdout_split's upload of a row slice of the reader's host arrays (rowptr rebased to u32)
static int upload_slice(xf_holdout *s, const uint64_t *rowptr, const uint64_t *keys,
                        const int32_t *fgid, const float *vals, const int32_t *labels,
                        size_t row_begin, size_t row_end, hipStream_t st, uint32_t *R_up,
                        uint32_t *NNZ_up) {
  XF_REQUIRE(s && rowptr && row_begin <= row_end, "xf_holdout_split: bad argument");
  const size_t R = row_end - row_begin;
  XF_REQUIRE(R == 0 || labels, "xf_holdout_split: %zu rows without labels", R);
  const uint64_t base = rowptr[row_begin];
  XF_REQUIRE(rowptr[row_end] >= base, "xf_holdout_split: row offsets descend");
  const uint64_t nnz = rowptr[row_end] - base;
  XF_REQUIRE(R < 0xFFFFF000ull && nnz < 0xFFFFC000ull,
             "xf_holdout_split: a minibatch of %zu rows, %llu nonzeros is too large", R,
             (unsigned long long)nnz);
  XF_REQUIRE(nnz == 0 || keys, "xf_holdout_split: %llu nonzeros without keys",
             (unsigned long long)nnz);
  s->h_rowptr.resize(R + 1);
  for (size_t r = 0; r <= R; ++r) {
    const uint64_t at = rowptr[row_begin + r];
    XF_REQUIRE(at >= base && at - base <= nnz && (r == 0 || at - base >= s->h_rowptr[r - 1]),
               "xf_holdout_split: row offsets descend at row %zu", row_begin + r);
    s->h_rowptr[r] = (uint32_t)(at - base);
  }
  XF_TRY(grow(&s->u_rowptr, &s->ucap_rowptr, R + 1));
  XF_HIP(hipMemcpyAsync(s->u_rowptr, s->h_rowptr.data(), (R + 1) * 4, hipMemcpyHostToDevice, st));
  XF_TRY(grow(&s->u_keys, &s->ucap_keys, (size_t)nnz));
  if (fgid) XF_TRY(grow(&s->u_fgid, &s->ucap_fgid, (size_t)nnz));
  if (vals) XF_TRY(grow(&s->u_vals, &s->ucap_vals, (size_t)nnz));
  if (nnz) {
    XF_HIP(hipMemcpyAsync(s->u_keys, keys + base, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    if (fgid)
      XF_HIP(hipMemcpyAsync(s->u_fgid, fgid + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    if (vals)
      XF_HIP(hipMemcpyAsync(s->u_vals, vals + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  XF_TRY(grow(&s->u_labels, &s->ucap_labels, R));
  if (R) XF_HIP(hipMemcpyAsync(s->u_labels, labels + row_begin, R * 4, hipMemcpyHostToDevice, st));
  *R_up = (uint32_t)R;
  *NNZ_up = (uint32_t)nnz;
  return XF_OK;
}

extern "C" int xf_holdout_split(xf_holdout *s, uint64_t stream_id, uint64_t first_ordinal,
                                const uint64_t *rowptr, const uint64_t *keys, const int32_t *fgid,
                                const float *vals, const int32_t *labels, size_t row_begin,
                                size_t row_end, void *stream, xf_holdout_part *train,
                                xf_holdout_part *held) {
  uint32_t R = 0, nnz = 0;
  XF_TRY(upload_slice(s, rowptr, keys, fgid, vals, labels, row_begin, row_end,
                      (hipStream_t)stream, &R, &nnz));
  // (the host arrays may be pageable: the copies above have read them when they return; the
  // vector of rebased offsets lives until the next call.  R = 0: nothing waits, so wait here)
  if (R == 0) XF_HIP(hipStreamSynchronize((hipStream_t)stream));
  return xf_holdout_split_dev(s, stream_id, first_ordinal, s->u_keys, fgid ? s->u_fgid : nullptr,
                              vals ? s->u_vals : nullptr, s->u_rowptr, s->u_labels, R, nnz, stream,
                              train, held);
}
