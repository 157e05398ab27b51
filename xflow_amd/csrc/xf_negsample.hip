// xf_negsample.hip — negative subsampling with importance weights.
//
// On click data a few per cent of the rows are positives, and the first-epoch loop pays its key
// build and first-touch inserts for every negative.  The FTRL paper's "Subsampling Training Data":
// keep every positive, keep a negative with probability r, and multiply a kept negative's loss —
// hence its gradient — by w = 1/r: the expected gradient is unchanged.  Not in the reference.
//
// Like admission (xf_admit.hip) the sampler is a filter on a minibatch's CSR arrays ahead of any
// key build, but it drops whole ROWS and keeps no state: the decision is a hash of (seed, stream,
// the row's ordinal) — xf_negsample.h, one definition for the host and the kernels.
//
// Kernels:
//   k_ns_flag    a thread per row, kNsTile rows per workgroup: the decision and the row's length;
//                per tile the kept rows and kept nonzeros, packed into one 64-bit count (rows in the
//                high half — both stay below 2^32, so no carry), and the negatives seen / kept.
//                (rocPRIM's exclusive scan turns the tile counts into offsets.)
//   k_ns_place   the same tiles: a scan inside the workgroup gives every kept row its new index and
//                its new offset (stable); rowptr_out, labels_out and the row's SOURCE offset
//   k_ns_copy    a workgroup per kNsChunk OUTPUT nonzeros, lanes on consecutive ones: the row of an
//                output position is a binary search in rowptr_out over the rows the chunk touches
//                (found once per workgroup), the source position follows from the row's source
//                offset.  Writes are consecutive, reads consecutive inside a row: one row of 5000
//                nonzeros is three chunks of straight copies, 300 short rows are one chunk whose
//                lanes search a range of 300.  The grid covers the INPUT nonzeros (an upper bound
//                that needs no host wait); chunks beyond the kept total return at once.
//   k_weigh_negatives   the weight: loss[r] *= w on the rows with label 0, between a training
//                step's forward and its gradient (xf::weigh_negatives)
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <math.h>

#include <atomic>
#include <vector>

#include "xf_common.h"
#include "xf_negsample.h"
#include "xflow_amd.h"

namespace {

constexpr int kNsThreads = 256;
constexpr uint32_t kNsTile = 256;    // rows of one workgroup of the flag and the place pass
static_assert(kNsTile == kNsThreads, "a row per thread");
constexpr uint32_t kNsChunk = 2048;  // output nonzeros of one workgroup of the copy
constexpr int kNsPerThread = kNsChunk / kNsThreads;

// the row's decision and length; a row whose offsets descend or leave the arrays has length 0
__device__ inline bool ns_row(const uint32_t *__restrict__ rowptr,
                              const int32_t *__restrict__ labels, uint32_t r, uint32_t NNZ,
                              uint64_t base, uint64_t first_ordinal, uint64_t T, bool *negative,
                              uint32_t *len) {
  const uint32_t a = rowptr[r], b = rowptr[r + 1];
  *len = (b >= a && b <= NNZ) ? b - a : 0u;
  *negative = labels[r] == 0;
  return !*negative || xf::negsample_keep_row(base, first_ordinal + (uint64_t)r, T);
}

// sums over the workgroup of two 32-bit values; the result is valid in thread 0
__device__ inline void ns_block_sum2(uint32_t *a, uint32_t *b, uint32_t (*lds)[kNsThreads / 64]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    *a += __shfl_xor(*a, off, 64);
    *b += __shfl_xor(*b, off, 64);
  }
  const uint32_t t = threadIdx.x;
  if ((t & 63) == 0) {
    lds[0][t >> 6] = *a;
    lds[1][t >> 6] = *b;
  }
  __syncthreads();
  if (t == 0) {
    *a = *b = 0;
    for (int w = 0; w < kNsThreads / 64; ++w) {
      *a += lds[0][w];
      *b += lds[1][w];
    }
  }
  __syncthreads();
}

// tile_cnt[tile] = kept rows << 32 | kept nonzeros; tile_cnt[ntiles] = 0 (its exclusive sum: the
// totals); stat[0] += negatives seen, stat[1] += negatives kept (zero on entry)
__global__ __launch_bounds__(kNsThreads) void k_ns_flag(
    const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ labels, uint32_t R,
    uint32_t NNZ, uint64_t base, uint64_t first_ordinal, uint64_t T,
    uint64_t *__restrict__ tile_cnt, uint32_t ntiles, unsigned long long *stat) {
  __shared__ uint32_t lds[2][kNsThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x, r = tile * kNsTile + t;
  uint32_t rows = 0, nz = 0, nseen = 0, nkept = 0;
  if (r < R) {
    bool negative;
    uint32_t len;
    const bool keep = ns_row(rowptr, labels, r, NNZ, base, first_ordinal, T, &negative, &len);
    rows = keep ? 1u : 0u;
    nz = keep ? len : 0u;
    nseen = negative ? 1u : 0u;
    nkept = negative && keep ? 1u : 0u;
  }
  ns_block_sum2(&rows, &nz, lds);
  ns_block_sum2(&nseen, &nkept, lds);
  if (t == 0) {
    tile_cnt[tile] = (uint64_t)rows << 32 | nz;
    if (tile == 0) tile_cnt[ntiles] = 0;
    if (nseen) atomicAdd(&stat[0], (unsigned long long)nseen);
    if (nkept) atomicAdd(&stat[1], (unsigned long long)nkept);
  }
}

// kept row -> (new index j, new offset): rowptr_out[j], labels_out[j], src_off[j]; the last tile
// closes rowptr_out with the kept nonzeros.  A total that left the arrays (a caller's broken
// rowptr: rows that overlap) places nothing — the host refuses the call from the same total.
__global__ __launch_bounds__(kNsThreads) void k_ns_place(
    const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ labels, uint32_t R,
    uint32_t NNZ, uint64_t base, uint64_t first_ordinal, uint64_t T,
    const uint64_t *__restrict__ tile_off, uint32_t ntiles, uint32_t *__restrict__ rowptr_out,
    int32_t *__restrict__ labels_out, uint32_t *__restrict__ src_off) {
  __shared__ uint32_t wave_rows[kNsThreads / 64], wave_nz[kNsThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t r = tile * kNsTile + t;
  const uint64_t total = tile_off[ntiles];
  // (uniform: every thread reads the same word.  Overlapping rows can even carry into the row
  // half: both halves are checked, here, in the copy and on the host)
  if ((uint32_t)total > NNZ || (total >> 32) > R) return;
  bool keep = false, negative = false;
  uint32_t len = 0;
  if (r < R) keep = ns_row(rowptr, labels, r, NNZ, base, first_ordinal, T, &negative, &len);
  const uint32_t c_rows = keep ? 1u : 0u, c_nz = keep ? len : 0u;
  uint32_t i_rows = c_rows, i_nz = c_nz;  // inclusive scans of the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ur = __shfl_up(i_rows, off, 64), un = __shfl_up(i_nz, off, 64);
    if (lane >= (uint32_t)off) {
      i_rows += ur;
      i_nz += un;
    }
  }
  if (lane == 63) {
    wave_rows[wave] = i_rows;
    wave_nz[wave] = i_nz;
  }
  __syncthreads();
  const uint64_t off0 = tile_off[tile];
  uint32_t j = (uint32_t)(off0 >> 32) + i_rows - c_rows, at = (uint32_t)off0 + i_nz - c_nz;
  for (uint32_t w = 0; w < wave; ++w) {
    j += wave_rows[w];
    at += wave_nz[w];
  }
  if (keep) {  // (j < kept rows <= R, at <= kept nonzeros <= NNZ)
    rowptr_out[j] = at;
    labels_out[j] = labels[r];
    src_off[j] = rowptr[r];
  }
  if (tile == ntiles - 1 && t == 0) rowptr_out[(uint32_t)(total >> 32)] = (uint32_t)total;
}

// the last row j in [lo, hi] with rowptr_out[j] <= i (rowptr_out[lo] <= i holds on entry)
__device__ inline uint32_t ns_row_of(const uint32_t *__restrict__ rowptr_out, uint32_t lo,
                                     uint32_t hi, uint32_t i) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (rowptr_out[mid] <= i) lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kNsThreads) void k_ns_copy(
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ fgid,
    const float *__restrict__ vals, uint32_t R, uint32_t NNZ,
    const uint64_t *__restrict__ tile_off, uint32_t ntiles, const uint32_t *__restrict__ rowptr_out, const uint32_t *__restrict__ src_off,
    uint64_t *__restrict__ keys_out, int32_t *__restrict__ fgid_out,
    float *__restrict__ vals_out) {
  __shared__ uint32_t range[2];
  const uint64_t total = tile_off[ntiles];
  const uint32_t R_out = (uint32_t)(total >> 32), nnz_out = (uint32_t)total;
  const uint32_t c0 = blockIdx.x * kNsChunk, t = threadIdx.x;
  if (nnz_out > NNZ || R_out > R || c0 >= nnz_out) return;  // (uniform)
  const uint32_t c1 = min(c0 + kNsChunk, nnz_out);
  // (R_out >= 1 here: there are kept nonzeros; rowptr_out[0] = 0 <= every position)
  if (t < 2) range[t] = ns_row_of(rowptr_out, 0, R_out - 1, t == 0 ? c0 : c1 - 1);
  __syncthreads();
  const uint32_t lo = range[0], hi = range[1];
#pragma unroll
  for (int q = 0; q < kNsPerThread; ++q) {
    const uint32_t i = c0 + q * kNsThreads + t;
    if (i < c1) {
      const uint32_t j = ns_row_of(rowptr_out, lo, hi, i);
      const uint32_t src = src_off[j] + (i - rowptr_out[j]);
      if (src < NNZ) {  // (always, for row offsets that ascend)
        keys_out[i] = keys[src];
        if (fgid) fgid_out[i] = fgid[src];
        if (vals) vals_out[i] = vals[src];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_weigh_negatives(float *__restrict__ loss,
                                                          const int32_t *__restrict__ labels,
                                                          uint32_t R, float w) {
#pragma clang fp contract(off)
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  if (labels[r] == 0) loss[r] = w * loss[r];
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

int check_keep(const char *who, float keep) {
  XF_REQUIRE(isfinite(keep) && keep > 0.0f && keep <= 1.0f,
             "%s: neg_keep must be in (0, 1], not %g", who, (double)keep);
  return XF_OK;
}

}  // namespace

static std::atomic<uint64_t> g_weigh_launches{0};

int xf::weigh_negatives(float *loss, const int32_t *labels, uint32_t R, float w, hipStream_t s) {
  if (w == 1.0f || R == 0) return XF_OK;
  XF_REQUIRE(loss && labels, "weigh_negatives: null argument");
  hipLaunchKernelGGL(k_weigh_negatives, dim3((R + 255) / 256), dim3(256), 0, s, loss, labels, R, w);
  XF_HIP(hipGetLastError());
  g_weigh_launches.fetch_add(1, std::memory_order_relaxed);
  return XF_OK;
}

extern "C" uint64_t xf_weigh_negatives_launches(void) {
  return g_weigh_launches.load(std::memory_order_relaxed);
}

struct xf_negsample {
  float keep = 1.0f;
  uint64_t seed = 0, T = 0;
  uint64_t rows_seen = 0, rows_kept = 0, neg_seen = 0, neg_kept = 0;
  // the sampled minibatch (valid until the next apply)
  uint64_t *o_keys = nullptr;
  int32_t *o_fgid = nullptr, *o_labels = nullptr;
  float *o_vals = nullptr;
  uint32_t *o_rowptr = nullptr;
  size_t cap_keys = 0, cap_fgid = 0, cap_labels = 0, cap_vals = 0, cap_rowptr = 0;
  // scratch of the passes
  uint32_t *src_off = nullptr;
  uint64_t *tile_cnt = nullptr, *tile_off = nullptr;
  size_t cap_src = 0, cap_tcnt = 0, cap_toff = 0;
  char *scan_tmp = nullptr;
  size_t cap_scan = 0;
  unsigned long long *d_stat = nullptr;  // negatives seen, kept of the running apply
  uint64_t *h_back = nullptr;            // pinned: the totals and the two stats
  // xf_negsample_apply's copies of the host arrays
  uint64_t *u_keys = nullptr;
  int32_t *u_fgid = nullptr, *u_labels = nullptr;
  float *u_vals = nullptr;
  uint32_t *u_rowptr = nullptr;
  size_t ucap_keys = 0, ucap_fgid = 0, ucap_labels = 0, ucap_vals = 0, ucap_rowptr = 0;
  std::vector<uint32_t> h_rowptr;
};

extern "C" int xf_negsample_destroy(xf_negsample *s) {
  if (!s) return XF_OK;
  if (s->d_stat && !xf::device_poisoned()) {  // (d_stat: an apply has run)
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)s->o_keys, (void *)s->o_fgid, (void *)s->o_labels, (void *)s->o_vals,
                    (void *)s->o_rowptr, (void *)s->src_off, (void *)s->tile_cnt,
                    (void *)s->tile_off, (void *)s->scan_tmp, (void *)s->d_stat, (void *)s->u_keys,
                    (void *)s->u_fgid, (void *)s->u_labels, (void *)s->u_vals,
                    (void *)s->u_rowptr})
      if (p) (void)hipFree(p);
    if (s->h_back) (void)hipHostFree(s->h_back);
  }
  delete s;
  return XF_OK;
}

extern "C" int xf_negsample_create(xf_negsample **out, float keep, uint64_t seed) {
  XF_REQUIRE(out, "xf_negsample_create: null argument");
  *out = nullptr;
  XF_TRY(check_keep("xf_negsample_create", keep));
  xf_negsample *s = new xf_negsample;
  struct Guard {
    xf_negsample *s;
    ~Guard() {
      if (s) xf_negsample_destroy(s);
    }
  } guard{s};
  s->keep = keep;
  s->seed = seed;
  s->T = xf::negsample_threshold((double)keep);
  // (nothing on the device yet: the first apply allocates — the parameters and the weight are
  // host arithmetic)
  guard.s = nullptr;
  *out = s;
  return XF_OK;
}

extern "C" int xf_negsample_params(const xf_negsample *s, float *keep, uint64_t *seed) {
  XF_REQUIRE(s, "xf_negsample_params: null argument");
  if (keep) *keep = s->keep;
  if (seed) *seed = s->seed;
  return XF_OK;
}

extern "C" int xf_negsample_weight(const xf_negsample *s, float *weight) {
  XF_REQUIRE(s && weight, "xf_negsample_weight: null argument");
  *weight = 1.0f / s->keep;  // one fp32 division
  return XF_OK;
}

extern "C" int xf_negsample_keep(uint64_t seed, uint64_t stream, uint64_t ordinal, float keep) {
  if (!(keep > 0.0f && keep <= 1.0f)) return 0;
  return xf::negsample_keep_row(xf::negsample_base(seed, stream), ordinal,
                                xf::negsample_threshold((double)keep)) ? 1 : 0;
}

extern "C" int xf_negsample_stats(const xf_negsample *s, uint64_t *rows_seen, uint64_t *rows_kept,
                                  uint64_t *neg_seen, uint64_t *neg_kept) {
  XF_REQUIRE(s, "xf_negsample_stats: null argument");
  if (rows_seen) *rows_seen = s->rows_seen;
  if (rows_kept) *rows_kept = s->rows_kept;
  if (neg_seen) *neg_seen = s->neg_seen;
  if (neg_kept) *neg_kept = s->neg_kept;
  return XF_OK;
}

extern "C" int xf_negsample_apply_dev(xf_negsample *s, uint64_t stream_id, uint64_t first_ordinal,
                                      const uint64_t *d_keys, const int32_t *d_fgid,
                                      const float *d_vals, const uint32_t *d_rowptr,
                                      const int32_t *d_labels, uint32_t R, uint32_t NNZ,
                                      void *stream, const uint64_t **d_keys_out,
                                      const int32_t **d_fgid_out, const float **d_vals_out,
                                      const uint32_t **d_rowptr_out, const int32_t **d_labels_out,
                                      uint32_t *R_out, uint32_t *NNZ_out) {
  XF_REQUIRE(s && d_keys_out && d_rowptr_out && d_labels_out && R_out && NNZ_out,
             "xf_negsample_apply_dev: null argument");
  XF_REQUIRE(NNZ == 0 || (d_keys && R > 0),
             "xf_negsample_apply_dev: %u nonzeros need keys and rows (R = %u)", NNZ, R);
  XF_REQUIRE(R == 0 || (d_rowptr && d_labels),
             "xf_negsample_apply_dev: %u rows without row offsets or labels", R);
  XF_REQUIRE(NNZ < 0xFFFFFFFFu - 2 * kNsChunk && R < 0xFFFFFFFFu - 2 * kNsTile,
             "xf_negsample_apply_dev: a minibatch of %u rows, %u nonzeros is too large", R, NNZ);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t ntiles = (R + kNsTile - 1) / kNsTile;
  if (!s->d_stat) XF_HIP(hipMalloc((void **)&s->d_stat, 2 * sizeof(unsigned long long)));
  if (!s->h_back) XF_HIP(hipHostMalloc((void **)&s->h_back, 3 * sizeof(uint64_t)));
  XF_TRY(grow(&s->o_keys, &s->cap_keys, NNZ));
  if (d_fgid) XF_TRY(grow(&s->o_fgid, &s->cap_fgid, NNZ));
  if (d_vals) XF_TRY(grow(&s->o_vals, &s->cap_vals, NNZ));
  XF_TRY(grow(&s->o_rowptr, &s->cap_rowptr, (size_t)R + 1));
  XF_TRY(grow(&s->o_labels, &s->cap_labels, R));
  *d_keys_out = s->o_keys;
  if (d_fgid_out) *d_fgid_out = d_fgid ? s->o_fgid : nullptr;
  if (d_vals_out) *d_vals_out = d_vals ? s->o_vals : nullptr;
  *d_rowptr_out = s->o_rowptr;
  *d_labels_out = s->o_labels;
  *R_out = *NNZ_out = 0;
  if (R == 0) {  // no row to decide on: the one zero offset (asynchronous, nothing to read back)
    XF_HIP(hipMemsetAsync(s->o_rowptr, 0, 4, st));
    return XF_OK;
  }
  XF_TRY(grow(&s->src_off, &s->cap_src, R));
  XF_TRY(grow(&s->tile_cnt, &s->cap_tcnt, (size_t)ntiles + 1));
  XF_TRY(grow(&s->tile_off, &s->cap_toff, (size_t)ntiles + 1));
  size_t tb = 0;
  XF_HIP(rocprim::exclusive_scan((void *)nullptr, tb, s->tile_cnt, s->tile_off, (uint64_t)0,
                                 (size_t)ntiles + 1, rocprim::plus<uint64_t>(), st));
  XF_TRY(grow(&s->scan_tmp, &s->cap_scan, tb));
  const uint64_t base = xf::negsample_base(s->seed, stream_id);
  XF_HIP(hipMemsetAsync(s->d_stat, 0, 2 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_ns_flag, dim3(ntiles), dim3(kNsThreads), 0, st, d_rowptr, d_labels, R, NNZ,
                     base, first_ordinal, s->T, s->tile_cnt, ntiles, s->d_stat);
  XF_HIP(hipGetLastError());
  XF_HIP(rocprim::exclusive_scan((void *)s->scan_tmp, tb, s->tile_cnt, s->tile_off, (uint64_t)0,
                                 (size_t)ntiles + 1, rocprim::plus<uint64_t>(), st));
  hipLaunchKernelGGL(k_ns_place, dim3(ntiles), dim3(kNsThreads), 0, st, d_rowptr, d_labels, R, NNZ,
                     base, first_ordinal, s->T, (const uint64_t *)s->tile_off, ntiles, s->o_rowptr,
                     s->o_labels, s->src_off);
  if (NNZ)
    hipLaunchKernelGGL(k_ns_copy, dim3((NNZ + kNsChunk - 1) / kNsChunk), dim3(kNsThreads), 0, st,
                       d_keys, d_fgid, d_vals, R, NNZ, (const uint64_t *)s->tile_off, ntiles,
                       (const uint32_t *)s->o_rowptr, (const uint32_t *)s->src_off, s->o_keys,
                       s->o_fgid, s->o_vals);
  XF_HIP(hipGetLastError());
  XF_HIP(hipMemcpyAsync(s->h_back, s->tile_off + ntiles, 8, hipMemcpyDeviceToHost, st));
  XF_HIP(hipMemcpyAsync(s->h_back + 1, s->d_stat, 16, hipMemcpyDeviceToHost, st));
  XF_HIP(hipStreamSynchronize(st));  // the one wait: the two counts (and the stats)
  const uint64_t total = s->h_back[0];
  XF_REQUIRE((uint32_t)total <= NNZ && (total >> 32) <= R,
             "xf_negsample_apply_dev: the kept rows hold %u nonzeros of %u: the row offsets overlap",
             (uint32_t)total, NNZ);
  *R_out = (uint32_t)(total >> 32);
  *NNZ_out = (uint32_t)total;
  s->rows_seen += R;
  s->rows_kept += *R_out;
  s->neg_seen += s->h_back[1];
  s->neg_kept += s->h_back[2];
  return XF_OK;
}

// xf_negsample_apply's upload of a row slice of the reader's host arrays (rowptr rebased to u32)
static int upload_slice(xf_negsample *s, const uint64_t *rowptr, const uint64_t *keys,
                        const int32_t *fgid, const float *vals, const int32_t *labels,
                        size_t row_begin, size_t row_end, hipStream_t st, uint32_t *R_up,
                        uint32_t *NNZ_up) {
  XF_REQUIRE(s && rowptr && row_begin <= row_end, "xf_negsample_apply: bad argument");
  const size_t R = row_end - row_begin;
  XF_REQUIRE(R == 0 || labels, "xf_negsample_apply: %zu rows without labels", R);
  const uint64_t base = rowptr[row_begin];
  XF_REQUIRE(rowptr[row_end] >= base, "xf_negsample_apply: row offsets descend");
  const uint64_t nnz = rowptr[row_end] - base;
  XF_REQUIRE(R < 0xFFFFFF00ull && nnz < 0xFFFFE000ull,
             "xf_negsample_apply: a minibatch of %zu rows, %llu nonzeros is too large", R,
             (unsigned long long)nnz);
  XF_REQUIRE(nnz == 0 || keys, "xf_negsample_apply: %llu nonzeros without keys",
             (unsigned long long)nnz);
  s->h_rowptr.resize(R + 1);
  for (size_t r = 0; r <= R; ++r) {
    const uint64_t at = rowptr[row_begin + r];
    XF_REQUIRE(at >= base && at - base <= nnz && (r == 0 || at - base >= s->h_rowptr[r - 1]),
               "xf_negsample_apply: row offsets descend at row %zu", row_begin + r);
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

extern "C" int xf_negsample_apply(xf_negsample *s, uint64_t stream_id, uint64_t first_ordinal,
                                  const uint64_t *rowptr, const uint64_t *keys,
                                  const int32_t *fgid, const float *vals, const int32_t *labels,
                                  size_t row_begin, size_t row_end, void *stream,
                                  const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                                  const float **d_vals_out, const uint32_t **d_rowptr_out,
                                  const int32_t **d_labels_out, uint32_t *R_out,
                                  uint32_t *NNZ_out) {
  uint32_t R = 0, nnz = 0;
  XF_TRY(upload_slice(s, rowptr, keys, fgid, vals, labels, row_begin, row_end,
                      (hipStream_t)stream, &R, &nnz));
  // (the host arrays may be pageable: the copies above have read them when they return; the
  // vector of rebased offsets lives until the next call.  R = 0: nothing waits, so wait here)
  if (R == 0) XF_HIP(hipStreamSynchronize((hipStream_t)stream));
  return xf_negsample_apply_dev(s, stream_id, first_ordinal, s->u_keys,
                                fgid ? s->u_fgid : nullptr, vals ? s->u_vals : nullptr,
                                s->u_rowptr, s->u_labels, R, nnz, stream, d_keys_out, d_fgid_out,
                                d_vals_out, d_rowptr_out, d_labels_out, R_out, NNZ_out);
}
