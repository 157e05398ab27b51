// xf_gauc.hip — grouped AUC on the held-out rows: a log of (id, code) records and its reduction.
//
// A held row leaves one record: the id of its group (its slice id by xf_slices' rule) and the
// code of its score and class (xf_gauc.h: one definition for the host and the kernel).  The AUC
// inside a group needs the group's records ordered by score, so the device keeps the records, not
// sums: two arrays that grow, ids (u64) and codes (u32).  A reduce orders them by (id, code) —
// two stable passes of xf_sort_key_pos, by code and then by id — and one segmented pass forms,
// per group, P, N, U2 and T in exact integers.  Every floating-point figure is formed on the host
// (xf_gauc_host.cc).  The result depends on the multiset of records alone and is compared with ==.
// Not in the reference.
//
// Kernels:
//   k_ga_pack     kGaPackRows rows per workgroup, lanes on consecutive rows: the row's code; the
//                 rows without a record are counted (LDS, then one global add per counter); the
//                 workgroup takes its records' places in the log with ONE 64-bit add.
//   k_ga_widen, k_ga_gather_ids, k_ga_gather_codes   the sort's plumbing: the codes as 64-bit keys,
//                 the ids in code order, the codes in (id, code) order.
//   k_ga_tile     kGaTile sorted records per workgroup, four consecutive ones a thread: the heads
//                 of groups and of runs of equal score, every record's count of the tile's
//                 negatives before it (with the two flags in its top bits), and the tile's
//                 {negatives, group heads, last group head, last run head}.  One rocPRIM exclusive
//                 scan over the tiles' words.
//   k_ga_groups   the same tiles.  With E(i) = the negatives before record i (the tile's base + the
//                 record's word), g(i) and r(i) the heads of i's group and run (max-scans), a
//                 positive adds E(i) + E(r) - 2 E(g) to its group's U2 and E(i) - E(r) to its T: a
//                 run's negatives sort in front of its positives, so E(i) - E(g) is neg_below +
//                 neg_b and E(r) - E(g) is neg_below.  The terms are prefix-summed in the
//                 workgroup; the last record of a group (or of the tile) takes the group's sums as
//                 a difference of two prefixes.  A group inside one tile is stored, a group that
//                 crosses tiles is added with one 64-bit atomic per word and tile — so one group of
//                 every record costs a tile four atomics, and 10^6 groups of two records none.
//   No scratch, no spills (tools/spill_check.sh).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <atomic>
#include <new>

#include "xf_common.h"
#include "xf_gauc.h"
#include "xflow_amd.h"

namespace {

constexpr int kGaThreads = 256;
constexpr uint32_t kGaPackPer = 4;
constexpr uint32_t kGaPackRows = kGaThreads * kGaPackPer;  // rows of a pack workgroup
constexpr uint32_t kGaPer = 4;
constexpr uint32_t kGaTile = kGaThreads * kGaPer;  // records of a reduce workgroup
constexpr uint32_t kGaHeadG = 1u << 30, kGaHeadR = 1u << 31, kGaNegMask = kGaHeadG - 1;
constexpr size_t E = XF_GAUC_WORDS + 1;  // words of an entry: the id, then P, N, U2, T

// the device's counters
enum : uint32_t { kCntN = 0, kCntNone = 1, kCntOther = 3, kCntWords = 5 };

// a tile's word, and the exclusive "sum" of the tiles before one: heads are record index + 1
struct __attribute__((aligned(16))) GaAgg {
  uint32_t neg, heads, gh, rh;
};
struct GaPlus {
  __host__ __device__ GaAgg operator()(const GaAgg &a, const GaAgg &b) const {
    return GaAgg{a.neg + b.neg, a.heads + b.heads, a.gh > b.gh ? a.gh : b.gh,
                 a.rh > b.rh ? a.rh : b.rh};
  }
};

struct OpAdd {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// the exclusive scan (identity 0) of x over the workgroup's threads; *total: over all of them.
// tmp: kGaThreads / 64 words of LDS, free again when the call returns.
template <typename T, typename Op>
__device__ inline T wg_scan(T x, Op op, T *tmp, T *total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T u = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc = op(inc, u);
  }
  T exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = 0;
  if (lane == 63) tmp[wave] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < kGaThreads / 64; ++w) {
    const T v = tmp[w];
    if (w < wave) base = op(base, v);
    tot = op(tot, v);
  }
  __syncthreads();
  *total = tot;
  return op(base, exc);
}

__global__ __launch_bounds__(kGaThreads) void k_ga_pack(
    const float *__restrict__ loss, const int32_t *__restrict__ labels,
    const uint64_t *__restrict__ id, uint32_t R, uint64_t *__restrict__ log_ids,
    uint32_t *__restrict__ log_codes, uint64_t cap, unsigned long long *__restrict__ cnt) {
  __shared__ uint32_t tmp[kGaThreads / 64];
  __shared__ uint32_t s_cnt[4];
  __shared__ unsigned long long s_base;
  const uint32_t t = threadIdx.x;
  if (t < 4) s_cnt[t] = 0;
  __syncthreads();
  uint64_t rid[kGaPackPer];
  uint32_t rcode[kGaPackPer], mine = 0;
#pragma unroll
  for (uint32_t k = 0; k < kGaPackPer; ++k) {
    const uint64_t r = (uint64_t)blockIdx.x * kGaPackRows + k * kGaThreads + t;
    rcode[k] = XF_GAUC_OTHER;
    rid[k] = 0;
    if (r < R) {
      const int32_t label = labels[r];
      const uint32_t code = xf::gauc_code(loss[r], label), pos = label != 0 ? 1u : 0u;
      const uint64_t i = id[r];
      if (code == XF_GAUC_OTHER) {
        atomicAdd(&s_cnt[2 + pos], 1u);
      } else if (i == XF_SLICE_NONE) {
        atomicAdd(&s_cnt[pos], 1u);
      } else {
        rcode[k] = code;
        rid[k] = i;
        ++mine;
      }
    }
  }
  uint32_t total;
  const uint32_t before = wg_scan(mine, OpAdd(), tmp, &total);
  if (t == 0)
    s_base = total ? __hip_atomic_fetch_add(&cnt[kCntN], (unsigned long long)total,
                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                   : 0ull;
  __syncthreads();
  if (t < 4 && s_cnt[t])
    __hip_atomic_fetch_add(&cnt[kCntNone + t], (unsigned long long)s_cnt[t], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  uint64_t at = s_base + before;
#pragma unroll
  for (uint32_t k = 0; k < kGaPackPer; ++k) {
    if (rcode[k] != XF_GAUC_OTHER) {
      if (at < cap) {  // (always: the host sized the log for every row appended so far)
        log_ids[at] = rid[k];
        log_codes[at] = rcode[k];
      }
      ++at;
    }
  }
}

__global__ __launch_bounds__(kGaThreads) void k_ga_widen(const uint32_t *__restrict__ codes,
                                                         uint32_t n, uint64_t *__restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * kGaThreads + threadIdx.x;
  if (i < n) keys[i] = codes[i];
}

__global__ __launch_bounds__(kGaThreads) void k_ga_gather_ids(
    const uint64_t *__restrict__ ids, const uint32_t *__restrict__ pos, uint32_t n,
    uint64_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kGaThreads + threadIdx.x;
  if (i < n) {
    const uint32_t p = pos[i];
    out[i] = p < n ? ids[p] : 0;  // (p < n: a position of the sort)
  }
}

__global__ __launch_bounds__(kGaThreads) void k_ga_gather_codes(
    const uint64_t *__restrict__ code_keys, const uint32_t *__restrict__ pos, uint32_t n,
    uint32_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kGaThreads + threadIdx.x;
  if (i < n) {
    const uint32_t p = pos[i];
    out[i] = p < n ? (uint32_t)code_keys[p] : 0u;
  }
}

// word[i] = the tile's negatives before i | kGaHeadG | kGaHeadR; agg[tile]; agg[ntiles] = 0 (its
// exclusive sum: the totals)
__global__ __launch_bounds__(kGaThreads) void k_ga_tile(
    const uint64_t *__restrict__ sid, const uint32_t *__restrict__ codes, uint32_t n,
    uint32_t *__restrict__ word, GaAgg *__restrict__ agg, uint32_t ntiles) {
  __shared__ uint32_t tmp[kGaThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x;
  const uint32_t i0 = tile * kGaTile + t * kGaPer;  // (n < 2^30: no wrap)
  uint64_t prev_id = 0;
  uint32_t prev_score = 0;
  if (i0 > 0 && i0 < n) {
    prev_id = sid[i0 - 1];
    prev_score = codes[i0 - 1] >> 1;
  }
  uint32_t w[kGaPer], neg = 0, heads = 0, gh = 0, rh = 0;
#pragma unroll
  for (uint32_t k = 0; k < kGaPer; ++k) {
    const uint32_t i = i0 + k;
    w[k] = 0;
    if (i < n) {
      const uint64_t id = sid[i];
      const uint32_t c = codes[i], score = c >> 1;
      const bool g = i == 0 || id != prev_id, r = g || score != prev_score;
      w[k] = neg | (g ? kGaHeadG : 0u) | (r ? kGaHeadR : 0u);  // (neg: inside the thread so far)
      if (g) {
        ++heads;
        gh = i + 1;
      }
      if (r) rh = i + 1;
      neg += (c & 1u) ? 0u : 1u;
      prev_id = id;
      prev_score = score;
    }
  }
  // (a tile holds at most 1024 negatives and 1024 heads: both sums in one word)
  uint32_t both;
  const uint32_t before = wg_scan(neg | (heads << 16), OpAdd(), tmp, &both) & 0xFFFFu;
  uint32_t gh_all, rh_all;
  (void)wg_scan(gh, OpMax(), tmp, &gh_all);
  (void)wg_scan(rh, OpMax(), tmp, &rh_all);
#pragma unroll
  for (uint32_t k = 0; k < kGaPer; ++k)
    if (i0 + k < n) word[i0 + k] = w[k] + before;  // (before + the thread's < 2^30)
  if (t == 0) {
    agg[tile] = GaAgg{both & 0xFFFFu, both >> 16, gh_all, rh_all};
    if (tile == 0) agg[ntiles] = GaAgg{0, 0, 0, 0};
  }
}

// the negatives before record j in the whole sorted log
__device__ inline uint32_t ga_neg_before(const GaAgg *__restrict__ pre,
                                         const uint32_t *__restrict__ word, uint32_t j) {
  return pre[j / kGaTile].neg + (word[j] & kGaNegMask);
}

// entries[g] = (id, P, N, U2, T) of group g (zeroed before the launch), g < groups = the heads
__global__ __launch_bounds__(kGaThreads) void k_ga_groups(
    const uint64_t *__restrict__ sid, const uint32_t *__restrict__ codes,
    const uint32_t *__restrict__ word, const GaAgg *__restrict__ pre, uint32_t n,
    unsigned long long *__restrict__ entries, uint32_t groups) {
  __shared__ uint64_t tmp64[kGaThreads / 64];
  __shared__ uint32_t tmp[kGaThreads / 64];
  __shared__ uint64_t inc_u[kGaTile], inc_t[kGaTile];
  __shared__ uint32_t inc_p[kGaTile];
  const uint32_t tile = blockIdx.x, t = threadIdx.x;
  const uint32_t tile0 = tile * kGaTile, i0 = tile0 + t * kGaPer;
  const GaAgg base = pre[tile];
  uint32_t w[kGaPer + 1], c[kGaPer];
#pragma unroll
  for (uint32_t k = 0; k < kGaPer; ++k) {
    w[k] = i0 + k < n ? word[i0 + k] : 0u;
    c[k] = i0 + k < n ? codes[i0 + k] : 0u;
  }
  // (the record behind the thread's last: its group-head flag ends this thread's last group; the
  // end of the log ends one as well)
  w[kGaPer] = i0 + kGaPer < n ? word[i0 + kGaPer] : kGaHeadG;
  uint32_t heads = 0, pos = 0, gh = 0, rh = 0;
#pragma unroll
  for (uint32_t k = 0; k < kGaPer; ++k) {
    if (i0 + k < n) {
      if (w[k] & kGaHeadG) {
        ++heads;
        gh = i0 + k + 1;
      }
      if (w[k] & kGaHeadR) rh = i0 + k + 1;
      pos += c[k] & 1u;
    }
  }
  uint32_t unused;
  const uint32_t both = wg_scan(heads | (pos << 16), OpAdd(), tmp, &unused);
  uint32_t gh_run = wg_scan(gh, OpMax(), tmp, &unused), rh_run = wg_scan(rh, OpMax(), tmp, &unused);
  gh_run = gh_run > base.gh ? gh_run : base.gh;
  rh_run = rh_run > base.rh ? rh_run : base.rh;
  uint32_t heads_run = base.heads + (both & 0xFFFFu), pos_run = both >> 16;
  // pass 1: every record's head of group and of run, its group's number, its terms
  uint32_t g_of[kGaPer], grp[kGaPer];
  uint64_t u[kGaPer], tt[kGaPer], u_sum = 0, t_sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kGaPer; ++k) {
    const uint32_t i = i0 + k;
    u[k] = 0;
    tt[k] = 0;
    g_of[k] = 0;
    grp[k] = 0;
    if (i < n) {
      if (w[k] & kGaHeadG) {
        ++heads_run;
        gh_run = i + 1;
      }
      if (w[k] & kGaHeadR) rh_run = i + 1;
      // (record 0 heads a group and a run: gh_run, rh_run >= 1 and heads_run >= 1 from here on)
      g_of[k] = gh_run - 1;
      grp[k] = heads_run - 1;
      if (c[k] & 1u) {
        const uint64_t e_i = base.neg + (w[k] & kGaNegMask);
        const uint64_t e_g = ga_neg_before(pre, word, gh_run - 1);
        const uint64_t e_r = ga_neg_before(pre, word, rh_run - 1);
        u[k] = e_i + e_r - 2 * e_g;  // (e_g <= e_r <= e_i)
        tt[k] = e_i - e_r;
      }
      u_sum += u[k];
      t_sum += tt[k];
    }
  }
  uint64_t unused64;
  uint64_t u_run = wg_scan(u_sum, OpAdd(), tmp64, &unused64);
  uint64_t t_run = wg_scan(t_sum, OpAdd(), tmp64, &unused64);
#pragma unroll
  for (uint32_t k = 0; k < kGaPer; ++k) {
    const uint32_t l = t * kGaPer + k;
    u_run += u[k];
    t_run += tt[k];
    pos_run += (i0 + k < n) ? (c[k] & 1u) : 0u;
    inc_u[l] = u_run;
    inc_t[l] = t_run;
    inc_p[l] = pos_run;
  }
  __syncthreads();
  // pass 2: a group's last record in the tile takes the sums of the group's part in the tile
#pragma unroll
  for (uint32_t k = 0; k < kGaPer; ++k) {
    const uint32_t i = i0 + k, l = t * kGaPer + k;
    if (i >= n || grp[k] >= groups) continue;  // (grp < groups: the heads were counted alike)
    unsigned long long *e = entries + (size_t)grp[k] * E;
    if (w[k] & kGaHeadG) e[0] = sid[i];
    const bool ends = i + 1 >= n || (w[k + 1] & kGaHeadG) != 0;
    if (!ends && l != kGaTile - 1) continue;
    const bool from_here = g_of[k] >= tile0;
    const uint32_t a = from_here ? g_of[k] - tile0 : 0u;  // the part's first record in the tile
    const uint64_t P = inc_p[l] - (a ? inc_p[a - 1] : 0u);
    const uint64_t N = (uint64_t)(l - a + 1) - P;
    const uint64_t U = inc_u[l] - (a ? inc_u[a - 1] : 0ull);
    const uint64_t T = inc_t[l] - (a ? inc_t[a - 1] : 0ull);
    if (from_here && ends) {  // the whole group: nobody else writes these words
      e[1] = P;
      e[2] = N;
      e[3] = U;
      e[4] = T;
    } else {
      const unsigned long long v[4] = {P, N, U, T};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (v[q])
          __hip_atomic_fetch_add(&e[1 + q], v[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

inline uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

struct xf_gauc {
  // the log; upper: the host's bound on the records in it (every row appended since the count was
  // last read), which the arrays are sized for
  uint64_t *ids = nullptr;
  uint32_t *codes = nullptr;
  size_t cap = 0, upper = 0;
  unsigned long long *cnt = nullptr;  // kCntWords: the records, none[2], other[2]
  hipStream_t last = nullptr;         // the stream of the last append
  // the reduce's buffers
  uint64_t *a64 = nullptr, *b64 = nullptr, *c64 = nullptr;
  uint32_t *pos = nullptr, *scodes = nullptr, *word = nullptr;
  size_t cap_a = 0, cap_b = 0, cap_c = 0, cap_pos = 0, cap_sc = 0, cap_word = 0;
  GaAgg *agg = nullptr, *pre = nullptr;
  size_t cap_agg = 0, cap_pre = 0;
  char *scan_tmp = nullptr;
  size_t cap_scan = 0;
  unsigned long long *entries = nullptr;
  size_t cap_entries = 0;
};

static std::atomic<uint64_t> g_ga_launches{0};

extern "C" uint64_t xf_gauc_launches(void) { return g_ga_launches.load(std::memory_order_relaxed); }

extern "C" void xf_gauc_shape(uint32_t out[2]) {
  out[0] = kGaPackRows;
  out[1] = kGaTile;
}

extern "C" int xf_gauc_create(xf_gauc **out) {
  XF_REQUIRE(out, "xf_gauc_create: null argument");
  *out = nullptr;
  xf_gauc *g = new (std::nothrow) xf_gauc;
  XF_REQUIRE(g, "xf_gauc_create: out of memory");
  hipError_t e = hipMalloc((void **)&g->cnt, kCntWords * 8);
  if (e == hipSuccess) e = hipMemset(g->cnt, 0, kCntWords * 8);
  if (e != hipSuccess) {
    if (g->cnt) (void)hipFree(g->cnt);
    delete g;
    XF_HIP(e);
  }
  *out = g;
  return XF_OK;
}

extern "C" int xf_gauc_destroy(xf_gauc *g) {
  if (!g) return XF_OK;
  if (!xf::device_poisoned()) {
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)g->ids, (void *)g->codes, (void *)g->cnt, (void *)g->a64,
                    (void *)g->b64, (void *)g->c64, (void *)g->pos, (void *)g->scodes,
                    (void *)g->word, (void *)g->agg, (void *)g->pre, (void *)g->scan_tmp,
                    (void *)g->entries})
      if (p) (void)hipFree(p);
  }
  delete g;
  return XF_OK;
}

// the log sized for `need` records, what it holds kept (copied in the order of `st`)
static int ga_ensure(xf_gauc *g, size_t need, hipStream_t st) {
  if (need <= g->cap) return XF_OK;
  const size_t n = need + need / 2 + 1024;
  uint64_t *ids = nullptr;
  uint32_t *codes = nullptr;
  XF_HIP(hipMalloc((void **)&ids, n * 8));
  hipError_t e = hipMalloc((void **)&codes, n * 4);
  if (e != hipSuccess) {
    (void)hipFree(ids);
    XF_HIP(e);
  }
  const size_t keep = g->upper < g->cap ? g->upper : g->cap;
  if (keep) {
    if (g->last != st) e = hipStreamSynchronize(g->last);  // (the appends that wrote the old log)
    if (e == hipSuccess) e = hipMemcpyAsync(ids, g->ids, keep * 8, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(codes, g->codes, keep * 4, hipMemcpyDeviceToDevice, st);
  }
  if (e == hipSuccess && g->ids) e = hipStreamSynchronize(st);  // (the old log goes back)
  if (e != hipSuccess) {
    (void)hipFree(ids);
    (void)hipFree(codes);
    XF_HIP(e);
  }
  if (g->ids) (void)hipFree(g->ids);
  if (g->codes) (void)hipFree(g->codes);
  g->ids = ids;
  g->codes = codes;
  g->cap = n;
  return XF_OK;
}

extern "C" int xf_gauc_reserve(xf_gauc *g, uint64_t rows) {
  XF_REQUIRE(g, "xf_gauc_reserve: null argument");
  XF_REQUIRE(rows < xf::kGaucMaxRecords,
             "xf_gauc_reserve: %llu rows: a reduce takes fewer than 2^30 records",
             (unsigned long long)rows);
  return ga_ensure(g, (size_t)rows, g->last);
}

int xf::gauc_append(xf_gauc *g, const float *loss, const int32_t *labels, const uint64_t *id,
                    uint32_t R, hipStream_t s) {
  XF_REQUIRE(g, "gauc_append: null object");
  if (R == 0) return XF_OK;
  XF_REQUIRE(loss && labels && id, "gauc_append: null argument");
  XF_TRY(ga_ensure(g, g->upper + R, s));
  hipLaunchKernelGGL(k_ga_pack, dim3(blocks_of(R, kGaPackRows)), dim3(kGaThreads), 0, s, loss,
                     labels, id, R, g->ids, g->codes, (uint64_t)g->cap, g->cnt);
  XF_HIP(hipGetLastError());
  g->upper += R;
  g->last = s;
  g_ga_launches.fetch_add(1, std::memory_order_relaxed);
  return XF_OK;
}

extern "C" int xf_gauc_append_dev(xf_gauc *g, const float *d_loss, const int32_t *d_labels,
                                  const uint64_t *d_id, uint32_t R, void *stream) {
  XF_REQUIRE(g, "xf_gauc_append_dev: null object");
  XF_REQUIRE(R == 0 || (d_loss && d_labels && d_id), "xf_gauc_append_dev: null argument");
  return xf::gauc_append(g, d_loss, d_labels, d_id, R, (hipStream_t)stream);
}

// the counters as they stand (waits for the appends); upper = the records from here on
static int ga_counts(xf_gauc *g, unsigned long long cnt[kCntWords]) {
  XF_HIP(hipMemcpyAsync(cnt, g->cnt, kCntWords * 8, hipMemcpyDeviceToHost, g->last));
  XF_HIP(hipStreamSynchronize(g->last));
  XF_REQUIRE(cnt[kCntN] <= g->cap, "xf_gauc: the log counts %llu records in arrays of %zu",
             cnt[kCntN], g->cap);
  g->upper = (size_t)cnt[kCntN];
  return XF_OK;
}

extern "C" int xf_gauc_append(xf_gauc *g, const uint64_t *ids, const uint32_t *codes, uint64_t n) {
  XF_REQUIRE(g && (n == 0 || (ids && codes)), "xf_gauc_append: null argument");
  for (uint64_t i = 0; i < n; ++i) {
    XF_REQUIRE(ids[i] != XF_SLICE_NONE,
               "xf_gauc_append: record %llu has the id XF_SLICE_NONE: a row without a group leaves "
               "no record", (unsigned long long)i);
    XF_REQUIRE(codes[i] <= xf::kGaucCodeMax,
               "xf_gauc_append: record %llu has code %u: a code is at most %u (UINT32_MAX: a row "
               "that leaves no record)", (unsigned long long)i, codes[i], xf::kGaucCodeMax);
  }
  if (n == 0) return XF_OK;
  unsigned long long cnt[kCntWords];
  XF_TRY(ga_counts(g, cnt));
  const uint64_t have = cnt[kCntN];
  XF_TRY(ga_ensure(g, (size_t)(have + n), g->last));
  XF_HIP(hipMemcpyAsync(g->ids + have, ids, n * 8, hipMemcpyHostToDevice, g->last));
  XF_HIP(hipMemcpyAsync(g->codes + have, codes, n * 4, hipMemcpyHostToDevice, g->last));
  const unsigned long long now = have + n;
  XF_HIP(hipMemcpyAsync(g->cnt + kCntN, &now, 8, hipMemcpyHostToDevice, g->last));
  XF_HIP(hipStreamSynchronize(g->last));  // (the host arrays may be pageable, `now` is a local)
  g->upper = (size_t)now;
  return XF_OK;
}

extern "C" int xf_gauc_export(xf_gauc *g, uint64_t *ids, uint32_t *codes, uint64_t cap,
                              uint64_t *n) {
  XF_REQUIRE(g && n, "xf_gauc_export: null argument");
  unsigned long long cnt[kCntWords];
  XF_TRY(ga_counts(g, cnt));
  *n = cnt[kCntN];
  if (!ids && !codes) return XF_OK;  // (only the count)
  XF_REQUIRE(ids && codes, "xf_gauc_export: ids without codes, or the other way round");
  XF_REQUIRE(*n <= cap, "xf_gauc_export: %llu records do not fit arrays of %llu", cnt[kCntN],
             (unsigned long long)cap);
  if (*n) {
    XF_HIP(hipMemcpy(ids, g->ids, (size_t)*n * 8, hipMemcpyDeviceToHost));
    XF_HIP(hipMemcpy(codes, g->codes, (size_t)*n * 4, hipMemcpyDeviceToHost));
  }
  return XF_OK;
}

extern "C" int xf_gauc_reduce(xf_gauc *g, uint64_t *entries, uint64_t cap, uint64_t *n,
                              uint64_t *none, uint64_t *other, int reset) {
  XF_REQUIRE(g && n, "xf_gauc_reduce: null argument");
  XF_REQUIRE(entries || !reset,
             "xf_gauc_reduce: a reduce without entries only counts them and cannot reset");
  unsigned long long cnt[kCntWords];
  XF_TRY(ga_counts(g, cnt));
  const uint64_t m = cnt[kCntN];
  XF_REQUIRE(m < xf::kGaucMaxRecords,
             "xf_gauc_reduce: %llu records: a reduce takes fewer than 2^30 (XF_GAUC_MAX_RECORDS)",
             cnt[kCntN]);
  hipStream_t st = g->last;
  uint64_t groups = 0;
  const uint32_t mm = (uint32_t)m, ntiles = blocks_of(m, kGaTile);
  if (m) {
    XF_TRY(grow(&g->a64, &g->cap_a, (size_t)m));
    XF_TRY(grow(&g->b64, &g->cap_b, (size_t)m));
    XF_TRY(grow(&g->c64, &g->cap_c, (size_t)m));
    XF_TRY(grow(&g->pos, &g->cap_pos, (size_t)m));
    XF_TRY(grow(&g->scodes, &g->cap_sc, (size_t)m));
    XF_TRY(grow(&g->word, &g->cap_word, (size_t)m));
    XF_TRY(grow(&g->agg, &g->cap_agg, (size_t)ntiles + 1));
    XF_TRY(grow(&g->pre, &g->cap_pre, (size_t)ntiles + 1));
    size_t tb = 0;
    XF_HIP(rocprim::exclusive_scan((void *)nullptr, tb, g->agg, g->pre, GaAgg{0, 0, 0, 0},
                                   (size_t)ntiles + 1, GaPlus(), st));
    XF_TRY(grow(&g->scan_tmp, &g->cap_scan, tb + 1));
    const uint32_t per_thread = blocks_of(m, kGaThreads);
    // by code (a64: the codes as keys; b64, pos: sorted), then stably by id (c64: the ids in code
    // order; a64, pos: sorted)
    hipLaunchKernelGGL(k_ga_widen, dim3(per_thread), dim3(kGaThreads), 0, st,
                       (const uint32_t *)g->codes, mm, g->a64);
    XF_HIP(hipGetLastError());
    XF_TRY(xf_sort_key_pos(g->a64, mm, 0, xf::kGaucCodeMax, g->b64, g->pos, st, nullptr));
    hipLaunchKernelGGL(k_ga_gather_ids, dim3(per_thread), dim3(kGaThreads), 0, st,
                       (const uint64_t *)g->ids, (const uint32_t *)g->pos, mm, g->c64);
    XF_HIP(hipGetLastError());
    XF_TRY(xf_sort_key_pos(g->c64, mm, 0, UINT64_MAX, g->a64, g->pos, st, nullptr));
    hipLaunchKernelGGL(k_ga_gather_codes, dim3(per_thread), dim3(kGaThreads), 0, st,
                       (const uint64_t *)g->b64, (const uint32_t *)g->pos, mm, g->scodes);
    hipLaunchKernelGGL(k_ga_tile, dim3(ntiles), dim3(kGaThreads), 0, st, (const uint64_t *)g->a64,
                       (const uint32_t *)g->scodes, mm, g->word, g->agg, ntiles);
    XF_HIP(hipGetLastError());
    XF_HIP(rocprim::exclusive_scan((void *)g->scan_tmp, tb, g->agg, g->pre, GaAgg{0, 0, 0, 0},
                                   (size_t)ntiles + 1, GaPlus(), st));
    GaAgg total;
    XF_HIP(hipMemcpyAsync(&total, g->pre + ntiles, sizeof(GaAgg), hipMemcpyDeviceToHost, st));
    XF_HIP(hipStreamSynchronize(st));
    groups = total.heads;
  }
  *n = groups;
  for (int c = 0; c < 2; ++c) {
    if (none) none[c] = cnt[kCntNone + c];
    if (other) other[c] = cnt[kCntOther + c];
  }
  if (!entries) return XF_OK;
  XF_REQUIRE(groups <= cap,
             "xf_gauc_reduce: %llu groups do not fit an array of %llu entries; nothing was reset",
             (unsigned long long)groups, (unsigned long long)cap);
  if (groups) {
    XF_TRY(grow(&g->entries, &g->cap_entries, (size_t)groups * E));
    XF_HIP(hipMemsetAsync(g->entries, 0, (size_t)groups * E * 8, st));
    hipLaunchKernelGGL(k_ga_groups, dim3(ntiles), dim3(kGaThreads), 0, st,
                       (const uint64_t *)g->a64, (const uint32_t *)g->scodes,
                       (const uint32_t *)g->word, (const GaAgg *)g->pre, mm, g->entries,
                       (uint32_t)groups);
    XF_HIP(hipGetLastError());
    XF_HIP(hipMemcpyAsync(entries, g->entries, (size_t)groups * E * 8, hipMemcpyDeviceToHost, st));
    XF_HIP(hipStreamSynchronize(st));
  }
  if (reset) {
    XF_HIP(hipMemsetAsync(g->cnt, 0, kCntWords * 8, st));
    XF_HIP(hipStreamSynchronize(st));
    g->upper = 0;
  }
  return XF_OK;
}
