// xf_slices.hip — sliced progressive validation: progressive validation's counters kept per value
// of one field (per site, advertiser, slot ...).  A row's slice id is the key of its first nonzero
// of field F; a slice has seven 64-bit words (xf_slices.h).  The device only adds integers: the
// result depends on nothing but the rows' losses, labels and ids — not the launch shape or the
// arrival order of the atomics — and is compared with ==.  Every floating-point figure is formed
// on the host (xf_slices_host.cc).  Not in the reference.
//
// Kernels:
//   k_sl_extract      one wave per row, the row's fgids in the lanes: __ballot(fgid == F), first
//                set bit, that nonzero's key.  Rows longer than 64 take 64 at a time and stop at
//                the first chunk with a member.  Writes id[R] and nothing else.
//   k_sl_accumulate   kSlRows rows per workgroup, lanes on consecutive rows.  A minibatch puts
//                thousands of rows on a few hot slices, so (as k_pg_accumulate) a wave first folds
//                the lanes that share its first row's id into one contribution, and the workgroup
//                sums in LDS: an open-addressed table of kSlSlots entries keyed by id, kSlProbe
//                probes, 64-bit LDS atomics; the key and each of the seven words in an array of its
//                own, so lanes on different entries add to different banks.  After a barrier one
//                global find-or-insert per occupied entry: a relaxed agent-scope 64-bit CAS on the
//                key word, then relaxed agent-scope 64-bit adds into the entry's 64-byte line.  A
//                row that finds no LDS entry within the probes goes to the global table directly.
//   k_sl_export       ballot-compacts the occupied entries into a dense array and a count.
// No scratch, no spills (tools/spill_check.sh).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <vector>

#include "xf_common.h"
#include "xf_slices.h"
#include "xflow_amd.h"

namespace {

constexpr int kSlThreads = 256;
constexpr uint32_t kSlPerThread = 4;
constexpr uint32_t kSlRows = kSlThreads * kSlPerThread;  // rows of one accumulate workgroup
constexpr uint32_t kSlLog2Slots = 9;
constexpr uint32_t kSlSlots = 1u << kSlLog2Slots;
constexpr uint32_t kSlProbe = 8;
constexpr uint32_t kSlW = XF_SLICE_WORDS;
constexpr uint32_t kSlEntry = kSlW + 1;  // 64-bit words of a global entry: the key, the seven words
constexpr uint32_t kSxWaves = kSlThreads / 64;
constexpr uint32_t kSxRows = 64;  // rows of one extract workgroup
constexpr unsigned long long kSlEmpty = XF_SLICE_NONE;
static_assert(kSlSlots % kSlThreads == 0, "the flush walks the slots a thread stride at a time");
static_assert(kSlEntry * 8 == 64, "a global entry is one 64-byte line");

typedef unsigned long long u64;

// the global table: 2^b entries, then the `none` entry, then the `overflow` entry
struct SlTable {
  u64 *e;
  int b;
  uint32_t probes;
};

__device__ inline u64 sl_shfl(u64 v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}

__device__ inline u64 sl_wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off, 64);
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

// one contribution (a row's, a wave's fold or an LDS entry's sums) into the global table
__device__ inline void sl_global_add(const SlTable T, u64 id, const u64 (&c)[kSlW]) {
  const u64 mask = (1ull << T.b) - 1;
  u64 *e = T.e + (mask + 2) * kSlEntry;  // overflow
  if (id == kSlEmpty) {
    e = T.e + (mask + 1) * kSlEntry;  // none
  } else {
    u64 slot = xf::slices_home(id, T.b);  // (<= mask)
    for (uint32_t i = 0; i < T.probes; ++i) {
      u64 *k = T.e + slot * kSlEntry;
      u64 cur = __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kSlEmpty) {
        u64 expected = kSlEmpty;
        cur = __hip_atomic_compare_exchange_strong(k, &expected, id, __ATOMIC_RELAXED,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  ? id
                  : expected;
      }
      if (cur == id) {
        e = k;
        break;
      }
      slot = (slot + 1) & mask;
    }
  }
#pragma unroll
  for (uint32_t w = 0; w < kSlW; ++w)
    if (c[w])
      __hip_atomic_fetch_add(&e[1 + w], c[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the same into the workgroup's LDS table (entry kSlSlots: the rows without an id); a key that
// finds no entry within the probes goes to the global table
__device__ inline void sl_lds_add(u64 *s_key, u64 (*s_w)[kSlSlots + 1], const SlTable T, u64 id,
                                  const u64 (&c)[kSlW]) {
  uint32_t slot = kSlSlots;
  if (id != kSlEmpty) {
    slot = (uint32_t)((id * 0x9e3779b97f4a7c15ull) >> (64 - kSlLog2Slots));
    uint32_t i = 0;
    for (; i < kSlProbe; ++i) {
      const u64 prev = atomicCAS(&s_key[slot], kSlEmpty, id);
      if (prev == kSlEmpty || prev == id) break;
      slot = (slot + 1) & (kSlSlots - 1);
    }
    if (i == kSlProbe) {
      sl_global_add(T, id, c);
      return;
    }
  }
#pragma unroll
  for (uint32_t w = 0; w < kSlW; ++w)
    if (c[w]) atomicAdd(&s_w[w][slot], c[w]);
}

__global__ __launch_bounds__(kSlThreads) void k_sl_accumulate(
    const float *__restrict__ loss, const int32_t *__restrict__ labels,
    const uint64_t *__restrict__ id, uint32_t R, const uint32_t *__restrict__ terms,
    const SlTable T) {
  __shared__ u64 s_key[kSlSlots];
  __shared__ u64 s_w[kSlW][kSlSlots + 1];
  const uint32_t t = threadIdx.x, lane = t & 63;
  // the thread's rows first, all of them in flight together, then the gather of their terms (taken
  // a row at a time they would be two dependent trips to memory a row)
  const uint64_t r0 = (uint64_t)blockIdx.x * kSlRows;
  float l[kSlPerThread];
  int32_t lab[kSlPerThread];
  u64 keys[kSlPerThread];
  uint32_t ll[kSlPerThread];
#pragma unroll
  for (uint32_t i = 0; i < kSlPerThread; ++i) {
    const uint64_t r = r0 + i * kSlThreads + t;
    const bool valid = r < R;
    keys[i] = valid ? id[r] : 0;
    l[i] = valid ? loss[r] : 0.0f;
    lab[i] = valid ? labels[r] : 0;
  }
#pragma unroll
  for (uint32_t i = 0; i < kSlPerThread; ++i) {
    const uint32_t rank = xf::progress_rank(l[i]);  // (below XF_PROGRESS_RANKS: inside the table)
    ll[i] = rank < XF_PROGRESS_RANKS ? terms[rank] : 0u;
  }
  for (uint32_t i = t; i < kSlSlots; i += kSlThreads) s_key[i] = kSlEmpty;
  for (uint32_t i = t; i < kSlW * (kSlSlots + 1); i += kSlThreads) (&s_w[0][0])[i] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t i = 0; i < kSlPerThread; ++i) {
    const bool valid = r0 + i * kSlThreads + t < R;
    const u64 key = keys[i];
    u64 c[kSlW] = {0, 0, 0, 0, 0, 0, 0};
    if (valid) {
      const bool pos = lab[i] != 0;
      if (xf::progress_rank(l[i]) == XF_PROGRESS_RANKS) {
        c[xf::kSlOther] = 1;
      } else {
        const u64 q = xf::slices_qfix(l[i]), term = ll[i];
        c[xf::kSlN0] = pos ? 0 : 1;
        c[xf::kSlN1] = pos ? 1 : 0;
        c[xf::kSlQ0] = pos ? 0 : q;
        c[xf::kSlQ1] = pos ? q : 0;
        c[xf::kSlLl0] = pos ? 0 : term;
        c[xf::kSlLl1] = pos ? term : 0;
      }
    }
    const uint64_t vmask = __ballot(valid);
    if (vmask == 0) break;  // (uniform over the wave; later rows lie further out)
    const int leader = __ffsll((unsigned long long)vmask) - 1;
    const u64 lkey = sl_shfl(key, leader);
    const bool same = valid && key == lkey;
    u64 f[kSlW];
#pragma unroll
    for (uint32_t w = 0; w < kSlW; ++w) f[w] = sl_wave_sum(same ? c[w] : 0);
    if (lane == (uint32_t)leader) sl_lds_add(s_key, s_w, T, key, f);
    else if (valid && !same)
      sl_lds_add(s_key, s_w, T, key, c);
  }
  __syncthreads();
  for (uint32_t i = t; i < kSlSlots; i += kSlThreads) {
    const u64 key = s_key[i];
    if (key == kSlEmpty) continue;
    u64 c[kSlW];
#pragma unroll
    for (uint32_t w = 0; w < kSlW; ++w) c[w] = s_w[w][i];
    sl_global_add(T, key, c);
  }
  if (t < kSlW) {
    const u64 v = s_w[t][kSlSlots];
    if (v)
      __hip_atomic_fetch_add(&T.e[((1ull << T.b)) * kSlEntry + 1 + t], v, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

// id[r] = the key of row r's lowest-position nonzero with fgid == F, XF_SLICE_NONE without one; a
// row whose offsets descend or leave the arrays has length 0
__global__ __launch_bounds__(kSlThreads) void k_sl_extract(
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ fgid,
    const uint32_t *__restrict__ rowptr, uint32_t R, uint32_t NNZ, int32_t F,
    uint64_t *__restrict__ id) {
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (uint32_t k = wave; k < kSxRows; k += kSxWaves) {
    const uint64_t r = (uint64_t)blockIdx.x * kSxRows + k;
    if (r >= R) break;
    const uint32_t x = rowptr[r], y = rowptr[r + 1];
    const uint32_t len = (y >= x && y <= NNZ) ? y - x : 0u;
    uint64_t out = XF_SLICE_NONE;
    for (uint32_t c = 0; c < len; c += 64) {
      const bool in = lane < len - c;  // (x + c + lane < x + len <= NNZ)
      const int32_t fg = in ? fgid[x + c + lane] : 0;
      const uint64_t m = __ballot(in && fg == F);
      if (m) {
        out = keys[x + c + (uint32_t)(__ffsll((unsigned long long)m) - 1)];
        break;
      }
      if (len - c <= 64) break;  // (c + 64 may not wrap)
    }
    if (lane == 0) id[r] = out;
  }
}

// the occupied entries of the table, compacted in no particular order: out[pos] for pos < cap,
// *count = all of them (zero on entry)
__global__ __launch_bounds__(kSlThreads) void k_sl_export(const u64 *__restrict__ e, uint64_t n,
                                                          u64 *__restrict__ out, uint64_t cap,
                                                          u64 *count) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * kSlThreads;
  // (every lane of a wave runs the same number of turns: the ballots are whole)
  for (uint64_t base = (uint64_t)blockIdx.x * kSlThreads; base < n; base += stride) {
    const uint64_t i = base + threadIdx.x;
    const bool occ = i < n && e[i * kSlEntry] != kSlEmpty;
    const uint64_t m = __ballot(occ);
    if (m == 0) continue;
    u64 first = 0;
    if (lane == (uint32_t)(__ffsll((unsigned long long)m) - 1))
      first = __hip_atomic_fetch_add(count, (u64)__popcll(m), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    first = sl_shfl(first, __ffsll((unsigned long long)m) - 1);
    const uint64_t pos = first + (uint64_t)__popcll(m & ((1ull << lane) - 1));
    if (occ && pos < cap) {
#pragma unroll
      for (uint32_t w = 0; w < kSlEntry; ++w) out[pos * kSlEntry + w] = e[i * kSlEntry + w];
    }
  }
}

template <typename T>
int sl_grow(T **p, size_t *cap, size_t need) {
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

struct xf_slices {
  int32_t F = 0;
  int b = 0;
  u64 *e = nullptr;           // (2^b + 2) entries of kSlEntry words
  uint32_t *terms = nullptr;  // XF_PROGRESS_RANKS fixed-point row terms
  u64 *count = nullptr;       // the export's count
  u64 *dense = nullptr;       // the export's compacted entries
  size_t cap_dense = 0;
  hipStream_t last = nullptr;  // the stream of the last accumulate
  // the ids of the last extract (valid until the next), and xf_slices_extract's copies
  uint64_t *id = nullptr, *u_keys = nullptr;
  int32_t *u_fgid = nullptr;
  uint32_t *u_rowptr = nullptr;
  size_t cap_id = 0, ucap_keys = 0, ucap_fgid = 0, ucap_rowptr = 0;
  std::vector<uint32_t> h_rowptr;
  size_t entries() const { return ((size_t)1 << b) + 2; }
};

static std::atomic<uint64_t> g_sl_launches{0};

// every key empty, every word zero (the keys of the two extra entries are not read: zero)
static __global__ __launch_bounds__(kSlThreads) void k_sl_clear(u64 *__restrict__ e, uint64_t slots,
                                                         uint64_t words) {
  const uint64_t stride = (uint64_t)gridDim.x * kSlThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kSlThreads + threadIdx.x; i < words; i += stride)
    e[i] = (i % kSlEntry == 0 && i / kSlEntry < slots) ? kSlEmpty : 0ull;
}

static int sl_clear(xf_slices *s, hipStream_t st) {
  const uint64_t words = (uint64_t)s->entries() * kSlEntry;
  const uint64_t groups = (words + kSlThreads - 1) / kSlThreads;
  hipLaunchKernelGGL(k_sl_clear, dim3((uint32_t)std::min<uint64_t>(groups, 8192)),
                     dim3(kSlThreads), 0, st, s->e, 1ull << s->b, words);
  XF_HIP(hipGetLastError());
  return XF_OK;
}

int xf::slices_accumulate(xf_slices *s, const float *loss, const int32_t *labels,
                          const uint64_t *id, uint32_t R, hipStream_t st) {
  XF_REQUIRE(s, "slices_accumulate: null slices");
  if (R == 0 || !id) return XF_OK;
  XF_REQUIRE(loss && labels, "slices_accumulate: null argument");
  const SlTable T{s->e, s->b, xf::slices_probes(s->b)};
  hipLaunchKernelGGL(k_sl_accumulate, dim3((uint32_t)(((uint64_t)R + kSlRows - 1) / kSlRows)),
                     dim3(kSlThreads), 0, st, loss, labels, id, R, (const uint32_t *)s->terms, T);
  XF_HIP(hipGetLastError());
  s->last = st;
  g_sl_launches.fetch_add(1, std::memory_order_relaxed);
  return XF_OK;
}

extern "C" uint64_t xf_slices_launches(void) {
  return g_sl_launches.load(std::memory_order_relaxed);
}

extern "C" void xf_slices_shape(uint32_t out[5]) {
  out[0] = kSlRows;
  out[1] = kSlSlots;
  out[2] = kSlProbe;
  out[3] = xf::kSlicesProbeMax;
  out[4] = kSxRows;
}

extern "C" int xf_slices_destroy(xf_slices *s) {
  if (!s) return XF_OK;
  if (!xf::device_poisoned()) {
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)s->e, (void *)s->terms, (void *)s->count, (void *)s->dense,
                    (void *)s->id, (void *)s->u_keys, (void *)s->u_fgid, (void *)s->u_rowptr})
      if (p) (void)hipFree(p);
  }
  delete s;
  return XF_OK;
}

extern "C" int xf_slices_create(xf_slices **out, int32_t field, int log2_slots) {
  XF_REQUIRE(out, "xf_slices_create: null argument");
  *out = nullptr;
  XF_TRY(xf::slices_check_params("xf_slices_create", field, log2_slots));
  xf_slices *s = new (std::nothrow) xf_slices;
  XF_REQUIRE(s, "xf_slices_create: out of memory");
  s->F = field;
  s->b = log2_slots;
  std::vector<uint32_t> terms(XF_PROGRESS_RANKS);
  xf::slices_terms(terms.data());
  hipError_t e = hipMalloc((void **)&s->e, s->entries() * kSlEntry * 8);
  if (e == hipSuccess) e = hipMalloc((void **)&s->terms, (size_t)XF_PROGRESS_RANKS * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&s->count, 8);
  if (e == hipSuccess)
    e = hipMemcpy(s->terms, terms.data(), (size_t)XF_PROGRESS_RANKS * 4, hipMemcpyHostToDevice);
  int rc = XF_OK;
  if (e == hipSuccess) rc = sl_clear(s, nullptr);
  if (e == hipSuccess && rc == XF_OK) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess || rc != XF_OK) {
    xf_slices_destroy(s);
    if (rc != XF_OK) return rc;
    XF_HIP(e);
  }
  *out = s;
  return XF_OK;
}

extern "C" int xf_slices_params(const xf_slices *s, int32_t *field, int *log2_slots) {
  XF_REQUIRE(s, "xf_slices_params: null argument");
  if (field) *field = s->F;
  if (log2_slots) *log2_slots = s->b;
  return XF_OK;
}

extern "C" int xf_slices_extract_dev(xf_slices *s, const uint64_t *d_keys, const int32_t *d_fgid,
                                     const uint32_t *d_rowptr, uint32_t R, uint32_t NNZ,
                                     void *stream, const uint64_t **d_id_out) {
  XF_REQUIRE(s && d_id_out, "xf_slices_extract_dev: null argument");
  XF_REQUIRE(NNZ == 0 || (d_keys && d_fgid),
             "xf_slices_extract_dev: %u nonzeros need keys and field ids (d_keys or d_fgid is "
             "NULL)", NNZ);
  XF_REQUIRE(R == 0 || d_rowptr, "xf_slices_extract_dev: %u rows without row offsets", R);
  XF_REQUIRE(R < 0xFFFFFF00u, "xf_slices_extract_dev: a minibatch of %u rows is too large", R);
  XF_TRY(sl_grow(&s->id, &s->cap_id, R));
  *d_id_out = s->id;
  if (R == 0) return XF_OK;
  hipLaunchKernelGGL(k_sl_extract, dim3((R + kSxRows - 1) / kSxRows), dim3(kSlThreads), 0,
                     (hipStream_t)stream, d_keys, d_fgid, d_rowptr, R, NNZ, s->F, s->id);
  XF_HIP(hipGetLastError());
  return XF_OK;
}

extern "C" int xf_slices_extract(xf_slices *s, const uint64_t *rowptr, const uint64_t *keys,
                                 const int32_t *fgid, size_t row_begin, size_t row_end,
                                 void *stream, const uint64_t **d_id_out, uint32_t *R_out) {
  XF_REQUIRE(s && rowptr && d_id_out && R_out && row_begin <= row_end,
             "xf_slices_extract: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t R = row_end - row_begin;
  const uint64_t base = rowptr[row_begin];
  XF_REQUIRE(rowptr[row_end] >= base, "xf_slices_extract: row offsets descend");
  const uint64_t nnz = rowptr[row_end] - base;
  XF_REQUIRE(R < 0xFFFFFF00ull && nnz < 0xFFFFE000ull,
             "xf_slices_extract: a minibatch of %zu rows, %llu nonzeros is too large", R,
             (unsigned long long)nnz);
  XF_REQUIRE(nnz == 0 || (keys && fgid),
             "xf_slices_extract: %llu nonzeros need keys and field ids (keys or fgid is NULL)",
             (unsigned long long)nnz);
  s->h_rowptr.resize(R + 1);
  for (size_t r = 0; r <= R; ++r) {
    const uint64_t at = rowptr[row_begin + r];
    XF_REQUIRE(at >= base && at - base <= nnz && (r == 0 || at - base >= s->h_rowptr[r - 1]),
               "xf_slices_extract: row offsets descend at row %zu", row_begin + r);
    s->h_rowptr[r] = (uint32_t)(at - base);
  }
  XF_TRY(sl_grow(&s->u_rowptr, &s->ucap_rowptr, R + 1));
  XF_TRY(sl_grow(&s->u_keys, &s->ucap_keys, (size_t)nnz));
  XF_TRY(sl_grow(&s->u_fgid, &s->ucap_fgid, (size_t)nnz));
  XF_HIP(hipMemcpyAsync(s->u_rowptr, s->h_rowptr.data(), (R + 1) * 4, hipMemcpyHostToDevice, st));
  if (nnz) {
    XF_HIP(hipMemcpyAsync(s->u_keys, keys + base, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    XF_HIP(hipMemcpyAsync(s->u_fgid, fgid + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  // (the host arrays may be pageable: the copies above have read them when they return)
  *R_out = (uint32_t)R;
  return xf_slices_extract_dev(s, s->u_keys, s->u_fgid, s->u_rowptr, (uint32_t)R, (uint32_t)nnz,
                               stream, d_id_out);
}

extern "C" int xf_slices_accumulate_dev(xf_slices *s, const float *d_loss,
                                        const int32_t *d_labels, const uint64_t *d_id, uint32_t R,
                                        void *stream) {
  XF_REQUIRE(s, "xf_slices_accumulate_dev: null slices");
  XF_REQUIRE(R == 0 || (d_loss && d_labels && d_id), "xf_slices_accumulate_dev: null argument");
  return xf::slices_accumulate(s, d_loss, d_labels, d_id, R, (hipStream_t)stream);
}

extern "C" int xf_slices_read(xf_slices *s, uint64_t *entries, uint64_t cap, uint64_t *n,
                              uint64_t *none, uint64_t *overflow, int reset) {
  XF_REQUIRE(s && n, "xf_slices_read: null argument");
  XF_REQUIRE(entries || !reset,
             "xf_slices_read: a read without entries only counts them and cannot reset");
  const uint64_t slots = 1ull << s->b;
  if (!entries) cap = 0;
  if (cap > slots) cap = slots;
  hipStream_t st = s->last;
  XF_TRY(sl_grow(&s->dense, &s->cap_dense, (size_t)cap * kSlEntry));
  XF_HIP(hipMemsetAsync(s->count, 0, 8, st));
  const uint64_t groups = (slots + kSlThreads - 1) / kSlThreads;
  hipLaunchKernelGGL(k_sl_export, dim3((uint32_t)std::min<uint64_t>(groups, 4096)),
                     dim3(kSlThreads), 0, st, (const u64 *)s->e, slots, s->dense, cap, s->count);
  XF_HIP(hipGetLastError());
  u64 got = 0;
  XF_HIP(hipMemcpyAsync(&got, s->count, 8, hipMemcpyDeviceToHost, st));
  if (none)
    XF_HIP(hipMemcpyAsync(none, s->e + slots * kSlEntry + 1, kSlW * 8, hipMemcpyDeviceToHost, st));
  if (overflow)
    XF_HIP(hipMemcpyAsync(overflow, s->e + (slots + 1) * kSlEntry + 1, kSlW * 8,
                          hipMemcpyDeviceToHost, st));
  // (the compacted entries travel before their number is known: `cap` of them)
  if (cap)
    XF_HIP(hipMemcpyAsync(entries, s->dense, (size_t)cap * kSlEntry * 8, hipMemcpyDeviceToHost,
                          st));
  XF_HIP(hipStreamSynchronize(st));  // the one wait
  *n = got;
  if (!entries) return XF_OK;
  XF_REQUIRE(got <= cap,
             "xf_slices_read: %llu occupied entries do not fit an array of %llu; nothing was reset",
             (unsigned long long)got, (unsigned long long)cap);
  if (reset) {  // (only now is it known that nothing is lost: a second, short wait)
    XF_TRY(sl_clear(s, st));
    XF_HIP(hipStreamSynchronize(st));
  }
  struct Entry {
    uint64_t w[kSlEntry];
  };
  Entry *first = reinterpret_cast<Entry *>(entries);
  std::sort(first, first + got, [](const Entry &a, const Entry &b) { return a.w[0] < b.w[0]; });
  return XF_OK;
}
