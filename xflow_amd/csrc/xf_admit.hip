// xf_admit.hip — feature admission: a counting Bloom filter ahead of the key build.
//
// The table inserts a row for every key a Pull meets (ftrl.h:56).  On a power-law stream most
// keys occur once or twice; the FTRL paper's memory-saving section ("Bloom filter inclusion")
// lets a key into the model only once a counting Bloom filter has seen it N times.  Here that is
// a filter on a minibatch's CSR arrays BEFORE any key build: a nonzero whose key is not admitted
// is taken out of its row, the row keeps its label and its other nonzeros, and everything
// downstream sees an ordinary (smaller) minibatch.  Not in the reference.
//
// State: 2^L saturating 8-bit counters, h slots per key (xf_admit.h), a threshold N.  One call:
//   count   (update != 0)  every nonzero adds 1 to each of its h counters, saturating at N:
//           c[s] = min(N, c_old[s] + #{(nonzero, j) : slot_j(key) = s}) — independent of order
//   test    (a launch of its own: every counter of this minibatch is visible) a nonzero is kept
//           iff all h of its counters read N
//   compact kept nonzeros keep their order; rowptr, fgid and vals follow
//
// Kernels:
//   k_admit_count    a thread per nonzero.  The counters sit four to a 32-bit word, so an
//                    increment is a compare-and-swap on the word (an add would carry into the
//                    neighbour).  A counter that reads N needs no atomic at all: the word is
//                    loaded first and the CAS skipped — a plain load can only be stale towards a
//                    SMALLER count (counters never fall), which costs a CAS that fails and hands
//                    back the fresh word, on which saturation is checked again before any retry.
//                    Every iteration of the loop therefore either ends or follows somebody
//                    else's successful increment; a hot key goes read-only after N occurrences.
//   k_admit_test     a workgroup per tile of kAdmitTile nonzeros, eight consecutive ones per
//                    thread: the h counter bytes of each, one flag byte per nonzero, the tile's
//                    kept count.  (rocPRIM's exclusive scan turns the counts into offsets.)
//   k_admit_scatter  the same tiles: a scan of the flags inside the workgroup gives every kept
//                    nonzero its place (stable), keys / fgid / vals are copied there, and every
//                    nonzero's place-if-kept goes to pos[] ...
//   k_admit_rowptr   ... where rowptr_out[r] = pos[rowptr[r]] reads it: the kept nonzeros in
//                    front of the row.  A row may span many tiles, a tile many rows: neither
//                    kernel knows about rows.
//
// A filter shared by the ranks of a group (xf_admit_create_shared): one logical filter, the
// counters sharded by slot range (xf_admit.h: admit_per).  An apply is collective — the ranks'
// minibatches of one call are counted together, then every rank tests its own — and is one round
// trip around the compaction above:
//   k_admit_route_hist   the owner of every (nonzero, j): per-workgroup counts in LDS, one global
//                        add per workgroup and destination; the host reads the `world` totals
//   k_admit_route_place  32-bit local slots bucketed by owner into the send buffer; where[i*h + j]
//                        is the entry's place (a workgroup reserves its share of every bucket with
//                        one global add; the order inside a bucket is free)
//   all-to-all-v of the slots (4 B), then on the owner:
//   k_admit_count_slots  k_admit_count's load-then-CAS loop on the local counters
//   k_admit_answer       (a launch of its own) a byte per received slot: counter == N
//   all-to-all-v back (1 B), then
//   k_admit_test_answers k_admit_test's tiles: a nonzero's h answers ANDed through where[]; the
//                        same flag words and tile counts — scan, scatter and rowptr run unchanged
// No slot is deduplicated: the contract counts per occurrence.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "xf_admit.h"
#include "xf_common.h"
#include "xflow_amd.h"

namespace {

constexpr int kAdmitThreads = 256;
constexpr int kAdmitPerThread = 8;
constexpr uint32_t kAdmitTile = 2048;  // nonzeros of one workgroup of the test and the scatter
static_assert(kAdmitTile == kAdmitThreads * kAdmitPerThread, "a flag word per thread");
constexpr int kMaxHashes = 8;

struct Salts {
  uint64_t s[kMaxHashes];
};

__global__ __launch_bounds__(256) void k_admit_count(const uint64_t *__restrict__ keys,
                                                      uint32_t nnz, uint32_t *ctr, Salts salts,
                                                      int h, int L, uint32_t N) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += gridDim.x * blockDim.x) {
    const uint64_t key = keys[i];
    for (int j = 0; j < h; ++j) {
      const uint64_t slot = xf::admit_slot_salted(key, salts.s[j], L);
      uint32_t *word = ctr + (slot >> 2);
      const uint32_t shift = (uint32_t)(slot & 3) * 8;
      uint32_t w = *word;  // (may be stale: towards a smaller count only)
      while (((w >> shift) & 0xffu) < N) {
        // the byte is below N <= 255: adding 1 cannot carry into the neighbour
        const uint32_t seen = atomicCAS(word, w, w + (1u << shift));
        if (seen == w) break;
        w = seen;  // the fresh word: somebody else's increment landed in between
      }
    }
  }
}

// flags: a byte per nonzero (1 kept), padded with zeros to whole tiles
__global__ __launch_bounds__(kAdmitThreads) void k_admit_test(
    const uint64_t *__restrict__ keys, uint32_t nnz, const uint8_t *__restrict__ ctr, Salts salts,
    int h, int L, uint32_t N, uint64_t *__restrict__ flags, uint32_t *__restrict__ tile_cnt,
    uint32_t ntiles) {
  __shared__ uint32_t wave_cnt[kAdmitThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x;
  const uint32_t i0 = tile * kAdmitTile + t * kAdmitPerThread;  // (nnz < 2^32 - kAdmitTile)
  uint64_t f = 0;
#pragma unroll
  for (int q = 0; q < kAdmitPerThread; ++q) {
    const uint32_t i = i0 + q;
    if (i < nnz) {
      const uint64_t key = keys[i];
      bool keep = true;
      for (int j = 0; j < h; ++j)
        keep = keep && ctr[xf::admit_slot_salted(key, salts.s[j], L)] == N;
      if (keep) f |= 1ull << (8 * q);
    }
  }
  flags[(size_t)tile * kAdmitThreads + t] = f;
  uint32_t c = (uint32_t)__popcll(f);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((t & 63) == 0) wave_cnt[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kAdmitThreads / 64; ++w) s += wave_cnt[w];
    tile_cnt[tile] = s;
    if (tile == 0) tile_cnt[ntiles] = 0;  // (its exclusive sum is the number of kept nonzeros)
  }
}

__global__ __launch_bounds__(kAdmitThreads) void k_admit_scatter(
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ fgid,
    const float *__restrict__ vals, uint32_t nnz, const uint64_t *__restrict__ flags,
    const uint32_t *__restrict__ tile_off, uint64_t *__restrict__ keys_out,
    int32_t *__restrict__ fgid_out, float *__restrict__ vals_out, uint32_t *__restrict__ pos) {
  __shared__ uint32_t wave_sum[kAdmitThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t i0 = tile * kAdmitTile + t * kAdmitPerThread;
  const uint64_t f = flags[(size_t)tile * kAdmitThreads + t];
  const uint32_t c = (uint32_t)__popcll(f);
  uint32_t incl = c;  // inclusive scan of the wave's counts
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off, 64);
    if (lane >= (uint32_t)off) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t at = tile_off[tile] + incl - c;
  for (uint32_t w = 0; w < wave; ++w) at += wave_sum[w];
#pragma unroll
  for (int q = 0; q < kAdmitPerThread; ++q) {
    const uint32_t i = i0 + q;
    if (i < nnz) {
      pos[i] = at;
      if ((f >> (8 * q)) & 1) {  // (at < the number of kept nonzeros <= nnz)
        keys_out[at] = keys[i];
        if (fgid) fgid_out[at] = fgid[i];
        if (vals) vals_out[at] = vals[i];
        ++at;
      }
    }
  }
}

// rowptr_out[r] = kept nonzeros in front of row r; r == R: all of them.  An offset beyond nnz (a
// caller's broken rowptr) reads nothing out of bounds.
__global__ __launch_bounds__(256) void k_admit_rowptr(const uint32_t *__restrict__ rowptr,
                                                       uint32_t R, uint32_t nnz,
                                                       const uint32_t *__restrict__ pos,
                                                       const uint32_t *__restrict__ total,
                                                       uint32_t *__restrict__ rowptr_out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > R) return;
  const uint32_t at = rowptr[r];
  rowptr_out[r] = at < nnz ? pos[at] : *total;
}

// ---- the kernels of a shared filter
constexpr int kMaxWorld = 256;  // owners of the routing histogram (a workgroup's LDS counts)
constexpr uint32_t kRouteChunk = 256;  // nonzeros of one workgroup's turn

// owner(s) = s / per; per = 2^32 only for L = 32 on one rank, which owns everything
__device__ inline uint32_t owner_of(uint32_t slot, uint64_t per) {
  return (per >> 32) ? 0u : slot / (uint32_t)per;
}

// hist[d] += (nonzero, j) entries whose slot rank d owns
__global__ __launch_bounds__(256) void k_admit_route_hist(const uint64_t *__restrict__ keys,
                                                           uint32_t nnz, Salts salts, int h, int L,
                                                           uint64_t per, int world,
                                                           uint32_t *__restrict__ hist) {
  __shared__ uint32_t cnt[kMaxWorld];
  const uint32_t t = threadIdx.x;
  cnt[t] = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x * blockDim.x + t; i < nnz; i += gridDim.x * blockDim.x) {
    const uint64_t key = keys[i];
    for (int j = 0; j < h; ++j)
      atomicAdd(&cnt[owner_of((uint32_t)xf::admit_slot_salted(key, salts.s[j], L), per)], 1u);
  }
  __syncthreads();
  if (t < (uint32_t)world && cnt[t]) atomicAdd(&hist[t], cnt[t]);
}

// send[bucket of the owner] = the local slot, where[i * h + j] = its place in send.  hist: the
// totals of k_admit_route_hist (bucket d starts at their exclusive sum); cursor: zero on entry
__global__ __launch_bounds__(256) void k_admit_route_place(
    const uint64_t *__restrict__ keys, uint32_t nnz, Salts salts, int h, int L, uint64_t per,
    int world, const uint32_t *__restrict__ hist, uint32_t *__restrict__ cursor,
    uint32_t *__restrict__ send, uint32_t *__restrict__ where) {
  __shared__ uint32_t start[kMaxWorld], cnt[kMaxWorld], base[kMaxWorld];
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    uint32_t at = 0;
    for (int d = 0; d < world; ++d) {
      start[d] = at;
      at += hist[d];
    }
  }
  const uint32_t nchunks = (nnz + kRouteChunk - 1) / kRouteChunk;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    cnt[t] = 0;
    __syncthreads();
    const uint32_t i = c * kRouteChunk + t;
    uint32_t own[kMaxHashes] = {}, local[kMaxHashes] = {}, nth[kMaxHashes] = {};
    const uint64_t key = i < nnz ? keys[i] : 0;
#pragma unroll
    for (int j = 0; j < kMaxHashes; ++j) {
      if (j < h && i < nnz) {
        const uint32_t slot = (uint32_t)xf::admit_slot_salted(key, salts.s[j], L);
        own[j] = owner_of(slot, per);
        local[j] = slot - own[j] * (uint32_t)per;  // (wraps to slot when per = 2^32, owner 0)
        nth[j] = atomicAdd(&cnt[own[j]], 1u);
      }
    }
    __syncthreads();
    if (t < (uint32_t)world) base[t] = start[t] + (cnt[t] ? atomicAdd(&cursor[t], cnt[t]) : 0u);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kMaxHashes; ++j) {
      if (j < h && i < nnz) {
        const uint32_t at = base[own[j]] + nth[j];  // (< the sum of hist = nnz * h)
        send[at] = local[j];
        where[(size_t)i * h + j] = at;
      }
    }
    __syncthreads();  // (base and cnt are rewritten by the next turn)
  }
}

// the count of k_admit_count on slots that arrive as local slot numbers (nlocal of them here)
__global__ __launch_bounds__(256) void k_admit_count_slots(const uint32_t *__restrict__ slots,
                                                            size_t n, uint32_t *ctr,
                                                            uint64_t nlocal, uint32_t N) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t slot = slots[i];
    if (slot >= nlocal) continue;  // (a peer that partitions otherwise: nothing out of bounds)
    uint32_t *word = ctr + (slot >> 2);
    const uint32_t shift = (slot & 3) * 8;
    uint32_t w = *word;  // (may be stale: towards a smaller count only)
    while (((w >> shift) & 0xffu) < N) {
      const uint32_t seen = atomicCAS(word, w, w + (1u << shift));
      if (seen == w) break;
      w = seen;
    }
  }
}

__global__ __launch_bounds__(256) void k_admit_answer(const uint32_t *__restrict__ slots, size_t n,
                                                       const uint8_t *__restrict__ ctr,
                                                       uint64_t nlocal, uint32_t N,
                                                       uint8_t *__restrict__ ans) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t slot = slots[i];
    ans[i] = slot < nlocal && ctr[slot] == N;
  }
}

// k_admit_test with the counters' answers in place of the counters
__global__ __launch_bounds__(kAdmitThreads) void k_admit_test_answers(
    uint32_t nnz, const uint8_t *__restrict__ ans, const uint32_t *__restrict__ where, int h,
    uint64_t *__restrict__ flags, uint32_t *__restrict__ tile_cnt, uint32_t ntiles) {
  __shared__ uint32_t wave_cnt[kAdmitThreads / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x;
  const uint32_t i0 = tile * kAdmitTile + t * kAdmitPerThread;
  uint64_t f = 0;
#pragma unroll
  for (int q = 0; q < kAdmitPerThread; ++q) {
    const uint32_t i = i0 + q;
    if (i < nnz) {
      bool keep = true;
      for (int j = 0; j < h; ++j) keep = keep && ans[where[(size_t)i * h + j]] != 0;
      if (keep) f |= 1ull << (8 * q);
    }
  }
  flags[(size_t)tile * kAdmitThreads + t] = f;
  uint32_t c = (uint32_t)__popcll(f);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((t & 63) == 0) wave_cnt[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kAdmitThreads / 64; ++w) s += wave_cnt[w];
    tile_cnt[tile] = s;
    if (tile == 0) tile_cnt[ntiles] = 0;
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

struct xf_admit {
  xf::AdmitParams p;
  Salts salts;
  uint32_t *d_ctr = nullptr;  // 2^L counter bytes, four to a word
  uint64_t seen = 0, kept = 0;
  // the filtered minibatch (valid until the next apply)
  uint64_t *o_keys = nullptr;
  int32_t *o_fgid = nullptr;
  float *o_vals = nullptr;
  uint32_t *o_rowptr = nullptr;
  size_t cap_keys = 0, cap_fgid = 0, cap_vals = 0, cap_rowptr = 0;
  // scratch of the test and the scatter
  uint64_t *flags = nullptr;
  uint32_t *pos = nullptr, *tile_cnt = nullptr, *tile_off = nullptr;
  size_t cap_flags = 0, cap_pos = 0, cap_tcnt = 0, cap_toff = 0;
  char *scan_tmp = nullptr;
  size_t cap_scan = 0;
  uint32_t *h_total = nullptr;  // pinned
  // xf_admit_apply's copies of the host arrays
  uint64_t *u_keys = nullptr;
  int32_t *u_fgid = nullptr, *u_labels = nullptr;
  float *u_vals = nullptr;
  uint32_t *u_rowptr = nullptr;
  size_t ucap_keys = 0, ucap_fgid = 0, ucap_labels = 0, ucap_vals = 0, ucap_rowptr = 0;
  std::vector<uint32_t> h_rowptr;
  // a shared filter (xf_admit_create_shared on a group): d_ctr holds the slots [first, first + n)
  xf_group *g = nullptr;
  int rank = 0, world = 1;
  uint64_t first = 0, n = 0, per = 0;
  uint32_t *r_hist = nullptr;  // `world` bucket totals + `world` cursors
  uint32_t *r_send = nullptr, *r_where = nullptr, *r_recv = nullptr;
  uint8_t *r_ans_out = nullptr, *r_ans = nullptr;
  size_t cap_send = 0, cap_where = 0, cap_recv = 0, cap_ans_out = 0, cap_ans = 0;
  uint32_t *h_hist = nullptr;  // pinned
  std::vector<uint64_t> msg, all_msg, send_counts, recv_counts;
};

extern "C" int xf_admit_destroy(xf_admit *a) {
  if (!a) return XF_OK;
  if (!xf::device_poisoned()) {
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)a->d_ctr, (void *)a->o_keys, (void *)a->o_fgid, (void *)a->o_vals,
                    (void *)a->o_rowptr, (void *)a->flags, (void *)a->pos, (void *)a->tile_cnt,
                    (void *)a->tile_off, (void *)a->scan_tmp, (void *)a->u_keys,
                    (void *)a->u_fgid, (void *)a->u_labels, (void *)a->u_vals,
                    (void *)a->u_rowptr, (void *)a->r_hist, (void *)a->r_send, (void *)a->r_where,
                    (void *)a->r_recv, (void *)a->r_ans_out, (void *)a->r_ans})
      if (p) (void)hipFree(p);
    if (a->h_total) (void)hipHostFree(a->h_total);
    if (a->h_hist) (void)hipHostFree(a->h_hist);
  }
  delete a;
  return XF_OK;
}

extern "C" int xf_admit_create(xf_admit **out, int log2_slots, int hashes, int count,
                               uint64_t seed) {
  XF_REQUIRE(out, "xf_admit_create: null argument");
  *out = nullptr;
  XF_TRY(xf::admit_check_params("xf_admit_create", log2_slots, hashes, count));
  xf_admit *a = new xf_admit;
  struct Guard {
    xf_admit *a;
    ~Guard() {
      if (a) xf_admit_destroy(a);
    }
  } guard{a};
  a->p.L = log2_slots;
  a->p.h = hashes;
  a->p.N = count;
  a->p.seed = seed;
  a->n = a->per = 1ull << log2_slots;
  for (int j = 0; j < kMaxHashes; ++j) a->salts.s[j] = xf::admit_salt(seed, j);
  const size_t bytes = (size_t)1 << log2_slots;
  XF_HIP(hipMalloc((void **)&a->d_ctr, bytes));
  XF_HIP(hipMemset(a->d_ctr, 0, bytes));
  XF_HIP(hipHostMalloc((void **)&a->h_total, sizeof(uint32_t)));
  guard.a = nullptr;
  *out = a;
  return XF_OK;
}

// ---- a filter shared by the ranks of a group
extern "C" int xf_admit_create_shared(xf_admit **out, xf_group *g, int log2_slots, int hashes,
                                      int count, uint64_t seed) {
  XF_REQUIRE(out, "xf_admit_create_shared: null argument");
  *out = nullptr;
  if (!g) return xf_admit_create(out, log2_slots, hashes, count, seed);
  int rank = 0, world = 1;
  XF_TRY(xf_group_info(g, &rank, &world, nullptr));
  // every rank's parameters, compared before anything is allocated: the ranks agree on the error
  const uint64_t mine[4] = {(uint64_t)(int64_t)log2_slots, (uint64_t)(int64_t)hashes,
                            (uint64_t)(int64_t)count, seed};
  std::vector<uint64_t> all((size_t)world * 4);
  XF_TRY(xf_group_allgather_host(g, mine, sizeof(mine), all.data()));
  for (int r = 0; r < world; ++r)
    XF_REQUIRE(std::equal(mine, mine + 4, all.begin() + (size_t)r * 4),
               "xf_admit_create_shared: rank %d has admit_log2_slots=%lld admit_hashes=%lld "
               "admit_count=%lld seed=%llu, rank %d has admit_log2_slots=%d admit_hashes=%d "
               "admit_count=%d seed=%llu", r, (long long)all[(size_t)r * 4],
               (long long)all[(size_t)r * 4 + 1], (long long)all[(size_t)r * 4 + 2],
               (unsigned long long)all[(size_t)r * 4 + 3], rank, log2_slots, hashes, count,
               (unsigned long long)seed);
  XF_TRY(xf::admit_check_params("xf_admit_create_shared", log2_slots, hashes, count));
  XF_REQUIRE(world <= kMaxWorld, "xf_admit_create_shared: a shared filter routes to at most %d "
             "ranks (the routing histogram of a workgroup), not world %d", kMaxWorld, world);
  xf_admit *a = new xf_admit;
  struct Guard {
    xf_admit *a;
    ~Guard() {
      if (a) xf_admit_destroy(a);
    }
  } guard{a};
  a->p.L = log2_slots;
  a->p.h = hashes;
  a->p.N = count;
  a->p.seed = seed;
  for (int j = 0; j < kMaxHashes; ++j) a->salts.s[j] = xf::admit_salt(seed, j);
  a->g = g;
  a->rank = rank;
  a->world = world;
  a->per = xf::admit_per(log2_slots, world);
  XF_TRY(xf_admit_range(log2_slots, world, rank, &a->first, &a->n));
  // (a rank that owns nothing keeps one zero word: no null counter pointer in any launch)
  const size_t bytes = std::max<size_t>((size_t)a->n, 4);
  XF_HIP(hipMalloc((void **)&a->d_ctr, bytes));
  XF_HIP(hipMemset(a->d_ctr, 0, bytes));
  XF_HIP(hipMalloc((void **)&a->r_hist, (size_t)2 * kMaxWorld * sizeof(uint32_t)));
  XF_HIP(hipHostMalloc((void **)&a->h_total, sizeof(uint32_t)));
  XF_HIP(hipHostMalloc((void **)&a->h_hist, kMaxWorld * sizeof(uint32_t)));
  a->msg.resize((size_t)world + 2);
  a->all_msg.resize((size_t)world * (world + 2));
  a->send_counts.resize(world);
  a->recv_counts.resize(world);
  guard.a = nullptr;
  *out = a;
  return XF_OK;
}

extern "C" int xf_admit_range_of(const xf_admit *a, uint64_t *first, uint64_t *n) {
  XF_REQUIRE(a, "xf_admit_range_of: null argument");
  if (first) *first = a->first;
  if (n) *n = a->n;
  return XF_OK;
}

namespace {

// The first host collective of an apply on a shared filter: every rank's send counts, its `update`
// and whether its own argument checks failed (my_rc; the counts are zero then).  Every rank comes
// back with the same verdict, before any exchange: XF_EINVAL naming the rank.
int shared_agree(xf_admit *a, const char *who, int update, int my_rc) {
  const std::string my_msg = my_rc == XF_OK ? "" : xf_last_error();
  const int W = a->world;
  for (int d = 0; d < W; ++d) a->msg[d] = my_rc == XF_OK ? a->send_counts[d] : 0;
  a->msg[W] = update ? 1 : 0;
  a->msg[W + 1] = my_rc == XF_OK ? 0 : 1;
  XF_TRY(xf_group_allgather_host(a->g, a->msg.data(), a->msg.size() * 8, a->all_msg.data()));
  const size_t stride = (size_t)W + 2;
  for (int r = 0; r < W; ++r)
    if (a->all_msg[r * stride + W + 1]) {
      if (r == a->rank)
        return xf::set_error(XF_EINVAL, "%s: rank %d failed its argument checks: %s", who, r,
                             my_msg.c_str());
      return xf::set_error(XF_EINVAL, "%s: rank %d failed its argument checks (this is rank %d): "
                           "no rank has counted or filtered", who, r, a->rank);
    }
  for (int r = 1; r < W; ++r)
    XF_REQUIRE(a->all_msg[r * stride + W] == a->all_msg[W],
               "%s: rank %d passes update=%d, rank 0 update=%d: one apply on a shared filter takes "
               "the same update on every rank", who, r, (int)a->all_msg[r * stride + W],
               (int)a->all_msg[W]);
  for (int r = 0; r < W; ++r) a->recv_counts[r] = a->all_msg[r * stride + a->rank];
  return XF_OK;
}

int shared_check_args(const xf_admit *a, const uint64_t *d_keys, const uint32_t *d_rowptr,
                      uint32_t R, uint32_t NNZ, const void *k_out, const void *r_out,
                      const void *n_out) {
  XF_REQUIRE(k_out && r_out && n_out, "xf_admit_apply_dev: null argument");
  XF_REQUIRE(NNZ == 0 || (d_keys && d_rowptr && R > 0),
             "xf_admit_apply_dev: %u nonzeros need keys, row offsets and rows (R = %u)", NNZ, R);
  XF_REQUIRE(R == 0 || d_rowptr, "xf_admit_apply_dev: %u rows without row offsets", R);
  XF_REQUIRE(NNZ < 0xFFFFFFFFu - 2 * kAdmitTile && R < 0xFFFFFFFFu - 256,
             "xf_admit_apply_dev: a minibatch of %u rows, %u nonzeros is too large", R, NNZ);
  XF_REQUIRE((uint64_t)NNZ * (uint64_t)a->p.h < (1ull << 32),
             "xf_admit_apply_dev: %u nonzeros x admit_hashes=%d is 2^32 or more slots to route in "
             "one apply on a shared filter", NNZ, a->p.h);
  return XF_OK;
}

// route: the owner of every (nonzero, j), a histogram per destination (-> send_counts), the local
// slots bucketed by owner in r_send, every entry's place in r_where
int shared_route(xf_admit *a, const uint64_t *d_keys, uint32_t NNZ, hipStream_t s) {
  const int W = a->world, h = a->p.h, L = a->p.L;
  const size_t entries = (size_t)NNZ * h;
  XF_TRY(grow(&a->r_send, &a->cap_send, entries));
  XF_TRY(grow(&a->r_where, &a->cap_where, entries));
  XF_HIP(hipMemsetAsync(a->r_hist, 0, (size_t)2 * kMaxWorld * sizeof(uint32_t), s));
  const uint32_t grid = std::min<uint32_t>((NNZ + 255) / 256, 2048);
  hipLaunchKernelGGL(k_admit_route_hist, dim3(grid), dim3(256), 0, s, d_keys, NNZ, a->salts, h, L,
                     a->per, W, a->r_hist);
  XF_HIP(hipGetLastError());
  XF_HIP(hipMemcpyAsync(a->h_hist, a->r_hist, (size_t)W * 4, hipMemcpyDeviceToHost, s));
  // (the placing pass needs the totals on the device only: it runs under the host's read)
  hipLaunchKernelGGL(k_admit_route_place, dim3(grid), dim3(256), 0, s, d_keys, NNZ, a->salts, h, L,
                     a->per, W, (const uint32_t *)a->r_hist, a->r_hist + kMaxWorld, a->r_send,
                     a->r_where);
  XF_HIP(hipGetLastError());
  XF_HIP(hipStreamSynchronize(s));
  for (int d = 0; d < W; ++d) a->send_counts[d] = a->h_hist[d];
  return XF_OK;
}

// xf_admit_apply_dev on a shared filter: collective
int apply_shared(xf_admit *a, int update, const uint64_t *d_keys, const int32_t *d_fgid,
                 const float *d_vals, const uint32_t *d_rowptr, uint32_t R, uint32_t NNZ,
                 hipStream_t s, const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                 const float **d_vals_out, const uint32_t **d_rowptr_out, uint32_t *NNZ_out) {
  const int W = a->world, h = a->p.h;
  const uint32_t N = (uint32_t)a->p.N;
  const size_t entries = (size_t)NNZ * h;
  int rc = shared_check_args(a, d_keys, d_rowptr, R, NNZ, d_keys_out, d_rowptr_out, NNZ_out);
  std::fill(a->send_counts.begin(), a->send_counts.end(), 0);
  if (rc == XF_OK && NNZ) rc = shared_route(a, d_keys, NNZ, s);
  XF_TRY(shared_agree(a, "xf_admit_apply", update, rc));
  // ---- exchange: the slots to their owners, count, answer, the answers back
  size_t got = 0;
  for (int r = 0; r < W; ++r) got += (size_t)a->recv_counts[r];
  XF_TRY(grow(&a->r_send, &a->cap_send, entries));  // (no null buffer with NNZ = 0 either)
  XF_TRY(grow(&a->r_ans, &a->cap_ans, entries));
  XF_TRY(grow(&a->r_recv, &a->cap_recv, got));
  XF_TRY(grow(&a->r_ans_out, &a->cap_ans_out, got));
  XF_TRY(xf_group_alltoallv(a->g, a->r_send, a->send_counts.data(), a->r_recv,
                            a->recv_counts.data(), 4, 0, s));
  if (got) {
    const uint32_t grid = (uint32_t)std::min<size_t>((got + 255) / 256, 2048);
    if (update)
      hipLaunchKernelGGL(k_admit_count_slots, dim3(grid), dim3(256), 0, s,
                         (const uint32_t *)a->r_recv, got, a->d_ctr, a->n, N);
    hipLaunchKernelGGL(k_admit_answer, dim3(grid), dim3(256), 0, s, (const uint32_t *)a->r_recv,
                       got, (const uint8_t *)a->d_ctr, a->n, N, a->r_ans_out);
    XF_HIP(hipGetLastError());
  }
  XF_TRY(xf_group_alltoallv(a->g, a->r_ans_out, a->recv_counts.data(), a->r_ans,
                            a->send_counts.data(), 1, 0, s));
  // ---- test from the answers, then the compaction of every filter
  const uint32_t ntiles = (NNZ + kAdmitTile - 1) / kAdmitTile;
  XF_TRY(grow(&a->o_keys, &a->cap_keys, NNZ));
  if (d_fgid) XF_TRY(grow(&a->o_fgid, &a->cap_fgid, NNZ));
  if (d_vals) XF_TRY(grow(&a->o_vals, &a->cap_vals, NNZ));
  XF_TRY(grow(&a->o_rowptr, &a->cap_rowptr, (size_t)R + 1));
  *d_keys_out = a->o_keys;
  if (d_fgid_out) *d_fgid_out = d_fgid ? a->o_fgid : nullptr;
  if (d_vals_out) *d_vals_out = d_vals ? a->o_vals : nullptr;
  *d_rowptr_out = a->o_rowptr;
  *NNZ_out = 0;
  if (NNZ == 0) {
    XF_HIP(hipMemsetAsync(a->o_rowptr, 0, ((size_t)R + 1) * 4, s));
    XF_HIP(hipStreamSynchronize(s));
    return XF_OK;
  }
  XF_TRY(grow(&a->flags, &a->cap_flags, (size_t)ntiles * kAdmitThreads));
  XF_TRY(grow(&a->pos, &a->cap_pos, NNZ));
  XF_TRY(grow(&a->tile_cnt, &a->cap_tcnt, (size_t)ntiles + 1));
  XF_TRY(grow(&a->tile_off, &a->cap_toff, (size_t)ntiles + 1));
  size_t tb = 0;
  XF_HIP(rocprim::exclusive_scan((void *)nullptr, tb, a->tile_cnt, a->tile_off, 0u,
                                 (size_t)ntiles + 1, rocprim::plus<uint32_t>(), s));
  XF_TRY(grow(&a->scan_tmp, &a->cap_scan, tb));
  hipLaunchKernelGGL(k_admit_test_answers, dim3(ntiles), dim3(kAdmitThreads), 0, s, NNZ,
                     (const uint8_t *)a->r_ans, (const uint32_t *)a->r_where, h, a->flags,
                     a->tile_cnt, ntiles);
  XF_HIP(hipGetLastError());
  XF_HIP(rocprim::exclusive_scan((void *)a->scan_tmp, tb, a->tile_cnt, a->tile_off, 0u,
                                 (size_t)ntiles + 1, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(k_admit_scatter, dim3(ntiles), dim3(kAdmitThreads), 0, s, d_keys, d_fgid,
                     d_vals, NNZ, (const uint64_t *)a->flags, (const uint32_t *)a->tile_off,
                     a->o_keys, a->o_fgid, a->o_vals, a->pos);
  hipLaunchKernelGGL(k_admit_rowptr, dim3(R / 256 + 1), dim3(256), 0, s, d_rowptr, R, NNZ,
                     (const uint32_t *)a->pos, (const uint32_t *)(a->tile_off + ntiles),
                     a->o_rowptr);
  XF_HIP(hipGetLastError());
  XF_HIP(hipMemcpyAsync(a->h_total, a->tile_off + ntiles, 4, hipMemcpyDeviceToHost, s));
  XF_HIP(hipStreamSynchronize(s));
  *NNZ_out = *a->h_total;
  if (update) {
    a->seen += NNZ;
    a->kept += *NNZ_out;
  }
  return XF_OK;
}

}  // namespace

extern "C" int xf_admit_apply_dev(xf_admit *a, int update, const uint64_t *d_keys,
                                  const int32_t *d_fgid, const float *d_vals,
                                  const uint32_t *d_rowptr, uint32_t R, uint32_t NNZ, void *stream,
                                  const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                                  const float **d_vals_out, const uint32_t **d_rowptr_out,
                                  uint32_t *NNZ_out) {
  if (a && a->g)  // a shared filter: collective, argument checks included
    return apply_shared(a, update, d_keys, d_fgid, d_vals, d_rowptr, R, NNZ, (hipStream_t)stream,
                        d_keys_out, d_fgid_out, d_vals_out, d_rowptr_out, NNZ_out);
  XF_REQUIRE(a && d_keys_out && d_rowptr_out && NNZ_out, "xf_admit_apply_dev: null argument");
  XF_REQUIRE(NNZ == 0 || (d_keys && d_rowptr && R > 0),
             "xf_admit_apply_dev: %u nonzeros need keys, row offsets and rows (R = %u)", NNZ, R);
  XF_REQUIRE(R == 0 || d_rowptr, "xf_admit_apply_dev: %u rows without row offsets", R);
  XF_REQUIRE(NNZ < 0xFFFFFFFFu - 2 * kAdmitTile && R < 0xFFFFFFFFu - 256,
             "xf_admit_apply_dev: a minibatch of %u rows, %u nonzeros is too large", R, NNZ);
  hipStream_t s = (hipStream_t)stream;
  const uint32_t ntiles = (NNZ + kAdmitTile - 1) / kAdmitTile;
  XF_TRY(grow(&a->o_keys, &a->cap_keys, NNZ));
  if (d_fgid) XF_TRY(grow(&a->o_fgid, &a->cap_fgid, NNZ));
  if (d_vals) XF_TRY(grow(&a->o_vals, &a->cap_vals, NNZ));
  XF_TRY(grow(&a->o_rowptr, &a->cap_rowptr, (size_t)R + 1));
  *d_keys_out = a->o_keys;
  if (d_fgid_out) *d_fgid_out = d_fgid ? a->o_fgid : nullptr;
  if (d_vals_out) *d_vals_out = d_vals ? a->o_vals : nullptr;
  *d_rowptr_out = a->o_rowptr;
  *NNZ_out = 0;
  if (NNZ == 0) {  // nothing to count, test or move: R + 1 zero offsets
    XF_HIP(hipMemsetAsync(a->o_rowptr, 0, ((size_t)R + 1) * 4, s));
    XF_HIP(hipStreamSynchronize(s));
    return XF_OK;
  }
  XF_TRY(grow(&a->flags, &a->cap_flags, (size_t)ntiles * kAdmitThreads));
  XF_TRY(grow(&a->pos, &a->cap_pos, NNZ));
  XF_TRY(grow(&a->tile_cnt, &a->cap_tcnt, (size_t)ntiles + 1));
  XF_TRY(grow(&a->tile_off, &a->cap_toff, (size_t)ntiles + 1));
  size_t tb = 0;
  XF_HIP(rocprim::exclusive_scan((void *)nullptr, tb, a->tile_cnt, a->tile_off, 0u,
                                 (size_t)ntiles + 1, rocprim::plus<uint32_t>(), s));
  XF_TRY(grow(&a->scan_tmp, &a->cap_scan, tb));
  const uint32_t N = (uint32_t)a->p.N;
  if (update) {
    const uint32_t grid = std::min<uint32_t>((NNZ + 255) / 256, 8192);
    hipLaunchKernelGGL(k_admit_count, dim3(grid), dim3(256), 0, s, d_keys, NNZ, a->d_ctr,
                       a->salts, a->p.h, a->p.L, N);
  }
  hipLaunchKernelGGL(k_admit_test, dim3(ntiles), dim3(kAdmitThreads), 0, s, d_keys, NNZ,
                     (const uint8_t *)a->d_ctr, a->salts, a->p.h, a->p.L, N, a->flags, a->tile_cnt,
                     ntiles);
  XF_HIP(hipGetLastError());
  XF_HIP(rocprim::exclusive_scan((void *)a->scan_tmp, tb, a->tile_cnt, a->tile_off, 0u,
                                 (size_t)ntiles + 1, rocprim::plus<uint32_t>(), s));
  hipLaunchKernelGGL(k_admit_scatter, dim3(ntiles), dim3(kAdmitThreads), 0, s, d_keys, d_fgid,
                     d_vals, NNZ, (const uint64_t *)a->flags, (const uint32_t *)a->tile_off,
                     a->o_keys, a->o_fgid, a->o_vals, a->pos);
  hipLaunchKernelGGL(k_admit_rowptr, dim3(R / 256 + 1), dim3(256), 0, s, d_rowptr, R, NNZ,
                     (const uint32_t *)a->pos, (const uint32_t *)(a->tile_off + ntiles),
                     a->o_rowptr);
  XF_HIP(hipGetLastError());
  XF_HIP(hipMemcpyAsync(a->h_total, a->tile_off + ntiles, 4, hipMemcpyDeviceToHost, s));
  XF_HIP(hipStreamSynchronize(s));
  *NNZ_out = *a->h_total;
  if (update) {
    a->seen += NNZ;
    a->kept += *NNZ_out;
  }
  return XF_OK;
}

// xf_admit_apply's upload of a row slice of the reader's host arrays (rowptr rebased to u32)
static int upload_slice(xf_admit *a, const uint64_t *rowptr, const uint64_t *keys,
                        const int32_t *fgid, const float *vals, const int32_t *labels,
                        size_t row_begin, size_t row_end, hipStream_t s, uint32_t *R_up,
                        uint32_t *NNZ_up) {
  XF_REQUIRE(a && rowptr && row_begin <= row_end, "xf_admit_apply: bad argument");
  const size_t R = row_end - row_begin;
  const uint64_t base = rowptr[row_begin];
  XF_REQUIRE(rowptr[row_end] >= base, "xf_admit_apply: row offsets descend");
  const uint64_t nnz = rowptr[row_end] - base;
  XF_REQUIRE(R < 0xFFFFFF00ull && nnz < 0xFFFFE000ull,
             "xf_admit_apply: a minibatch of %zu rows, %llu nonzeros is too large", R,
             (unsigned long long)nnz);
  XF_REQUIRE(nnz == 0 || keys, "xf_admit_apply: %llu nonzeros without keys",
             (unsigned long long)nnz);
  a->h_rowptr.resize(R + 1);
  for (size_t r = 0; r <= R; ++r) {
    const uint64_t at = rowptr[row_begin + r];
    XF_REQUIRE(at >= base && at - base <= nnz && (r == 0 || at - base >= a->h_rowptr[r - 1]),
               "xf_admit_apply: row offsets descend at row %zu", row_begin + r);
    a->h_rowptr[r] = (uint32_t)(at - base);
  }
  XF_TRY(grow(&a->u_rowptr, &a->ucap_rowptr, R + 1));
  XF_HIP(hipMemcpyAsync(a->u_rowptr, a->h_rowptr.data(), (R + 1) * 4, hipMemcpyHostToDevice, s));
  XF_TRY(grow(&a->u_keys, &a->ucap_keys, (size_t)nnz));
  if (fgid) XF_TRY(grow(&a->u_fgid, &a->ucap_fgid, (size_t)nnz));
  if (vals) XF_TRY(grow(&a->u_vals, &a->ucap_vals, (size_t)nnz));
  if (nnz) {
    XF_HIP(hipMemcpyAsync(a->u_keys, keys + base, (size_t)nnz * 8, hipMemcpyHostToDevice, s));
    if (fgid)
      XF_HIP(hipMemcpyAsync(a->u_fgid, fgid + base, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
    if (vals)
      XF_HIP(hipMemcpyAsync(a->u_vals, vals + base, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
  }
  if (labels) {
    XF_TRY(grow(&a->u_labels, &a->ucap_labels, R));
    if (R)
      XF_HIP(hipMemcpyAsync(a->u_labels, labels + row_begin, R * 4, hipMemcpyHostToDevice, s));
  }
  *R_up = (uint32_t)R;
  *NNZ_up = (uint32_t)nnz;
  return XF_OK;
}

extern "C" int xf_admit_apply(xf_admit *a, int update, const uint64_t *rowptr,
                              const uint64_t *keys, const int32_t *fgid, const float *vals,
                              const int32_t *labels, size_t row_begin, size_t row_end,
                              void *stream, const uint64_t **d_keys_out,
                              const int32_t **d_fgid_out, const float **d_vals_out,
                              const uint32_t **d_rowptr_out, const int32_t **d_labels_out,
                              uint32_t *R_out, uint32_t *NNZ_out) {
  uint32_t R = 0, nnz = 0;
  const int rc = upload_slice(a, rowptr, keys, fgid, vals, labels, row_begin, row_end,
                              (hipStream_t)stream, &R, &nnz);
  // (a shared filter: the other ranks are in this apply — they hear of the failure, nobody waits)
  if (rc != XF_OK && a && a->g) return shared_agree(a, "xf_admit_apply", update, rc);
  XF_TRY(rc);
  if (d_labels_out) *d_labels_out = labels ? a->u_labels : nullptr;
  if (R_out) *R_out = R;
  // (the host arrays may be pageable: the copies above have read them when they return; the
  // vector of rebased offsets lives until the next call)
  return xf_admit_apply_dev(a, update, a->u_keys, fgid ? a->u_fgid : nullptr,
                            vals ? a->u_vals : nullptr, a->u_rowptr, R, nnz, stream, d_keys_out,
                            d_fgid_out, d_vals_out, d_rowptr_out, NNZ_out);
}

extern "C" int xf_admit_params(const xf_admit *a, int *log2_slots, int *hashes, int *count,
                               uint64_t *seed) {
  XF_REQUIRE(a, "xf_admit_params: null argument");
  if (log2_slots) *log2_slots = a->p.L;
  if (hashes) *hashes = a->p.h;
  if (count) *count = a->p.N;
  if (seed) *seed = a->p.seed;
  return XF_OK;
}

extern "C" int xf_admit_export(xf_admit *a, uint8_t *counters) {
  XF_REQUIRE(a && counters, "xf_admit_export: null argument");
  XF_HIP(hipDeviceSynchronize());
  // (a shared filter: this rank's range, a->n of the 2^L — a plain filter's a->n is all of them)
  if (a->n) XF_HIP(hipMemcpy(counters, a->d_ctr, (size_t)a->n, hipMemcpyDeviceToHost));
  return XF_OK;
}

extern "C" int xf_admit_import(xf_admit *a, const uint8_t *counters) {
  XF_REQUIRE(a && counters, "xf_admit_import: null argument");
  const size_t n = (size_t)a->n;  // (a shared filter: this rank's range)
  for (size_t i = 0; i < n; ++i)
    XF_REQUIRE(counters[i] <= (uint32_t)a->p.N,
               "xf_admit_import: counter %zu holds %u, above admit_count=%d", (size_t)a->first + i,
               (unsigned)counters[i], a->p.N);
  XF_HIP(hipDeviceSynchronize());
  if (n) XF_HIP(hipMemcpy(a->d_ctr, counters, n, hipMemcpyHostToDevice));
  return XF_OK;
}

// COLLECTIVE: the ranges go to rank 0 (in rank order: slot order), which writes the file of a
// one-worker filter; every rank returns rank 0's verdict
static int save_shared(xf_admit *a, const char *path) {
  std::vector<uint8_t> mine((size_t)a->n + 1), all;
  XF_TRY(xf_admit_export(a, mine.data()));
  std::vector<uint64_t> sizes(a->world);
  for (int r = 0; r < a->world; ++r) {
    uint64_t first = 0;
    XF_TRY(xf_admit_range(a->p.L, a->world, r, &first, &sizes[r]));
  }
  if (a->rank == 0) all.resize((size_t)1 << a->p.L);
  XF_TRY(xf_group_gatherv_host(a->g, mine.data(), (size_t)a->n, all.data(), sizes.data()));
  int32_t rc = a->rank == 0 ? xf::admit_file_write(path, a->p, all.data()) : XF_OK;
  std::vector<int32_t> rcs(a->world);
  XF_TRY(xf_group_allgather_host(a->g, &rc, 4, rcs.data()));
  if (rcs[0] != XF_OK && a->rank != 0)
    return xf::set_error(rcs[0], "xf_admit_save: rank 0 could not write %s", path);
  return rcs[0];
}

// COLLECTIVE: every rank reads its own range of the file; a refusal on one rank is one on all
static int load_shared(xf_admit *a, const char *path) {
  std::vector<uint8_t> c;
  int32_t rc = xf::admit_file_read_range(path, a->p, a->first, a->n, &c);
  c.resize((size_t)a->n + 1);  // (a rank that owns nothing: no null pointer)
  if (rc == XF_OK) rc = xf_admit_import(a, c.data());
  const std::string my_msg = rc == XF_OK ? "" : xf_last_error();
  std::vector<int32_t> rcs(a->world);
  XF_TRY(xf_group_allgather_host(a->g, &rc, 4, rcs.data()));
  if (rc != XF_OK) return xf::set_error(rc, "%s", my_msg.c_str());
  for (int r = 0; r < a->world; ++r)
    if (rcs[r] != XF_OK)
      return xf::set_error(rcs[r], "xf_admit_load: rank %d could not load its range of %s", r,
                           path);
  return XF_OK;
}

extern "C" int xf_admit_save(xf_admit *a, const char *path) {
  XF_REQUIRE(a && path, "xf_admit_save: null argument");
  if (a->g) return save_shared(a, path);
  std::vector<uint8_t> c((size_t)1 << a->p.L);
  XF_TRY(xf_admit_export(a, c.data()));
  return xf::admit_file_write(path, a->p, c.data());
}

extern "C" int xf_admit_load(xf_admit *a, const char *path) {
  XF_REQUIRE(a && path, "xf_admit_load: null argument");
  if (a->g) return load_shared(a, path);
  std::vector<uint8_t> c;
  XF_TRY(xf::admit_file_read(path, a->p, &c));
  return xf_admit_import(a, c.data());
}

extern "C" int xf_admit_stats(const xf_admit *a, uint64_t *nonzeros_seen,
                              uint64_t *nonzeros_kept) {
  XF_REQUIRE(a, "xf_admit_stats: null argument");
  if (nonzeros_seen) *nonzeros_seen = a->seen;
  if (nonzeros_kept) *nonzeros_kept = a->kept;
  return XF_OK;
}
