// xf_progress.hip — progressive validation: the device side only counts.
//
// Every training step writes loss[r] = sigmoid(..) - label for every row between its forward and
// its gradient.  Under the weights the step is about to change that is the example's held-out
// loss (the FTRL paper's progressive validation, VW's "average loss").  A progress object keeps
// counts[class][rank] of the rows' loss ranks (xf_progress.h: one definition for the host and the
// kernel) and other[class]; every floating-point figure is formed on the host from the counts
// (xf_progress_host.cc).  Integer adds only: the counts depend on nothing but the losses and the
// labels — not the launch shape, the arrival order of the atomics, the world size or the ingest
// path — and are compared with ==.  Not in the reference.
//
// Kernel:
//   k_pg_accumulate   kPgRows rows per workgroup, lanes on consecutive rows.  Many rows of a
//                minibatch share few words (a fresh table puts every row on rank C), and adds of
//                every lane to one word are the slowest shape a global atomic has.  So a wave first
//                folds the lanes that share its first row's word into one add of their count, and
//                the workgroup sums in LDS: an open-addressed table of kPgSlots (word + 1, count)
//                pairs, kPgProbe probes, LDS atomics.  After a barrier one relaxed agent-scope
//                64-bit global add per occupied slot.  A row that finds no slot within the probes
//                adds straight to global memory.  No scratch, no spills (tools/spill_check.sh).
#include <hip/hip_runtime.h>

#include <atomic>
#include <new>

#include "xf_common.h"
#include "xf_progress.h"
#include "xflow_amd.h"

namespace {

constexpr int kPgThreads = 256;
constexpr uint32_t kPgPerThread = 4;
constexpr uint32_t kPgRows = kPgThreads * kPgPerThread;  // rows of one workgroup
constexpr uint32_t kPgLog2Slots = 9;
constexpr uint32_t kPgSlots = 1u << kPgLog2Slots;
constexpr uint32_t kPgProbe = 8;
static_assert(kPgSlots % kPgThreads == 0, "the flush walks the slots a thread stride at a time");

__device__ inline void pg_global_add(unsigned long long *__restrict__ words, uint32_t word,
                                     uint32_t n) {
  // (word < kProgressWords by construction: xf::progress_word)
  __hip_atomic_fetch_add(&words[word], (unsigned long long)n, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// key = word + 1 (0: an empty slot)
__device__ inline void pg_add(uint32_t *keys, uint32_t *cnts,
                              unsigned long long *__restrict__ words, uint32_t key, uint32_t n) {
  uint32_t slot = (key * 2654435761u) >> (32 - kPgLog2Slots);
  for (uint32_t i = 0; i < kPgProbe; ++i) {
    const uint32_t prev = atomicCAS(&keys[slot], 0u, key);
    if (prev == 0u || prev == key) {
      atomicAdd(&cnts[slot], n);
      return;
    }
    slot = (slot + 1) & (kPgSlots - 1);
  }
  pg_global_add(words, key - 1, n);
}

__global__ __launch_bounds__(kPgThreads) void k_pg_accumulate(
    const float *__restrict__ loss, const int32_t *__restrict__ labels, uint32_t R,
    unsigned long long *__restrict__ words) {
  __shared__ uint32_t keys[kPgSlots], cnts[kPgSlots];
  const uint32_t t = threadIdx.x, lane = t & 63;
  for (uint32_t i = t; i < kPgSlots; i += kPgThreads) {
    keys[i] = 0;
    cnts[i] = 0;
  }
  __syncthreads();
  const uint64_t r0 = (uint64_t)blockIdx.x * kPgRows;
#pragma unroll
  for (uint32_t i = 0; i < kPgPerThread; ++i) {
    const uint64_t r = r0 + i * kPgThreads + t;
    const uint32_t key = r < R ? xf::progress_word(loss[r], labels[r]) + 1u : 0u;
    const uint64_t valid = __ballot(key != 0u);
    if (valid == 0) continue;  // (uniform over the wave)
    const int leader = __ffsll((unsigned long long)valid) - 1;
    const uint32_t lkey = __shfl(key, leader, 64);
    const uint64_t same = __ballot(key == lkey);
    if (lane == (uint32_t)leader) pg_add(keys, cnts, words, key, (uint32_t)__popcll(same));
    else if (key != 0u && key != lkey)
      pg_add(keys, cnts, words, key, 1u);
  }
  __syncthreads();
  for (uint32_t i = t; i < kPgSlots; i += kPgThreads)
    if (cnts[i]) pg_global_add(words, keys[i] - 1, cnts[i]);
}

}  // namespace

struct xf_progress {
  unsigned long long *words = nullptr;  // counts[2][RANKS], other[2]
  hipStream_t last = nullptr;           // the stream of the last accumulate
};

static std::atomic<uint64_t> g_pg_launches{0};

int xf::progress_accumulate(xf_progress *p, const float *loss, const int32_t *labels, uint32_t R,
                            hipStream_t s) {
  XF_REQUIRE(p, "progress_accumulate: null progress");
  if (R == 0) return XF_OK;
  XF_REQUIRE(loss && labels, "progress_accumulate: null argument");
  hipLaunchKernelGGL(k_pg_accumulate, dim3((uint32_t)(((uint64_t)R + kPgRows - 1) / kPgRows)), dim3(kPgThreads), 0, s,
                     loss, labels, R, p->words);
  XF_HIP(hipGetLastError());
  p->last = s;
  g_pg_launches.fetch_add(1, std::memory_order_relaxed);
  return XF_OK;
}

extern "C" uint64_t xf_progress_launches(void) {
  return g_pg_launches.load(std::memory_order_relaxed);
}

extern "C" void xf_progress_shape(uint32_t out[3]) {
  out[0] = kPgRows;
  out[1] = kPgSlots;
  out[2] = kPgProbe;
}

extern "C" int xf_progress_create(xf_progress **out) {
  XF_REQUIRE(out, "xf_progress_create: null argument");
  *out = nullptr;
  xf_progress *p = new (std::nothrow) xf_progress;
  XF_REQUIRE(p, "xf_progress_create: out of memory");
  hipError_t e = hipMalloc((void **)&p->words, (size_t)xf::kProgressWords * 8);
  if (e == hipSuccess) e = hipMemset(p->words, 0, (size_t)xf::kProgressWords * 8);
  if (e != hipSuccess) {
    if (p->words) (void)hipFree(p->words);
    delete p;
    XF_HIP(e);
  }
  *out = p;
  return XF_OK;
}

extern "C" int xf_progress_destroy(xf_progress *p) {
  if (!p) return XF_OK;
  if (p->words && !xf::device_poisoned()) (void)hipFree(p->words);
  delete p;
  return XF_OK;
}

extern "C" int xf_progress_accumulate_dev(xf_progress *p, const float *d_loss,
                                          const int32_t *d_labels, uint32_t R, void *stream) {
  XF_REQUIRE(p, "xf_progress_accumulate_dev: null progress");
  XF_REQUIRE(R == 0 || (d_loss && d_labels), "xf_progress_accumulate_dev: null argument");
  return xf::progress_accumulate(p, d_loss, d_labels, R, (hipStream_t)stream);
}

extern "C" int xf_progress_read(xf_progress *p, uint64_t *counts, uint64_t *other, int reset) {
  XF_REQUIRE(p && counts && other, "xf_progress_read: null argument");
  const size_t nc = 2 * (size_t)XF_PROGRESS_RANKS;
  XF_HIP(hipMemcpyAsync(counts, p->words, nc * 8, hipMemcpyDeviceToHost, p->last));
  XF_HIP(hipMemcpyAsync(other, p->words + nc, 2 * 8, hipMemcpyDeviceToHost, p->last));
  if (reset) XF_HIP(hipMemsetAsync(p->words, 0, (size_t)xf::kProgressWords * 8, p->last));
  XF_HIP(hipStreamSynchronize(p->last));
  return XF_OK;
}
