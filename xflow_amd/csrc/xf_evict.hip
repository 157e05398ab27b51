// xf_evict.hip — table eviction: the kernels that judge the rows of a settled FTRL table of dim 1
// and compact the survivors (xf_table_evict, xf_table.hip, is the host side: it owns the tiers
// and the two state buffers).  Not in the reference: its std::unordered_map only grows (ftrl.h:84).
//
// A row is DROPPED iff  w == 0.0f (either sign of zero)  and  n < n_below,  n the row's
// accumulated sum of squared gradients; a NaN n compares false and is kept.  A settled table has
// key r in state row r, so the pass is a stable stream compaction of three parallel arrays
// (bkeys, w, nz) by one predicate.  Three launches, none of which waits for another workgroup:
//   k_ev_mark     one workgroup per block of kEvBlock consecutive rows: w and nz read coalesced,
//                 the keep predicate as one __ballot word per wavefront and 64 rows — the bit
//                 mask, n / 8 bytes — and the block's survivor count
//   k_ev_scan     the block counts -> where every block's survivors go (one workgroup that walks
//                 the counts kEvThreads at a time with a carry: any number of blocks)
//   k_ev_compact  the same blocks read their 64 mask words; a survivor's rank = the block's base
//                 (the scan) + the popcounts of the words before its own (a wave scan, kept in
//                 LDS) + mbcnt of its own word; key, w and nz move to that rank.  Stable, so the
//                 keys stay sorted and a block writes one contiguous span.  No row list exists.
// Bytes (DESIGN 3 "Eviction"): mark reads 12 per row and writes 1/8; compact reads 1/8 per row and
// moves 20 per survivor (read + write: 40).  No scratch, no spills (tools/spill_check.sh).
#include <hip/hip_runtime.h>

#include "xf_common.h"
#include "xf_evict.h"
#include "xflow_amd.h"

namespace {

constexpr int kEvThreads = 256;
constexpr uint32_t kEvWaves = kEvThreads / 64;
constexpr uint32_t kEvBlock = 4096;                    // rows of one workgroup
constexpr uint32_t kEvWords = kEvBlock / 64;           // mask words of one workgroup
constexpr uint32_t kEvPasses = kEvBlock / kEvThreads;  // rows per thread
static_assert(kEvWords == 64, "one wavefront scans a block's mask words, a word per lane");

__global__ void __launch_bounds__(kEvThreads)
k_ev_mark(const float *__restrict__ w, const float2 *__restrict__ nz, size_t n, float n_below,
          unsigned long long *__restrict__ mask /* [blocks * kEvWords] */,
          uint32_t *__restrict__ cnt /* [blocks + 1] */) {
  __shared__ uint32_t wsum[kEvWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const size_t r0 = (size_t)blockIdx.x * kEvBlock;
  uint32_t kept = 0;  // (wave-uniform)
#pragma unroll
  for (uint32_t p = 0; p < kEvPasses; ++p) {
    const size_t r = r0 + (size_t)p * kEvThreads + tid;
    bool keep = false;
    if (r < n) {
      const float wr = w[r];
      const float nr = nz[r].x;
      keep = !(wr == 0.0f && nr < n_below);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) mask[(size_t)blockIdx.x * kEvWords + p * kEvWaves + wave] = m;
    kept += (uint32_t)__popcll(m);
  }
  if (lane == 0) wsum[wave] = kept;
  __syncthreads();
  if (tid == 0) {
    uint32_t total = 0;
    for (uint32_t v = 0; v < kEvWaves; ++v) total += wsum[v];
    cnt[blockIdx.x] = total;
  }
}

// cnt[0 .. n) -> its exclusive scan in place, the total in cnt[n]
__global__ void __launch_bounds__(kEvThreads)
k_ev_scan(uint32_t *__restrict__ cnt, uint32_t n) {
  __shared__ uint32_t wsum[kEvWaves];
  __shared__ uint32_t carry_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += kEvThreads) {  // workgroup-uniform
    const uint32_t i = base + tid;
    const uint32_t x = i < n ? cnt[i] : 0u;
    uint32_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o);
      if ((int)lane >= o) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t pre = carry_s;
    for (uint32_t v = 0; v < wave; ++v) pre += wsum[v];
    if (i < n) cnt[i] = pre + inc - x;
    __syncthreads();
    if (tid == kEvThreads - 1) carry_s = pre + inc;
    __syncthreads();
  }
  if (tid == 0) cnt[n] = carry_s;
}

__global__ void __launch_bounds__(kEvThreads)
k_ev_compact(const uint64_t *__restrict__ keys, const float *__restrict__ w,
             const float2 *__restrict__ nz, const unsigned long long *__restrict__ mask,
             const uint32_t *__restrict__ base, uint64_t *__restrict__ out_keys,
             float *__restrict__ w2, float2 *__restrict__ nz2) {
  __shared__ unsigned long long words[kEvWords];
  __shared__ uint32_t before[kEvWords];  // survivors of the block in the words before this one
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t at = base[blockIdx.x];
  if (base[blockIdx.x + 1] == at) return;  // (workgroup-uniform: every row of the block goes)
  if (wave == 0) {
    const unsigned long long m = mask[(size_t)blockIdx.x * kEvWords + lane];
    const uint32_t x = (uint32_t)__popcll(m);
    uint32_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o);
      if ((int)lane >= o) inc += y;
    }
    words[lane] = m;
    before[lane] = inc - x;
  }
  __syncthreads();
  const size_t r0 = (size_t)blockIdx.x * kEvBlock;
#pragma unroll
  for (uint32_t p = 0; p < kEvPasses; ++p) {
    const uint32_t j = p * kEvWaves + wave;
    const unsigned long long m = words[j];
    // (a set bit is a row below the table's count: k_ev_mark set none for the others)
    if ((m >> lane) & 1ull) {
      const uint32_t below = __builtin_amdgcn_mbcnt_hi(
          (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const size_t r = r0 + (size_t)p * kEvThreads + tid;
      const size_t o = (size_t)at + before[j] + below;
      out_keys[o] = keys[r];
      w2[o] = w[r];
      nz2[o] = nz[r];
    }
  }
}

}  // namespace

namespace xf {

size_t evict_blocks(size_t n) { return (n + kEvBlock - 1) / kEvBlock; }
size_t evict_mask_words(size_t n) { return evict_blocks(n) * kEvWords; }

int evict_mark_scan(const float *w, const float2 *nz, size_t n, float n_below,
                    unsigned long long *mask, uint32_t *cnt, hipStream_t s) {
  const size_t blocks = evict_blocks(n);
  XF_REQUIRE(n > 0 && blocks < 0x7FFFFFFFull, "evict: %zu rows in one pass", n);
  hipLaunchKernelGGL(k_ev_mark, dim3((unsigned)blocks), dim3(kEvThreads), 0, s, w, nz, n, n_below,
                     mask, cnt);
  hipLaunchKernelGGL(k_ev_scan, dim3(1), dim3(kEvThreads), 0, s, cnt, (uint32_t)blocks);
  XF_HIP(hipGetLastError());
  return XF_OK;
}

int evict_compact(const uint64_t *keys, const float *w, const float2 *nz, size_t n,
                  const unsigned long long *mask, const uint32_t *base, uint64_t *out_keys,
                  float *w2, float2 *nz2, hipStream_t s) {
  hipLaunchKernelGGL(k_ev_compact, dim3((unsigned)evict_blocks(n)), dim3(kEvThreads), 0, s, keys, w,
                     nz, mask, base, out_keys, w2, nz2);
  XF_HIP(hipGetLastError());
  return XF_OK;
}

}  // namespace xf

extern "C" void xf_evict_shape(uint32_t out[2]) {
  out[0] = kEvBlock;
  out[1] = 64;
}
