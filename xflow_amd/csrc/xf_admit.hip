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
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <vector>

#include "xf_admit.h"
#include "xf_common.h"

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
};

extern "C" int xf_admit_destroy(xf_admit *a) {
  if (!a) return XF_OK;
  if (!xf::device_poisoned()) {
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)a->d_ctr, (void *)a->o_keys, (void *)a->o_fgid, (void *)a->o_vals,
                    (void *)a->o_rowptr, (void *)a->flags, (void *)a->pos, (void *)a->tile_cnt,
                    (void *)a->tile_off, (void *)a->scan_tmp, (void *)a->u_keys,
                    (void *)a->u_fgid, (void *)a->u_labels, (void *)a->u_vals,
                    (void *)a->u_rowptr})
      if (p) (void)hipFree(p);
    if (a->h_total) (void)hipHostFree(a->h_total);
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
  for (int j = 0; j < kMaxHashes; ++j) a->salts.s[j] = xf::admit_salt(seed, j);
  const size_t bytes = (size_t)1 << log2_slots;
  XF_HIP(hipMalloc((void **)&a->d_ctr, bytes));
  XF_HIP(hipMemset(a->d_ctr, 0, bytes));
  XF_HIP(hipHostMalloc((void **)&a->h_total, sizeof(uint32_t)));
  guard.a = nullptr;
  *out = a;
  return XF_OK;
}

extern "C" int xf_admit_apply_dev(xf_admit *a, int update, const uint64_t *d_keys,
                                  const int32_t *d_fgid, const float *d_vals,
                                  const uint32_t *d_rowptr, uint32_t R, uint32_t NNZ, void *stream,
                                  const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                                  const float **d_vals_out, const uint32_t **d_rowptr_out,
                                  uint32_t *NNZ_out) {
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

extern "C" int xf_admit_apply(xf_admit *a, int update, const uint64_t *rowptr,
                              const uint64_t *keys, const int32_t *fgid, const float *vals,
                              const int32_t *labels, size_t row_begin, size_t row_end,
                              void *stream, const uint64_t **d_keys_out,
                              const int32_t **d_fgid_out, const float **d_vals_out,
                              const uint32_t **d_rowptr_out, const int32_t **d_labels_out,
                              uint32_t *R_out, uint32_t *NNZ_out) {
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
  hipStream_t s = (hipStream_t)stream;
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
  if (d_labels_out) *d_labels_out = labels ? a->u_labels : nullptr;
  if (R_out) *R_out = (uint32_t)R;
  // (the host arrays may be pageable: the copies above have read them when they return; the
  // vector of rebased offsets lives until the next call)
  return xf_admit_apply_dev(a, update, a->u_keys, fgid ? a->u_fgid : nullptr,
                            vals ? a->u_vals : nullptr, a->u_rowptr, (uint32_t)R, (uint32_t)nnz,
                            stream, d_keys_out, d_fgid_out, d_vals_out, d_rowptr_out, NNZ_out);
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
  XF_HIP(hipMemcpy(counters, a->d_ctr, (size_t)1 << a->p.L, hipMemcpyDeviceToHost));
  return XF_OK;
}

extern "C" int xf_admit_import(xf_admit *a, const uint8_t *counters) {
  XF_REQUIRE(a && counters, "xf_admit_import: null argument");
  const size_t n = (size_t)1 << a->p.L;
  for (size_t i = 0; i < n; ++i)
    XF_REQUIRE(counters[i] <= (uint32_t)a->p.N,
               "xf_admit_import: counter %zu holds %u, above admit_count=%d", i,
               (unsigned)counters[i], a->p.N);
  XF_HIP(hipDeviceSynchronize());
  XF_HIP(hipMemcpy(a->d_ctr, counters, n, hipMemcpyHostToDevice));
  return XF_OK;
}

extern "C" int xf_admit_save(xf_admit *a, const char *path) {
  XF_REQUIRE(a && path, "xf_admit_save: null argument");
  std::vector<uint8_t> c((size_t)1 << a->p.L);
  XF_TRY(xf_admit_export(a, c.data()));
  return xf::admit_file_write(path, a->p, c.data());
}

extern "C" int xf_admit_load(xf_admit *a, const char *path) {
  XF_REQUIRE(a && path, "xf_admit_load: null argument");
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
