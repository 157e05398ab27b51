// xf_bin.hip — value binning: a GPU stage ahead of the cross (bin=F:n,...).
//
// A count or price field enters w.x and the FM pair terms raw: one weight has to serve the values
// 1 and 40 000.  The stage replaces a listed field's value by the key of the equal-frequency
// bucket it falls into: (key, fgid, val) -> (bin_key(key, fgid, lut[code(val)]), fgid, 1.0f).  The
// buckets are learned from the data: a histogram pass over the fitted nonzeros (k_bin_count), a
// cut of the cumulative counts on the host (xf_bin_lut_from_counts, once per run) and an
// elementwise rewrite (k_bin_apply).  Everything is integer-exact; the definition is xf_bin.h's,
// one for the host and the kernels.  Not in the reference.
//
// k_bin_count (1024 threads; a workgroup walks tiles of 4096 nonzeros, the grid strides):
//   one streaming pass over (fgid, vals), 8 bytes a nonzero.  The histograms are privatised in
//   LDS, 4096 32-bit counters = 16 KiB per listed field; a workgroup owns a group of up to
//   kBinGroup = 8 fields (128 KiB + the 2 KiB slot table) and blockIdx.y walks the groups of a
//   longer spec over the same stream.  fgid -> slot through an open-addressing table of 256
//   entries in LDS.  Numeric fields pile onto a few codes (0, 1, 2, ...), so lanes of a wave that
//   hold the same (slot, code) are combined before the add: up to kBinCombineRounds times the
//   first pending lane's value is broadcast, the lanes that hold it are balloted and that lane
//   adds their number; what is still pending after the rounds is spread over many counters and
//   adds 1 each.  A 32-bit counter cannot wrap: a workgroup counts at most NNZ < 2^32 nonzeros.
//   At the end only the nonzero counters go to the 64-bit totals, by 64-bit atomic adds.
// k_bin_apply (256 threads, tiles of 1024 nonzeros):
//   one streaming pass over (keys, fgid, vals) to new keys and vals, 16 bytes read and 12 written
//   a nonzero; the inputs are never written.  The byte LUTs (4 KiB a field, 256 KiB at most) are
//   read from global memory, where they stay cache-resident; the slot table is in LDS.
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "xf_bin.h"
#include "xf_common.h"
#include "xf_rownorm.h"  // rownorm_check_slice: the check of a row slice's offsets
#include "xflow_amd.h"

namespace {

using xf::kBinCodes;
using xf::kBinGroup;
using xf::kBinTable;
constexpr uint32_t kBinCombineRounds = 4;
constexpr uint32_t kBinNone = 0xffffffffu;
// the count of binned nonzeros is spread over counters on cache lines of their own (xf_rownorm.hip)
constexpr uint32_t kBinSlots = 256, kBinSlotStride = 16;
constexpr size_t kBinTableBytes = 2 * kBinTable * sizeof(int32_t);
constexpr size_t kBinCountLdsMax = kBinTableBytes + (size_t)kBinGroup * kBinCodes * 4;
#ifdef XF_EXPERIMENTS
constexpr uint32_t kBinApplyLdsFields = 32;  // 128 KiB of LUTs beside the slot table
#endif

std::atomic<uint64_t> g_launches{0};

// the slot of field f (its index in the spec), -1: not listed.  tf / ts: the table in LDS
__device__ __forceinline__ int32_t bin_slot(const int32_t *tf, const int32_t *ts, int32_t f) {
  uint32_t h = xf::bin_table_home(f);
  for (;;) {
    const int32_t at = tf[h];
    if (at == f) return ts[h];  // (f = -1 meets an empty entry: ts is -1 there)
    if (at < 0) return -1;
    h = (h + 1) & (kBinTable - 1);
  }
}

// hist[b] += 1 for every lane whose b is not kBinNone, equal b's of a wave combined
__device__ __forceinline__ void bin_combine_add(uint32_t *hist, uint32_t b, uint32_t lane) {
  bool pending = b != kBinNone;
  unsigned long long active = __ballot(pending);
  for (uint32_t round = 0; round < kBinCombineRounds && active; ++round) {  // (wave-uniform)
    const int leader = __ffsll(active) - 1;
    const uint32_t lb = (uint32_t)__shfl((int)b, leader, 64);
    const bool mine = pending && b == lb;
    const unsigned long long same = __ballot(mine);
    if ((int)lane == leader) atomicAdd(hist + lb, (uint32_t)__popcll(same));
    if (mine) pending = false;
    active &= ~same;
  }
  if (pending) atomicAdd(hist + b, 1u);
}

// totals[(slot * 4096) + code] += the nonzeros i < NNZ with fgid[i] = the slot's field and
// code(vals[i]) = code, for the slots of group blockIdx.y.  tab: tf[256] then ts[256].
__global__ __launch_bounds__(xf::kBinCountThreads) void k_bin_count(
    const int32_t *__restrict__ fgid, const float *__restrict__ vals, uint32_t NNZ, uint32_t ntiles,
    const int32_t *__restrict__ tab, uint32_t n, unsigned long long *totals) {
  extern __shared__ uint32_t bin_lds[];
  const int32_t *tf = (const int32_t *)bin_lds, *ts = tf + kBinTable;
  uint32_t *hist = bin_lds + 2 * kBinTable;
  const uint32_t t = threadIdx.x, lane = t & 63;
  const uint32_t first = blockIdx.y * kBinGroup;
  const uint32_t gs = n - first < kBinGroup ? n - first : kBinGroup;  // (the grid has first < n)
  if (t < 2 * kBinTable) bin_lds[t] = (uint32_t)tab[t];
  for (uint32_t i = t; i < gs * kBinCodes; i += xf::kBinCountThreads) hist[i] = 0;
  __syncthreads();
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t base = tile * xf::kBinCountTile + t;  // (NNZ < 2^32 - 8192: no wrap)
    int32_t f[4];
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t i = base + (uint32_t)j * xf::kBinCountThreads;
      f[j] = i < NNZ ? fgid[i] : -1;
      v[j] = i < NNZ ? vals[i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t s = (uint32_t)bin_slot(tf, ts, f[j]) - first;  // (-1 - first: out of range)
      bin_combine_add(hist, s < gs ? s * kBinCodes + xf::bin_code(v[j]) : kBinNone, lane);
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < gs * kBinCodes; i += xf::kBinCountThreads) {
    const uint32_t c = hist[i];
    if (c) atomicAdd(totals + (size_t)first * kBinCodes + i, (unsigned long long)c);
  }
}

// out_keys[i], out_vals[i] = the rewrite of nonzero i; the counters of binned_total (kBinSlots of
// them, kBinSlotStride words apart) together += the nonzeros that were rewritten
// kLds (the measured-and-not-adopted variant, -DXF_EXPERIMENTS; profiles/bin/README.md): the n
// LUTs are staged in dynamic LDS behind the slot table (n <= kBinApplyLdsFields) and gathered there
template <bool kLds>
__global__ __launch_bounds__(xf::kBinApplyThreads) void k_bin_apply(
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ fgid,
    const float *__restrict__ vals, uint32_t NNZ, uint32_t ntiles, const int32_t *__restrict__ tab,
    const uint8_t *__restrict__ lut, uint32_t n, uint64_t *__restrict__ out_keys,
    float *__restrict__ out_vals, unsigned long long *binned_total) {
  extern __shared__ uint32_t bin_lds[];
  int32_t *tbl = (int32_t *)bin_lds;
  const int32_t *tf = tbl, *ts = tbl + kBinTable;
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < 2 * kBinTable; i += xf::kBinApplyThreads) tbl[i] = tab[i];
  if (kLds) {  // (n x 4096 bytes as words: the LUTs are 4 KiB each and hipMalloc-aligned)
    uint32_t *dst = bin_lds + 2 * kBinTable;
    const uint32_t *src = (const uint32_t *)lut;
    for (uint32_t i = t; i < n * (kBinCodes / 4); i += xf::kBinApplyThreads) dst[i] = src[i];
  }
  const uint8_t *lds_lut = (const uint8_t *)(bin_lds + 2 * kBinTable);
  __syncthreads();
  uint32_t binned = 0;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t base = tile * xf::kBinApplyTile + t;
    uint64_t k[4];
    int32_t f[4];
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t i = base + (uint32_t)j * xf::kBinApplyThreads;
      const bool in = i < NNZ;
      k[j] = in ? keys[i] : 0;
      f[j] = in ? fgid[i] : -1;
      v[j] = in ? vals[i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t i = base + (uint32_t)j * xf::kBinApplyThreads;
      if (i >= NNZ) continue;
      const int32_t s = bin_slot(tf, ts, f[j]);
      if (s >= 0) {
        const uint32_t at = (uint32_t)s * kBinCodes + xf::bin_code(v[j]);
        const uint32_t b = kLds ? lds_lut[at] : lut[at];
        k[j] = xf::bin_key(k[j], f[j], b);
        v[j] = 1.0f;
        ++binned;
      }
      out_keys[i] = k[j];
      out_vals[i] = v[j];
    }
  }
  uint32_t c = binned;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) c += __shfl_xor(c, off, 64);
  if ((t & 63) == 0 && c)
    atomicAdd(binned_total + (size_t)((blockIdx.x * 4 + (t >> 6)) & (kBinSlots - 1)) * kBinSlotStride,
              (unsigned long long)c);
}

// zeroes n words (a fresh allocation's first use, in the order of the stream)
__global__ __launch_bounds__(256) void k_bin_zero(unsigned long long *p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    p[i] = 0;
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

struct xf_bin {
  int n = 0;
  int32_t field[xf::kBinMaxFields], bins[xf::kBinMaxFields];
  bool fitted = false;
  uint64_t seen = 0;          // nonzeros through the applies (counted on the host)
  std::vector<uint8_t> lut;   // n x 4096 once fitted
  int32_t *d_tab = nullptr;   // the slot table: tf[256], ts[256]
  unsigned long long *d_counts = nullptr;  // n x 4096 totals (from the first count on)
  uint8_t *d_lut = nullptr;
  unsigned long long *d_binned = nullptr;  // the running counts of binned nonzeros (kBinSlots)
  // the rewritten keys and values (valid until the next apply)
  uint64_t *o_keys = nullptr;
  float *o_vals = nullptr;
  size_t cap_keys = 0, cap_vals = 0;
  // the host entries' copies of the host arrays
  uint64_t *u_keys = nullptr;
  int32_t *u_fgid = nullptr, *u_labels = nullptr;
  float *u_vals = nullptr;
  uint32_t *u_rowptr = nullptr;
  size_t ucap_keys = 0, ucap_fgid = 0, ucap_labels = 0, ucap_vals = 0, ucap_rowptr = 0;
  std::vector<uint32_t> h_rowptr;
};

static int bin_table_on_device(xf_bin *b) {
  if (b->d_tab) return XF_OK;
  int32_t tab[2 * kBinTable];
  xf::bin_build_table(b->field, b->n, tab, tab + kBinTable);
  XF_HIP(hipMalloc((void **)&b->d_tab, sizeof(tab)));
  // (a blocking copy from the stack: it has read `tab` when it returns)
  XF_HIP(hipMemcpy(b->d_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
  return XF_OK;
}

static int bin_lut_on_device(xf_bin *b) {
  if (!b->d_lut) XF_HIP(hipMalloc((void **)&b->d_lut, b->lut.size()));
  XF_HIP(hipMemcpy(b->d_lut, b->lut.data(), b->lut.size(), hipMemcpyHostToDevice));
  return XF_OK;
}

extern "C" int xf_bin_create(xf_bin **out, const int32_t *field, const int32_t *bins, int n) {
  XF_REQUIRE(out, "xf_bin_create: out is NULL");
  *out = nullptr;
  XF_TRY(xf::bin_check_spec("xf_bin_create", field, bins, n));
  xf_bin *b = new xf_bin;
  b->n = n;
  for (int p = 0; p < n; ++p) {
    b->field[p] = field[p];
    b->bins[p] = bins[p];
  }
  // (nothing on the device yet: the first count, fit or apply allocates)
  *out = b;
  return XF_OK;
}

extern "C" int xf_bin_destroy(xf_bin *b) {
  if (!b) return XF_OK;
  if ((b->d_tab || b->d_lut || b->u_rowptr || b->u_fgid) && !xf::device_poisoned()) {
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)b->d_tab, (void *)b->d_counts, (void *)b->d_lut, (void *)b->d_binned,
                    (void *)b->o_keys, (void *)b->o_vals, (void *)b->u_keys, (void *)b->u_fgid,
                    (void *)b->u_labels, (void *)b->u_vals, (void *)b->u_rowptr})
      if (p) (void)hipFree(p);
  }
  delete b;
  return XF_OK;
}

extern "C" int xf_bin_params(const xf_bin *b, int32_t *field, int32_t *bins, int cap, int *n) {
  XF_REQUIRE(b && n, "xf_bin_params: null argument");
  *n = b->n;
  if (!field && !bins) return XF_OK;
  XF_REQUIRE(field && bins && cap >= b->n, "xf_bin_params: the spec holds %d pairs, the arrays %d",
             b->n, cap);
  for (int p = 0; p < b->n; ++p) {
    field[p] = b->field[p];
    bins[p] = b->bins[p];
  }
  return XF_OK;
}

extern "C" uint64_t xf_bin_launches(void) { return g_launches.load(std::memory_order_relaxed); }

extern "C" int xf_bin_count_dev(xf_bin *b, const int32_t *d_fgid, const float *d_vals,
                                uint32_t NNZ, void *stream) {
  XF_REQUIRE(b, "xf_bin_count_dev: the stage is NULL");
  XF_REQUIRE(!b->fitted, "xf_bin_count_dev: the stage is fitted: its buckets are frozen and no "
             "more nonzeros are counted");
  XF_REQUIRE(NNZ == 0 || (d_fgid && d_vals),
             "xf_bin_count_dev: %u nonzeros need field ids (d_fgid) and values (d_vals)", NNZ);
  XF_REQUIRE(NNZ < 0xFFFFE000u, "xf_bin_count_dev: %u nonzeros are too many for one call", NNZ);
  if (NNZ == 0) return XF_OK;  // (nothing is launched)
  hipStream_t st = (hipStream_t)stream;
  XF_TRY(bin_table_on_device(b));
  const size_t words = (size_t)b->n * kBinCodes;
  if (!b->d_counts) {
    XF_HIP(hipMalloc((void **)&b->d_counts, words * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_bin_zero, dim3(64), dim3(256), 0, st, b->d_counts, words);
    XF_HIP(hipGetLastError());
  }
  static std::atomic<bool> attr_done{false};
  if (!attr_done.load(std::memory_order_acquire)) {
    XF_HIP(hipFuncSetAttribute((const void *)k_bin_count, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kBinCountLdsMax));
    attr_done.store(true, std::memory_order_release);
  }
  const uint32_t ntiles = (NNZ + xf::kBinCountTile - 1) / xf::kBinCountTile;
  const uint32_t gx = ntiles < xf::kBinCountMaxGrid ? ntiles : xf::kBinCountMaxGrid;
  const uint32_t groups = ((uint32_t)b->n + kBinGroup - 1) / kBinGroup;
  const uint32_t gs = (uint32_t)b->n < kBinGroup ? (uint32_t)b->n : kBinGroup;
  hipLaunchKernelGGL(k_bin_count, dim3(gx, groups), dim3(xf::kBinCountThreads),
                     kBinTableBytes + (size_t)gs * kBinCodes * 4, st, d_fgid, d_vals, NNZ, ntiles,
                     b->d_tab, (uint32_t)b->n, b->d_counts);
  XF_HIP(hipGetLastError());
  g_launches.fetch_add(1, std::memory_order_relaxed);
  return XF_OK;
}

extern "C" int xf_bin_count(xf_bin *b, const uint64_t *rowptr, const int32_t *fgid,
                            const float *vals, size_t row_begin, size_t row_end, void *stream) {
  XF_REQUIRE(b, "xf_bin_count: the stage is NULL");
  XF_REQUIRE(rowptr, "xf_bin_count: rowptr is NULL");
  XF_REQUIRE(!b->fitted, "xf_bin_count: the stage is fitted: its buckets are frozen and no more "
             "nonzeros are counted");
  uint32_t nnz = 0;
  XF_TRY(xf::rownorm_check_slice("xf_bin_count", rowptr, row_begin, row_end, &b->h_rowptr, &nnz));
  XF_REQUIRE(nnz == 0 || (fgid && vals), "xf_bin_count: %u nonzeros need field ids (fgid) and "
             "values (vals)", nnz);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t base = rowptr[row_begin];
  XF_TRY(grow(&b->u_fgid, &b->ucap_fgid, (size_t)nnz));
  XF_TRY(grow(&b->u_vals, &b->ucap_vals, (size_t)nnz));
  if (nnz) {
    XF_HIP(hipMemcpyAsync(b->u_fgid, fgid + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    XF_HIP(hipMemcpyAsync(b->u_vals, vals + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  return xf_bin_count_dev(b, b->u_fgid, b->u_vals, nnz, stream);
}

extern "C" int xf_bin_counts(const xf_bin *b, uint64_t *count, size_t cap) {
  XF_REQUIRE(b && count, "xf_bin_counts: null argument");
  const size_t words = (size_t)b->n * kBinCodes;
  XF_REQUIRE(cap >= words, "xf_bin_counts: %d fields have %zu counters, the array %zu", b->n, words,
             cap);
  if (!b->d_counts) {  // (nothing was counted)
    for (size_t i = 0; i < words; ++i) count[i] = 0;
    return XF_OK;
  }
  XF_HIP(hipDeviceSynchronize());  // (behind every count's kernel, whatever its stream)
  XF_HIP(hipMemcpy(count, b->d_counts, words * 8, hipMemcpyDeviceToHost));
  return XF_OK;
}

extern "C" int xf_bin_set_lut(xf_bin *b, const uint8_t *lut, size_t bytes) {
  XF_REQUIRE(b && lut, "xf_bin_set_lut: null argument");
  const size_t want = (size_t)b->n * kBinCodes;
  XF_REQUIRE(bytes == want, "xf_bin_set_lut: %d fields have %zu LUT bytes, not %zu", b->n, want,
             bytes);
  for (int p = 0; p < b->n; ++p)
    for (uint32_t c = 0; c < kBinCodes; ++c)
      XF_REQUIRE(lut[(size_t)p * kBinCodes + c] <= b->bins[p],
                 "xf_bin_set_lut: bucket %d at code %u of field %d, which has %d (and NaN's)",
                 (int)lut[(size_t)p * kBinCodes + c], c, b->field[p], b->bins[p]);
  b->lut.assign(lut, lut + want);
  XF_HIP(hipDeviceSynchronize());  // (an apply in flight still reads the LUTs it was given)
  XF_TRY(bin_lut_on_device(b));
  b->fitted = true;
  return XF_OK;
}

extern "C" int xf_bin_fit(xf_bin *b) {
  XF_REQUIRE(b, "xf_bin_fit: the stage is NULL");
  XF_REQUIRE(!b->fitted, "xf_bin_fit: the stage is fitted already");
  std::vector<uint64_t> count((size_t)b->n * kBinCodes);
  XF_TRY(xf_bin_counts(b, count.data(), count.size()));
  std::vector<uint8_t> lut((size_t)b->n * kBinCodes);
  for (int p = 0; p < b->n; ++p)
    XF_TRY(xf_bin_lut_from_counts(count.data() + (size_t)p * kBinCodes, b->bins[p],
                                  lut.data() + (size_t)p * kBinCodes));
  return xf_bin_set_lut(b, lut.data(), lut.size());
}

extern "C" int xf_bin_lut(const xf_bin *b, uint8_t *lut, size_t cap) {
  XF_REQUIRE(b && lut, "xf_bin_lut: null argument");
  XF_REQUIRE(b->fitted, "xf_bin_lut: the stage is not fitted (xf_bin_fit, xf_bin_set_lut or "
             "xf_bin_load first)");
  XF_REQUIRE(cap >= b->lut.size(), "xf_bin_lut: %d fields have %zu LUT bytes, the array %zu", b->n,
             b->lut.size(), cap);
  memcpy(lut, b->lut.data(), b->lut.size());
  return XF_OK;
}

extern "C" int xf_bin_save(const xf_bin *b, const char *path) {
  XF_REQUIRE(b && path, "xf_bin_save: null argument");
  XF_REQUIRE(b->fitted, "xf_bin_save: the stage is not fitted: there are no LUTs to save");
  return xf::bin_file_write(path, b->field, b->bins, b->n, b->lut.data());
}

extern "C" int xf_bin_load(xf_bin *b, const char *path) {
  XF_REQUIRE(b && path, "xf_bin_load: null argument");
  std::vector<uint8_t> lut;
  XF_TRY(xf::bin_file_read(path, b->field, b->bins, b->n, &lut));
  return xf_bin_set_lut(b, lut.data(), lut.size());
}

extern "C" int xf_bin_stats(const xf_bin *b, uint64_t *nonzeros_seen, uint64_t *nonzeros_binned) {
  XF_REQUIRE(b, "xf_bin_stats: the stage is NULL");
  if (nonzeros_seen) *nonzeros_seen = b->seen;
  if (nonzeros_binned) {
    unsigned long long v = 0;
    if (b->d_binned) {  // (behind every apply's kernel, whatever its stream — the one wait)
      std::vector<unsigned long long> h((size_t)kBinSlots * kBinSlotStride);
      XF_HIP(hipDeviceSynchronize());
      XF_HIP(hipMemcpy(h.data(), b->d_binned, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < kBinSlots; ++i) v += h[(size_t)i * kBinSlotStride];
    }
    *nonzeros_binned = (uint64_t)v;
  }
  return XF_OK;
}

extern "C" int xf_bin_apply_dev(xf_bin *b, const uint64_t *d_keys, const int32_t *d_fgid,
                                const float *d_vals, uint32_t NNZ, void *stream,
                                const uint64_t **d_keys_out, const float **d_vals_out) {
  XF_REQUIRE(b, "xf_bin_apply_dev: the stage is NULL");
  XF_REQUIRE(b->fitted, "xf_bin_apply_dev: the stage is not fitted (xf_bin_fit, xf_bin_set_lut or "
             "xf_bin_load first)");
  XF_REQUIRE(d_keys_out && d_vals_out, "xf_bin_apply_dev: a required output (d_keys_out, "
             "d_vals_out) is NULL");
  XF_REQUIRE(NNZ == 0 || (d_keys && d_fgid && d_vals),
             "xf_bin_apply_dev: %u nonzeros need keys (d_keys), field ids (d_fgid) and values "
             "(d_vals)", NNZ);
  XF_REQUIRE(NNZ < 0xFFFFE000u, "xf_bin_apply_dev: a minibatch of %u nonzeros is too large", NNZ);
  hipStream_t st = (hipStream_t)stream;
  XF_TRY(grow(&b->o_keys, &b->cap_keys, (size_t)NNZ));
  XF_TRY(grow(&b->o_vals, &b->cap_vals, (size_t)NNZ));
  *d_keys_out = b->o_keys;
  *d_vals_out = b->o_vals;
  if (NNZ == 0) return XF_OK;  // (no nonzero: nothing is launched)
  XF_TRY(bin_table_on_device(b));
  if (!b->d_binned) {
    const size_t words = (size_t)kBinSlots * kBinSlotStride;
    XF_HIP(hipMalloc((void **)&b->d_binned, words * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_bin_zero, dim3(16), dim3(256), 0, st, b->d_binned, words);
    XF_HIP(hipGetLastError());
  }
  const uint32_t ntiles = (NNZ + xf::kBinApplyTile - 1) / xf::kBinApplyTile;
  const uint32_t grid = ntiles < xf::kBinApplyMaxGrid ? ntiles : xf::kBinApplyMaxGrid;
#ifdef XF_EXPERIMENTS  // exp_knob 410: the LUTs staged in LDS, for the specs that fit
  if (xf::exp_knob() == 410 && (uint32_t)b->n <= kBinApplyLdsFields) {
    static std::atomic<bool> lds_attr_done{false};
    if (!lds_attr_done.load(std::memory_order_acquire)) {
      XF_HIP(hipFuncSetAttribute((const void *)k_bin_apply<true>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(kBinTableBytes + (size_t)kBinApplyLdsFields * kBinCodes)));
      lds_attr_done.store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(k_bin_apply<true>, dim3(grid), dim3(xf::kBinApplyThreads),
                       kBinTableBytes + (size_t)b->n * kBinCodes, st, d_keys, d_fgid, d_vals, NNZ,
                       ntiles, b->d_tab, b->d_lut, (uint32_t)b->n, b->o_keys, b->o_vals,
                       b->d_binned);
  } else
#endif
    hipLaunchKernelGGL(k_bin_apply<false>, dim3(grid), dim3(xf::kBinApplyThreads), kBinTableBytes,
                       st, d_keys, d_fgid, d_vals, NNZ, ntiles, b->d_tab, b->d_lut, (uint32_t)b->n,
                       b->o_keys, b->o_vals, b->d_binned);
  XF_HIP(hipGetLastError());
  g_launches.fetch_add(1, std::memory_order_relaxed);
  b->seen += NNZ;
  return XF_OK;
}

extern "C" int xf_bin_apply(xf_bin *b, const uint64_t *rowptr, const uint64_t *keys,
                            const int32_t *fgid, const float *vals, const int32_t *labels,
                            size_t row_begin, size_t row_end, void *stream,
                            const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                            const float **d_vals_out, const uint32_t **d_rowptr_out,
                            const int32_t **d_labels_out, uint32_t *R_out, uint32_t *NNZ_out) {
  XF_REQUIRE(b, "xf_bin_apply: the stage is NULL");
  XF_REQUIRE(rowptr, "xf_bin_apply: rowptr is NULL");
  XF_REQUIRE(d_keys_out && d_vals_out && d_rowptr_out && R_out && NNZ_out,
             "xf_bin_apply: a required output (d_keys_out, d_vals_out, d_rowptr_out, R_out, "
             "NNZ_out) is NULL");
  XF_REQUIRE(b->fitted, "xf_bin_apply: the stage is not fitted (xf_bin_fit, xf_bin_set_lut or "
             "xf_bin_load first)");
  uint32_t nnz = 0;
  XF_TRY(xf::rownorm_check_slice("xf_bin_apply", rowptr, row_begin, row_end, &b->h_rowptr, &nnz));
  XF_REQUIRE(nnz == 0 || (keys && fgid && vals), "xf_bin_apply: %u nonzeros need keys, field ids "
             "(fgid) and values (vals)", nnz);
  hipStream_t st = (hipStream_t)stream;
  const size_t R = row_end - row_begin;
  const uint64_t base = rowptr[row_begin];
  XF_TRY(grow(&b->u_rowptr, &b->ucap_rowptr, R + 1));
  XF_HIP(hipMemcpyAsync(b->u_rowptr, b->h_rowptr.data(), (R + 1) * 4, hipMemcpyHostToDevice, st));
  XF_TRY(grow(&b->u_keys, &b->ucap_keys, (size_t)nnz));
  XF_TRY(grow(&b->u_fgid, &b->ucap_fgid, (size_t)nnz));
  XF_TRY(grow(&b->u_vals, &b->ucap_vals, (size_t)nnz));
  if (nnz) {
    XF_HIP(hipMemcpyAsync(b->u_keys, keys + base, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    XF_HIP(hipMemcpyAsync(b->u_fgid, fgid + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    XF_HIP(hipMemcpyAsync(b->u_vals, vals + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  XF_TRY(grow(&b->u_labels, &b->ucap_labels, R));
  if (R && labels)
    XF_HIP(hipMemcpyAsync(b->u_labels, labels + row_begin, R * 4, hipMemcpyHostToDevice, st));
  // (the host arrays may be pageable: the copies above have read them when they return; the
  // vector of rebased offsets lives until the next call.  No nonzero: nothing waits, so wait here)
  if (nnz == 0) XF_HIP(hipStreamSynchronize(st));
  *R_out = (uint32_t)R;
  *NNZ_out = nnz;
  if (d_fgid_out) *d_fgid_out = b->u_fgid;
  *d_rowptr_out = b->u_rowptr;
  if (d_labels_out) *d_labels_out = labels ? b->u_labels : nullptr;
  return xf_bin_apply_dev(b, b->u_keys, b->u_fgid, b->u_vals, nnz, stream, d_keys_out, d_vals_out);
}
