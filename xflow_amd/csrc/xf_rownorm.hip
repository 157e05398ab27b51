// xf_rownorm.hip — row normalisation: a GPU stage ahead of the key build (row_norm=l2).
//
// A row of 17 tokens and a row of 39 tokens plus its crosses put very different mass into w.x, and
// more still into the pair terms of FM / field-aware FM.  The stage gives every row of a minibatch
// unit L2 length over the nonzeros the model actually receives: it is the last stage, behind the
// cross (which adds nonzeros) and admission (which removes them).  The definition is xf_rownorm.h's,
// one for the host and the kernel.  Not in the reference.
//
// Like the other stages it works on a minibatch's CSR arrays and keeps no state but its statistics;
// it changes the values only: keys, fgid, offsets and labels stay the caller's arrays.
//
// Kernel k_rn_l2 (a workgroup is 256 threads and owns kRownormRows = 16 consecutive rows at a
// time; the grid strides over the tiles):
//   16 lanes share a row (the click rows hold 17 .. 39 tokens, more with crosses: one to four
//   aligned blocks of 16 positions; 64 lanes would idle for half of every such row).  A block's
//   squares go through a 16-lane xor-butterfly (levels 0 .. 3 of the tree); the block sums go on
//   through the tree as a binary counter whose level l lives in lane l of the group (two registers:
//   levels 0 .. 15 and 16 .. 31), so a row of any length takes the same path and nothing is indexed
//   in registers.  A row of at most four blocks keeps its values in registers between the sum and
//   the scaling (4 bytes read and 4 written per nonzero); a longer row reads them a second time.
//   Every loop is uniform over the 16 lanes of a group, and a shuffle only reads lanes of its own
//   group, so groups of one wave may diverge.  No LDS, no atomics but one per wave for the count
//   of scaled rows, spread over 256 counters on cache lines of their own.
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "xf_common.h"
#include "xf_rownorm.h"
#include "xflow_amd.h"

namespace {

constexpr int kRnThreads = 256;
constexpr uint32_t kRnG = xf::kRownormLanes, kRnW = xf::kRownormRows;
constexpr uint32_t kRnMaxGrid = 4096;
// the count of scaled rows is spread over kRnSlots counters, each on a 128-byte line of its own:
// one counter took every wave's atomic one after the other, 11.5 ns each — 0.19 of the 0.215 ms
// of a 64 MiB block of click rows (profiles/rownorm/README.md)
constexpr uint32_t kRnSlots = 256, kRnSlotStride = 16;
static_assert(kRnG == 16 && kRnG * kRnW == (uint32_t)kRnThreads, "16 lanes a row, 16 rows");

std::atomic<uint64_t> g_launches{0};

// levels 0 .. 3 of the tree over one aligned block of 16 positions: every lane of the group
// returns the block's sum (a + b and b + a are the same bits)
__device__ __forceinline__ double rn_bfly(double v) {
#pragma unroll
  for (int off = 1; off < (int)kRnG; off <<= 1) v += __shfl_xor(v, off, (int)kRnG);
  return v;
}

__device__ __forceinline__ double rn_level(double stk0, double stk1, uint32_t l) {
  return __shfl(l < 16 ? stk0 : stk1, (int)(l & 15), (int)kRnG);
}

// out[i] = the normalised vals[i]; sumsq[r] = the row's s (when asked for); the counters of
// scaled_total (kRnSlots of them, kRnSlotStride words apart) together += the rows that were
// scaled.  A row whose offsets descend or leave the arrays has length 0.
__global__ __launch_bounds__(kRnThreads) void k_rn_l2(
    const float *__restrict__ vals, const uint32_t *__restrict__ rowptr, uint32_t R, uint32_t NNZ,
    uint32_t ntiles, float *__restrict__ out, double *__restrict__ sumsq,
    unsigned long long *scaled_total) {
  const uint32_t t = threadIdx.x, gl = t & (kRnG - 1), g = t / kRnG;
  uint32_t scaled = 0;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t r = tile * kRnW + g;
    if (r >= R) continue;
    const uint32_t a = rowptr[r], e = rowptr[r + 1];
    const uint32_t len = (e >= a && e <= NNZ) ? e - a : 0u;
    const uint32_t nblk = (len + kRnG - 1) / kRnG;
    if (nblk <= 4) {
      const bool in0 = gl < len, in1 = gl + 16 < len, in2 = gl + 32 < len, in3 = gl + 48 < len;
      const float x0 = in0 ? vals[a + gl] : 0.0f, x1 = in1 ? vals[a + gl + 16] : 0.0f;
      const float x2 = in2 ? vals[a + gl + 32] : 0.0f, x3 = in3 ? vals[a + gl + 48] : 0.0f;
      double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
      if (nblk > 0) b0 = rn_bfly(xf::rownorm_sq(x0));
      if (nblk > 1) b1 = rn_bfly(xf::rownorm_sq(x1));
      if (nblk > 2) b2 = rn_bfly(xf::rownorm_sq(x2));
      if (nblk > 3) b3 = rn_bfly(xf::rownorm_sq(x3));
      const double s = (b0 + b1) + (b2 + b3);  // (a missing block is the padding: + 0.0)
      if (gl == 0 && sumsq) sumsq[r] = s;
      if (xf::rownorm_scales(s)) {
        const double rs = xf::rownorm_rs(s);
        ++scaled;
        if (in0) out[a + gl] = xf::rownorm_y(x0, rs);
        if (in1) out[a + gl + 16] = xf::rownorm_y(x1, rs);
        if (in2) out[a + gl + 32] = xf::rownorm_y(x2, rs);
        if (in3) out[a + gl + 48] = xf::rownorm_y(x3, rs);
      } else {
        if (in0) out[a + gl] = x0;
        if (in1) out[a + gl + 16] = x1;
        if (in2) out[a + gl + 32] = x2;
        if (in3) out[a + gl + 48] = x3;
      }
      continue;
    }
    // a longer row: the block sums through the binary counter, level l in lane l of the group
    double stk0 = 0.0, stk1 = 0.0;
    for (uint32_t b = 0; b < nblk; ++b) {
      const uint32_t i = b * kRnG + gl;
      const float x = i < len ? vals[a + i] : 0.0f;
      double carry = rn_bfly(xf::rownorm_sq(x));
      uint32_t l = 0;
      for (; (b >> l) & 1u; ++l) carry = rn_level(stk0, stk1, l) + carry;
      if (gl == (l & 15)) {
        if (l < 16) stk0 = carry;
        else
          stk1 = carry;
      }
    }
    double s = 0.0;
    bool have = false;
    for (uint32_t l = 0; l < 32 && (nblk >> l) != 0; ++l)
      if ((nblk >> l) & 1u) {
        const double v = rn_level(stk0, stk1, l);
        s = have ? v + s : v;
        have = true;
      }
    if (gl == 0 && sumsq) sumsq[r] = s;
    const bool sc = xf::rownorm_scales(s);
    const double rs = sc ? xf::rownorm_rs(s) : 1.0;
    if (sc) ++scaled;
    for (uint32_t b = 0; b < nblk; ++b) {
      const uint32_t i = b * kRnG + gl;
      if (i < len) {
        const float x = vals[a + i];
        out[a + i] = sc ? xf::rownorm_y(x, rs) : x;
      }
    }
  }
  // the scaled rows of this wave's four groups (every lane of a group holds its group's count)
  uint32_t c = scaled;
  c += __shfl_xor(c, 16, 64);
  c += __shfl_xor(c, 32, 64);
  if ((t & 63) == 0 && c)
    atomicAdd(scaled_total + (size_t)((blockIdx.x * 4 + (t >> 6)) & (kRnSlots - 1)) * kRnSlotStride,
              (unsigned long long)c);
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

struct xf_rownorm {
  int kind = XF_ROWNORM_L2;
  uint64_t rows_seen = 0;
  // the normalised values and the rows' sums (valid until the next apply)
  float *o_vals = nullptr;
  double *o_sumsq = nullptr;
  size_t cap_vals = 0, cap_sumsq = 0;
  unsigned long long *d_scaled = nullptr;  // the running counts of scaled rows (kRnSlots of them)
  // xf_rownorm_apply's copies of the host arrays
  uint64_t *u_keys = nullptr;
  int32_t *u_fgid = nullptr, *u_labels = nullptr;
  float *u_vals = nullptr;
  uint32_t *u_rowptr = nullptr;
  size_t ucap_keys = 0, ucap_fgid = 0, ucap_labels = 0, ucap_vals = 0, ucap_rowptr = 0;
  std::vector<uint32_t> h_rowptr;
};

extern "C" int xf_rownorm_create(xf_rownorm **out, int kind) {
  XF_REQUIRE(out, "xf_rownorm_create: out is NULL");
  *out = nullptr;
  XF_TRY(xf::rownorm_check_kind("xf_rownorm_create", kind));
  xf_rownorm *n = new xf_rownorm;
  n->kind = kind;
  // (nothing on the device yet: the first apply allocates)
  *out = n;
  return XF_OK;
}

extern "C" int xf_rownorm_destroy(xf_rownorm *n) {
  if (!n) return XF_OK;
  if ((n->d_scaled || n->o_vals || n->u_rowptr) && !xf::device_poisoned()) {  // (an apply has run)
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)n->o_vals, (void *)n->o_sumsq, (void *)n->d_scaled, (void *)n->u_keys,
                    (void *)n->u_fgid, (void *)n->u_labels, (void *)n->u_vals,
                    (void *)n->u_rowptr})
      if (p) (void)hipFree(p);
  }
  delete n;
  return XF_OK;
}

extern "C" uint64_t xf_rownorm_launches(void) { return g_launches.load(std::memory_order_relaxed); }

extern "C" int xf_rownorm_stats(const xf_rownorm *n, uint64_t *rows_seen, uint64_t *rows_scaled) {
  XF_REQUIRE(n, "xf_rownorm_stats: the stage is NULL");
  if (rows_seen) *rows_seen = n->rows_seen;
  if (rows_scaled) {
    unsigned long long v = 0;
    // (behind every apply's kernel, whatever its stream — the one wait)
    if (n->d_scaled) {
      std::vector<unsigned long long> h((size_t)kRnSlots * kRnSlotStride);
      XF_HIP(hipDeviceSynchronize());
      XF_HIP(hipMemcpy(h.data(), n->d_scaled, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < kRnSlots; ++i) v += h[(size_t)i * kRnSlotStride];
    }
    *rows_scaled = (uint64_t)v;
  }
  return XF_OK;
}

extern "C" int xf_rownorm_apply_dev(xf_rownorm *n, const float *d_vals, const uint32_t *d_rowptr,
                                    uint32_t R, uint32_t NNZ, void *stream,
                                    const float **d_vals_out, const double **d_sumsq_out) {
  XF_REQUIRE(n, "xf_rownorm_apply_dev: the stage is NULL");
  XF_REQUIRE(d_vals_out, "xf_rownorm_apply_dev: d_vals_out is NULL");
  XF_REQUIRE(NNZ == 0 || (d_vals && R > 0),
             "xf_rownorm_apply_dev: %u nonzeros need values (d_vals) and rows (R = %u)", NNZ, R);
  XF_REQUIRE(R == 0 || d_rowptr, "xf_rownorm_apply_dev: %u rows without row offsets (d_rowptr)", R);
  XF_REQUIRE(NNZ < 0xFFFFE000u && R < 0xFFFFFF00u,
             "xf_rownorm_apply_dev: a minibatch of %u rows, %u nonzeros is too large", R, NNZ);
  hipStream_t st = (hipStream_t)stream;
  XF_TRY(grow(&n->o_vals, &n->cap_vals, (size_t)NNZ));
  if (d_sumsq_out) XF_TRY(grow(&n->o_sumsq, &n->cap_sumsq, (size_t)R));
  *d_vals_out = n->o_vals;
  if (d_sumsq_out) *d_sumsq_out = n->o_sumsq;
  if (R == 0) return XF_OK;  // (no row: nothing is launched)
  if (!n->d_scaled) {
    const size_t bytes = (size_t)kRnSlots * kRnSlotStride * sizeof(unsigned long long);
    XF_HIP(hipMalloc((void **)&n->d_scaled, bytes));
    XF_HIP(hipMemsetAsync(n->d_scaled, 0, bytes, st));
  }
  const uint32_t ntiles = (R + kRnW - 1) / kRnW;
  const uint32_t grid = ntiles < kRnMaxGrid ? ntiles : kRnMaxGrid;
  hipLaunchKernelGGL(k_rn_l2, dim3(grid), dim3(kRnThreads), 0, st, d_vals, d_rowptr, R, NNZ, ntiles,
                     n->o_vals, d_sumsq_out ? n->o_sumsq : nullptr, n->d_scaled);
  XF_HIP(hipGetLastError());
  g_launches.fetch_add(1, std::memory_order_relaxed);
  n->rows_seen += R;
  return XF_OK;
}

// xf_rownorm_apply's upload of a row slice of the reader's host arrays (rowptr rebased to u32), as
// the cross's upload_slice
static int upload_slice(xf_rownorm *n, const uint64_t *rowptr, const uint64_t *keys,
                        const int32_t *fgid, const float *vals, const int32_t *labels,
                        size_t row_begin, size_t row_end, hipStream_t st, uint32_t *R_up,
                        uint32_t *NNZ_up) {
  XF_REQUIRE(n, "xf_rownorm_apply: the stage is NULL");
  XF_REQUIRE(rowptr, "xf_rownorm_apply: rowptr is NULL");
  uint32_t nnz = 0;
  XF_TRY(xf::rownorm_check_slice("xf_rownorm_apply", rowptr, row_begin, row_end, &n->h_rowptr,
                                 &nnz));
  const size_t R = row_end - row_begin;
  const uint64_t base = rowptr[row_begin];
  XF_REQUIRE(nnz == 0 || keys, "xf_rownorm_apply: %u nonzeros without keys", nnz);
  XF_REQUIRE(nnz == 0 || vals, "xf_rownorm_apply: the stage needs the nonzeros' values (vals is "
             "NULL for %u nonzeros)", nnz);
  XF_TRY(grow(&n->u_rowptr, &n->ucap_rowptr, R + 1));
  XF_HIP(hipMemcpyAsync(n->u_rowptr, n->h_rowptr.data(), (R + 1) * 4, hipMemcpyHostToDevice, st));
  XF_TRY(grow(&n->u_keys, &n->ucap_keys, (size_t)nnz));
  if (fgid) XF_TRY(grow(&n->u_fgid, &n->ucap_fgid, (size_t)nnz));
  XF_TRY(grow(&n->u_vals, &n->ucap_vals, (size_t)nnz));
  if (nnz) {
    XF_HIP(hipMemcpyAsync(n->u_keys, keys + base, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    if (fgid)
      XF_HIP(hipMemcpyAsync(n->u_fgid, fgid + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    XF_HIP(hipMemcpyAsync(n->u_vals, vals + base, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  XF_TRY(grow(&n->u_labels, &n->ucap_labels, R));
  if (R && labels)
    XF_HIP(hipMemcpyAsync(n->u_labels, labels + row_begin, R * 4, hipMemcpyHostToDevice, st));
  *R_up = (uint32_t)R;
  *NNZ_up = nnz;
  return XF_OK;
}

extern "C" int xf_rownorm_apply(xf_rownorm *n, const uint64_t *rowptr, const uint64_t *keys,
                                const int32_t *fgid, const float *vals, const int32_t *labels,
                                size_t row_begin, size_t row_end, void *stream,
                                const uint64_t **d_keys_out, const int32_t **d_fgid_out,
                                const float **d_vals_out, const uint32_t **d_rowptr_out,
                                const int32_t **d_labels_out, uint32_t *R_out, uint32_t *NNZ_out,
                                const double **d_sumsq_out) {
  XF_REQUIRE(d_keys_out && d_vals_out && d_rowptr_out && R_out && NNZ_out,
             "xf_rownorm_apply: a required output (d_keys_out, d_vals_out, d_rowptr_out, R_out, "
             "NNZ_out) is NULL");
  uint32_t R = 0, nnz = 0;
  XF_TRY(upload_slice(n, rowptr, keys, fgid, vals, labels, row_begin, row_end, (hipStream_t)stream,
                      &R, &nnz));
  // (the host arrays may be pageable: the copies above have read them when they return; the
  // vector of rebased offsets lives until the next call.  R = 0: nothing waits, so wait here)
  if (R == 0) XF_HIP(hipStreamSynchronize((hipStream_t)stream));
  *R_out = R;
  *NNZ_out = nnz;
  *d_keys_out = n->u_keys;
  if (d_fgid_out) *d_fgid_out = fgid ? n->u_fgid : nullptr;
  *d_rowptr_out = n->u_rowptr;
  if (d_labels_out) *d_labels_out = labels ? n->u_labels : nullptr;
  return xf_rownorm_apply_dev(n, n->u_vals, n->u_rowptr, R, nnz, stream, d_vals_out, d_sumsq_out);
}
