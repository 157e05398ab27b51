// xf_scalar_probe.hip — the scalar functions of xf_device.h on the GPU, one input at a time
// (xf_scalar_probe) and over whole blocks of the 2^32 floats, digested (xf_scalar_sweep).
//
// The parity of every forward and every step with the reference rests on sigmoid_ref, sqrtf, the
// fp32 division and div_by_rows giving the host's float for EVERY input.  The kernels here call
// those functions as they stand in xf_device.h — no copies — so that tests/test_gpu_scalar.py
// can compare them with the oracle on all 2^32 bit patterns: 65536 digests of 65536 inputs each,
// equal or not, and the elementwise probe to name the input when a digest is not.
#include <hip/hip_runtime.h>

#include "xf_common.h"
#include "xf_device.h"
#include "xflow_amd.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kSweepBlock = 1u << 16;   // inputs per digest
constexpr uint32_t kSweepBlocks = 1u << 16;  // digests of a whole sweep

template <int OP>
__device__ __forceinline__ float scalar_op(float a, float b, uint32_t param) {
#pragma clang fp contract(off)
  if (OP == XF_SCALAR_SIGMOID) return xf::sigmoid_ref(a);
  if (OP == XF_SCALAR_SQRT) return sqrtf(a);
  if (OP == XF_SCALAR_DIV) return a / b;
  return xf::div_by_rows(a, param);
}

template <int OP>
__global__ void __launch_bounds__(kBlock)
k_scalar_probe(const float *__restrict__ a, const float *__restrict__ b, uint32_t param, size_t n,
               float *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    out[i] = scalar_op<OP>(a[i], OP == XF_SCALAR_DIV ? b[i] : 0.0f, param);
}

// one workgroup per block of 65536 inputs, 256 per thread; the 256 sums meet through the wave
// shuffle and four LDS words, and thread 0 stores the digest
template <int OP>
__global__ void __launch_bounds__(kBlock)
k_scalar_sweep(uint32_t param, uint32_t first_block, uint64_t *__restrict__ digests) {
  __shared__ uint64_t s_part[kBlock / 64];
  const uint32_t base = (first_block + blockIdx.x) << 16;
  uint64_t sum = 0;
  for (uint32_t j = threadIdx.x; j < kSweepBlock; j += kBlock) {
    const uint32_t u = base + j;
    uint32_t r = __float_as_uint(scalar_op<OP>(__uint_as_float(u), 0.0f, param));
    if ((r & 0x7FFFFFFFu) > 0x7F800000u) r = 0x7FC00000u;  // any NaN
    sum += xf::mix64((uint64_t)u << 32 | r);
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t d = 0;
    for (int w = 0; w < kBlock / 64; ++w) d += s_part[w];
    digests[blockIdx.x] = d;
  }
}

template <int OP>
hipError_t launch_probe(const float *da, const float *db, uint32_t param, size_t n, float *dout) {
  const size_t blocks = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_scalar_probe<OP>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)),
                     dim3(kBlock), 0, nullptr, da, db, param, n, dout);
  return hipGetLastError();
}

template <int OP>
hipError_t launch_sweep(uint32_t param, uint32_t first_block, uint32_t nblocks, uint64_t *dd) {
  hipLaunchKernelGGL(k_scalar_sweep<OP>, dim3(nblocks), dim3(kBlock), 0, nullptr, param,
                     first_block, dd);
  return hipGetLastError();
}

}  // namespace

extern "C" int xf_scalar_probe(int op, const float *a, const float *b, uint32_t param, size_t n,
                               float *out) {
  XF_REQUIRE(op >= XF_SCALAR_SIGMOID && op <= XF_SCALAR_DIV_ROWS, "xf_scalar_probe: unknown op %d",
             op);
  XF_REQUIRE(a && out && (op != XF_SCALAR_DIV || b), "xf_scalar_probe: null argument");
  XF_REQUIRE(op != XF_SCALAR_DIV_ROWS || param >= 1, "xf_scalar_probe: a row count is >= 1");
  if (n == 0) return XF_OK;
  float *da = nullptr, *db = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void **)&da, n * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&dout, n * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(da, a, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess && op == XF_SCALAR_DIV) {
    e = hipMalloc((void **)&db, n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(db, b, n * sizeof(float), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    switch (op) {
      case XF_SCALAR_SIGMOID: e = launch_probe<XF_SCALAR_SIGMOID>(da, db, param, n, dout); break;
      case XF_SCALAR_SQRT: e = launch_probe<XF_SCALAR_SQRT>(da, db, param, n, dout); break;
      case XF_SCALAR_DIV: e = launch_probe<XF_SCALAR_DIV>(da, db, param, n, dout); break;
      default: e = launch_probe<XF_SCALAR_DIV_ROWS>(da, db, param, n, dout); break;
    }
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  XF_HIP(e);
  return XF_OK;
}

extern "C" int xf_scalar_sweep(int op, uint32_t param, uint32_t first_block, uint32_t nblocks,
                               uint64_t *digests) {
  XF_REQUIRE(op == XF_SCALAR_SIGMOID || op == XF_SCALAR_SQRT || op == XF_SCALAR_DIV_ROWS,
             "xf_scalar_sweep: op %d has no sweep (the unary ops and XF_SCALAR_DIV_ROWS have)", op);
  XF_REQUIRE(op != XF_SCALAR_DIV_ROWS || param >= 1, "xf_scalar_sweep: a row count is >= 1");
  XF_REQUIRE(first_block <= kSweepBlocks && nblocks <= kSweepBlocks - first_block,
             "xf_scalar_sweep: blocks %u .. %u + %u lie past the 65536 there are", first_block,
             first_block, nblocks);
  if (nblocks == 0) return XF_OK;
  XF_REQUIRE(digests, "xf_scalar_sweep: null argument");
  uint64_t *dd = nullptr;
  hipError_t e = hipMalloc((void **)&dd, (size_t)nblocks * sizeof(uint64_t));
  if (e == hipSuccess) {
    switch (op) {
      case XF_SCALAR_SIGMOID:
        e = launch_sweep<XF_SCALAR_SIGMOID>(param, first_block, nblocks, dd);
        break;
      case XF_SCALAR_SQRT:
        e = launch_sweep<XF_SCALAR_SQRT>(param, first_block, nblocks, dd);
        break;
      default:
        e = launch_sweep<XF_SCALAR_DIV_ROWS>(param, first_block, nblocks, dd);
        break;
    }
  }
  if (e == hipSuccess)
    e = hipMemcpy(digests, dd, (size_t)nblocks * sizeof(uint64_t), hipMemcpyDeviceToHost);
  (void)hipFree(dd);
  XF_HIP(e);
  return XF_OK;
}
