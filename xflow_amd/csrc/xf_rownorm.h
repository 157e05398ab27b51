// xf_rownorm.h — row normalisation (xf_rownorm.hip): the definition, shared by the host and the
// kernel, and the host-only pieces (xf_rownorm_host.cc) that need no GPU.
//
// A row has nonzeros x_0 .. x_{m-1} in row order (a key that occurs twice counts twice).
//   s    = the sum of (double)x_i * (double)x_i — every product exact in fp64 — added by the
//          pairwise tree over the positions in row order, padded with +0.0 to a power of two:
//          level 0 adds positions (0,1), (2,3), ...; level 1 adds those sums in adjacent pairs; ...
//          Every addend is >= 0, so the padding changes no bit and its width does not matter: a
//          16-lane xor-butterfly computes the tree of an aligned block of 16 positions, and the
//          block sums go on through the same tree (rownorm_tree below, a binary counter).
//   s > 0 and finite:  rs = 1.0 / sqrt(s) in fp64, y_i = (float)((double)x_i * rs)
//                      (division, square root and product IEEE fp64; the product is formed in
//                      fp64 so that a row of subnormals does not overflow an fp32 scale)
//   otherwise:         y_i = x_i bit for bit (an empty row, a row of zeros, a row holding a NaN or
//                      an infinity)
// Built without fast-math and without contraction (xflow_amd/build.py), as the whole library is.
#ifndef XF_ROWNORM_H_
#define XF_ROWNORM_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define XF_RN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define XF_RN_HD inline
#endif

namespace xf {

constexpr uint32_t kRownormLanes = 16;  // lanes that share a row: one aligned block of positions
constexpr uint32_t kRownormRows = 16;   // rows of a workgroup (256 threads)

XF_RN_HD double rownorm_sq(float x) { return (double)x * (double)x; }

// is a row with this sum scaled?  (false for 0, an infinity and a NaN)
XF_RN_HD bool rownorm_scales(double s) { return s > 0.0 && s <= 1.7976931348623157e308; }

XF_RN_HD double rownorm_rs(double s) { return 1.0 / sqrt(s); }

XF_RN_HD float rownorm_y(float x, double rs) { return (float)((double)x * rs); }

// The tree as a binary counter: push() takes the sums of consecutive aligned blocks (single
// positions on the host), level l holds the sum of 2^l blocks; total() folds what is left from
// the lowest level up — the zero padding of the definition adds nothing.
struct rownorm_tree {
  double level[64];
  uint64_t n = 0;
  void push(double v) {
    int l = 0;
    for (; (n >> l) & 1; ++l) v = level[l] + v;
    level[l] = v;
    ++n;
  }
  double total() const {
    double acc = 0.0;
    bool have = false;
    for (int l = 0; l < 64; ++l)
      if ((n >> l) & 1) {
        acc = have ? level[l] + acc : level[l];
        have = true;
      }
    return acc;
  }
};

// ---- host only (xf_rownorm_host.cc)
// rows [row_begin, row_end) of a block's offsets, rebased to u32 into out[0 .. R]: XF_EINVAL naming
// `who` where they descend, leave the slice's range, or the slice is too large for a minibatch
int rownorm_check_slice(const char *who, const uint64_t *rowptr, size_t row_begin, size_t row_end,
                        std::vector<uint32_t> *out, uint32_t *NNZ);
int rownorm_check_kind(const char *who, int kind);

}  // namespace xf
#endif  // XF_ROWNORM_H_
