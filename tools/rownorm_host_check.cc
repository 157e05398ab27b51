// rownorm_host_check.cc — the host side of row normalisation (xflow_amd/csrc/xf_rownorm_host.cc:
// the definition as host code, the check of a row slice's offsets, the kind, the shape) driven
// from a main of its own, for a run under the host sanitizers.  No GPU, no Python:
//
//   hipcc -std=c++17 -g -O1 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -fno-sanitize-recover=all -Iinclude -Ixflow_amd/csrc tools/rownorm_host_check.cc \
//     xflow_amd/csrc/xf_rownorm_host.cc xflow_amd/csrc/xf_io.cc -o /tmp/rownorm_host_check \
//     -lpthread && /tmp/rownorm_host_check
//
// Covers: xf_rownorm_row on rows of 0 .. 5000 nonzeros against a recursive walk of the tree
// written here, in place and out of place, with and without the sum; the special rows (zeros, one
// subnormal, FLT_MAX, a NaN, an infinity); the power-of-two recipe; the refusals naming their
// argument; the offset check on good slices (a slice in the middle of a block, an empty slice,
// empty rows) and on every kind of bad one (descending inside, below the slice's base, begin
// behind end, null), each refusal leaving the vector usable.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "xf_common.h"
#include "xf_rownorm.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, xf_last_error());
  }
}

static bool names(const char *word) { return strstr(xf_last_error(), word) != nullptr; }

// the sum of positions [lo, lo + w) of the zero-padded squares
static double walk(const std::vector<double> &sq, size_t lo, size_t w) {
  if (lo >= sq.size()) return 0.0;
  if (w == 1) return sq[lo];
  return walk(sq, lo, w / 2) + walk(sq, lo + w / 2, w / 2);
}

static uint64_t bits(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u;
}

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main() {
  // the definition against the recursive walk
  uint64_t state = 0x9e3779b97f4a7c15ull;
  auto next = [&state]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
  };
  const size_t lens[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097,
                         5000};
  for (size_t m : lens) {
    std::vector<float> x(m), y(m, -7.0f);
    std::vector<double> sq(m);
    for (size_t i = 0; i < m; ++i) {
      const uint32_t r = next();
      x[i] = ldexpf((float)(r & 0xFFFFFF) / 16777216.0f + 0.5f, (int)(r >> 24 & 15) - 8);
      if ((r >> 28) == 0) x[i] = 0.0f;
      if (r >> 31) x[i] = -x[i];
      sq[i] = (double)x[i] * (double)x[i];
    }
    size_t w = 1;
    while (w < m) w *= 2;
    const double want = m ? walk(sq, 0, w) : 0.0;
    double s = -1.0;
    expect(xf_rownorm_row(x.data(), m, y.data(), &s) == XF_OK && bits(s) == bits(want),
           "the tree's sum");
    bool same = true;
    double len2 = 0.0;
    for (size_t i = 0; i < m; ++i) {
      const float e = want > 0 ? (float)((double)x[i] * (1.0 / sqrt(want))) : x[i];
      same = same && bits(e) == bits(y[i]);
      len2 += (double)y[i] * (double)y[i];
    }
    expect(same, "the scaled values");
    expect(!(want > 0) || fabs(len2 - 1.0) <= ldexp(1.0, -22), "unit length");
    std::vector<float> z = x;  // in place, without the sum
    expect(xf_rownorm_row(z.data(), m, z.data(), nullptr) == XF_OK &&
               (m == 0 || memcmp(z.data(), y.data(), m * 4) == 0), "in place");
  }

  // the special rows
  {
    const float zeros[4] = {0.0f, -0.0f, -0.0f, 0.0f};
    float y[10];
    double s = 1.0;
    expect(xf_rownorm_row(zeros, 4, y, &s) == XF_OK && bits(s) == 0 && memcmp(y, zeros, 16) == 0,
           "a row of zeros is unchanged");
    const float sub[1] = {-1e-45f};
    expect(xf_rownorm_row(sub, 1, y, &s) == XF_OK && y[0] == -1.0f && s > 0, "one subnormal");
    const float big[3] = {3.4028234664e38f, -3.4028234664e38f, 3.4028234664e38f};
    expect(xf_rownorm_row(big, 3, y, &s) == XF_OK && isfinite(s) && s > 1e77 &&
               fabsf(y[0] - 0.57735026f) < 1e-6f && y[1] == -y[0], "FLT_MAX stays finite in fp64");
    const float withnan[3] = {1.0f, NAN, 2.0f}, withinf[3] = {1.0f, -INFINITY, 2.0f};
    expect(xf_rownorm_row(withnan, 3, y, &s) == XF_OK && isnan(s) &&
               memcmp(y, withnan, 12) == 0, "a row with a NaN is unchanged");
    expect(xf_rownorm_row(withinf, 3, y, &s) == XF_OK && isinf(s) &&
               memcmp(y, withinf, 12) == 0, "a row with an infinity is unchanged");
    // the recipe: 8 x +-1 and 2 x +-2: s = 16, y = x / 4
    const float rec[10] = {1, -1, 2, 1, 1, -2, 1, -1, 1, 1};
    expect(xf_rownorm_row(rec, 10, y, &s) == XF_OK && s == 16.0, "the recipe's sum");
    for (int i = 0; i < 10; ++i) expect(y[i] == rec[i] * 0.25f, "the recipe's values");
    expect(xf_rownorm_row(nullptr, 0, nullptr, &s) == XF_OK && bits(s) == 0, "an empty row");
  }

  // the refusals
  {
    float y[2];
    const float x[2] = {1, 2};
    expect(xf_rownorm_row(nullptr, 2, y, nullptr) == XF_EINVAL && names("x is NULL"), "null x");
    expect(xf_rownorm_row(x, 2, nullptr, nullptr) == XF_EINVAL && names("y is NULL"), "null y");
    expect(xf::rownorm_check_kind("t", XF_ROWNORM_L2) == XF_OK, "the kind");
    expect(xf::rownorm_check_kind("t", 0) == XF_EINVAL && names("XF_ROWNORM_L2") &&
               xf::rownorm_check_kind("t", 2) == XF_EINVAL, "a bad kind");
    uint32_t shape[2] = {0, 0};
    xf_rownorm_shape(shape);
    xf_rownorm_shape(nullptr);
    expect(shape[0] == xf::kRownormLanes && shape[1] == xf::kRownormRows &&
               shape[0] * shape[1] == 256, "the shape");
  }

  // the offsets of a row slice
  {
    const uint64_t rp[8] = {0, 3, 3, 10, 10, 10, 14, 20};
    std::vector<uint32_t> out;
    uint32_t nnz = 99;
    expect(xf::rownorm_check_slice("t", rp, 0, 7, &out, &nnz) == XF_OK && nnz == 20 &&
               out.size() == 8 && out[7] == 20 && out[2] == 3, "the whole block");
    expect(xf::rownorm_check_slice("t", rp, 2, 6, &out, &nnz) == XF_OK && nnz == 11 &&
               out.size() == 5 && out[0] == 0 && out[1] == 7 && out[4] == 11,
           "a slice in the middle");
    expect(xf::rownorm_check_slice("t", rp, 4, 4, &out, &nnz) == XF_OK && nnz == 0 &&
               out.size() == 1 && out[0] == 0, "an empty slice");
    expect(xf::rownorm_check_slice("t", rp, 3, 5, &out, &nnz) == XF_OK && nnz == 0 &&
               out.size() == 3, "empty rows");
    const uint64_t down[5] = {0, 3, 2, 5, 6}, below[4] = {4, 2, 5, 6}, ends[3] = {5, 6, 4};
    expect(xf::rownorm_check_slice("t", down, 0, 4, &out, &nnz) == XF_EINVAL &&
               names("descend at row 2"), "offsets that descend inside");
    expect(xf::rownorm_check_slice("t", below, 0, 3, &out, &nnz) == XF_EINVAL && names("descend"),
           "an offset below the slice's first");
    expect(xf::rownorm_check_slice("t", ends, 0, 2, &out, &nnz) == XF_EINVAL && names("descend"),
           "a last offset below the first");
    expect(xf::rownorm_check_slice("t", rp, 5, 4, &out, &nnz) == XF_EINVAL && names("row_begin"),
           "begin behind end");
    expect(xf::rownorm_check_slice("t", nullptr, 0, 1, &out, &nnz) == XF_EINVAL, "null offsets");
    expect(xf::rownorm_check_slice("t", rp, 1, 3, &out, &nnz) == XF_OK && nnz == 7 &&
               out.size() == 3, "the vector lives on");
  }

  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("rownorm_host_check: all checks passed\n");
  return 0;
}
