// xf_rownorm_host.cc — the host side of row normalisation that needs no GPU: the definition of
// xf_rownorm.h as host code (xf_rownorm_row), the check of a row slice's offsets, the kind and the
// launch shape.  Plain C++: it also builds into a stand-alone program under the host sanitizers
// (tools/rownorm_host_check.cc).
#include <string.h>

#include "xf_common.h"
#include "xf_rownorm.h"

namespace xf {

int rownorm_check_kind(const char *who, int kind) {
  XF_REQUIRE(kind == XF_ROWNORM_L2, "%s: kind must be XF_ROWNORM_L2 (%d), not %d", who,
             (int)XF_ROWNORM_L2, kind);
  return XF_OK;
}

int rownorm_check_slice(const char *who, const uint64_t *rowptr, size_t row_begin, size_t row_end,
                        std::vector<uint32_t> *out, uint32_t *NNZ) {
  XF_REQUIRE(rowptr && out && NNZ, "%s: null row offsets", who);
  XF_REQUIRE(row_begin <= row_end, "%s: row_begin %zu is behind row_end %zu", who, row_begin,
             row_end);
  const size_t R = row_end - row_begin;
  const uint64_t base = rowptr[row_begin];
  XF_REQUIRE(rowptr[row_end] >= base, "%s: row offsets descend", who);
  const uint64_t nnz = rowptr[row_end] - base;
  XF_REQUIRE(R < 0xFFFFFF00ull && nnz < 0xFFFFE000ull,
             "%s: a minibatch of %zu rows, %llu nonzeros is too large", who, R,
             (unsigned long long)nnz);
  out->resize(R + 1);
  uint32_t *o = out->data();
  for (size_t r = 0; r <= R; ++r) {
    const uint64_t at = rowptr[row_begin + r];
    XF_REQUIRE(at >= base && at - base <= nnz && (r == 0 || at - base >= o[r - 1]),
               "%s: row offsets descend at row %zu", who, row_begin + r);
    o[r] = (uint32_t)(at - base);
  }
  *NNZ = (uint32_t)nnz;
  return XF_OK;
}

}  // namespace xf

extern "C" int xf_rownorm_row(const float *x, size_t m, float *y, double *sumsq) {
  XF_REQUIRE(m == 0 || x, "xf_rownorm_row: x is NULL for a row of %zu nonzeros", m);
  XF_REQUIRE(m == 0 || y, "xf_rownorm_row: y is NULL for a row of %zu nonzeros", m);
  xf::rownorm_tree t;
  for (size_t i = 0; i < m; ++i) t.push(xf::rownorm_sq(x[i]));
  const double s = t.total();
  if (sumsq) *sumsq = s;
  if (xf::rownorm_scales(s)) {
    const double rs = xf::rownorm_rs(s);
    for (size_t i = 0; i < m; ++i) y[i] = xf::rownorm_y(x[i], rs);
  } else if (m && y != x) {
    memmove(y, x, m * sizeof(float));
  }
  return XF_OK;
}

extern "C" void xf_rownorm_shape(uint32_t out[2]) {
  if (!out) return;
  out[0] = xf::kRownormLanes;
  out[1] = xf::kRownormRows;
}
