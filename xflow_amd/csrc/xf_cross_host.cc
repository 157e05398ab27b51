// xf_cross_host.cc — the host side of feature crosses that needs no GPU: the spec's parser and
// check, the exported key function and the emit's two knobs (xf_cross.h).  Plain C++: it also
// builds into a stand-alone program under the host sanitizers (tools/cross_host_check.cc).
#include <string.h>

#include <atomic>
#include <string>

#include "xf_common.h"
#include "xf_cross.h"

namespace xf {

int cross_check_spec(const char *who, const int32_t *fa, const int32_t *fb, long npairs) {
  XF_REQUIRE(npairs >= 1 && npairs <= kCrossMaxPairs,
             "%s: a cross spec holds 1 .. %d pairs, not %ld", who, kCrossMaxPairs, npairs);
  XF_REQUIRE(fa && fb, "%s: null field arrays", who);
  for (long p = 0; p < npairs; ++p) {
    XF_REQUIRE(fa[p] >= 0 && fb[p] >= 0,
               "%s: pair %ld is %d*%d: a field id is in 0 .. 2147483647", who, p, fa[p], fb[p]);
    XF_REQUIRE(fa[p] != fb[p], "%s: pair %ld is %d*%d: a field is not crossed with itself", who,
               p, fa[p], fb[p]);
    for (long q = 0; q < p; ++q)
      XF_REQUIRE(fa[q] != fa[p] || fb[q] != fb[p], "%s: the pair %d*%d is listed twice (%ld and %ld)",
                 who, fa[p], fb[p], q, p);
  }
  return XF_OK;
}

int cross_check_base(const char *who, long fgid_base, long npairs) {
  XF_REQUIRE(fgid_base >= 0 && fgid_base + npairs <= 2147483648l,
             "%s: cross_fgid_base=%ld with %ld pairs: the crossed fields %ld .. %ld must lie in "
             "0 .. 2147483647", who, fgid_base, npairs, fgid_base, fgid_base + npairs - 1);
  return XF_OK;
}

namespace {
std::atomic<uint32_t> g_short_max{64}, g_lds_chunks{2048};

// decimal digits only, at most 2^31 - 1; false: not such a number
bool field_id(const std::string &s, int32_t *out) {
  if (s.empty() || s.size() > 10) return false;
  uint64_t v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint64_t)(c - '0');
  }
  if (v > 2147483647ull) return false;
  *out = (int32_t)v;
  return true;
}
}  // namespace

uint32_t cross_short_max() { return g_short_max.load(std::memory_order_relaxed); }
uint32_t cross_lds_chunks() { return g_lds_chunks.load(std::memory_order_relaxed); }

int cross_set_knob(const char *name, double value) {
  if (!strcmp(name, "cross_short_max") && value >= 0 && value <= 64)
    g_short_max.store((uint32_t)value, std::memory_order_relaxed);
  else if (!strcmp(name, "cross_lds_chunks") && value >= 1 && value <= 2048)
    g_lds_chunks.store((uint32_t)value, std::memory_order_relaxed);
  else
    return -1;
  return XF_OK;
}

}  // namespace xf

extern "C" uint64_t xf_cross_key(uint64_t ka, uint64_t kb, int32_t fa, int32_t fb) {
  return xf::cross_key(ka, kb, fa, fb);
}

extern "C" int xf_cross_parse(const char *spec, int32_t *fa, int32_t *fb, int cap, int *npairs) {
  XF_REQUIRE(spec && fa && fb && npairs, "xf_cross_parse: null argument");
  *npairs = 0;
  const std::string s = spec;
  XF_REQUIRE(!s.empty(), "xf_cross_parse: the cross spec is empty (write it as 2*3,16*17)");
  int32_t a[xf::kCrossMaxPairs], b[xf::kCrossMaxPairs];
  int n = 0;
  for (size_t at = 0;;) {
    const size_t comma = s.find(',', at);
    const std::string piece = s.substr(at, comma == std::string::npos ? comma : comma - at);
    XF_REQUIRE(n < xf::kCrossMaxPairs, "xf_cross_parse: more than %d pairs: '%s' is pair %d",
               xf::kCrossMaxPairs, piece.c_str(), n + 1);
    const size_t star = piece.find('*');
    XF_REQUIRE(star != std::string::npos && xf::field_id(piece.substr(0, star), &a[n]) &&
                   xf::field_id(piece.substr(star + 1), &b[n]),
               "xf_cross_parse: '%s' is not a pair A*B of decimal field ids in 0 .. 2147483647 "
               "(no blanks, no signs; pairs are separated by one comma)", piece.c_str());
    XF_REQUIRE(a[n] != b[n], "xf_cross_parse: '%s' crosses a field with itself", piece.c_str());
    for (int q = 0; q < n; ++q)
      XF_REQUIRE(a[q] != a[n] || b[q] != b[n], "xf_cross_parse: the pair '%s' is listed twice",
                 piece.c_str());
    ++n;
    if (comma == std::string::npos) break;
    at = comma + 1;
  }
  XF_REQUIRE(n <= cap, "xf_cross_parse: the spec holds %d pairs, the arrays %d", n, cap);
  for (int p = 0; p < n; ++p) {
    fa[p] = a[p];
    fb[p] = b[p];
  }
  *npairs = n;
  return XF_OK;
}
