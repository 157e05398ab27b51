// xf_bin_host.cc — the host side of value binning that needs no GPU: the spec's parser and check,
// the exported code and key functions, the slot table, the cut of a field's counts to its LUT and
// the LUT file (xf_bin.h).  Plain C++, no GPU.
#include <stdio.h>
#include <string.h>

#include <string>

#include "xf_bin.h"
#include "xf_common.h"

namespace xf {

int bin_check_spec(const char *who, const int32_t *field, const int32_t *bins, long n) {
  XF_REQUIRE(n >= 1 && n <= kBinMaxFields, "%s: a bin spec holds 1 .. %d field:bins pairs, not %ld",
             who, kBinMaxFields, n);
  XF_REQUIRE(field && bins, "%s: null spec arrays", who);
  for (long p = 0; p < n; ++p) {
    XF_REQUIRE(field[p] >= 0, "%s: pair %ld is %d:%d: a field id is in 0 .. 2147483647", who, p,
               field[p], bins[p]);
    XF_REQUIRE(bins[p] >= 2 && bins[p] <= 255,
               "%s: pair %ld is %d:%d: bins lies in 2 .. 255 (a bucket id is a byte, and NaN has "
               "one of its own)", who, p, field[p], bins[p]);
    for (long q = 0; q < p; ++q)
      XF_REQUIRE(field[q] != field[p], "%s: the field %d is listed twice (%ld and %ld)", who,
                 field[p], q, p);
  }
  return XF_OK;
}

void bin_build_table(const int32_t *field, int n, int32_t tf[kBinTable], int32_t ts[kBinTable]) {
  for (uint32_t h = 0; h < kBinTable; ++h) tf[h] = ts[h] = -1;
  for (int s = 0; s < n; ++s) {
    uint32_t h = bin_table_home(field[s]);
    while (tf[h] >= 0) h = (h + 1) & (kBinTable - 1);
    tf[h] = field[s];
    ts[h] = s;
  }
}

namespace {
const char kBinMagic[8] = {'X', 'F', 'B', 'I', 'N', 'S', '0', '1'};

// decimal digits only, at most `max`; false: not such a number
bool number(const std::string &s, uint64_t max, int32_t *out) {
  if (s.empty() || s.size() > 10) return false;
  uint64_t v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint64_t)(c - '0');
  }
  if (v > max) return false;
  *out = (int32_t)v;
  return true;
}

std::string spec_text(const int32_t *field, const int32_t *bins, int n) {
  std::string s;
  for (int p = 0; p < n; ++p)
    s += (p ? "," : "") + std::to_string(field[p]) + ":" + std::to_string(bins[p]);
  return s;
}
}  // namespace

int bin_file_write(const char *path, const int32_t *field, const int32_t *bins, int n,
                   const uint8_t *lut) {
  XF_REQUIRE(path && field && bins && lut, "xf_bin_save: null argument");
  FILE *f = fopen(path, "wb");
  if (!f) return set_error(XF_EIO, "xf_bin_save: cannot write %s", path);
  const uint32_t head[2] = {(uint32_t)n, 0u};
  bool ok = fwrite(kBinMagic, 1, 8, f) == 8 && fwrite(head, 4, 2, f) == 2;
  for (int p = 0; ok && p < n; ++p) {
    const int32_t pair[2] = {field[p], bins[p]};
    ok = fwrite(pair, 4, 2, f) == 2;
  }
  ok = ok && fwrite(lut, kBinCodes, (size_t)n, f) == (size_t)n;
  ok = (fclose(f) == 0) && ok;
  if (!ok) return set_error(XF_EIO, "xf_bin_save: short write to %s", path);
  return XF_OK;
}

int bin_file_read(const char *path, const int32_t *field, const int32_t *bins, int n,
                  std::vector<uint8_t> *lut) {
  XF_REQUIRE(path && field && bins && lut, "xf_bin_load: null argument");
  FILE *f = fopen(path, "rb");
  if (!f) return set_error(XF_EIO, "xf_bin_load: cannot read %s", path);
  char magic[8];
  uint32_t head[2] = {0, 0};
  std::vector<int32_t> pairs;
  bool ok = fread(magic, 1, 8, f) == 8 && !memcmp(magic, kBinMagic, 8) && fread(head, 4, 2, f) == 2 &&
            head[0] >= 1 && head[0] <= (uint32_t)kBinMaxFields && head[1] == 0;
  if (ok) {
    pairs.resize(2 * (size_t)head[0]);
    ok = fread(pairs.data(), 4, pairs.size(), f) == pairs.size();
  }
  if (!ok) {
    fclose(f);
    return set_error(XF_EIO, "xf_bin_load: %s is not a file of bin LUTs (or is cut short)", path);
  }
  std::vector<int32_t> ff(head[0]), fb(head[0]);
  bool same = (int)head[0] == n;
  for (uint32_t p = 0; p < head[0]; ++p) {
    ff[p] = pairs[2 * p];
    fb[p] = pairs[2 * p + 1];
    same = same && ff[p] == field[p] && fb[p] == bins[p];
  }
  if (!same) {
    fclose(f);
    return set_error(XF_EINVAL, "xf_bin_load: %s was fitted for bin=%s, not for bin=%s", path,
                     spec_text(ff.data(), fb.data(), (int)head[0]).c_str(),
                     spec_text(field, bins, n).c_str());
  }
  lut->resize((size_t)n * kBinCodes);
  ok = fread(lut->data(), kBinCodes, (size_t)n, f) == (size_t)n;
  fclose(f);
  if (!ok) return set_error(XF_EIO, "xf_bin_load: %s is cut short", path);
  for (int p = 0; p < n; ++p)
    for (uint32_t c = 0; c < kBinCodes; ++c)
      if ((*lut)[(size_t)p * kBinCodes + c] > bins[p])
        return set_error(XF_EIO, "xf_bin_load: %s holds bucket %d for field %d, which has %d", path,
                         (int)(*lut)[(size_t)p * kBinCodes + c], field[p], bins[p]);
  return XF_OK;
}

}  // namespace xf

extern "C" uint32_t xf_bin_code(float v) { return xf::bin_code(v); }

extern "C" uint64_t xf_bin_key(uint64_t key, int32_t f, uint32_t b) {
  return xf::bin_key(key, f, b);
}

extern "C" int xf_bin_lut_from_counts(const uint64_t *count, int bins, uint8_t *lut) {
  XF_REQUIRE(count && lut, "xf_bin_lut_from_counts: null argument");
  XF_REQUIRE(bins >= 2 && bins <= 255, "xf_bin_lut_from_counts: bins lies in 2 .. 255, not %d", bins);
  const uint64_t limit = 1ull << 56;
  uint64_t T = 0;
  for (uint32_t c = 0; c < xf::kBinNanCode; ++c) {
    XF_REQUIRE(count[c] < limit && T + count[c] < limit,
               "xf_bin_lut_from_counts: 2^56 or more fitted nonzeros (code %u takes the total past "
               "it): the cut's product would leave 64 bits", c);
    T += count[c];
  }
  uint64_t C = 0;  // the exclusive prefix
  for (uint32_t c = 0; c < xf::kBinNanCode; ++c) {
    uint64_t b = T ? C * (uint64_t)bins / T : 0;
    if (b > (uint64_t)bins - 1) b = (uint64_t)bins - 1;
    lut[c] = (uint8_t)b;
    C += count[c];
  }
  lut[xf::kBinNanCode] = (uint8_t)bins;
  return XF_OK;
}

extern "C" int xf_bin_parse(const char *spec, int32_t *field, int32_t *bins, int cap, int *n_out) {
  XF_REQUIRE(spec && field && bins && n_out, "xf_bin_parse: null argument");
  *n_out = 0;
  const std::string s = spec;
  XF_REQUIRE(!s.empty(), "xf_bin_parse: the bin spec is empty (write it as 13:32,14:32)");
  int32_t f[xf::kBinMaxFields], b[xf::kBinMaxFields];
  int n = 0;
  for (size_t at = 0;;) {
    const size_t comma = s.find(',', at);
    const std::string piece = s.substr(at, comma == std::string::npos ? comma : comma - at);
    XF_REQUIRE(n < xf::kBinMaxFields, "xf_bin_parse: more than %d pairs: '%s' is pair %d",
               xf::kBinMaxFields, piece.c_str(), n + 1);
    const size_t colon = piece.find(':');
    XF_REQUIRE(colon != std::string::npos &&
                   xf::number(piece.substr(0, colon), 2147483647ull, &f[n]) &&
                   xf::number(piece.substr(colon + 1), 2147483647ull, &b[n]),
               "xf_bin_parse: '%s' is not a pair FIELD:BINS of decimal numbers, the field in 0 .. "
               "2147483647 (no blanks, no signs; pairs are separated by one comma)", piece.c_str());
    XF_REQUIRE(b[n] >= 2 && b[n] <= 255, "xf_bin_parse: '%s': bins lies in 2 .. 255", piece.c_str());
    for (int q = 0; q < n; ++q)
      XF_REQUIRE(f[q] != f[n], "xf_bin_parse: the field of '%s' is listed twice", piece.c_str());
    ++n;
    if (comma == std::string::npos) break;
    at = comma + 1;
  }
  XF_REQUIRE(n <= cap, "xf_bin_parse: the spec holds %d pairs, the arrays %d", n, cap);
  for (int p = 0; p < n; ++p) {
    field[p] = f[p];
    bins[p] = b[p];
  }
  *n_out = n;
  return XF_OK;
}

extern "C" void xf_bin_shape(uint32_t out[4]) {
  if (!out) return;
  out[0] = xf::kBinCountTile;
  out[1] = xf::kBinGroup;
  out[2] = xf::kBinCountMaxGrid;
  out[3] = xf::kBinApplyTile;
}
