// xf_bin.h — value binning (xf_bin.hip): what the host and the device side share — the code of a
// value, the key of a binned nonzero, the hash of the field-to-slot table — and the host-only
// pieces (the spec's parser and check, the cut of the counts, the LUT file; xf_bin_host.cc) that
// need no GPU.
//
// A listed numeric field's nonzero (key, fgid, val) becomes (bin_key(key, fgid, lut[code(val)]),
// fgid, 1.0f): the value is replaced by the key of the equal-frequency bucket it falls into.
//   code(val): 12 bits, monotone in val: the sign, the exponent and 3 mantissa bits of the float
//              (-0.0 counts as +0.0; every NaN has code 4095, which nothing else reaches)
//   lut[c]   : a byte per code, cut from the exact 64-bit counts of the fitted nonzeros
//              (bin_lut_from_counts); NaN has the bucket `bins` of its own
#ifndef XF_BIN_H_
#define XF_BIN_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "xf_admit.h"  // admit_mix64: xf_device.h's mix64 for both sides
#include "xflow_amd.h"

namespace xf {

constexpr int kBinMaxFields = 64;
constexpr uint32_t kBinCodes = 1u << XF_BIN_CODE_BITS;  // 4096 codes a field
constexpr uint32_t kBinNanCode = kBinCodes - 1;
constexpr uint32_t kBinTable = 256;  // entries of the open-addressing field-to-slot table
// k_bin_count: a workgroup of kBinCountThreads owns the LDS histograms of up to kBinGroup listed
// fields (16 KiB each: 128 KiB, + 2 KiB of slot table, of a CU's 160 KiB) and walks tiles of
// kBinCountTile nonzeros; a second grid dimension walks the groups of a longer spec
constexpr uint32_t kBinGroup = 8;
constexpr uint32_t kBinCountThreads = 1024, kBinCountTile = 4 * kBinCountThreads;
constexpr uint32_t kBinCountMaxGrid = 512;
// k_bin_apply: 256 threads, tiles of 1024 nonzeros
constexpr uint32_t kBinApplyThreads = 256, kBinApplyTile = 4 * kBinApplyThreads;
constexpr uint32_t kBinApplyMaxGrid = 4096;

XF_ADMIT_HD uint32_t bin_code_bits(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return kBinNanCode;  // a NaN of any sign and payload
  if (u == 0x80000000u) u = 0;                               // -0.0 counts as +0.0
  const uint32_t k = (u >> 31) ? ~u : (u | 0x80000000u);
  return k >> (32 - XF_BIN_CODE_BITS);
}

XF_ADMIT_HD uint32_t bin_code(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return bin_code_bits(u);
}

// bin_key = mix64(mix64(key ^ XF_BIN_SALT) + (f << 32 | b)), 64-bit wrapping
XF_ADMIT_HD uint64_t bin_key(uint64_t key, int32_t f, uint32_t b) {
  return admit_mix64(admit_mix64(key ^ XF_BIN_SALT) + (((uint64_t)(uint32_t)f << 32) | b));
}

// where the probe for field f starts in the slot table (linear probing from there)
XF_ADMIT_HD uint32_t bin_table_home(int32_t f) {
  return ((uint32_t)f * 0x9e3779b1u) >> 24;
}

// ---- host only (xf_bin_host.cc)
// 1 .. 64 pairs, the fields distinct and >= 0, bins in 2 .. 255: XF_EINVAL naming `who` and the
// offending pair
int bin_check_spec(const char *who, const int32_t *field, const int32_t *bins, long n);
// the slot table of a spec: tf[h] = the field that lives at h (-1: empty), ts[h] = its index in
// the spec (-1: empty); at most 64 of the 256 entries are taken, so every probe ends
void bin_build_table(const int32_t *field, int n, int32_t tf[kBinTable], int32_t ts[kBinTable]);
// The LUT file: a 16-byte header — the magic "XFBINS01", the number of fields as u32 and a
// reserved 0 — then the (field, bins) pairs as int32 and the 4096-byte LUTs in spec order.
int bin_file_write(const char *path, const int32_t *field, const int32_t *bins, int n,
                   const uint8_t *lut);
// reads a file written for exactly this spec (XF_EINVAL naming both otherwise; XF_EIO: missing,
// short or not such a file — the message names the path) into lut (n * 4096 bytes)
int bin_file_read(const char *path, const int32_t *field, const int32_t *bins, int n,
                  std::vector<uint8_t> *lut);

}  // namespace xf
#endif  // XF_BIN_H_
