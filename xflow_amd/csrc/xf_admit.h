// xf_admit.h — feature admission (xf_admit.hip): what the host and the device side share — the
// slot function of the counting Bloom filter — and the host-only pieces (the parameter check and
// the counter file, xf_admit_host.cc) that need no GPU.
#ifndef XF_ADMIT_H_
#define XF_ADMIT_H_

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define XF_ADMIT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define XF_ADMIT_HD inline
#endif

namespace xf {

// xf_device.h's mix64 (add the golden constant, then the splitmix64 finaliser), for both sides
XF_ADMIT_HD uint64_t admit_mix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// the j-th salt of a filter: mix64(seed + j); a kernel computes its h salts once per thread
XF_ADMIT_HD uint64_t admit_salt(uint64_t seed, int j) { return admit_mix64(seed + (uint64_t)j); }

// slot_j(key) = mix64(key ^ mix64(seed + j)) >> (64 - L), L in 2 .. 32
XF_ADMIT_HD uint64_t admit_slot_salted(uint64_t key, uint64_t salt, int L) {
  return admit_mix64(key ^ salt) >> (64 - L);
}
XF_ADMIT_HD uint64_t admit_slot(uint64_t key, uint64_t seed, int L, int j) {
  return admit_slot_salted(key, admit_salt(seed, j), L);
}

// ---- a filter shared by the `world` ranks of a group: the counters sharded by slot range.
// per = 4 * ceil(ceil(2^L / world) / 4) slots a rank (whole counter words); rank r owns
// [r * per, min((r + 1) * per, 2^L)) — possibly nothing; owner(s) = s / per, and the local slot
// s - owner * per fits 32 bits for every L <= 32
XF_ADMIT_HD uint64_t admit_per(int L, int world) {
  const uint64_t slots = 1ull << L, w = (uint64_t)world;
  return ((slots + w - 1) / w + 3) / 4 * 4;
}

// ---- host only (xf_admit_host.cc)
struct AdmitParams {
  int L = 0, h = 0, N = 0;
  uint64_t seed = 0;
};
// L in 2 .. 32, h in 1 .. 8, N in 1 .. 255: XF_EINVAL naming `who` and the offender
int admit_check_params(const char *who, long L, long h, long N);
// The counter file: a 40-byte header — the magic "XFADMIT1", L, h, N as u32 + a reserved 0, the
// seed and the number of counters as u64 — and the 2^L counters, a byte each.
int admit_file_write(const char *path, const AdmitParams &p, const uint8_t *counters);
// reads a file written for exactly `want` (XF_EINVAL naming both parameter sets otherwise; XF_EIO:
// missing, short or not such a file — the message names the path) into `counters` (2^L bytes)
int admit_file_read(const char *path, const AdmitParams &want, std::vector<uint8_t> *counters);
// the same refusals, but only the counters [first, first + n) are read (and looked at): what a
// rank of a shared filter loads.  The file must still be as long as its header says.
int admit_file_read_range(const char *path, const AdmitParams &want, uint64_t first, uint64_t n,
                          std::vector<uint8_t> *counters);

}  // namespace xf
#endif  // XF_ADMIT_H_
