// xf_admit_host.cc — the host side of feature admission that needs no GPU: the parameter check,
// the exported slot function and the counter file (xf_admit.h).  Plain C++: it also builds into a
// stand-alone program under the host sanitizers (tools/admit_host_check.cc).
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "xf_admit.h"
#include "xf_common.h"

namespace xf {

int admit_check_params(const char *who, long L, long h, long N) {
  XF_REQUIRE(L >= 2 && L <= 32, "%s: admit_log2_slots must be in 2 .. 32, not %ld", who, L);
  XF_REQUIRE(h >= 1 && h <= 8, "%s: admit_hashes must be in 1 .. 8, not %ld", who, h);
  XF_REQUIRE(N >= 1 && N <= 255, "%s: admit_count must be in 1 .. 255, not %ld", who, N);
  return XF_OK;
}

namespace {
const char kMagic[8] = {'X', 'F', 'A', 'D', 'M', 'I', 'T', '1'};
struct FileHeader {
  char magic[8];
  uint32_t L, h, N, reserved;
  uint64_t seed, slots;
};
static_assert(sizeof(FileHeader) == 40, "the counter file's header is 40 bytes");

struct File {
  FILE *f = nullptr;
  ~File() {
    if (f) fclose(f);
  }
};
}  // namespace

int admit_file_write(const char *path, const AdmitParams &p, const uint8_t *counters) {
  XF_REQUIRE(path && counters, "xf_admit_save: null argument");
  XF_TRY(admit_check_params("xf_admit_save", p.L, p.h, p.N));
  FileHeader hd;
  memset(&hd, 0, sizeof(hd));
  memcpy(hd.magic, kMagic, 8);
  hd.L = (uint32_t)p.L;
  hd.h = (uint32_t)p.h;
  hd.N = (uint32_t)p.N;
  hd.seed = p.seed;
  hd.slots = 1ull << p.L;
  File out;
  out.f = fopen(path, "wb");
  if (!out.f) return set_error(XF_EIO, "xf_admit_save: cannot open %s for writing", path);
  bool ok = fwrite(&hd, sizeof(hd), 1, out.f) == 1 &&
            fwrite(counters, 1, (size_t)hd.slots, out.f) == (size_t)hd.slots;
  ok = fclose(out.f) == 0 && ok;
  out.f = nullptr;
  if (!ok) return set_error(XF_EIO, "xf_admit_save: short write to %s", path);
  return XF_OK;
}

// the header of `path`, checked against `want`; the file is left open behind the header
static int admit_file_open(const char *path, const AdmitParams &want, File *in) {
  XF_TRY(admit_check_params("xf_admit_load", want.L, want.h, want.N));
  in->f = fopen(path, "rb");
  if (!in->f) return set_error(XF_EIO, "xf_admit_load: cannot open the admission file %s", path);
  FileHeader hd;
  if (fread(&hd, sizeof(hd), 1, in->f) != 1 || memcmp(hd.magic, kMagic, 8) != 0)
    return set_error(XF_EIO, "xf_admit_load: %s is not an admission file", path);
  XF_REQUIRE(hd.L == (uint32_t)want.L && hd.h == (uint32_t)want.h && hd.N == (uint32_t)want.N &&
                 hd.seed == want.seed,
             "xf_admit_load: %s was saved with admit_log2_slots=%u admit_hashes=%u admit_count=%u "
             "seed=%llu, this filter has admit_log2_slots=%d admit_hashes=%d admit_count=%d "
             "seed=%llu", path, hd.L, hd.h, hd.N, (unsigned long long)hd.seed, want.L, want.h,
             want.N, (unsigned long long)want.seed);
  const uint64_t slots = 1ull << want.L;
  if (hd.slots != slots)
    return set_error(XF_EIO, "xf_admit_load: %s names %llu counters, 2^%d = %llu expected", path,
                     (unsigned long long)hd.slots, want.L, (unsigned long long)slots);
  return XF_OK;
}

int admit_file_read(const char *path, const AdmitParams &want, std::vector<uint8_t> *counters) {
  XF_REQUIRE(path && counters, "xf_admit_load: null argument");
  File in;
  XF_TRY(admit_file_open(path, want, &in));
  const uint64_t slots = 1ull << want.L;
  counters->resize((size_t)slots);
  if (fread(counters->data(), 1, (size_t)slots, in.f) != (size_t)slots)
    return set_error(XF_EIO, "xf_admit_load: %s ends before its %llu counters", path,
                     (unsigned long long)slots);
  for (size_t i = 0; i < (size_t)slots; ++i)
    if ((*counters)[i] > (uint32_t)want.N)
      return set_error(XF_EIO, "xf_admit_load: %s: counter %zu holds %u, above admit_count=%d",
                       path, i, (unsigned)(*counters)[i], want.N);
  return XF_OK;
}

int admit_file_read_range(const char *path, const AdmitParams &want, uint64_t first, uint64_t n,
                          std::vector<uint8_t> *counters) {
  XF_REQUIRE(path && counters, "xf_admit_load: null argument");
  File in;
  XF_TRY(admit_file_open(path, want, &in));
  const uint64_t slots = 1ull << want.L;
  XF_REQUIRE(first <= slots && n <= slots - first,
             "xf_admit_load: the range [%llu, +%llu) lies outside the 2^%d counters",
             (unsigned long long)first, (unsigned long long)n, want.L);
  // (a file cut short is damaged for every rank, whichever range lost its counters)
  if (fseeko(in.f, 0, SEEK_END) != 0 || (uint64_t)ftello(in.f) < sizeof(FileHeader) + slots)
    return set_error(XF_EIO, "xf_admit_load: %s ends before its %llu counters", path,
                     (unsigned long long)slots);
  counters->resize((size_t)n);
  if (fseeko(in.f, (off_t)(sizeof(FileHeader) + first), SEEK_SET) != 0 ||
      fread(counters->data(), 1, (size_t)n, in.f) != (size_t)n)
    return set_error(XF_EIO, "xf_admit_load: %s ends before its %llu counters", path,
                     (unsigned long long)slots);
  for (size_t i = 0; i < (size_t)n; ++i)
    if ((*counters)[i] > (uint32_t)want.N)
      return set_error(XF_EIO, "xf_admit_load: %s: counter %llu holds %u, above admit_count=%d",
                       path, (unsigned long long)(first + i), (unsigned)(*counters)[i], want.N);
  return XF_OK;
}

}  // namespace xf

extern "C" uint64_t xf_admit_slot(uint64_t key, uint64_t seed, int L, int j) {
  if (L < 2 || L > 32 || j < 0) return 0;
  return xf::admit_slot(key, seed, L, j);
}

extern "C" int xf_admit_range(int log2_slots, int world, int rank, uint64_t *first, uint64_t *n) {
  XF_REQUIRE(log2_slots >= 2 && log2_slots <= 32,
             "xf_admit_range: admit_log2_slots must be in 2 .. 32, not %d", log2_slots);
  XF_REQUIRE(world >= 1 && rank >= 0 && rank < world, "xf_admit_range: rank %d of world %d", rank,
             world);
  const uint64_t slots = 1ull << log2_slots, per = xf::admit_per(log2_slots, world);
  const uint64_t lo = std::min(slots, (uint64_t)rank * per), hi = std::min(slots, lo + per);
  if (first) *first = lo;
  if (n) *n = hi - lo;
  return XF_OK;
}
