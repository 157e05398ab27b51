// xf_admit_host.cc — the host side of feature admission that needs no GPU: the parameter check,
// the exported slot function and the counter file (xf_admit.h).  Plain C++: it also builds into a
// stand-alone program under the host sanitizers (tools/admit_host_check.cc).
#include <stdio.h>
#include <string.h>

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

int admit_file_read(const char *path, const AdmitParams &want, std::vector<uint8_t> *counters) {
  XF_REQUIRE(path && counters, "xf_admit_load: null argument");
  XF_TRY(admit_check_params("xf_admit_load", want.L, want.h, want.N));
  File in;
  in.f = fopen(path, "rb");
  if (!in.f) return set_error(XF_EIO, "xf_admit_load: cannot open the admission file %s", path);
  FileHeader hd;
  if (fread(&hd, sizeof(hd), 1, in.f) != 1 || memcmp(hd.magic, kMagic, 8) != 0)
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

}  // namespace xf

extern "C" uint64_t xf_admit_slot(uint64_t key, uint64_t seed, int L, int j) {
  if (L < 2 || L > 32 || j < 0) return 0;
  return xf::admit_slot(key, seed, L, j);
}
