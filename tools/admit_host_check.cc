// admit_host_check.cc — the host side of feature admission (xflow_amd/csrc/xf_admit_host.cc: the
// parameter check, the slot function, the counter file) driven from a main of its own, for a run
// under the host sanitizers.  No GPU, no Python:
//
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//     -Iinclude -Ixflow_amd/csrc tools/admit_host_check.cc xflow_amd/csrc/xf_admit_host.cc \
//     xflow_amd/csrc/xf_io.cc -o /tmp/admit_host_check -lpthread && /tmp/admit_host_check /tmp
//
// Covers: every out-of-range parameter; a save / load round trip; loads of hand-made files — a
// missing one, a wrong magic, a header that ends early, each of the four parameters off by one,
// a wrong counter count, a file that ends inside its counters, a counter above the threshold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "xf_admit.h"
#include "xf_common.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, xf_last_error());
  }
}

static bool names(const char *word) { return strstr(xf_last_error(), word) != nullptr; }

static void write_raw(const std::string &path, const std::vector<uint8_t> &bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
    fprintf(stderr, "cannot write %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
}

// a counter file made by hand: the layout xf_admit.h documents
static std::vector<uint8_t> raw_file(uint32_t L, uint32_t h, uint32_t N, uint64_t seed,
                                     uint64_t slots, size_t counters, uint8_t value) {
  std::vector<uint8_t> b(40 + counters, value);
  memcpy(&b[0], "XFADMIT1", 8);
  const uint32_t zero = 0;
  memcpy(&b[8], &L, 4);
  memcpy(&b[12], &h, 4);
  memcpy(&b[16], &N, 4);
  memcpy(&b[20], &zero, 4);
  memcpy(&b[24], &seed, 8);
  memcpy(&b[32], &slots, 8);
  return b;
}

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/admit_host_check.admit";

  // parameters
  expect(xf::admit_check_params("t", 10, 3, 2) == XF_OK, "good parameters");
  expect(xf::admit_check_params("t", 1, 3, 2) == XF_EINVAL && names("admit_log2_slots"), "L = 1");
  expect(xf::admit_check_params("t", 33, 3, 2) == XF_EINVAL && names("admit_log2_slots"), "L = 33");
  expect(xf::admit_check_params("t", 10, 0, 2) == XF_EINVAL && names("admit_hashes"), "h = 0");
  expect(xf::admit_check_params("t", 10, 9, 2) == XF_EINVAL && names("admit_hashes"), "h = 9");
  expect(xf::admit_check_params("t", 10, 3, 0) == XF_EINVAL && names("admit_count"), "N = 0");
  expect(xf::admit_check_params("t", 10, 3, 256) == XF_EINVAL && names("admit_count"), "N = 256");

  // the slot function: inside the range at both ends of L, 0 outside the parameters
  for (int L : {2, 32})
    for (int j = 0; j < 8; ++j)
      for (uint64_t key : {0ull, 1ull, ~0ull, 1ull << 63})
        expect(xf_admit_slot(key, ~0ull, L, j) < (1ull << L), "slot inside 2^L");
  expect(xf_admit_slot(5, 0, 1, 0) == 0 && xf_admit_slot(5, 0, 33, 0) == 0 &&
             xf_admit_slot(5, 0, 10, -1) == 0, "slot of bad parameters");

  // round trip
  xf::AdmitParams p;
  p.L = 10;
  p.h = 3;
  p.N = 5;
  p.seed = 0xfedcba9876543210ull;
  std::vector<uint8_t> c(1u << p.L), back;
  for (size_t i = 0; i < c.size(); ++i) c[i] = (uint8_t)(i % 6);
  expect(xf::admit_file_write(path.c_str(), p, c.data()) == XF_OK, "write");
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_OK && back == c, "read back");
  expect(xf::admit_file_write((dir + "/no/such/dir/f").c_str(), p, c.data()) == XF_EIO, "no dir");
  expect(xf::admit_file_write(nullptr, p, c.data()) == XF_EINVAL, "null path");
  expect(xf::admit_file_read(path.c_str(), p, nullptr) == XF_EINVAL, "null vector");

  // other parameters: XF_EINVAL naming both sets
  for (int which = 0; which < 4; ++which) {
    xf::AdmitParams q = p;
    if (which == 0) q.L = 11;
    if (which == 1) q.h = 4;
    if (which == 2) q.N = 6;
    if (which == 3) q.seed += 1;
    expect(xf::admit_file_read(path.c_str(), q, &back) == XF_EINVAL && names("saved with") &&
               names("this filter has"), "other parameters");
  }

  // hand-made files
  expect(xf::admit_file_read((dir + "/admit_host_check.none").c_str(), p, &back) == XF_EIO &&
             names("admit_host_check.none"), "missing file");
  write_raw(path, std::vector<uint8_t>(17, 'x'));
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_EIO && names("not an admission file"),
         "header ends early");
  std::vector<uint8_t> f = raw_file(10, 3, 5, p.seed, 1024, 1024, 5);
  f[0] = 'Y';
  write_raw(path, f);
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_EIO && names("not an admission file"),
         "wrong magic");
  write_raw(path, raw_file(10, 3, 5, p.seed, 1024, 1024, 5));
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_OK && back.size() == 1024 &&
             back[1023] == 5, "hand-made file");
  write_raw(path, raw_file(10, 3, 5, p.seed, 512, 1024, 5));
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_EIO && names("512"), "counter count");
  write_raw(path, raw_file(10, 3, 5, p.seed, 1024, 1000, 5));
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_EIO && names("ends before"),
         "ends inside its counters");
  write_raw(path, raw_file(10, 3, 5, p.seed, 1024, 1024, 6));
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_EIO && names("above admit_count"),
         "counter above the threshold");
  write_raw(path, raw_file(0xffffffffu, 3, 5, p.seed, 1024, 0, 0));
  expect(xf::admit_file_read(path.c_str(), p, &back) == XF_EINVAL, "absurd header");
  remove(path.c_str());

  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("admit_host_check: all checks passed\n");
  return 0;
}
