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
// A shared filter's host side: xf_admit_range over L x world (disjoint, ordered, word-aligned,
// covering, empty ranges last); the file rank 0 writes from the gathered ranges, byte for byte the
// one-worker file; every rank's ranged read of it, of a file cut short in another rank's range, and
// of a counter above the threshold inside and outside its own range.
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

  // ---- a shared filter: the slot partition
  for (int L : {2, 3, 10, 26, 32})
    for (int world : {1, 2, 3, 7, 8, 255, 256}) {
      uint64_t at = 0;
      bool empty_seen = false, ok = true;
      for (int r = 0; r < world; ++r) {
        uint64_t first = 1, n = 1;
        ok = ok && xf_admit_range(L, world, r, &first, &n) == XF_OK && first == at &&
             first % 4 == 0 && n % 4 == 0 && !(empty_seen && n) && n <= (1ull << 32);
        empty_seen = empty_seen || n == 0;
        at += n;
      }
      expect(ok && at == (1ull << L), "the ranges partition the slots");
    }
  {
    uint64_t first = 0, n = 0;
    expect(xf_admit_range(2, 3, 1, &first, &n) == XF_OK && first == 4 && n == 0, "L 2, world 3");
    expect(xf_admit_range(10, 1, 0, nullptr, nullptr) == XF_OK, "null outputs");
    expect(xf_admit_range(1, 1, 0, &first, &n) == XF_EINVAL && names("admit_log2_slots"), "L = 1");
    expect(xf_admit_range(10, 0, 0, &first, &n) == XF_EINVAL, "world 0");
    expect(xf_admit_range(10, 3, 3, &first, &n) == XF_EINVAL && names("rank 3"), "rank = world");
    expect(xf_admit_range(10, 3, -1, &first, &n) == XF_EINVAL, "rank -1");
  }
  // ---- the gathered write and the ranged reads
  for (int world : {1, 3, 7}) {
    // what rank 0 holds after the gather: the ranks' ranges one after the other
    std::vector<uint8_t> gathered;
    for (int r = 0; r < world; ++r) {
      uint64_t first = 0, n = 0;
      expect(xf_admit_range(p.L, world, r, &first, &n) == XF_OK, "range");
      gathered.insert(gathered.end(), c.begin() + first, c.begin() + first + n);
    }
    expect(gathered == c, "the gathered ranges are the counters in slot order");
    expect(xf::admit_file_write(path.c_str(), p, gathered.data()) == XF_OK, "gathered write");
    expect(xf::admit_file_read(path.c_str(), p, &back) == XF_OK && back == c, "one worker reads it");
    for (int r = 0; r < world; ++r) {
      uint64_t first = 0, n = 0;
      xf_admit_range(p.L, world, r, &first, &n);
      expect(xf::admit_file_read_range(path.c_str(), p, first, n, &back) == XF_OK &&
                 back == std::vector<uint8_t>(c.begin() + first, c.begin() + first + n),
             "a rank reads its range");
    }
  }
  expect(xf::admit_file_read_range(path.c_str(), p, 1024, 0, &back) == XF_OK && back.empty(),
         "a rank that owns nothing");
  expect(xf::admit_file_read_range(path.c_str(), p, 1000, 25, &back) == XF_EINVAL &&
             names("outside"), "a range beyond the counters");
  expect(xf::admit_file_read_range(path.c_str(), p, 1025, 0, &back) == XF_EINVAL, "first > 2^L");
  expect(xf::admit_file_read_range(path.c_str(), p, 0, 4, nullptr) == XF_EINVAL, "null vector");
  {
    xf::AdmitParams q = p;
    q.N = 6;
    expect(xf::admit_file_read_range(path.c_str(), q, 0, 4, &back) == XF_EINVAL &&
               names("saved with"), "ranged read, other parameters");
  }
  write_raw(path, raw_file(10, 3, 5, p.seed, 1024, 1000, 5));
  expect(xf::admit_file_read_range(path.c_str(), p, 0, 344, &back) == XF_EIO &&
             names("ends before"), "cut short in another rank's range");
  f = raw_file(10, 3, 5, p.seed, 1024, 1024, 5);
  f[40 + 700] = 6;
  write_raw(path, f);
  expect(xf::admit_file_read_range(path.c_str(), p, 688, 336, &back) == XF_EIO &&
             names("counter 700") && names("above admit_count"), "a bad counter in its range");
  expect(xf::admit_file_read_range(path.c_str(), p, 0, 344, &back) == XF_OK && back.size() == 344,
         "a bad counter in another rank's range is that rank's to refuse");
  remove(path.c_str());

  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("admit_host_check: all checks passed\n");
  return 0;
}
