// cross_host_check.cc — the host side of feature crosses (xflow_amd/csrc/xf_cross_host.cc: the
// spec's parser, the key function, the create-time checks, the emit's knobs) driven from a main of
// its own, for a run under the host sanitizers.  No GPU, no Python:
//
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//     -Iinclude -Ixflow_amd/csrc tools/cross_host_check.cc xflow_amd/csrc/xf_cross_host.cc \
//     xflow_amd/csrc/xf_io.cc -o /tmp/cross_host_check -lpthread && /tmp/cross_host_check
//
// Covers: the six known answers of the key; the parser on good specs (one pair, two, both orders,
// the ends of the id range, 32 pairs, arrays of exactly the spec's size) and on every malformed one
// (empty, a self-cross, a pair twice, 33 pairs, a wrong separator, a missing id, a sign, 2^31, a
// blank, a leading and a trailing comma, an id of 30 digits, arrays too small), each refusal
// naming its piece; the create-time checks of the spec and of the base; the knobs' ranges.
#include <stdio.h>
#include <string.h>

#include <string>

#include "xf_common.h"
#include "xf_cross.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, xf_last_error());
  }
}

static bool names(const char *word) { return strstr(xf_last_error(), word) != nullptr; }

static bool refused(const std::string &spec, const char *piece) {
  int32_t fa[32], fb[32];
  int n = -1;
  return xf_cross_parse(spec.c_str(), fa, fb, 32, &n) == XF_EINVAL && n == 0 && names(piece);
}

static std::string chain(int npairs) {
  std::string s;
  for (int p = 0; p < npairs; ++p)
    s += (p ? "," : "") + std::to_string(p) + "*" + std::to_string(p + 1);
  return s;
}

int main() {
  // the key
  const struct {
    uint64_t ka, kb;
    int32_t fa, fb;
    uint64_t want;
  } known[] = {{0, 0, 0, 1, 0xb18a02f46d8d86c3ull},
               {1, 2, 3, 4, 0x9e115e4b8512df01ull},
               {2, 1, 3, 4, 0x2ab13db52cdaf5f3ull},
               {1, 2, 4, 3, 0x9ad29f2584d7d0f9ull},
               {~0ull, ~0ull, 2147483647, 0, 0x6597064ef50b7085ull},
               {0x0123456789abcdefull, 0xfedcba9876543210ull, 17, 16, 0x3d29a0d61dd42f35ull}};
  for (const auto &k : known)
    expect(xf_cross_key(k.ka, k.kb, k.fa, k.fb) == k.want, "a known answer of xf_cross_key");
  expect(xf::cross_sat_add(~0ull - 1, 1) == ~0ull && xf::cross_sat_add(~0ull, 5) == ~0ull &&
             xf::cross_sat_add(1ull << 63, 1ull << 63) == ~0ull && xf::cross_sat_add(3, 4) == 7,
         "the saturating sum");

  // the parser: good specs
  int32_t fa[32], fb[32];
  int n = 0;
  expect(xf_cross_parse("2*3", fa, fb, 32, &n) == XF_OK && n == 1 && fa[0] == 2 && fb[0] == 3,
         "2*3");
  expect(xf_cross_parse("2*3,16*17", fa, fb, 2, &n) == XF_OK && n == 2 && fa[1] == 16 &&
             fb[1] == 17, "2*3,16*17 into arrays of two");
  expect(xf_cross_parse("3*2,2*3", fa, fb, 32, &n) == XF_OK && n == 2, "both orders");
  expect(xf_cross_parse("0*2147483647", fa, fb, 32, &n) == XF_OK && fa[0] == 0 &&
             fb[0] == 2147483647, "the ends of the id range");
  expect(xf_cross_parse(chain(32).c_str(), fa, fb, 32, &n) == XF_OK && n == 32 && fa[31] == 31 &&
             fb[31] == 32, "32 pairs");
  // ... and malformed ones
  expect(refused("", "empty"), "the empty spec");
  expect(refused("2*2", "'2*2'"), "a self-cross");
  expect(refused("2*3,2*3", "'2*3'"), "a pair twice");
  expect(refused(chain(33), "'32*33'"), "33 pairs");
  expect(refused("2x3", "'2x3'"), "a wrong separator");
  expect(refused("2*", "'2*'"), "a missing id");
  expect(refused("*3", "'*3'"), "a missing first id");
  expect(refused("-1*3", "'-1*3'"), "a sign");
  expect(refused("2*2147483648", "'2*2147483648'"), "2^31");
  expect(refused("2*123456789012345678901234567890", "'2*1234"), "an id of 30 digits");
  expect(refused("2*3 ", "'2*3 '"), "a blank");
  expect(refused("2*3,", "''"), "a trailing comma");
  expect(refused(",2*3", "''"), "a leading comma");
  expect(refused("2*3,,4*5", "''"), "two commas");
  expect(xf_cross_parse("2*3,16*17", fa, fb, 1, &n) == XF_EINVAL && n == 0 && names("2 pairs"),
         "arrays too small");
  expect(xf_cross_parse(nullptr, fa, fb, 32, &n) == XF_EINVAL, "a null spec");

  // the create-time checks
  const int32_t a2[3] = {2, 4, 2}, b2[3] = {3, 5, 3}, self[1] = {7}, neg[1] = {-1};
  expect(xf::cross_check_spec("t", a2, b2, 2) == XF_OK, "a good spec");
  expect(xf::cross_check_spec("t", a2, b2, 3) == XF_EINVAL && names("2*3"), "a pair twice");
  expect(xf::cross_check_spec("t", self, self, 1) == XF_EINVAL && names("7*7"), "a self-cross");
  expect(xf::cross_check_spec("t", neg, a2, 1) == XF_EINVAL && names("-1*2"), "a negative id");
  expect(xf::cross_check_spec("t", a2, b2, 0) == XF_EINVAL && names("1 .. 32"), "no pair");
  expect(xf::cross_check_spec("t", a2, b2, 33) == XF_EINVAL && names("1 .. 32"), "33 pairs");
  expect(xf::cross_check_spec("t", nullptr, b2, 1) == XF_EINVAL, "null arrays");
  expect(xf::cross_check_base("t", 0, 32) == XF_OK && xf::cross_check_base("t", 2147483647, 1) ==
             XF_OK, "good bases");
  expect(xf::cross_check_base("t", -1, 1) == XF_EINVAL && names("cross_fgid_base=-1"), "base -1");
  expect(xf::cross_check_base("t", 2147483647, 2) == XF_EINVAL, "a base that leaves int32");

  // the knobs
  expect(xf::cross_short_max() == 64 && xf::cross_lds_chunks() == 2048, "the knobs' defaults");
  expect(xf::cross_set_knob("cross_short_max", 0) == XF_OK && xf::cross_short_max() == 0 &&
             xf::cross_set_knob("cross_short_max", 65) != XF_OK &&
             xf::cross_set_knob("cross_short_max", 64) == XF_OK, "cross_short_max in 0 .. 64");
  expect(xf::cross_set_knob("cross_lds_chunks", 0) != XF_OK &&
             xf::cross_set_knob("cross_lds_chunks", 4096) != XF_OK &&
             xf::cross_set_knob("cross_lds_chunks", 16) == XF_OK && xf::cross_lds_chunks() == 16,
         "cross_lds_chunks in 1 .. 2048");
  expect(xf::cross_set_knob("something_else", 1) != XF_OK, "another knob's name");

  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("cross_host_check: all checks passed\n");
  return 0;
}
