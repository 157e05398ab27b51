// holdout_host_check.cc — the host side of held-out validation (xflow_amd/csrc/
// xf_holdout_host.cc: the exported decision of a row and the early-stop rule) driven from a main
// of its own, for a run under the host sanitizers.  No GPU, no Python:
//
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//     -Iinclude -Ixflow_amd/csrc tools/holdout_host_check.cc xflow_amd/csrc/xf_holdout_host.cc \
//     -o /tmp/holdout_host_check && /tmp/holdout_host_check
//
// Covers: the decision at the edge shares (0 holds nothing, a share outside [0, 1) holds nothing,
// 1 - 2^-24 holds nearly everything), ordinals across 2^32 and at the wrap of 2^64 against the
// header's formula written out again, the held share of 2^20 ordinals, that the salt separates
// the decision from an unsalted hash of the same seed; the stop rule on hand-written curves
// (strict improvement, ties, delta, NaN, P = 1, n < P, n = 0) and its quiet refusals, with curves
// that end exactly at their last element (a read past it is the sanitizer's to report).
#include <math.h>
#include <stdio.h>

#include <vector>

#include "xf_holdout.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAILED: %s\n", what);
  }
}

static uint64_t mix(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

static bool stops(std::vector<double> curve, int patience, double delta, int want_best) {
  // (a heap copy of exactly n doubles: one past the end is out of bounds)
  int best = 99;
  const int s = xf_holdout_should_stop(curve.data(), (int)curve.size(), patience, delta, &best);
  expect(best == want_best, "the best epoch of a curve");
  return s == 1;
}

int main() {
  expect(XF_HOLDOUT_SALT == 0x6a09e667f3bcc909ull, "the salt");
  const uint64_t seeds[] = {0, 12345, 0xfedcba9876543210ull}, streams[] = {0, 3};
  const uint64_t firsts[] = {0, 0xFFFFFFF0ull, 0xFFFFFFFFFFFFFFF0ull};
  const float shares[] = {0.0f, ldexpf(1, -32), 0.001f, 0.25f, 0.5f, 1.0f - ldexpf(1, -24)};
  for (uint64_t seed : seeds)
    for (uint64_t stream : streams)
      for (uint64_t first : firsts)
        for (float share : shares) {
          const uint64_t T = (uint64_t)floor((double)share * 4294967296.0);
          for (uint64_t i = 0; i < 32; ++i) {
            const uint64_t ordinal = first + i;  // (wraps past 2^64 - 1)
            const bool want = (mix(mix(seed ^ stream ^ XF_HOLDOUT_SALT) + ordinal) >> 32) < T;
            expect(xf_holdout_held(seed, stream, ordinal, share) == (want ? 1 : 0),
                   "the decision against the header's formula");
            if (share == 0.0f)
              expect(!xf_holdout_held(seed, stream, ordinal, share), "share 0 holds nothing");
          }
        }
  for (float bad : {-0.5f, 1.0f, 1.5f, NAN, INFINITY})
    for (uint64_t o = 0; o < 64; ++o)
      expect(xf_holdout_held(1, 2, o, bad) == 0, "a share outside [0, 1) holds nothing");
  long held = 0, nearly = 0, same = 0;
  const long n = 1 << 20;
  for (long o = 0; o < n; ++o) {
    const bool h = xf_holdout_held(7, 1, (uint64_t)o, 0.25f);
    held += h;
    nearly += xf_holdout_held(7, 1, (uint64_t)o, 1.0f - ldexpf(1, -24));
    same += h == ((mix(mix(7 ^ 1) + (uint64_t)o) >> 32) < (1ull << 30));  // the unsalted hash
  }
  // 5 sigma of Binomial(n, p): 5 sqrt(p (1 - p) / n)
  expect(fabs((double)held / n - 0.25) <= 5 * sqrt(0.25 * 0.75 / n), "the held share at 0.25");
  expect(nearly >= n - 8, "1 - 2^-24 holds nearly everything");
  // independent of the unsalted decision: they agree on 0.25 * 0.25 + 0.75 * 0.75 = 0.625
  expect(fabs((double)same / n - 0.625) <= 5 * sqrt(0.625 * 0.375 / n), "the salt separates");

  expect(!stops({0.5, 0.4, 0.3, 0.2}, 1, 0.0, 3), "strict improvement never stops");
  expect(stops({0.5, 0.4, 0.41}, 1, 0.0, 1), "one worse epoch, P = 1");
  expect(!stops({0.5, 0.4, 0.41}, 2, 0.0, 1), "one worse epoch, P = 2");
  expect(stops({0.5, 0.4, 0.41, 0.42}, 2, 0.0, 1), "two worse epochs, P = 2");
  expect(stops({0.5, 0.4, 0.4}, 1, 0.0, 1), "a tie is no improvement");
  expect(stops({0.5, 0.45}, 1, 0.1, 0), "delta: not below best - delta");
  expect(!stops({0.5, 0.39}, 1, 0.1, 1), "delta: below best - delta");
  expect(!stops({0.5, NAN}, 1, 0.0, 0), "a NaN never stops");
  expect(stops({0.5, NAN, 0.6}, 1, 0.0, 0), "a NaN never improves");
  expect(!stops({0.5, NAN, 0.4}, 1, 0.0, 2), "an improvement after a NaN");
  expect(!stops({NAN, NAN}, 1, 0.0, -1), "NaN only: no best");
  expect(!stops({0.5}, 1, 0.0, 0), "one epoch");
  expect(!stops({0.5, 0.6}, 3, 0.0, 0), "n < P");
  expect(!stops({0.5, 0.6, 0.7}, 0, 0.0, 0), "P = 0 is off");
  expect(!stops({}, 1, 0.0, -1), "no epoch");
  int best = 5;
  const double one[1] = {0.5};
  expect(xf_holdout_should_stop(nullptr, 4, 1, 0.0, &best) == 0 && best == -1, "a null curve");
  expect(xf_holdout_should_stop(one, 1, 1, -1.0, &best) == 0 && best == -1, "a negative delta");
  expect(xf_holdout_should_stop(one, 1, 1, NAN, &best) == 0 && best == -1, "a NaN delta");
  expect(xf_holdout_should_stop(one, 1, 1, 0.0, nullptr) == 0, "best may be null");
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("holdout_host_check: ok\n");
  return 0;
}
