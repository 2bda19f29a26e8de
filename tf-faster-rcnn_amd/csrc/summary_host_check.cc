// Stand-alone sanitizer harness for csrc/summary_math.h (not part of libfrcnn_hip.so):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/summary_host_check.cc -o summary_host_check && ./summary_host_check
// The compile-time table (what the device kernel's constant is initialised with) against a run-time evaluation of the loop in a heap block
// of exactly 1551 doubles; the bucket rule against std::upper_bound on the hand-made values of tests/test_summary_cpu.py, on the two
// float32 neighbours of every limit inside float32's range and on 2^22 seeded bit patterns.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "summary_math.h"

static constexpr SummaryLimits kStatic = summary_make_limits();

static int fail(const char* what, double a, double b) {
  printf("FAILED %s: %.17g %.17g\n", what, a, b);
  return 1;
}

int main() {
  double* lim = (double*)malloc(sizeof(double) * SUMMARY_BUCKETS);
  {
    const SummaryLimits L = summary_make_limits();
    memcpy(lim, L.v, sizeof(double) * SUMMARY_BUCKETS);
  }
  if (memcmp(lim, kStatic.v, sizeof(double) * SUMMARY_BUCKETS)) return fail("compile-time table != run-time table", 0, 0);
  {                                                         // histogram.cc's own loop, written out independently
    int n = 0;
    for (double v = 1e-12; v < 1e20; v *= 1.1) {
      if (n >= SUMMARY_POS) return fail("more than 774 positive limits", v, n);
      if (lim[SUMMARY_POS + 2 + n] != v || lim[SUMMARY_POS - n] != -v) return fail("limit", lim[SUMMARY_POS + 2 + n], v);
      ++n;
    }
    if (n != SUMMARY_POS) return fail("positive limit count", n, SUMMARY_POS);
  }
  if (lim[0] != -DBL_MAX || lim[SUMMARY_BUCKETS - 1] != DBL_MAX || lim[SUMMARY_POS + 1] != 0.0 || signbit(lim[SUMMARY_POS + 1]))
    return fail("ends / zero", lim[0], lim[SUMMARY_POS + 1]);
  for (int i = 1; i < SUMMARY_BUCKETS; ++i)
    if (!(lim[i - 1] < lim[i])) return fail("not increasing", lim[i - 1], lim[i]);

  auto want = [&](double x) { return (int)(std::upper_bound(lim, lim + SUMMARY_BUCKETS, x) - lim); };
  const float hand[] = {0.0f, -0.0f, 1e-13f, -1e-13f, 1e-12f, 1.0f, 1.1f, FLT_MAX, -FLT_MAX};
  const int hand_bucket[] = {776, 776, 776, 775, 776, 1066, 1067, 1550, 1};
  for (int i = 0; i < 9; ++i)
    if (summary_bucket(lim, (double)hand[i]) != hand_bucket[i]) return fail("hand-made value", hand[i], summary_bucket(lim, (double)hand[i]));
  long pairs = 0;
  for (int i = 1; i < SUMMARY_BUCKETS - 1; ++i) {
    if (i == SUMMARY_POS + 1 || fabs(lim[i]) > (double)FLT_MAX) continue;
    float below = (float)lim[i];                            // nearest float32, then stepped to the two sides of the limit
    while ((double)below >= lim[i]) below = nextafterf(below, -INFINITY);
    const float above = nextafterf(below, INFINITY);
    if ((double)above == lim[i]) return fail("a float32 equals a limit", above, lim[i]);
    if (summary_bucket(lim, (double)below) != i || summary_bucket(lim, (double)above) != i + 1) return fail("bracketing pair", below, above);
    ++pairs;
  }
  uint32_t s = 12345u;
  long finite = 0;
  for (int i = 0; i < (1 << 22); ++i) {
    s = s * 1664525u + 1013904223u;
    float x;
    memcpy(&x, &s, 4);
    if (!summary_finite_bits(s)) {
      if (isfinite(x)) return fail("finite_bits", x, 0);
      continue;
    }
    if (!isfinite(x)) return fail("finite_bits", x, 1);
    ++finite;
    const int b = summary_bucket(lim, (double)x);
    if (b != want((double)x) || b < 1 || b > SUMMARY_BUCKETS - 1) return fail("random value", x, b);
  }
  free(lim);
  printf("ok: 1551 limits, %ld bracketing pairs, %ld random finite values\n", pairs, finite);
  return 0;
}
