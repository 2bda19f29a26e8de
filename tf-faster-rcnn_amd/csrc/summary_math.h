// TensorFlow's default histogram buckets (tensorflow/core/lib/histogram/histogram.cc, InitDefaultBucketsInner) and the bucket rule of
// Histogram::Add, as plain host + device C++: csrc/summary_stats.hip, the host entry frcnn_summary_limits and the stand-alone harness
// csrc/summary_host_check.cc all include this one statement.
//
//   v = 1e-12; while (v < 1e20) { push v; v *= 1.1; }    774 values, by REPEATED MULTIPLICATION in double (never pow: the limits must
//   then DBL_MAX;                                         match TensorFlow's bit for bit, and the product chain rounds 773 times)
//   negated and reversed in front, 0.0 between            -> 1551 limits, strictly increasing, limits[775] == 0.0
//
// bucket(x) = index of the first limit > (double)x (std::upper_bound).  +-0.0 fall in bucket 776 (limit 1e-12); every finite float lands in
// [1, 1550] because limits[0] = -DBL_MAX is never greater and limits[1550] = DBL_MAX always is.  Non-finite values have no bucket.
#pragma once
#include <float.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SUMMARY_HD __host__ __device__ __forceinline__
#else
#define SUMMARY_HD inline
#endif

#define SUMMARY_POS 774                       // positive limits below DBL_MAX
#define SUMMARY_BUCKETS (2 * SUMMARY_POS + 3) // 1551
#define SUMMARY_ZERO_BUCKET (SUMMARY_POS + 2) // 776: where +-0.0 are counted

struct SummaryLimits {
  double v[SUMMARY_BUCKETS];
};

// constexpr: the device copy is a constant-initialised table (IEEE double products, round to nearest even, whoever evaluates them --
// summary_host_check.cc compares the compile-time table with a run-time evaluation of the same loop).
SUMMARY_HD constexpr SummaryLimits summary_make_limits() {
  SummaryLimits L = {};
  double v = 1e-12;
  int n = 0;
  while (v < 1e20) {
    L.v[SUMMARY_POS + 2 + n] = v;             // 776 ...
    L.v[SUMMARY_POS - n] = -v;                // 774 ... downwards
    ++n;
    v *= 1.1;
  }
  // n == SUMMARY_POS here (checked by the harness and by tests/test_summary_cpu.py through frcnn_summary_limits)
  L.v[SUMMARY_POS + 2 + n] = DBL_MAX;
  L.v[SUMMARY_POS - n] = -DBL_MAX;
  L.v[SUMMARY_POS + 1] = 0.0;
  return L;
}

// upper_bound over `limits` (any address space the caller copied the table to): 11 probes, no early exit, x finite
SUMMARY_HD int summary_bucket(const double* limits, double x) {
  int lo = 0, len = SUMMARY_BUCKETS;          // first index in [lo, lo + len) whose limit is > x; lo + len if none
  while (len > 0) {
    const int half = len >> 1;
    if (limits[lo + half] > x) {
      len = half;
    } else {
      lo += half + 1;
      len -= half + 1;
    }
  }
  return lo;
}

SUMMARY_HD bool summary_finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }
