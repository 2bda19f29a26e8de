// Soft-NMS (Bodla et al. 2017, "Improving Object Detection With One Line of Code"), the per-class rule as plain host + device C++:
// csrc/detect_post.hip (the kernels k_perclass_soft_nms / k_soft_nms and the host entry frcnn_soft_nms_host) and the stand-alone
// harness csrc/soft_nms_host_check.cc include this one statement.
//
//   candidates   n boxes x1,y1,x2,y2 (float32), their float32 scores, each one's original row index r
//   IoU          the arithmetic of iou_suppresses (csrc/common.h): float32, "+1" widths, rmax / rmin, one rounding per operation (every
//                TU is built with -ffp-contract=off), IEEE division; the VALUE ovr comes back, not a decision
//   the loop     1. among the unselected candidates the largest key softnms_key(current score, r): the largest score, ties to the lower r
//                2. that score < min_score: stop
//                3. emit (box, current score, r)
//                4. every other unselected candidate j: score_j = score_j * w(ov(picked, j)), ONE float32 multiply
//                5. back to 1
//   linear (1)   w = 1.0f - ov where the hard rule would have suppressed -- rule CPU: ov >= thresh_to_f32(thresh); rule GPU:
//                ov > (float)thresh -- else 1.0f: linear decays exactly the set hard NMS deletes
//   gaussian (2) w = (float)E(-((double)ov * (double)ov) / sigma) for every j; sigma a double > 0
//   E(x), x <= 0 softnms_exp_neg below: IEEE double + - * / and integer bit operations only, no exp() / expf() on either side, so host
//                and gfx950 return the same bits; E(x) = 0 for x < -150.  Against libm's exp over every ov = i * 2^-24, i = 0 ... 2^24,
//                sigma in {0.1, 0.5, 2.0} (csrc/soft_nms_host_check.cc, profiles/soft_nms.txt): largest relative distance in double
//                2.2e-16; float32 weights that differ from (float)exp(...): 0 of 50331651, none by more than 1 ulp.
//
// Scores only fall, so the emission order is non-increasing in the final score and needs no sort; a candidate never emitted is dropped.
// Scores and boxes are finite (a NaN has no place in the order).  A weight of exactly 1.0f leaves the score's bits as they are, so the
// multiply may be skipped where ov == 0 (E(-0.0) == 1.0 exactly) or where the linear test fails.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SOFTNMS_HD __host__ __device__ __forceinline__
#else
#define SOFTNMS_HD inline
#endif

#define SOFTNMS_LINEAR 1
#define SOFTNMS_GAUSSIAN 2
#define SOFTNMS_RULE_CPU 0                    // == FRCNN_NMS_RULE_CPU
#define SOFTNMS_RULE_GPU 1                    // == FRCNN_NMS_RULE_GPU
#define SOFTNMS_MAX 1024                      // candidates per class

SOFTNMS_HD uint32_t softnms_f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
SOFTNMS_HD float softnms_bits_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// sortable_u32(score) of csrc/common.h and its order: (score descending, r ascending) <=> key descending; never 0 for a finite score;
// -0.0 and +0.0 share one value (r decides between them), every NaN maps to 0xffffffff, above +inf.  The score that is written out is
// read from where it is kept (cur[] here, the lane's registers on the device), never rebuilt from the key.
SOFTNMS_HD uint32_t softnms_sortable(float f) {
  uint32_t b = softnms_f32_bits(f);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SOFTNMS_HD uint64_t softnms_key(float score, uint32_t r) { return ((uint64_t)softnms_sortable(score) << 32) | (uint64_t)(0xffffffffu - r); }

SOFTNMS_HD float softnms_rmax(float a, float b) { return a >= b ? a : b; }
SOFTNMS_HD float softnms_rmin(float a, float b) { return a <= b ? a : b; }
SOFTNMS_HD float softnms_area(float x1, float y1, float x2, float y2) { return ((x2 - x1) + 1.0f) * ((y2 - y1) + 1.0f); }
// a = the picked box, b = the candidate; aa / ab their softnms_area
SOFTNMS_HD float softnms_iou(float ax1, float ay1, float ax2, float ay2, float aa, float bx1, float by1, float bx2, float by2, float ab) {
  const float xx1 = softnms_rmax(ax1, bx1), yy1 = softnms_rmax(ay1, by1);
  const float xx2 = softnms_rmin(ax2, bx2), yy2 = softnms_rmin(ay2, by2);
  const float w = softnms_rmax(0.0f, (xx2 - xx1) + 1.0f);
  const float h = softnms_rmax(0.0f, (yy2 - yy1) + 1.0f);
  const float inter = w * h;
  return inter / ((aa + ab) - inter);
}

// exp(x) for x <= 0: x = k ln2 + r with k = round(x / ln2), |r| <= 0.35 (ln2 split so that k * hi is exact), the Taylor polynomial of
// degree 13 in r by Horner (the first dropped term is below 4e-18), times 2^k built from its exponent bits (k >= -217: always normal).
SOFTNMS_HD double softnms_exp_neg(double x) {
  if (x < -150.0) return 0.0;
  if (!(x < 0.0)) return 1.0;
  const double t = x * 1.4426950408889634074;
  const long long k = (long long)(t - 0.5);
  const double kd = (double)k;
  const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const uint64_t bits = (uint64_t)(1023 + k) << 52;
  double s;
  __builtin_memcpy(&s, &bits, 8);
  return p * s;
}

// the float32 threshold the linear test compares with (thresh_to_f32 of csrc/common.h for the CPU rule)
inline float softnms_thresh_f32(double thresh, int rule) {
  float f = (float)thresh;
  if (rule == SOFTNMS_RULE_CPU && (double)f < thresh) f = nextafterf(f, INFINITY);
  return f;
}

SOFTNMS_HD float softnms_weight_linear(float ov, float thr, int rule) {
  const bool hit = rule == SOFTNMS_RULE_CPU ? ov >= thr : ov > thr;
  return hit ? 1.0f - ov : 1.0f;
}
SOFTNMS_HD float softnms_weight_gaussian(float ov, double sigma) {
  if (ov == 0.0f) return 1.0f;                                       // E(-0.0) is exactly 1.0
  return (float)softnms_exp_neg(-((double)ov * (double)ov) / sigma);
}
SOFTNMS_HD float softnms_weight(float ov, int method, float thr, int rule, double sigma) {
  return method == SOFTNMS_LINEAR ? softnms_weight_linear(ov, thr, rule) : softnms_weight_gaussian(ov, sigma);
}

inline bool softnms_args_ok(int rule, int method, double sigma, float min_score) {
  return (rule == SOFTNMS_RULE_CPU || rule == SOFTNMS_RULE_GPU) && (method == SOFTNMS_LINEAR || method == SOFTNMS_GAUSSIAN) &&
         sigma > 0 && min_score == min_score;
}

// The loop as written, one class on the host.  dets [n,5] = x1,y1,x2,y2,score (row i is candidate r = i); cur [n] scratch (the current
// scores), key [n] scratch (0 = selected).  out_dets [n,5] / out_index [n]: the emitted rows in order, the rest 0 / -1.  -> the count
inline int softnms_host(const float* dets, int n, float thr, int rule, int method, double sigma, float min_score, float* cur,
                        uint64_t* key, float* out_dets, int* out_index) {
  for (int i = 0; i < n; ++i) cur[i] = dets[5 * (size_t)i + 4], key[i] = softnms_key(cur[i], (uint32_t)i);
  int m = 0;
  for (;;) {
    int best = -1;
    for (int i = 0; i < n; ++i)
      if (key[i] != 0 && (best < 0 || key[i] > key[best])) best = i;
    if (best < 0 || cur[best] < min_score) break;
    const float* a = dets + 5 * (size_t)best;
    const float aa = softnms_area(a[0], a[1], a[2], a[3]);
    float* o = out_dets + 5 * (size_t)m;
    o[0] = a[0], o[1] = a[1], o[2] = a[2], o[3] = a[3], o[4] = cur[best];
    out_index[m++] = best;
    key[best] = 0;
    for (int j = 0; j < n; ++j) {
      if (key[j] == 0) continue;
      const float* b = dets + 5 * (size_t)j;
      const float ov = softnms_iou(a[0], a[1], a[2], a[3], aa, b[0], b[1], b[2], b[3], softnms_area(b[0], b[1], b[2], b[3]));
      cur[j] = cur[j] * softnms_weight(ov, method, thr, rule, sigma);
      key[j] = softnms_key(cur[j], (uint32_t)j);
    }
  }
  for (int i = m; i < n; ++i) {
    float* o = out_dets + 5 * (size_t)i;
    o[0] = o[1] = o[2] = o[3] = o[4] = 0.0f;
    out_index[i] = -1;
  }
  return m;
}
