// Stand-alone sanitizer harness for csrc/iouloss_math.h (not part of libfrcnn_hip.so; host only, never loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -ffp-contract=off -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/iou_loss_host_check.cc -o iou_loss_host_check && ./iou_loss_host_check
// 1. iouloss_host on the edge cases, every buffer a heap block of exactly the size it may touch, all four kinds: no active slice, a
//    disjoint pair, an identical pair, a box enclosed in the other, dw / dh above the clamp, a NaN in an active and in an inactive slice,
//    RoI references (ref_cols 5) with K = 3, and 64 / 65 / 257 rows (the wave and block edges of the order of additions).
// 2. iouloss_exp against libm's exp over x = -12 + i 16.2 / 2^20 and iouloss_atan against atan over x = +-2^(i / 2^16 - 8),
//    i = 0 ... 2^20: the largest relative distance in double.  Condition: below 1e-15 each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "iouloss_math.h"

static int failures = 0;
static void expect(bool ok, const char* what, int kind) {
  if (!ok) printf("FAILED %s (kind %d)\n", what, kind), ++failures;
}

struct Case {
  long long N;
  int K, ref_cols;
  float *pred, *tgt, *iw, *ow, *refs, *grad, loss;
};
static Case make(long long N, int K, int ref_cols) {
  const size_t e = 4 * (size_t)N * K;
  Case c = {N, K, ref_cols, (float*)calloc(e, 4), (float*)calloc(e, 4), (float*)calloc(e, 4), (float*)calloc(e, 4),
            (float*)calloc((size_t)N * ref_cols, 4), (float*)malloc(e * 4), 0.0f};
  for (long long r = 0; r < N; ++r) {
    float* a = c.refs + r * ref_cols + (ref_cols == 5 ? 1 : 0);
    a[0] = 100.0f + 3.0f * (float)(r % 50), a[1] = 90.0f, a[2] = a[0] + 50.0f, a[3] = 160.0f;
  }
  return c;
}
static void set4(float* p, float a, float b, float c, float d) { p[0] = a, p[1] = b, p[2] = c, p[3] = d; }
// slice s active with weight ow, pred p*, target the fixed t0
static void slice(Case& c, long long s, float px, float py, float pw, float ph, float ow) {
  set4(c.pred + 4 * s, px, py, pw, ph), set4(c.tgt + 4 * s, 0.05f, -0.1f, 0.2f, -0.15f), set4(c.iw + 4 * s, 1, 1, 1, 1), set4(c.ow + 4 * s, ow, ow, ow, ow);
}
static void run(Case& c, int kind, const float* stds) {
  const float means[4] = {0, 0, 0, 0};
  memset(c.grad, 0xff, 16 * (size_t)c.N * c.K);                    // every element must be written
  iouloss_host(c.pred, c.tgt, c.iw, c.ow, c.N, c.K, c.refs, c.ref_cols, means, stds, kind, 1.0f, 1.0f, &c.loss, c.grad);
}
static void done(Case& c) { free(c.pred), free(c.tgt), free(c.iw), free(c.ow), free(c.refs), free(c.grad); }
static bool all_zero(const float* g, int n) {
  for (int i = 0; i < n; ++i)
    if (g[i] != 0.0f) return false;
  return true;
}
static bool all_finite(const float* g, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!iouloss_finite((double)g[i])) return false;
  return true;
}

int main() {
  const float one[4] = {1, 1, 1, 1}, head[4] = {0.1f, 0.1f, 0.2f, 0.2f};
  for (int kind = IOULOSS_IOU; kind <= IOULOSS_CIOU; ++kind) {
    {                                                                                       // no active slice: +0, all zero
      Case c = make(7, 2, 5);
      for (int i = 0; i < 56; ++i) c.pred[i] = NAN;
      run(c, kind, head);
      expect(c.loss == 0.0f && !signbit(c.loss) && all_zero(c.grad, 56), "no active slice", kind);
      done(c);
    }
    {                                                                                       // disjoint, identical, enclosed, clamped
      Case c = make(5, 1, 4);
      slice(c, 0, 3.05f, -0.05f, 0.3f, -0.25f, 0.25f), slice(c, 1, 0.05f, -0.1f, 0.2f, -0.15f, 0.25f), slice(c, 2, 0.07f, -0.07f, -0.8f, -0.95f, 0.25f);
      slice(c, 3, 0.1f, 0.0f, 5.0f, 0.3f, 0.25f), slice(c, 4, 0.0f, 0.2f, 0.1f, 4.5f, 0.25f);
      run(c, kind, one);
      expect(all_finite(c.grad, 20) && iouloss_finite((double)c.loss) && c.loss > 0.0f, "finite", kind);
      expect(kind == IOULOSS_IOU ? all_zero(c.grad, 4) : !all_zero(c.grad, 4), "disjoint: only the IoU kind has no gradient", kind);
      expect(c.grad[4] == 0.0f && c.grad[5] == 0.0f, "identical: the centre does not move the loss", kind);
      expect(c.grad[14] == 0.0f && c.grad[15] != 0.0f && c.grad[18] != 0.0f && c.grad[19] == 0.0f, "a clamped coordinate has gradient 0", kind);
      c.pred[9] = NAN;                                                                      // a NaN in the active slice 2
      const float g0 = c.grad[0], g12 = c.grad[12];
      run(c, kind, one);
      expect(c.loss != c.loss && c.grad[8] != c.grad[8] && c.grad[11] != c.grad[11] && c.grad[0] == g0 && c.grad[12] == g12, "NaN in an active slice", kind);
      set4(c.iw + 8, 0, 0, 0, 0);                                                           // the same slice inactive
      run(c, kind, one);
      expect(c.loss == c.loss && all_zero(c.grad + 8, 4) && c.grad[0] == g0, "NaN in an inactive slice", kind);
      done(c);
    }
    const long long rows[4] = {64, 65, 257, 70};                                            // wave and block edges; RoI references with K = 3
    for (int i = 0; i < 4; ++i) {
      Case c = make(rows[i], i == 3 ? 3 : 1, i == 3 ? 5 : 4);
      const long long S = c.N * c.K;
      for (long long s = 0; s < S; s += 2) slice(c, s, 0.01f * (float)(s % 17), -0.02f * (float)(s % 5), 0.3f, -0.1f, 0.01f);
      run(c, kind, i == 3 ? head : one);
      double sum = 0.0;                                                                     // the plain serial sum agrees to float32 rounding
      float g[4];
      const float zero[4] = {0, 0, 0, 0};
      const IouLossNorm nm = iouloss_norm(zero, i == 3 ? head : one);
      for (long long s = 0; s < S; ++s) {
        const float* a = c.refs + (s / c.K) * c.ref_cols + (c.ref_cols == 5 ? 1 : 0);
        sum += iouloss_slice(a, c.pred + 4 * s, c.tgt + 4 * s, c.iw + 4 * s, c.ow[4 * s], nm, kind, 1.0, g);
      }
      expect(all_finite(c.grad, 4 * (size_t)S) && fabs((double)c.loss - sum) <= 1e-6 * sum && all_zero(c.grad + 4, 4) && !all_zero(c.grad, 4), "rows", kind);
      done(c);
    }
  }
  const float bad_std[4] = {0.1f, 0.0f, 0.2f, 0.2f};
  expect(iouloss_args_ok(1, 1, 4, one, one, 1, 1.0f, 1.0f) && !iouloss_args_ok(0, 1, 4, one, one, 1, 1.0f, 1.0f) &&
         !iouloss_args_ok(1, 0, 4, one, one, 1, 1.0f, 1.0f) && !iouloss_args_ok(1, 1, 3, one, one, 1, 1.0f, 1.0f) &&
         !iouloss_args_ok(1, 1, 4, one, one, 0, 1.0f, 1.0f) && !iouloss_args_ok(1, 1, 4, one, one, 5, 1.0f, 1.0f) &&
         !iouloss_args_ok(1, 1, 4, one, bad_std, 1, 1.0f, 1.0f) && !iouloss_args_ok(1, 1, 4, one, one, 1, NAN, 1.0f) &&
         !iouloss_args_ok(1, 1, 4, one, one, 1, INFINITY, 1.0f) && !iouloss_args_ok(1, 1, 4, one, one, 1, 1.0f, 0.0f) &&
         iouloss_args_ok(1, 1, 5, one, one, 4, -2.0f, 3.0f), "argument rule", 0);
  expect(iouloss_exp(0.0) == 1.0 && iouloss_exp(-800.0) == 0.0 && iouloss_atan(0.0) == 0.0 && iouloss_atan(1.0) == 0.78539816339744830962 &&
         iouloss_atan(-1.0) == -iouloss_atan(1.0), "exp / atan at the ends", 0);

  double worst_exp = 0.0, worst_atan = 0.0;
  for (long long i = 0; i <= (1ll << 20); ++i) {
    const double x = -12.0 + (double)i * 16.2 / 1048576.0, want = exp(x), got = iouloss_exp(x);
    const double rel = fabs(got - want) / want;
    if (rel > worst_exp) worst_exp = rel;
    const double y = exp2((double)i / 65536.0 - 8.0);
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      const double w2 = atan(sgn * y), g2 = iouloss_atan(sgn * y);
      const double r2 = fabs(g2 - w2) / fabs(w2);
      if (r2 > worst_atan) worst_atan = r2;
    }
  }
  printf("sweep: largest relative distance in double, exp %.3g atan %.3g\n", worst_exp, worst_atan);
  expect(worst_exp < 1e-15 && worst_atan < 1e-15, "exp / atan too far from libm", 0);
  printf(failures ? "iou_loss_host_check: %d FAILED\n" : "iou_loss_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
