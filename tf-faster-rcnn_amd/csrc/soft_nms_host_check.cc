// Stand-alone sanitizer harness for csrc/softnms_math.h (not part of libfrcnn_hip.so; host only, never loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/soft_nms_host_check.cc -o soft_nms_host_check && ./soft_nms_host_check
// 1. softnms_host on the edge cases, every buffer a heap block of exactly the size the statement may touch: n = 0, n = 1, all scores
//    equal (ties go to the lower row), identical boxes, min_score = 0 (everything is emitted), a sigma so small that E returns 0.
// 2. softnms_exp_neg against libm's exp over every ov = i * 2^-24, i = 0 ... 2^24, for sigma in {0.1, 0.5, 2.0}: the largest relative
//    distance in double and the number of ov whose float32 weight differs from (float)exp(...).  Condition: no float32 weight is more
//    than 1 ulp away.  Measured (x86-64, glibc): largest relative distance 2.2e-16; differing float32 weights 0 of 50331651.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "softnms_math.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
  if (!ok) printf("FAILED %s\n", what), ++failures;
}

struct Run {
  int n, m;
  float* out;
  int* idx;
};
// one class through the statement; out / idx are heap blocks of exactly n rows
static Run run(const float* dets, int n, double thresh, int rule, int method, double sigma, float min_score) {
  const size_t nn = n ? (size_t)n : 1;
  float* d = (float*)malloc(sizeof(float) * 5 * nn);
  if (n) memcpy(d, dets, sizeof(float) * 5 * (size_t)n);
  float* cur = (float*)malloc(sizeof(float) * nn);
  uint64_t* key = (uint64_t*)malloc(sizeof(uint64_t) * nn);
  Run r = {n, 0, (float*)malloc(sizeof(float) * 5 * nn), (int*)malloc(sizeof(int) * nn)};
  r.m = softnms_host(d, n, softnms_thresh_f32(thresh, rule), rule, method, sigma, min_score, cur, key, r.out, r.idx);
  free(key), free(cur), free(d);
  return r;
}
static void done(Run& r) { free(r.out), free(r.idx); }

static int ulp_distance(float a, float b) {
  const int64_t x = (int64_t)softnms_f32_bits(a), y = (int64_t)softnms_f32_bits(b);       // both weights are >= 0
  return (int)(x > y ? x - y : y - x);
}

int main() {
  {                                                                                         // n = 0
    Run r = run(nullptr, 0, 0.3, SOFTNMS_RULE_CPU, SOFTNMS_LINEAR, 0.5, 0.001f);
    expect(r.m == 0, "n = 0");
    done(r);
  }
  {                                                                                         // n = 1, above and below min_score
    const float d[5] = {1, 2, 30, 40, 0.5f};
    Run r = run(d, 1, 0.3, SOFTNMS_RULE_GPU, SOFTNMS_GAUSSIAN, 0.5, 0.001f);
    expect(r.m == 1 && r.idx[0] == 0 && r.out[4] == 0.5f && r.out[2] == 30.0f, "n = 1");
    done(r);
    r = run(d, 1, 0.3, SOFTNMS_RULE_GPU, SOFTNMS_GAUSSIAN, 0.5, 0.75f);
    expect(r.m == 0 && r.idx[0] == -1 && r.out[4] == 0.0f, "n = 1 below min_score");
    done(r);
  }
  {                                                                                         // all scores equal, disjoint boxes: row order
    float d[5 * 6];
    for (int i = 0; i < 6; ++i) d[5 * i] = 100.0f * i, d[5 * i + 1] = 0, d[5 * i + 2] = 100.0f * i + 20, d[5 * i + 3] = 20, d[5 * i + 4] = 0.25f;
    for (int method = 1; method <= 2; ++method) {
      Run r = run(d, 6, 0.3, SOFTNMS_RULE_CPU, method, 0.5, 0.001f);
      bool ok = r.m == 6;
      for (int i = 0; i < 6 && ok; ++i) ok = r.idx[i] == i && r.out[5 * i + 4] == 0.25f;
      expect(ok, "equal scores, disjoint boxes");
      done(r);
    }
  }
  {                                                                                         // identical boxes: IoU 1 with every other one
    float d[5 * 4];
    for (int i = 0; i < 4; ++i) d[5 * i] = 3, d[5 * i + 1] = 4, d[5 * i + 2] = 50, d[5 * i + 3] = 60, d[5 * i + 4] = 0.9f - 0.1f * i;
    Run r = run(d, 4, 0.3, SOFTNMS_RULE_CPU, SOFTNMS_LINEAR, 0.5, 0.001f);                  // w = 1 - 1 = 0: the rest falls to 0 < min_score
    expect(r.m == 1 && r.idx[0] == 0 && r.idx[1] == -1, "identical boxes, linear");
    done(r);
    r = run(d, 4, 0.3, SOFTNMS_RULE_CPU, SOFTNMS_LINEAR, 0.5, 0.0f);                        // min_score = 0: all four, the decayed ones at 0.0
    expect(r.m == 4 && r.idx[1] == 1 && r.idx[3] == 3 && r.out[5 + 4] == 0.0f && r.out[15 + 4] == 0.0f, "identical boxes, min_score = 0");
    done(r);
    r = run(d, 4, 0.3, SOFTNMS_RULE_GPU, SOFTNMS_GAUSSIAN, 0.5, 0.001f);                    // w = exp(-2) each time a box is picked
    const float w = (float)softnms_exp_neg(-2.0);
    expect(r.m == 4 && r.out[5 + 4] == d[9] * w && r.out[10 + 4] == (d[14] * w) * w,"identical boxes, gaussian");
    expect(r.out[4] >= r.out[9] && r.out[9] >= r.out[14] && r.out[14] >= r.out[19], "non-increasing");
    done(r);
    r = run(d, 4, 0.3, SOFTNMS_RULE_GPU, SOFTNMS_GAUSSIAN, 1e-3, 0.0f);                     // -1 / 1e-3 < -150: E = 0
    expect(softnms_exp_neg(-1.0 / 1e-3) == 0.0 && r.m == 4 && r.out[4] == 0.9f && r.out[9] == 0.0f && r.idx[1] == 1, "E = 0");
    done(r);
  }
  expect(softnms_exp_neg(0.0) == 1.0 && softnms_exp_neg(-0.0) == 1.0 && softnms_exp_neg(-150.5) == 0.0, "E at the ends");
  expect(!softnms_args_ok(2, 1, 0.5, 0.0f) && !softnms_args_ok(0, 3, 0.5, 0.0f) && !softnms_args_ok(0, 1, 0.0, 0.0f) &&
         !softnms_args_ok(0, 1, NAN, 0.0f) && !softnms_args_ok(0, 1, 0.5, NAN) && softnms_args_ok(1, 2, 0.5, 0.0f), "argument rule");

  double worst = 0.0;
  long long differ = 0, beyond = 0, total = 0;
  const double sigmas[3] = {0.1, 0.5, 2.0};
  for (int s = 0; s < 3; ++s)
    for (long long i = 0; i <= (1ll << 24); ++i) {
      const float ov = (float)i * (1.0f / 16777216.0f);
      const double x = -((double)ov * (double)ov) / sigmas[s];
      const double want = exp(x), got = softnms_exp_neg(x);
      if (want > 0) {
        const double rel = fabs(got - want) / want;
        if (rel > worst) worst = rel;
      }
      const int u = ulp_distance((float)got, (float)want);
      differ += u != 0, beyond += u > 1, ++total;
    }
  printf("E sweep: largest relative distance from exp in double %.3g; float32 weights that differ %lld of %lld, more than 1 ulp away %lld\n",
         worst, differ, total, beyond);
  expect(beyond == 0, "a float32 weight more than 1 ulp from (float)exp");
  printf(failures ? "soft_nms_host_check: %d FAILED\n" : "soft_nms_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
