// Stand-alone sanitizer harness for csrc/ohem_math.h (not part of libfrcnn_hip.so; host only, never loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -ffp-contract=off -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/ohem_host_check.cc -o ohem_host_check && ./ohem_host_check
// 1. the statement on the edge cases, every buffer a heap block of exactly the size it may touch: no valid row, one row, fewer
//    candidates than the batch (they repeat), identical rows (ties go to the lower row), everything suppressed but one, NMS off, a NaN
//    logit (ranks first), a row that is neither foreground nor background.
// 2. ohem_log against libm's log over x = 1 + i 80 / 2^20 (the class sum for C = 81) and x = 2^(i / 2^16 - 8) (the width ratios),
//    softnms_exp_neg against exp over x = -i 40 / 2^20, i = 0 ... 2^20: the largest relative distance in double, and how many float32
//    roundings differ.  Condition: none by more than 1 ulp.  Measured (x86-64, glibc): log 4.7e-16, exp 2.2e-16, 0 of 3145731 differ.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ohem_math.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
  if (!ok) printf("FAILED %s\n", what), ++failures;
}

struct Case {
  int N, n, G, C, B;
  float *rois, *gt, *cls, *pred;                       // [N,5] [G,5] [N,C] [N,4C]
  OhemRow* rw;
  int *keep, counts[4];
};
static Case make(int N, int n, int G, int C, int B) {
  Case c = {N, n, G, C, B, (float*)calloc(5 * (size_t)N, 4), (float*)calloc(5 * (size_t)G, 4), (float*)calloc((size_t)N * C, 4),
            (float*)calloc((size_t)N * 4 * C, 4), (OhemRow*)calloc(N, sizeof(OhemRow)), (int*)calloc(B, sizeof(int)), {0, 0, 0, 0}};
  return c;
}
static void box(float* r, float x1, float y1, float x2, float y2) { r[1] = x1, r[2] = y1, r[3] = x2, r[4] = y2; }       // a roi row: (image, box)
static void gtbox(float* g, float x1, float y1, float x2, float y2, float cls) { g[0] = x1, g[1] = y1, g[2] = x2, g[3] = y2, g[4] = cls; }
static void run(Case& c, double nms_thresh, int rule) {
  OhemNorm nm = {{0, 0, 0, 0}, {0.1, 0.1, 0.2, 0.2}, {1, 1, 1, 1}};
  for (int r = 0; r < c.N; ++r) {
    OhemRow o;
    o.key = 0, o.loss = 0.0f, o.kind = -1, o.assigned = 0;
    if (r < c.n) o = ohem_score_row(c.rois + 5 * (size_t)r, (uint32_t)r, c.gt, c.G, c.C, c.cls + (size_t)r * c.C, c.pred + (size_t)r * 4 * c.C, 0.5, 0.5, 0.1, nm);
    c.rw[r] = o;
  }
  int* order = (int*)malloc(sizeof(int) * c.N);
  int* P = (int*)malloc(sizeof(int) * c.N);
  unsigned char* kept = (unsigned char*)malloc(c.N);
  ohem_select_rows(c.rw, c.rois, c.N, c.B, softnms_thresh_f32(nms_thresh, rule), nms_thresh > 0.0, rule, order, P, kept, c.keep, c.counts);
  // the rows go out through the same function as in the library, into blocks of exactly B rows
  float *o_rois = (float*)malloc(20 * (size_t)c.B), *o_sc = (float*)malloc(4 * (size_t)c.B), *o_lab = (float*)malloc(4 * (size_t)c.B);
  float *o_t = (float*)malloc(16 * (size_t)c.B * c.C), *o_i = (float*)malloc(16 * (size_t)c.B * c.C), *o_o = (float*)malloc(16 * (size_t)c.B * c.C);
  float* sc = (float*)calloc(c.N, 4);
  for (int s = 0; s < c.B; ++s) ohem_emit_row(s, c.keep[s], c.rw, c.rois, sc, c.gt, c.C, nm, o_rois, o_sc, o_lab, o_t, o_i, o_o);
  for (int s = 0; s < c.B; ++s) expect(c.keep[s] < 0 ? o_rois[5 * s + 3] == 0.0f : o_rois[5 * s + 3] == c.rois[5 * c.keep[s] + 3], "emitted roi");
  free(order), free(P), free(kept), free(o_rois), free(o_sc), free(o_lab), free(o_t), free(o_i), free(o_o), free(sc);
}
static void done(Case& c) { free(c.rois), free(c.gt), free(c.cls), free(c.pred), free(c.rw), free(c.keep); }

static int ulps(float a, float b) {
  int32_t x, y;
  memcpy(&x, &a, 4), memcpy(&y, &b, 4);
  if (x < 0) x = (int32_t)0x80000000 - x;
  if (y < 0) y = (int32_t)0x80000000 - y;
  const int64_t d = (int64_t)x - y;
  return (int)(d < 0 ? -d : d);
}

int main() {
  const int C = 21;
  {                                                                                         // no valid row
    Case c = make(4, 0, 1, C, 3);
    gtbox(c.gt, 10, 10, 50, 50, 3);
    run(c, 0.7, 0);
    expect(c.keep[0] == -1 && c.keep[2] == -1 && c.counts[0] + c.counts[1] + c.counts[2] + c.counts[3] == 0, "n = 0");
    done(c);
  }
  {                                                                                         // one foreground row, batch of 4: it repeats
    Case c = make(1, 1, 1, C, 4);
    gtbox(c.gt, 10, 10, 50, 50, 3), box(c.rois, 12, 11, 50, 52);
    run(c, 0.7, 1);
    expect(c.keep[0] == 0 && c.keep[3] == 0 && c.counts[0] == 4 && c.counts[1] == 0 && c.counts[2] == 1, "one row repeats");
    expect(c.rw[0].kind == 1 && c.rw[0].loss > 3.0f && c.rw[0].loss < 3.3f, "uniform logits: log 21 plus a small box term");
    done(c);
  }
  {   // six rows: 0-3 identical background boxes with equal loss, 4 foreground, 5 far away from everything with bg_lo 0.1 (neither)
    Case c = make(6, 6, 1, C, 4);
    gtbox(c.gt, 100, 100, 200, 200, 7);
    for (int r = 0; r < 4; ++r) box(c.rois + 5 * r, 100, 100, 140, 160);                    // IoU 0.24: background
    box(c.rois + 20, 101, 99, 199, 202), box(c.rois + 25, 400, 400, 450, 450);
    for (int r = 0; r < 6; ++r) c.cls[r * C + 7] = 2.0f;                                    // the background rows lose more
    run(c, 0.7, 0);
    expect(c.rw[5].kind == -1 && c.rw[5].key == 0 && c.counts[2] == 1 && c.counts[3] == 4, "candidates");
    // order: 0 1 2 3 (equal loss, by row) then 4; NMS keeps 0 and 4, then the suppressed 1 2 in order; output: fg first
    expect(c.keep[0] == 4 && c.keep[1] == 0 && c.keep[2] == 1 && c.keep[3] == 2 && c.counts[0] == 1 && c.counts[1] == 3, "suppressed rows follow");
    run(c, 0.0, 0);                                                                         // NMS off: 0 1 2 3
    expect(c.keep[0] == 0 && c.keep[3] == 3 && c.counts[0] == 0 && c.counts[1] == 4, "NMS off");
    c.cls[4 * C + 2] = NAN;                                                                 // a NaN logit ranks first
    run(c, 0.0, 0);
    expect(c.keep[0] == 4 && c.keep[1] == 0 && c.keep[3] == 2 && c.rw[4].loss != c.rw[4].loss, "NaN first");
    c.cls[4 * C + 2] = 0.0f, c.pred[4 * 4 * C + 4 * 7 + 1] = INFINITY;
    run(c, 0.0, 0);
    expect(c.keep[0] == 4 && c.rw[4].loss != c.rw[4].loss, "an infinite prediction is NaN too");
    done(c);
  }
  expect(!ohem_args_ok(4, 1, 21, 4, 1.5, 0) && !ohem_args_ok(4, 1, 21, 4, NAN, 0) && !ohem_args_ok(4, 0, 21, 4, 0.7, 0) &&
         !ohem_args_ok(4, 1, 21, 4, 0.7, 2) && ohem_args_ok(4, 1, 21, 4, -1.0, 1) && ohem_args_ok(4, 1, 21, 4, 1.0, 0), "argument rule");
  expect(ohem_log(1.0) == 0.0 && ohem_log(0.0) != ohem_log(0.0) && ohem_log(-1.0) != ohem_log(-1.0) && ohem_log(INFINITY) != ohem_log(INFINITY), "log at the ends");
  expect(ohem_key(NAN, 3) > ohem_key(1e30f, 0) && ohem_key(INFINITY, 3) == ohem_key(NAN, 3) && ohem_key(1.0f, 2) > ohem_key(1.0f, 3) &&
         ohem_key(2.0f, 9) > ohem_key(1.0f, 0) && ohem_key_row(ohem_key(0.5f, 77)) == 77, "keys");

  double worst_log = 0.0, worst_exp = 0.0;
  long long differ = 0, beyond = 0, total = 0;
  for (long long i = 0; i <= (1ll << 20); ++i) {
    const double xs[2] = {1.0 + (double)i * 80.0 / 1048576.0, exp2((double)i / 65536.0 - 8.0)};
    for (int k = 0; k < 2; ++k) {
      const double want = log(xs[k]), got = ohem_log(xs[k]);
      if (want != 0.0) {
        const double rel = fabs(got - want) / fabs(want);
        if (rel > worst_log) worst_log = rel;
      }
      const int u = ulps((float)got, (float)want);
      differ += u != 0, beyond += u > 1, ++total;
    }
    const double x = -(double)i * 40.0 / 1048576.0, want = exp(x), got = softnms_exp_neg(x);
    const double rel = fabs(got - want) / want;
    if (rel > worst_exp) worst_exp = rel;
    const int u = ulps((float)got, (float)want);
    differ += u != 0, beyond += u > 1, ++total;
  }
  printf("sweep: largest relative distance in double, log %.3g exp %.3g; float32 roundings that differ %lld of %lld, more than 1 ulp away %lld\n",
         worst_log, worst_exp, differ, total, beyond);
  expect(beyond == 0 && worst_log < 1e-15 && worst_exp < 1e-15, "log / exp too far from libm");
  printf(failures ? "ohem_host_check: %d FAILED\n" : "ohem_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
