// Stand-alone sanitizer harness for csrc/boxvote_math.h (not part of libfrcnn_hip.so; host only, never loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/box_vote_host_check.cc -o box_vote_host_check && ./box_vote_host_check
// Every buffer is a heap block of exactly the size the statement may touch.
// 1. boxvote_host for n = 1, 2, 63, 64, 65, 130, 300, 1024 candidates in clusters, kept = every third candidate and kept = all n, at
//    vote_thresh 0.8, 0.5 and 1.0: scores untouched, every coordinate finite and inside the span of the candidates' coordinates, at 1.0 the
//    input bits (the candidates are distinct), at 0.5 some box moves once n >= 63; m = 0 and n = 0; a kept row that is no candidate; a
//    degenerate box (no "+1" area: IoU 0 with itself) stays.
// 2. boxvote_merge_host for (B, R, C) = (1, 1, 2), (2, 48, 3), (1, 512, 3) with counts 0, R, in between, below 0 and above R, with and
//    without bbox_pred and with num_rois NULL, against the rule written out a second time below.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "boxvote_math.h"

static int failures = 0;
static void expect(bool ok, const char* what, int a = 0, int b = 0) {
  if (!ok) printf("FAILED %s (%d, %d)\n", what, a, b), ++failures;
}

static uint32_t lcg_state = 12345u;
static float unit() {                                  // [0, 1)
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return (float)(lcg_state >> 8) * (1.0f / 16777216.0f);
}
static float* block(size_t floats) { return (float*)malloc(sizeof(float) * (floats ? floats : 1)); }

// n distinct boxes around n / 12 + 1 centres (at most 8), scores in (0.002, 1)
static float* clustered(int n) {
  float* d = block(5 * (size_t)n);
  const int centres = n / 12 + 1 > 8 ? 8 : n / 12 + 1;
  for (int i = 0; i < n; ++i) {
    const int c = i % centres;
    const float cx = 100.0f + 85.0f * c, cy = 120.0f + 50.0f * c, bw = 80.0f + 15.0f * c, bh = 70.0f + 12.0f * c;
    const float x = cx + (unit() - 0.5f) * 0.5f * bw, y = cy + (unit() - 0.5f) * 0.5f * bh;
    const float w = bw * (0.7f + 0.6f * unit()), h = bh * (0.7f + 0.6f * unit());
    float* o = d + 5 * (size_t)i;
    o[0] = x - w / 2, o[1] = y - h / 2, o[2] = x + w / 2, o[3] = y + h / 2, o[4] = 0.002f + 0.997f * unit();
  }
  return d;
}

static long long moved_total = 0, rows_total = 0;

static void vote_case(int n, int step) {
  float* cands = clustered(n);
  const int m = (n + step - 1) / step;
  float* kept = block(5 * (size_t)m);
  for (int i = 0; i < m; ++i) memcpy(kept + 5 * (size_t)i, cands + 5 * (size_t)(i * step), sizeof(float) * 5);
  float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};            // x and y spans of all candidates
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 4; ++k) {
      const float v = cands[5 * (size_t)i + k];
      lo[k & 1] = v < lo[k & 1] ? v : lo[k & 1], hi[k & 1] = v > hi[k & 1] ? v : hi[k & 1];
    }
  const double thresholds[3] = {0.8, 0.5, 1.0};
  for (int t = 0; t < 3; ++t) {
    float* out = block(5 * (size_t)m);
    boxvote_host(kept, m, cands, n, thresholds[t], out);
    int moved = 0;
    for (int i = 0; i < m; ++i) {
      const float *a = kept + 5 * (size_t)i, *o = out + 5 * (size_t)i;
      expect(memcmp(a + 4, o + 4, sizeof(float)) == 0, "the score changed", n, i);
      for (int k = 0; k < 4; ++k) expect(isfinite(o[k]) && o[k] >= lo[k & 1] && o[k] <= hi[k & 1], "a coordinate left the candidates' span", n, i);
      moved += memcmp(a, o, sizeof(float) * 4) != 0;
    }
    if (t == 2) expect(moved == 0, "vote_thresh 1.0 on distinct boxes changed bits", n, moved);
    if (t == 1 && n >= 63) expect(moved > 0, "vote_thresh 0.5 moved nothing", n, step);
    moved_total += moved, rows_total += m;
    free(out);
  }
  free(kept), free(cands);
}

static void vote_edges() {
  float* cands = clustered(8);
  float* out = block(5);
  boxvote_host(cands, 0, cands, 8, 0.5, out);                                    // m = 0: nothing is written
  boxvote_host(cands, 1, cands, 0, 0.5, out);                                    // n = 0: no voter, the row comes back
  expect(memcmp(out, cands, sizeof(float) * 5) == 0, "n = 0");
  const float far_away[5] = {5000, 5000, 5100, 5100, 0.5f};                      // overlaps no candidate and is none itself
  boxvote_host(far_away, 1, cands, 8, 0.5, out);
  expect(memcmp(out, far_away, sizeof(float) * 5) == 0, "a kept row without voters");
  const float degenerate[5] = {900, 10, 799, 50, 0.5f};                          // x2 < x1 - 1: w = 0, IoU 0 with itself
  boxvote_host(degenerate, 1, degenerate, 1, 0.5, out);
  expect(memcmp(out, degenerate, sizeof(float) * 5) == 0, "a degenerate box");
  const float two[10] = {10, 10, 50, 50, 0.75f, 10, 10, 50, 50, 0.25f};          // the same box twice: the mean of equal values
  float* out2 = block(10);
  boxvote_host(two, 2, two, 2, 1.0, out2);
  expect(out2[0] == 10.0f && out2[2] == 50.0f && out2[4] == 0.75f && out2[9] == 0.25f, "identical boxes");
  const float pair[10] = {0, 0, 99, 99, 0.75f, 0, 0, 99, 79, 0.25f};             // IoU 0.8: both vote at 0.8 -> (0.75 * 99 + 0.25 * 79) / 1
  boxvote_host(pair, 1, pair, 2, 0.8, out2);
  expect(out2[3] == 94.0f && out2[2] == 99.0f && out2[4] == 0.75f, "the weighted mean of two voters");
  boxvote_host(pair, 1, pair, 2, 0.81, out2);
  expect(out2[3] == 99.0f, "the second box does not vote above its IoU");
  expect(boxvote_thresh_ok(1.0) && boxvote_thresh_ok(1e-9) && !boxvote_thresh_ok(0.0) && !boxvote_thresh_ok(-0.5) &&
         !boxvote_thresh_ok(1.0000001) && !boxvote_thresh_ok(NAN), "argument rule");
  free(out2), free(out), free(cands);
}

static void merge_case(int B, int R, int C, const int* num, bool with_pred) {
  const size_t rows = (size_t)2 * B * R;
  float *prob = block(rows * C), *pred = with_pred ? block(rows * 4 * C) : nullptr, *rois = block(rows * 5);
  for (size_t i = 0; i < rows * C; ++i) prob[i] = unit();
  if (pred)
    for (size_t i = 0; i < rows * 4 * C; ++i) pred[i] = unit() - 0.5f;
  for (size_t i = 0; i < rows; ++i) {
    float* r = rois + 5 * i;
    r[0] = (float)(i / R), r[1] = 600.0f * unit(), r[2] = 400.0f * unit(), r[3] = r[1] + 1.0f + 190.0f * unit(), r[4] = r[2] + 1.0f + 190.0f * unit();
  }
  float *o_prob = block(rows * C), *o_pred = with_pred ? block(rows * 4 * C) : nullptr, *o_rois = block(rows * 5);
  int* o_num = (int*)malloc(sizeof(int) * B);
  const float width = 800.0f;
  boxvote_merge_host(prob, pred, rois, num, B, R, C, width, o_prob, o_pred, o_rois, o_num);
  for (int b = 0; b < B; ++b) {
    int n0 = num ? num[2 * b] : R, n1 = num ? num[2 * b + 1] : R;
    n0 = n0 < 0 ? 0 : n0 > R ? R : n0, n1 = n1 < 0 ? 0 : n1 > R ? R : n1;
    expect(o_num[b] == n0 + n1, "merged count", b, o_num[b]);
    for (int rp = 0; rp < 2 * R; ++rp) {
      const size_t dst = (size_t)b * 2 * R + rp;
      const bool first = rp < n0, second = !first && rp < n0 + n1;
      const size_t src = first ? (size_t)(2 * b) * R + rp : (size_t)(2 * b + 1) * R + (rp - n0);
      bool ok = true;
      for (int j = 0; j < C; ++j) ok = ok && o_prob[dst * C + j] == (first || second ? prob[src * C + j] : 0.0f);
      for (int k = 0; pred && k < 4 * C; ++k) {
        const float want = first ? pred[src * 4 * C + k] : second ? (k % 4 == 0 ? -pred[src * 4 * C + k] : pred[src * 4 * C + k]) : 0.0f;
        ok = ok && o_pred[dst * 4 * C + k] == want;
      }
      const float* s = rois + 5 * src;
      const float want[5] = {first || second ? s[0] : 0.0f, first ? s[1] : second ? 799.0f - s[3] : 0.0f, first || second ? s[2] : 0.0f,
                             first ? s[3] : second ? 799.0f - s[1] : 0.0f, first || second ? s[4] : 0.0f};
      ok = ok && memcmp(want, o_rois + 5 * dst, sizeof(want)) == 0;
      expect(ok, "merged row", b, rp);
    }
  }
  free(o_num), free(o_rois), free(o_pred), free(o_prob), free(rois), free(pred), free(prob);
}

int main() {
  const int sizes[8] = {1, 2, 63, 64, 65, 130, 300, 1024};
  for (int i = 0; i < 8; ++i) vote_case(sizes[i], 3), vote_case(sizes[i], 1);
  vote_edges();
  printf("voting: %lld of %lld kept rows moved over 8 sizes x 2 kept lists x 3 thresholds\n", moved_total, rows_total);
  const int one[2] = {1, 0}, none[2] = {0, 0};
  merge_case(1, 1, 2, one, true), merge_case(1, 1, 2, none, false);
  const int a[4] = {48, 0, 17, 48}, b[4] = {0, 31, -3, 53}, c[2] = {512, 512}, d[2] = {500, 7};
  merge_case(2, 48, 3, a, true), merge_case(2, 48, 3, b, true), merge_case(2, 48, 3, b, false), merge_case(2, 48, 3, nullptr, true);
  merge_case(1, 512, 3, c, true), merge_case(1, 512, 3, d, false);
  printf("merge: 8 cases\n");
  printf(failures ? "box_vote_host_check: %d FAILED\n" : "box_vote_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
