// Stand-alone sanitizer harness for csrc/recall_math.h (not part of libfrcnn_hip.so):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/recall_host_check.cc -o recall_host_check && ./recall_host_check
// Walks three cases of tests/golden/recall.npz, written out as literals, through recall_match_image_host with every buffer a heap block of
// exactly the size the statement may touch: the hand case (an uncovered gt records 0.0 and consumes candidate 0; of two identical
// candidates the first wins), the empty cases (no candidates / no gts / ordinary, with the offsets of one call) and fewer candidates
// than gts (-1.0 in the remaining slots, the flag set, nothing else written).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "recall_math.h"

static int fail(const char* what, double a, double b) {
  printf("FAILED %s: %.17g %.17g\n", what, a, b);
  return 1;
}

template <typename T>
static T* heap(const T* src, size_t n) {
  T* p = (T*)malloc(sizeof(T) * (n ? n : 1));
  if (n) memcpy(p, src, sizeof(T) * n);
  return p;
}

// one image through the statement; returns the flag, `out` (G doubles, pre-filled with 7.0) is the caller's
static int match(const float* boxes, int stride, long long n, float scale, const double* gt, long long G, double* out) {
  float* b = heap(boxes, (size_t)n * stride);
  double* q = heap(gt, (size_t)G * 4);
  double* m = (double*)malloc(sizeof(double) * (size_t)(n * G ? n * G : 1));
  int flag = 7;
  recall_match_image_host(b, stride, n, scale, q, G, m, out, &flag);
  free(m), free(q), free(b);
  return flag;
}

int main() {
  // the IoU of [12,12,48,48] with the gt [10,10,50,50]: 37*37 / 41*41, the two areas and their quotient rounded once each
  const double iou_hand = (37.0 * 37.0) / (37.0 * 37.0 + 41.0 * 41.0 - 37.0 * 37.0);
  {
    const double gt[] = {10, 10, 50, 50, 200, 200, 240, 240};
    const float cand[] = {300, 300, 310, 310, 12, 12, 48, 48, 12, 12, 48, 48};
    double* out = (double*)malloc(sizeof(double) * 2);
    out[0] = out[1] = 7.0;
    if (match(cand, 4, 3, 1.0f, gt, 2, out) != 0) return fail("hand: flag", 0, 0);
    if (out[0] != iou_hand || out[1] != 0.0) return fail("hand: picks", out[0], out[1]);
    // the same candidates as rois * 2 with stride 5 and scale 2: the float32 division gives the same boxes back
    const float rois[] = {0, 600, 600, 620, 620, 0, 24, 24, 96, 96, 0, 24, 24, 96, 96};
    out[0] = out[1] = 7.0;
    if (match(rois, 5, 3, 2.0f, gt, 2, out) != 0 || out[0] != iou_hand || out[1] != 0.0) return fail("hand: stride 5", out[0], out[1]);
    // one candidate retired by the zero match: with candidate 0 gone the covered gt is still matched by candidate 1 when the order of
    // the gts is swapped (the uncovered one comes first but the covered one holds the larger maximum)
    const double gt_swapped[] = {200, 200, 240, 240, 10, 10, 50, 50};
    out[0] = out[1] = 7.0;
    if (match(cand, 4, 3, 1.0f, gt_swapped, 2, out) != 0 || out[0] != iou_hand || out[1] != 0.0) return fail("hand: swapped", out[0], out[1]);
    free(out);
  }
  {
    // three images of one call: gt offsets 0, 3, 3, 5; candidate rows 0, 2, 4
    const double gt[] = {5, 5, 40, 60, 50, 20, 90, 80, 100, 100, 160, 150, 20, 30, 80, 90, 120, 40, 200, 140};
    const float cand[] = {1, 2, 30, 40, 5, 5, 50, 50, 25, 28, 85, 95, 300, 300, 320, 320, 118, 44, 190, 150, 22, 30, 78, 88};
    const long long gt_off[] = {0, 3, 3, 5}, start[] = {0, 0, 2}, count[] = {0, 2, 4};
    double* out = (double*)malloc(sizeof(double) * 5);
    for (int i = 0; i < 5; ++i) out[i] = 7.0;
    for (int i = 0; i < 3; ++i) {
      const long long n = recall_rows(start[i], count[i], 4, 6, 0), G = gt_off[i + 1] - gt_off[i];
      if (n != count[i]) return fail("empty: rows", (double)n, (double)count[i]);
      const int flag = match(cand + 4 * start[i], 4, n, 1.0f, gt + 4 * gt_off[i], G, out + gt_off[i]);
      if (flag != 0) return fail("empty: flag", i, flag);
    }
    if (out[0] != 7.0 || out[1] != 7.0 || out[2] != 7.0) return fail("empty: an image without candidates wrote a slot", out[0], out[1]);
    // image 2: candidate 3 = [22,30,78,88] inside gt 0 = [20,30,80,90] (57*59 / 61*61), candidate 2 against gt 1
    const double a = (57.0 * 59.0) / (57.0 * 59.0 + 61.0 * 61.0 - 57.0 * 59.0);
    const double iw = 190.0 - 120.0 + 1, ih = 140.0 - 44.0 + 1;
    const double b = iw * ih / ((190.0 - 118.0 + 1) * (150.0 - 44.0 + 1) + (200.0 - 120.0 + 1) * (140.0 - 40.0 + 1) - iw * ih);
    if (out[3] != a || out[4] != b || !(a >= b)) return fail("empty: picks of the ordinary image", out[3], out[4]);
    if (recall_rows(0, 4, 4, 6, 2) != 2 || recall_rows(5, 4, 4, 6, 0) != 1 || recall_rows(0, -3, 4, 6, 0) != 0 || recall_rows(7, 1, 4, 6, 0) != 0)
      return fail("recall_rows", 0, 0);
    free(out);
  }
  {
    // 5 candidates against 7 gts: candidates k = gt k, so five picks of exactly 1.0, then the rows are gone
    double gt[28];
    float cand[20];
    for (int k = 0; k < 7; ++k) {
      gt[4 * k] = 40.0 * k, gt[4 * k + 1] = 10, gt[4 * k + 2] = 40.0 * k + 30, gt[4 * k + 3] = 50;
      if (k < 5)
        for (int j = 0; j < 4; ++j) cand[4 * k + j] = (float)gt[4 * k + j];
    }
    double* out = (double*)malloc(sizeof(double) * 7);
    for (int i = 0; i < 7; ++i) out[i] = 7.0;
    if (match(cand, 4, 5, 1.0f, gt, 7, out) != 1) return fail("few: flag", 0, 0);
    for (int i = 0; i < 7; ++i)
      if (out[i] != (i < 5 ? 1.0 : RECALL_RETIRED)) return fail("few: slot", i, out[i]);
    free(out);
  }
  if (recall_workspace_bytes(2000, 70) < 2000 * 70 * 8 || recall_coord(600.0f, 1.6f) != (double)(600.0f / 1.6f)) return fail("sizes", 0, 0);
  printf("ok: hand (3 forms), empty (3 images of one call), few (5 against 7)\n");
  return 0;
}
