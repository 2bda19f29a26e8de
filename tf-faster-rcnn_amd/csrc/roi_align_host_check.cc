// Stand-alone sanitizer harness for csrc/roialign_math.h (not part of libfrcnn_hip.so; host only, never loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/roi_align_host_check.cc -o roi_align_host_check && ./roi_align_host_check
// Every buffer is a heap block of exactly the size the statement may touch.  The edge inputs of tests/test_roi_align_cpu.py: two images
// of 5 x 6 at stride 16 and six RoIs (interior; hanging over the top-left corner; over the bottom-right corner; degenerate; the whole
// map; the second image), then a row with image index 7, one with -1 and one of NaNs, at (P, S) = (7,2), (7,1), (7,3), (2,1), (14,4) and
// C = 1, 4, 5.
// 1. forward(ones) == (number of non-zeroed samples of the bin) / S^2 within 4 ulp of 1, with the count taken from roialign_tap again;
//    rows without an image and the NaN row are zero.
// 2. sum(backward(ones)) == (sum of the tap weights of all non-zeroed samples) / S^2, the weights summed in double from roialign_tap;
//    the backward ADDS to what dfeat holds.
// 3. roialign_classify_host at (7, 2) gives the branch counts the tests assert.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "roialign_math.h"

static int failures = 0;
static void expect(bool ok, const char* what, int a = 0, int b = 0) {
  if (!ok) printf("FAILED %s (%d, %d)\n", what, a, b), ++failures;
}
static float* block(size_t floats) { return (float*)malloc(sizeof(float) * (floats ? floats : 1)); }

static const int H = 5, W = 6, N = 2, R = 9;
static const float STRIDE = 16.0f;
static const float ROIS[R][5] = {{0, 8, 8, 70, 60},  {0, -40, -40, 30, 30}, {0, 60, 50, 140, 120}, {0, 50, 50, 40, 40},     {0, 0, 0, 95, 79},
                                 {1, 16, 16, 48, 48}, {7, 16, 16, 48, 48},   {-1, 16, 16, 48, 48},  {0, NAN, NAN, NAN, NAN}};

static void run(int P, int S, int C) {
  float* rois = block(5 * R);
  memcpy(rois, ROIS, sizeof(ROIS));
  float* feat = block((size_t)N * H * W * C);
  for (size_t i = 0; i < (size_t)N * H * W * C; ++i) feat[i] = 1.0f;
  float* out = block((size_t)R * P * P * C);
  roialign_fwd_host(feat, N, H, W, C, rois, R, STRIDE, P, S, nullptr, false, out);
  double weights = 0.0;                                                            // of the image-0 RoIs 0..4 (the backward reads no index)
  for (int r = 0; r < R; ++r) {
    const RoiAlignGeom g = roialign_geom(rois + 5 * r, 1.0f / STRIDE, P);
    const bool has_image = roialign_image(rois[5 * r], N) >= 0;
    for (int ph = 0; ph < P; ++ph)
      for (int pw = 0; pw < P; ++pw) {
        int valid = 0;
        for (int iy = 0; iy < S; ++iy)
          for (int ix = 0; ix < S; ++ix) {
            const RoiAlignTap ty = roialign_tap(roialign_coord(g.sy, g.bin_h, ph, iy, S), H);
            const RoiAlignTap tx = roialign_tap(roialign_coord(g.sx, g.bin_w, pw, ix, S), W);
            if ((ty.kind | tx.kind) & ROIALIGN_ZERO) continue;
            ++valid;
            expect(ty.lo >= 0 && ty.hi < H && tx.lo >= 0 && tx.hi < W && ty.lo <= ty.hi && tx.lo <= tx.hi, "a tap outside the map", r, ph);
            if (r < 5) weights += ((double)ty.h + (double)ty.l) * ((double)tx.h + (double)tx.l);
          }
        const float want = has_image ? (float)valid / (float)(S * S) : 0.0f;
        for (int c = 0; c < C; ++c) {
          const float got = out[(((size_t)r * P + ph) * P + pw) * C + c];
          expect(fabsf(got - want) <= 4.0f * 5.9604645e-8f, "forward(ones) is not the share of non-zeroed samples", r, ph * P + pw);
        }
      }
  }
  float* dout = block((size_t)5 * P * P * C);
  for (size_t i = 0; i < (size_t)5 * P * P * C; ++i) dout[i] = 1.0f;
  float *dfeat = block((size_t)H * W * C), *row = block((size_t)W * C);
  for (size_t i = 0; i < (size_t)H * W * C; ++i) dfeat[i] = 0.5f;
  roialign_bwd_host(dout, H, W, C, rois, 5, STRIDE, P, S, dfeat, row);
  double total = 0.0;
  for (size_t i = 0; i < (size_t)H * W * C; ++i) total += (double)dfeat[i] - 0.5;
  const double want = weights / (double)(S * S) * C;
  expect(fabs(total - want) <= 1e-4 * want, "sum(backward(ones)) is not the weight sum", P, S);
  roialign_bwd_host(dout, H, W, C, rois, 0, STRIDE, P, S, dfeat, row);             // R = 0 adds nothing and reads nothing
  printf("P = %2d S = %d C = %d: sum(backward(ones)) = %.6f, weight sum / S^2 = %.6f\n", P, S, C, total, want);
  free(row), free(dfeat), free(dout), free(out), free(feat), free(rois);
}

int main() {
  const int cases[5][2] = {{7, 2}, {7, 1}, {7, 3}, {2, 1}, {14, 4}};
  const int channels[3] = {1, 4, 5};
  for (int k = 0; k < 5; ++k)
    for (int c = 0; c < 3; ++c) run(cases[k][0], cases[k][1], channels[c]);
  long long* counts = (long long*)malloc(sizeof(long long) * 4 * 6);
  float* rois = block(5 * 6);
  memcpy(rois, ROIS, sizeof(float) * 5 * 6);
  roialign_classify_host(H, W, rois, 6, STRIDE, 7, 2, counts);
  const long long want[6][3] = {{0, 0, 0}, {115, 45, 0}, {160, 0, 27}, {0, 0, 28}, {0, 0, 64}, {0, 0, 0}};
  for (int r = 0; r < 6; ++r) {
    printf("RoI %d: %lld zeroed, %lld clamped low, %lld clamped high, %lld on an integer coordinate\n", r + 1, counts[4 * r], counts[4 * r + 1],
           counts[4 * r + 2], counts[4 * r + 3]);
    expect(counts[4 * r] == want[r][0] && counts[4 * r + 1] == want[r][1] && counts[4 * r + 2] == want[r][2], "branch counts", r);
  }
  expect(counts[4 * 2 + 3] == 6, "integer coordinates of RoI 3");
  free(rois), free(counts);
  printf(failures ? "roi_align_host_check: %d FAILED\n" : "roi_align_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
