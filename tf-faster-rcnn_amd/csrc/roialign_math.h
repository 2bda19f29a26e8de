// RoIAlign (He et al. 2017, "Mask R-CNN"; Detectron's RoIAlign with aligned = False: no half-pixel shift), stated ONCE for the kernels and
// the host entries of csrc/roi_align.hip and the stand-alone harness csrc/roi_align_host_check.cc.
//
//   scale = 1 / feat_stride; RoI row (img, x1, y1, x2, y2) in scaled-image pixels
//   sx = x1 * scale, ex = x2 * scale (y alike); roi_w = max(ex - sx, 1), roi_h = max(ey - sy, 1); bin_w = roi_w / P, bin_h = roi_h / P
//   S x S samples per bin:  y = (sy + ph * bin_h) + ((iy + 0.5) * bin_h) / S,  x alike
//   a sample with y < -1 || y > H || x < -1 || x > W contributes 0 (a NaN coordinate counts as outside)
//   otherwise y = max(y, 0), y_low = (int)y; y_low >= H - 1: y_low = y_high = H - 1 and y = y_low; else y_high = y_low + 1 (x alike)
//   ly = y - y_low, hy = 1 - ly; the four tap weights are the products hy*hx, hy*lx, ly*hx, ly*lx
//   sample = ((hy*hx*v1 + hy*lx*v2) + ly*hx*v3) + ly*lx*v4;  output = (0 + the non-zeroed samples in (iy, ix) order) / (float)(S*S)
//   gradient of a tap = (dout / (float)(S*S)) * weight
// All arithmetic is float32 with one rounding per operation (every TU is built with -ffp-contract=off), left to right as written here.
// The rule separates per axis: a coordinate gives (low, high, l, h, kind) on its own, and a sample is zeroed iff either axis is outside.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ROIALIGN_HD __host__ __device__ __forceinline__
#else
#define ROIALIGN_HD inline
#endif

#define ROIALIGN_MAX_SAMPLES 4                // S
#define ROIALIGN_MAX_AXIS 128                 // P * S: the sample rows (columns) of one RoI, the size of the kernels' tap tables

// what a coordinate met on its way to a tap pair (a sample's kind: ZERO if either axis is, else the union of both axes)
#define ROIALIGN_ZERO 1                       // outside [-1, n]: the sample contributes 0
#define ROIALIGN_LOW 2                        // in [-1, 0): clamped to 0
#define ROIALIGN_HIGH 4                       // low >= n - 1: both taps on the last row (column)
#define ROIALIGN_INT 8                        // the coordinate, as computed, is an integer

struct RoiAlignGeom { float sx, sy, bin_w, bin_h; };
struct RoiAlignTap { int lo, hi; float l, h; int kind; };

ROIALIGN_HD RoiAlignGeom roialign_geom(const float* roi, float scale, int P) {
  const float sx = roi[1] * scale, sy = roi[2] * scale, ex = roi[3] * scale, ey = roi[4] * scale;
  float roi_w = ex - sx, roi_h = ey - sy;
  roi_w = roi_w >= 1.0f ? roi_w : 1.0f;       // max(., 1); a NaN width becomes 1 and the NaN start still zeroes every sample
  roi_h = roi_h >= 1.0f ? roi_h : 1.0f;
  RoiAlignGeom g;
  g.sx = sx, g.sy = sy, g.bin_w = roi_w / (float)P, g.bin_h = roi_h / (float)P;
  return g;
}

// sample i of S in bin p along one axis
ROIALIGN_HD float roialign_coord(float start, float bin, int p, int i, int S) {
  return (start + (float)p * bin) + (((float)i + 0.5f) * bin) / (float)S;
}

// coordinate v on an axis of n cells -> tap pair and weights; lo and hi are inside [0, n - 1] whenever the kind is not ZERO
ROIALIGN_HD RoiAlignTap roialign_tap(float v, int n) {
  RoiAlignTap t;
  t.lo = t.hi = 0, t.l = 0.0f, t.h = 0.0f, t.kind = ROIALIGN_ZERO;
  if (!(v >= -1.0f && v <= (float)n)) return t;
  t.kind = ((float)(int)v == v) ? ROIALIGN_INT : 0;
  if (v < 0.0f) v = 0.0f, t.kind |= ROIALIGN_LOW;
  int lo = (int)v;
  if (lo >= n - 1) {
    lo = n - 1, t.hi = lo, v = (float)lo, t.kind |= ROIALIGN_HIGH;
  } else {
    t.hi = lo + 1;
  }
  t.lo = lo, t.l = v - (float)lo, t.h = 1.0f - t.l;
  return t;
}

ROIALIGN_HD int roialign_sample_kind(int ky, int kx) { return ((ky | kx) & ROIALIGN_ZERO) ? ROIALIGN_ZERO : (ky | kx); }

// image index of a RoI row: the crop kernel's (int)roi[0] with its zero row for everything outside [0, N) (and for NaN)
ROIALIGN_HD int roialign_image(float f, int N) { return (f > -1.0f && f < (float)N) ? (int)f : -1; }

ROIALIGN_HD float roialign_sample(float hy, float ly, float hx, float lx, float v1, float v2, float v3, float v4) {
  return (((hy * hx) * v1 + (hy * lx) * v2) + (ly * hx) * v3) + (ly * lx) * v4;
}

// ---- host statements: the per-element order of the kernels, over host pointers -------------------------------------------------------
// forward: feat [N][H][W][C], rois [R][5] -> out [R][P][P][C]; bias (or NULL) added after the mean, then ReLU if relu
inline void roialign_fwd_host(const float* feat, int N, int H, int W, int C, const float* rois, int R, float stride, int P, int S,
                              const float* bias, bool relu, float* out) {
  const float scale = 1.0f / stride, count = (float)(S * S);
  for (int r = 0; r < R; ++r) {
    const float* roi = rois + 5 * (size_t)r;
    float* o = out + (size_t)r * P * P * C;
    const int img = roialign_image(roi[0], N);
    if (img < 0) {
      for (size_t k = 0; k < (size_t)P * P * C; ++k) o[k] = 0.0f;
      continue;
    }
    const float* f = feat + (size_t)img * H * W * C;
    const RoiAlignGeom g = roialign_geom(roi, scale, P);
    for (int ph = 0; ph < P; ++ph)
      for (int pw = 0; pw < P; ++pw)
        for (int c = 0; c < C; ++c) {
          float acc = 0.0f;
          for (int iy = 0; iy < S; ++iy) {
            const RoiAlignTap ty = roialign_tap(roialign_coord(g.sy, g.bin_h, ph, iy, S), H);
            if (ty.kind & ROIALIGN_ZERO) continue;
            for (int ix = 0; ix < S; ++ix) {
              const RoiAlignTap tx = roialign_tap(roialign_coord(g.sx, g.bin_w, pw, ix, S), W);
              if (tx.kind & ROIALIGN_ZERO) continue;
              acc += roialign_sample(ty.h, ty.l, tx.h, tx.l, f[((size_t)ty.lo * W + tx.lo) * C + c], f[((size_t)ty.lo * W + tx.hi) * C + c],
                                     f[((size_t)ty.hi * W + tx.lo) * C + c], f[((size_t)ty.hi * W + tx.hi) * C + c]);
            }
          }
          float v = acc / count;
          if (bias) v += bias[c];
          if (relu) v = v < 0.0f ? 0.0f : v;          // act_relu of csrc/common.h: a NaN stays
          o[((size_t)ph * P + pw) * C + c] = v;
        }
  }
}

// backward, one image (rois[:, 0] is not read): dfeat [H][W][C] += the gradient of dout [R][P][P][C].  Every feature element sums its
// contributions from 0 in (roi, ph, iy, pw, ix, tap) order and the sum is added to dfeat once: the kernel's order.
// row [W * C] is scratch.
inline void roialign_bwd_host(const float* dout, int H, int W, int C, const float* rois, int R, float stride, int P, int S, float* dfeat,
                              float* row) {
  const float scale = 1.0f / stride, count = (float)(S * S);
  for (int h = 0; h < H; ++h) {
    for (size_t k = 0; k < (size_t)W * C; ++k) row[k] = 0.0f;
    for (int r = 0; r < R; ++r) {
      const RoiAlignGeom g = roialign_geom(rois + 5 * (size_t)r, scale, P);
      for (int ph = 0; ph < P; ++ph)
        for (int iy = 0; iy < S; ++iy) {
          const RoiAlignTap ty = roialign_tap(roialign_coord(g.sy, g.bin_h, ph, iy, S), H);
          if ((ty.kind & ROIALIGN_ZERO) || (ty.lo != h && ty.hi != h)) continue;
          for (int pw = 0; pw < P; ++pw) {
            const float* d = dout + (((size_t)r * P + ph) * P + pw) * C;
            for (int ix = 0; ix < S; ++ix) {
              const RoiAlignTap tx = roialign_tap(roialign_coord(g.sx, g.bin_w, pw, ix, S), W);
              if (tx.kind & ROIALIGN_ZERO) continue;
              float *a = row + (size_t)tx.lo * C, *b = row + (size_t)tx.hi * C;
              for (int c = 0; c < C; ++c) {
                const float gv = d[c] / count;
                if (ty.lo == h) a[c] += gv * (ty.h * tx.h), b[c] += gv * (ty.h * tx.l);
                if (ty.hi == h) a[c] += gv * (ty.l * tx.h), b[c] += gv * (ty.l * tx.l);
              }
            }
          }
        }
    }
    float* drow = dfeat + (size_t)h * W * C;
    for (size_t k = 0; k < (size_t)W * C; ++k) drow[k] += row[k];
  }
}

// kinds of the P*S x P*S samples of each RoI on an H x W map: counts [R][4] = zeroed, clamped-low, clamped-high, on an integer coordinate
inline void roialign_classify_host(int H, int W, const float* rois, int R, float stride, int P, int S, long long* counts) {
  const float scale = 1.0f / stride;
  for (int r = 0; r < R; ++r) {
    const RoiAlignGeom g = roialign_geom(rois + 5 * (size_t)r, scale, P);
    long long* c = counts + 4 * (size_t)r;
    c[0] = c[1] = c[2] = c[3] = 0;
    for (int i = 0; i < P * S; ++i)
      for (int j = 0; j < P * S; ++j) {
        const int k = roialign_sample_kind(roialign_tap(roialign_coord(g.sy, g.bin_h, i / S, i % S, S), H).kind,
                                           roialign_tap(roialign_coord(g.sx, g.bin_w, j / S, j % S, S), W).kind);
        c[0] += (k & ROIALIGN_ZERO) != 0, c[1] += (k & ROIALIGN_LOW) != 0, c[2] += (k & ROIALIGN_HIGH) != 0, c[3] += (k & ROIALIGN_INT) != 0;
      }
  }
}
