// The drawing rule of frcnn_draw_detections, stated ONCE for the host (frcnn_draw_detections_host) and the kernel (csrc/draw.hip).  No HIP
// includes.  For each record k < min(count, max_dets) in record order -- (x1, y1, x2, y2, score, class), as Network.detect_device leaves
// them -- with score >= conf:
//   outline  X = rintf(x) in float32; the box is intersected with the image; of [X1..X2] x [Y1..Y2] the pixels outside
//            [X1+t..X2-t] x [Y1+t..Y2-t] take the class colour colours[class % num_colours] (BGR)
//   plate    the label "<class name> d.ddd" (m = min(1000, (int)(score * 1000.0f + 0.5f)) thousandths) in a 5 x 7 bitmap font magnified by
//            the integer `scale`, advance 6 * scale, padding 2: a filled rectangle in the class colour with black text, directly above
//            the box, or inside it at the top where that would leave the picture; clipped at the right and bottom borders
// Records with a coordinate that is NaN or beyond +-2^20, x2 < x1 or y2 < y1 after rounding, no pixel in the image or a class outside
// [0, num_classes) are skipped.  Later records paint over earlier ones, the plate of a record over its outline: a pixel takes the LAST
// primitive that covers it, so it can be found by walking the records backwards and no byte is ever written twice.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DRAW_HD __host__ __device__ __forceinline__
#else
#define DRAW_HD inline
#endif

enum { DRAW_GLYPH_FIRST = 32, DRAW_GLYPH_COUNT = 95, DRAW_PAD = 2 };      // glyphs [95][7]: printable ASCII, a row's bit 4 is its left column

struct DrawParams {
  int h, w, max_dets, thickness, scale, num_classes, label_stride, num_colours;
  float conf;
};

struct DrawRec {
  int x1, y1, x2, y2;                // the clipped box, inclusive
  int px0, py0, px1, py1;            // the clipped plate, px1 / py1 exclusive
  int cls, name_len, m;
  unsigned char b, g, r;
};

DRAW_HD bool draw_coord(float v, int* out) {
  if (!(v >= -1048576.0f && v <= 1048576.0f)) return false;      // NaN fails both
  *out = (int)rintf(v);
  return true;
}

// false: the record draws nothing
DRAW_HD bool draw_prepare(const float* rec, const DrawParams& P, const unsigned char* labels, const unsigned char* colours, DrawRec* R) {
  int X1, Y1, X2, Y2;
  if (!draw_coord(rec[0], &X1) || !draw_coord(rec[1], &Y1) || !draw_coord(rec[2], &X2) || !draw_coord(rec[3], &Y2)) return false;
  const float score = rec[4], fc = rec[5];
  if (!(score >= P.conf) || !(fc >= 0.0f && fc < (float)P.num_classes)) return false;
  if (X2 < X1 || Y2 < Y1) return false;
  R->x1 = X1 < 0 ? 0 : X1, R->y1 = Y1 < 0 ? 0 : Y1;
  R->x2 = X2 > P.w - 1 ? P.w - 1 : X2, R->y2 = Y2 > P.h - 1 ? P.h - 1 : Y2;
  if (R->x2 < R->x1 || R->y2 < R->y1) return false;
  R->cls = (int)fc;
  const unsigned char* name = labels + (size_t)R->cls * P.label_stride;
  int n = P.label_stride;                                        // the first NUL, every byte of the row read: no load waits for a branch
  for (int i = P.label_stride - 1; i >= 0; --i) n = name[i] ? n : i;
  R->name_len = n;
  const float ms = score * 1000.0f + 0.5f;
  R->m = ms >= 1000.0f ? 1000 : (ms > 0.0f ? (int)ms : 0);
  const int pw = (n + 6) * 6 * P.scale + 2 * DRAW_PAD, ph = 7 * P.scale + 2 * DRAW_PAD;
  R->px0 = R->x1;
  R->py0 = R->y1 - ph >= 0 ? R->y1 - ph : R->y1;
  R->px1 = R->px0 + pw > P.w ? P.w : R->px0 + pw;
  R->py1 = R->py0 + ph > P.h ? P.h : R->py0 + ph;
  const unsigned char* c = colours + 3 * (R->cls % P.num_colours);
  R->b = c[0], R->g = c[1], R->r = c[2];
  return true;
}

// character i of the label
DRAW_HD int draw_label_char(const DrawRec& R, const DrawParams& P, const unsigned char* labels, int i) {
  if (i < R.name_len) return labels[(size_t)R.cls * P.label_stride + i];
  switch (i - R.name_len) {
    case 0: return ' ';
    case 1: return '0' + R.m / 1000;
    case 2: return '.';
    case 3: return '0' + (R.m / 100) % 10;
    case 4: return '0' + (R.m / 10) % 10;
    default: return '0' + R.m % 10;
  }
}

// true: the record covers pixel (x, y), whose colour is written to bgr[0..2]
DRAW_HD bool draw_pixel(const DrawRec& R, const DrawParams& P, const unsigned char* labels, const unsigned char* glyphs, int x, int y,
                        unsigned char* bgr) {
  if (x >= R.px0 && x < R.px1 && y >= R.py0 && y < R.py1) {
    const int tx = x - R.px0 - DRAW_PAD, ty = y - R.py0 - DRAW_PAD, adv = 6 * P.scale;
    bool ink = false;
    if (tx >= 0 && ty >= 0 && tx < (R.name_len + 6) * adv && ty < 7 * P.scale) {
      const int ci = tx / adv, gx = (tx - ci * adv) / P.scale, gy = ty / P.scale;
      const int ch = draw_label_char(R, P, labels, ci) - DRAW_GLYPH_FIRST;
      if (gx < 5 && ch >= 0 && ch < DRAW_GLYPH_COUNT) ink = (glyphs[ch * 7 + gy] >> (4 - gx)) & 1;
    }
    bgr[0] = ink ? 0 : R.b, bgr[1] = ink ? 0 : R.g, bgr[2] = ink ? 0 : R.r;
    return true;
  }
  if (x >= R.x1 && x <= R.x2 && y >= R.y1 && y <= R.y2) {
    const int t = P.thickness;
    if (x >= R.x1 + t && x <= R.x2 - t && y >= R.y1 + t && y <= R.y2 - t) return false;
    bgr[0] = R.b, bgr[1] = R.g, bgr[2] = R.r;
    return true;
  }
  return false;
}

// what a call accepts
DRAW_HD bool draw_params_ok(const DrawParams& P) {
  return P.h >= 1 && P.w >= 1 && P.h <= 65535 && P.w <= 65535 && P.max_dets >= 0 && P.thickness >= 1 && P.thickness <= 64 && P.scale >= 1 &&
         P.scale <= 16 && P.num_classes >= 1 && P.label_stride >= 1 && P.label_stride <= 64 && P.num_colours >= 1;
}
