// Stand-alone sanitizer harness for csrc/jpeg_encode_host.h and csrc/draw_math.h (not part of libfrcnn_hip.so):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/jpeg_encode_host_check.cc -o jpeg_encode_host_check && ./jpeg_encode_host_check
// Seeded images of the sizes the tests use, every sampling, three qualities: the host encode and the Huffman stage run on heap blocks of
// EXACTLY the sizes handed over (image, planes, coefficient buffer, output), so a read or write one byte outside any of them is reported; the
// Huffman stage runs at every cap from 0 up to the bound in steps of 61 and at the exact size and one byte less; its output is decoded
// again by csrc/jpeg_host.h and must return the buffer that went in.  jpeg_div_trunc is compared with `/` for every numerator below 2^17
// (the DCT's outputs stay below 2^15 + 1020) and every divisor 8 q, q = 1 .. 255.  The drawing rule paints seeded records, NaN and far
// coordinates among them, on an exact-size image.
#include <stdio.h>
#include <stdlib.h>

#include "draw_math.h"
#include "jpeg_encode_host.h"

static unsigned rnd_state = 12345u;
static unsigned rnd() { return (rnd_state = rnd_state * 1664525u + 1013904223u) >> 8; }

static long long encode_at(const void* coef, const JpegGeom& g, size_t cap) {
  unsigned char* out = (unsigned char*)malloc(cap ? cap : 1);
  const long long n = jpeg_host::entropy_encode(coef, g, cap ? out : nullptr, cap);
  if (n >= 0 && (size_t)n > cap) abort();
  free(out);
  return n;
}

static int check_image(int w, int h, int hs, int vs, int quality, int kind) {
  JpegGeom g;
  if (!jpeg_geom(w, h, 3, hs, vs, &g)) abort();
  unsigned char* bgr = (unsigned char*)malloc((size_t)w * h * 3);
  for (size_t i = 0; i < (size_t)w * h * 3; ++i) bgr[i] = kind == 0 ? (unsigned char)rnd() : (kind == 1 ? 0 : 255);
  unsigned char* planes = (unsigned char*)malloc(g.ws_bytes);
  unsigned char* coef = (unsigned char*)malloc(g.coef_bytes);
  if (jpeg_host::coefs_host(bgr, g, quality, planes, coef) != FRCNN_OK) abort();
  const size_t bound = jpeg_host::stream_bound(g);
  unsigned char* out = (unsigned char*)malloc(bound);
  const long long n = jpeg_host::entropy_encode(coef, g, out, bound);
  if (n <= 0 || (size_t)n > bound) abort();
  unsigned char* back = (unsigned char*)malloc(g.coef_bytes);
  if (jpeg_host::entropy_decode(out, (size_t)n, back, g.coef_bytes) != FRCNN_OK || memcmp(back, coef, g.coef_bytes) != 0) abort();
  if (encode_at(coef, g, (size_t)n) != n || encode_at(coef, g, (size_t)n - 1) != FRCNN_E_ARG || encode_at(coef, g, 0) != FRCNN_E_ARG) abort();
  int runs = 3;
  for (size_t cap = 0; cap <= bound; cap += 61, ++runs) {
    const long long r = encode_at(coef, g, cap);
    if (r != (cap >= (size_t)n ? n : (long long)FRCNN_E_ARG)) abort();
  }
  free(back), free(out), free(coef), free(planes), free(bgr);
  return runs;
}

static int check_draw(int h, int w) {
  static const char* names[3] = {"a", "person", "diningtable"};
  const int stride = 12, ncls = 3, ndet = 300;
  unsigned char* labels = (unsigned char*)calloc((size_t)ncls * stride, 1);
  for (int i = 0; i < ncls; ++i) memcpy(labels + i * stride, names[i], strlen(names[i]));
  memcpy(labels + 2 * stride, "diningtable!", 12);                 // a name that fills its row: no NUL inside it
  unsigned char* colours = (unsigned char*)malloc(2 * 3);
  unsigned char* glyphs = (unsigned char*)malloc(DRAW_GLYPH_COUNT * 7);
  for (int i = 0; i < 6; ++i) colours[i] = (unsigned char)rnd();
  for (int i = 0; i < DRAW_GLYPH_COUNT * 7; ++i) glyphs[i] = (unsigned char)(rnd() & 31);
  float* dets = (float*)malloc(sizeof(float) * 6 * ndet);
  for (int k = 0; k < ndet; ++k) {
    float* d = dets + 6 * k;
    d[0] = (float)(rnd() % (w + 60)) - 30.0f, d[1] = (float)(rnd() % (h + 60)) - 30.0f;
    d[2] = d[0] + (float)(rnd() % 90) - 5.0f, d[3] = d[1] + (float)(rnd() % 50) - 5.0f;
    d[4] = (float)(rnd() % 1001) / 1000.0f, d[5] = (float)(rnd() % 6) - 1.0f;
    if (k % 17 == 0) d[rnd() % 6] = NAN;
    if (k % 23 == 0) d[rnd() % 4] = (k & 1) ? 3e9f : -3e9f;
    if (k % 29 == 0) d[rnd() % 4] = (k & 1) ? INFINITY : -INFINITY;
  }
  unsigned char* im = (unsigned char*)malloc((size_t)h * w * 3);
  memset(im, 7, (size_t)h * w * 3);
  int drawn = 0;
  for (int scale = 1; scale <= 16; scale += 5)
    for (int t = 1; t <= 64; t += 21) {
      const DrawParams P = {h, w, ndet, t, scale, ncls, stride, 2, 0.3f};
      if (!draw_params_ok(P)) abort();
      for (int k = 0; k < ndet; ++k) {
        DrawRec R;
        if (!draw_prepare(dets + 6 * k, P, labels, colours, &R)) continue;
        ++drawn;
        if (R.x1 < 0 || R.y1 < 0 || R.x2 >= w || R.y2 >= h || R.px0 < 0 || R.py0 < 0 || R.px1 > w || R.py1 > h) abort();
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) draw_pixel(R, P, labels, glyphs, x, y, im + ((size_t)y * w + x) * 3);
      }
    }
  free(im), free(dets), free(glyphs), free(colours), free(labels);
  return drawn;
}

int main() {
  long long divs = 0;
  for (int q = 1; q <= 255; ++q) {
    const int d = q << 3;
    const float rd = jpeg_quant_rcp(q);
    for (int n = 0; n < (1 << 17); ++n, ++divs)
      if (jpeg_div_trunc(n, d, rd) != n / d) abort();
    for (int c = -40000; c <= 40000; c += 7) {
      const int want = c >= 0 ? (c + d / 2) / d : -((-c + d / 2) / d);
      if (jpeg_quantise(c, q, rd) != want) abort();
    }
  }
  static const int sizes[][2] = {{1, 1}, {8, 8}, {16, 16}, {7, 9}, {17, 23}, {33, 50}, {48, 64}, {31, 97}, {2, 2049}};
  static const int samp[][2] = {{1, 1}, {2, 1}, {2, 2}};
  static const int quals[] = {1, 75, 100};
  int images = 0, runs = 0;
  for (auto& s : sizes)
    for (auto& m : samp)
      for (int q : quals)
        for (int kind = 0; kind < (q == 100 ? 3 : 1); ++kind, ++images) runs += check_image(s[1], s[0], m[0], m[1], q, kind);
  const int drawn = check_draw(64, 96) + check_draw(7, 5);
  printf("ok: %lld divisions, %d images, %d Huffman runs, %d records drawn\n", divs, images, runs, drawn);
  return 0;
}
