// Host half of the JPEG encoder (no HIP includes): the quality -> quantisation table rule, the host statement of the coefficient stage
// (the arithmetic of csrc/jpeg_math.h, the same code the kernels of csrc/jpeg_encode.hip run) and the Huffman stage, which writes a
// complete baseline file from the coefficient buffer: SOI, JFIF APP0, DQT, SOF0, the four Annex K Huffman tables, ONE interleaved scan
// without restart markers, EOI.  Thread-safe, no allocation; nothing is written at or beyond out + cap.
//
// The coefficient buffer is the decoder's (csrc/jpeg_host.h): uint16 quant[3][64] in natural order, then int16 coefficients per component,
// [blocks_y][blocks_x][64] in natural order, padded to whole MCUs.  Three components, luma 1x1 / 2x1 / 2x2.
#pragma once
#include "jpeg_host.h"

namespace jpeg_host {

static const unsigned char K_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                         69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                         81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
static const unsigned char K_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                           99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3: code counts per length 1..16, then the symbols
static const unsigned char K_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const unsigned char K_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char K_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const unsigned char K_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// out[0] luminance, out[1] chrominance, natural order
static inline void quant_tables(int quality, uint16_t* out) {
  for (int i = 0; i < 64; ++i) {
    out[i] = (uint16_t)jpeg_quality_entry(K_LUMA[i], quality);
    out[64 + i] = (uint16_t)jpeg_quality_entry(K_CHROMA[i], quality);
  }
}

// planes: g.ws_bytes of scratch.  The host statement of frcnn_jpeg_coefs: the three MCU-padded sample planes (what k_jpeg_ycc writes),
// then every block (what k_jpeg_fdct writes).
static inline int coefs_host(const unsigned char* bgr, const JpegGeom& g, int quality, unsigned char* planes, void* coef_h) {
  const int hs = g.mode == JPEG_S11 ? 1 : 2, vs = g.mode == JPEG_S22 ? 2 : 1;
  const int w = g.w, h = g.h;
  uint16_t* q = (uint16_t*)coef_h;
  quant_tables(quality, q);
  memcpy(q + 128, q + 64, 128);
  unsigned char* Y = planes + g.plane_off[0];
  for (int sy = 0; sy < g.by[0] * 8; ++sy)
    for (int sx = 0; sx < g.bx[0] * 8; ++sx) {
      const unsigned char* p = bgr + ((size_t)jpeg_luma_src_row(sy, h) * w + jpeg_src_col(sx, w)) * 3;
      int y, cb, cr;
      jpeg_bgr_to_ycc(p[0], p[1], p[2], &y, &cb, &cr);
      Y[(size_t)sy * g.pitch[0] + sx] = (unsigned char)y;
    }
  for (int cy = 0; cy < g.by[1] * 8; ++cy)
    for (int cx = 0; cx < g.bx[1] * 8; ++cx) {
      int sb[4], sr[4], n = 0;
      const int r0 = jpeg_chroma_src_row(cy, g.ch) * vs;
      for (int j = 0; j < vs; ++j)
        for (int i = 0; i < hs; ++i, ++n) {
          const unsigned char* p = bgr + ((size_t)jpeg_luma_src_row(r0 + j, h) * w + jpeg_src_col(cx * hs + i, w)) * 3;
          int y;
          jpeg_bgr_to_ycc(p[0], p[1], p[2], &y, &sb[n], &sr[n]);
        }
      int cb = sb[0], cr = sr[0];
      if (g.mode == JPEG_S21) cb = jpeg_down_h2v1(sb[0], sb[1], cx), cr = jpeg_down_h2v1(sr[0], sr[1], cx);
      if (g.mode == JPEG_S22) cb = jpeg_down_h2v2(sb[0], sb[1], sb[2], sb[3], cx), cr = jpeg_down_h2v2(sr[0], sr[1], sr[2], sr[3], cx);
      planes[g.plane_off[1] + (size_t)cy * g.pitch[1] + cx] = (unsigned char)cb;
      planes[g.plane_off[2] + (size_t)cy * g.pitch[2] + cx] = (unsigned char)cr;
    }
  int16_t* coef = (int16_t*)((char*)coef_h + 384);
  const int rbx = (w + 7) / 8, rby = (h + 7) / 8;
  for (int c = 0; c < 3; ++c)
    for (int by = 0; by < g.by[c]; ++by)
      for (int bx = 0; bx < g.bx[c]; ++bx) {
        int sy = by, sx = bx;
        const bool dummy = c == 0 && jpeg_dummy_source(by, bx, hs, rbx, rby, &sy, &sx);
        int16_t* o = coef + ((size_t)g.blk_base[c] + (size_t)by * g.bx[c] + bx) * 64;
        jpeg_fdct_block(planes + g.plane_off[c] + (size_t)sy * 8 * g.pitch[c] + (size_t)sx * 8, g.pitch[c], q + 64 * c, o);
        if (dummy) memset(o + 1, 0, 126);
      }
  return FRCNN_OK;
}

// ---- the Huffman stage -------------------------------------------------------------------------------------------------------------------
struct EncHuff {
  uint16_t code[256];
  unsigned char size[256];           // 0: the symbol has no code
};

static inline void build_enc_huff(const unsigned char* counts, const unsigned char* vals, EncHuff* h) {
  memset(h, 0, sizeof(*h));
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < counts[len - 1]; ++i, ++k) h->code[vals[k]] = (uint16_t)code++, h->size[vals[k]] = (unsigned char)len;
    code <<= 1;
  }
}

// Bounded byte sink + MSB-first bit writer with FF 00 stuffing.  Past `end` nothing is stored and `over` is set.
struct Sink {
  unsigned char *p, *end;
  bool over;
  uint64_t acc;
  int n;
  inline void byte(unsigned b) {
    if (p < end) *p++ = (unsigned char)b;
    else over = true;
  }
  inline void be16(unsigned v) { byte(v >> 8), byte(v & 255); }
  inline void bytes(const unsigned char* s, int k) {
    for (int i = 0; i < k; ++i) byte(s[i]);
  }
  inline void bits(unsigned v, int k) {                          // k <= 26
    acc = (acc << k) | (v & ((1u << k) - 1)), n += k;
    while (n >= 8) {
      const unsigned b = (unsigned)(acc >> (n - 8)) & 255;
      byte(b);
      if (b == 0xFF) byte(0);
      n -= 8;
    }
  }
  inline void flush() {
    if (n) bits(0x7F, 8 - n);                                    // pad with ones
  }
};

static inline int nbits_of(int v) {
  v = v < 0 ? -v : v;
  return v ? 32 - __builtin_clz((unsigned)v) : 0;
}

static inline int encode_block(Sink& s, const EncHuff& dc, const EncHuff& ac, int* pred, const int16_t* blk) {
  const int diff = (int)blk[0] - *pred;
  *pred = blk[0];
  int nb = nbits_of(diff);
  if (nb > 11) return FRCNN_E_ARG;
  s.bits(dc.code[nb], dc.size[nb]);
  if (nb) s.bits((unsigned)(diff < 0 ? diff - 1 : diff), nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[ZIGZAG[k]];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run > 15; run -= 16) s.bits(ac.code[0xF0], ac.size[0xF0]);
    nb = nbits_of(v);
    if (nb > 10) return FRCNN_E_ARG;
    s.bits(ac.code[(run << 4) | nb], ac.size[(run << 4) | nb]);
    s.bits((unsigned)(v < 0 ? v - 1 : v), nb);
    run = 0;
  }
  if (run) s.bits(ac.code[0], ac.size[0]);
  return FRCNN_OK;
}

// An upper bound of what entropy_encode writes for this geometry: the headers, and per block 64 symbols of at most 16 + 10 bits, every
// byte of them stuffed.
static inline size_t stream_bound(const JpegGeom& g) { return 1024 + (size_t)g.nblk * 416; }

static inline void dht(Sink& s, int tc_th, const unsigned char* counts, const unsigned char* vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += counts[i];
  s.be16(0xFFC4), s.be16((unsigned)(2 + 1 + 16 + n)), s.byte((unsigned)tc_th), s.bytes(counts, 16), s.bytes(vals, n);
}

// -> bytes written (> 0), FRCNN_E_ARG: cap too small, a table entry outside 1..255 or a coefficient outside baseline's range
static inline long long entropy_encode(const void* coef_h, const JpegGeom& g, unsigned char* out, size_t cap) {
  if (!coef_h || (!out && cap) || g.ncomp != 3) return FRCNN_E_ARG;
  const int hs = g.mode == JPEG_S11 ? 1 : 2, vs = g.mode == JPEG_S22 ? 2 : 1;
  const uint16_t* q = (const uint16_t*)coef_h;
  for (int i = 0; i < 192; ++i)
    if (q[i] < 1 || q[i] > 255) return FRCNN_E_ARG;
  const bool third = memcmp(q + 64, q + 128, 128) != 0;          // Cr with a table of its own
  Sink s = {out, out + cap, false, 0, 0};
  static const unsigned char APP0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  s.be16(0xFFD8), s.bytes(APP0, 18);
  for (int t = 0; t < (third ? 3 : 2); ++t) {
    s.be16(0xFFDB), s.be16(67), s.byte((unsigned)t);
    for (int i = 0; i < 64; ++i) s.byte(q[64 * t + ZIGZAG[i]]);
  }
  s.be16(0xFFC0), s.be16(17), s.byte(8), s.be16((unsigned)g.h), s.be16((unsigned)g.w), s.byte(3);
  s.byte(1), s.byte((unsigned)((hs << 4) | vs)), s.byte(0);
  s.byte(2), s.byte(0x11), s.byte(1);
  s.byte(3), s.byte(0x11), s.byte(third ? 2 : 1);
  dht(s, 0x00, K_DC_BITS[0], K_DC_VALS), dht(s, 0x10, K_AC_BITS[0], K_AC_VALS[0]);
  dht(s, 0x01, K_DC_BITS[1], K_DC_VALS), dht(s, 0x11, K_AC_BITS[1], K_AC_VALS[1]);
  s.be16(0xFFDA), s.be16(12), s.byte(3), s.byte(1), s.byte(0x00), s.byte(2), s.byte(0x11), s.byte(3), s.byte(0x11), s.byte(0), s.byte(63), s.byte(0);
  EncHuff dc[2], ac[2];
  for (int t = 0; t < 2; ++t) build_enc_huff(K_DC_BITS[t], K_DC_VALS, &dc[t]), build_enc_huff(K_AC_BITS[t], K_AC_VALS[t], &ac[t]);
  const int16_t* coef = (const int16_t*)((const char*)coef_h + 384);
  int pred[3] = {0, 0, 0};
  const int mx = g.bx[0] / hs, my = g.by[0] / vs;
  for (int y = 0; y < my; ++y)
    for (int x = 0; x < mx; ++x) {
      for (int c = 0; c < 3; ++c) {
        const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1, t = c == 0 ? 0 : 1;
        for (int v = 0; v < cv; ++v)
          for (int hh = 0; hh < ch; ++hh) {
            const size_t blk = (size_t)g.blk_base[c] + (size_t)(y * cv + v) * g.bx[c] + (size_t)(x * ch + hh);
            if (encode_block(s, dc[t], ac[t], &pred[c], coef + blk * 64) != FRCNN_OK) return FRCNN_E_ARG;
          }
      }
      if (s.over) return FRCNN_E_ARG;
    }
  s.flush();
  s.be16(0xFFD9);
  return s.over ? (long long)FRCNN_E_ARG : (long long)(s.p - out);
}

}  // namespace jpeg_host
