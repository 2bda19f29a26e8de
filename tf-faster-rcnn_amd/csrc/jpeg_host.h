// Host half of the JPEG path (no HIP includes): the marker parser and the table-driven Huffman decoder of ONE interleaved baseline scan,
// and the host statement of the pixel stage (the arithmetic of csrc/jpeg_math.h, the same code the kernels run).
//
// Supported: SOF0 / 8-bit SOF1; 1 component, or 3 components with ids 1, 2, 3, no Adobe APP14 segment, chroma 1x1 and luma 1x1 / 2x1 /
// 2x2.  Everything else that is a JPEG is FRCNN_E_UNSUPPORTED, as is data that does not start with FF D8; a damaged stream is
// FRCNN_E_ARG.  The decoder never reads past data + n and never writes outside the coefficient buffer, whatever the bytes are.
//
// Coefficient buffer: uint16 quant[3][64] (natural order, a component's own table), then int16 coefficients, un-dequantised, component
// after component, each [blocks_y][blocks_x][64] in natural order, padded to whole MCUs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "frcnn_hip.h"
#include "jpeg_math.h"

namespace jpeg_host {

static const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

enum { LOOK = 9 };

struct Huff {
  bool defined;
  uint16_t look[1 << LOOK];          // (length << 8) | symbol for codes of <= LOOK bits, 0 = longer
  int maxcode[18];                   // largest code of each length (-1: none); [17] is a sentinel
  int valoff[17];                    // vals index of a length's first code minus that code
  unsigned char vals[256];
};

struct Header {
  int width, height, ncomp, hs, vs, restart_interval, sof;
  int comp_id[3], comp_h[3], comp_v[3], comp_tq[3], comp_td[3], comp_ta[3];
  bool have_sof, adobe, have_q[4];
  uint16_t quant[4][64];             // natural order
  Huff dc[4], ac[4];
  size_t scan;                       // offset of the first entropy-coded byte
};

static inline int build_huff(const unsigned char* counts, const unsigned char* vals, int nvals, Huff* h) {
  memset(h->look, 0, sizeof(h->look));
  memcpy(h->vals, vals, (size_t)nvals);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = counts[len - 1];
    if (code + cnt > (1 << len)) return FRCNN_E_ARG;          // more codes than the length has
    h->valoff[len] = k - code;
    if (len <= LOOK)
      for (int i = 0; i < cnt; ++i) {
        const uint16_t e = (uint16_t)((len << 8) | vals[k + i]);
        const int first = (code + i) << (LOOK - len);
        for (int j = 0; j < (1 << (LOOK - len)); ++j) h->look[first + j] = e;
      }
    k += cnt;
    code += cnt;
    h->maxcode[len] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  h->maxcode[17] = 0x7fffffff;
  h->defined = true;
  return FRCNN_OK;
}

static inline int rd16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// Markers up to and including SOS.
static inline int parse_header(const unsigned char* d, size_t n, Header* H) {
  if (!d || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return FRCNN_E_UNSUPPORTED;
  memset(H, 0, sizeof(*H));
  size_t p = 2;
  for (;;) {
    if (p >= n) return FRCNN_E_ARG;
    if (d[p] != 0xFF) return FRCNN_E_ARG;
    while (p < n && d[p] == 0xFF) ++p;                          // fill bytes
    if (p >= n) return FRCNN_E_ARG;
    const int m = d[p++];
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return FRCNN_E_ARG;      // stuffing / RSTn / SOI / EOI before a scan
    if (p + 2 > n) return FRCNN_E_ARG;
    const int L = rd16(d + p);
    if (L < 2 || p + (size_t)L > n) return FRCNN_E_ARG;
    const unsigned char* s = d + p + 2;
    const int len = L - 2;
    p += (size_t)L;
    switch (m) {
      case 0xC0:
      case 0xC1: {
        if (H->have_sof || len < 6) return FRCNN_E_ARG;
        if (s[0] != 8) return FRCNN_E_UNSUPPORTED;              // 12-bit
        H->height = rd16(s + 1), H->width = rd16(s + 3), H->ncomp = s[5];
        if (H->height == 0) return FRCNN_E_UNSUPPORTED;         // DNL
        if (H->width == 0) return FRCNN_E_ARG;
        if (H->ncomp != 1 && H->ncomp != 3) return FRCNN_E_UNSUPPORTED;
        if (len != 6 + 3 * H->ncomp) return FRCNN_E_ARG;
        for (int c = 0; c < H->ncomp; ++c) {
          H->comp_id[c] = s[6 + 3 * c], H->comp_h[c] = s[7 + 3 * c] >> 4, H->comp_v[c] = s[7 + 3 * c] & 15, H->comp_tq[c] = s[8 + 3 * c];
          if (H->comp_h[c] < 1 || H->comp_h[c] > 4 || H->comp_v[c] < 1 || H->comp_v[c] > 4 || H->comp_tq[c] > 3) return FRCNN_E_ARG;
        }
        H->sof = m & 15;
        H->have_sof = true;
        break;
      }
      case 0xC4: {                                              // DHT
        int q = 0;
        while (q < len) {
          if (q + 17 > len) return FRCNN_E_ARG;
          const int tc = s[q] >> 4, th = s[q] & 15;
          if (tc > 1 || th > 3) return FRCNN_E_ARG;
          int total = 0;
          for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
          if (total > 256 || q + 17 + total > len) return FRCNN_E_ARG;
          const int rc = build_huff(s + q + 1, s + q + 17, total, tc ? &H->ac[th] : &H->dc[th]);
          if (rc != FRCNN_OK) return rc;
          q += 17 + total;
        }
        break;
      }
      case 0xDB: {                                              // DQT
        int q = 0;
        while (q < len) {
          const int pq = s[q] >> 4, tq = s[q] & 15;
          if (pq == 1) return FRCNN_E_UNSUPPORTED;              // 16-bit table
          if (pq > 1 || tq > 3 || q + 65 > len) return FRCNN_E_ARG;
          for (int i = 0; i < 64; ++i) H->quant[tq][ZIGZAG[i]] = s[q + 1 + i];
          H->have_q[tq] = true;
          q += 65;
        }
        break;
      }
      case 0xDD:                                                // DRI
        if (len != 2) return FRCNN_E_ARG;
        H->restart_interval = rd16(s);
        break;
      case 0xEE:                                                // APP14
        if (len >= 12 && memcmp(s, "Adobe", 5) == 0) H->adobe = true;
        break;
      case 0xDA: {                                              // SOS
        if (!H->have_sof || len < 1) return FRCNN_E_ARG;
        const int ns = s[0];
        if (ns < 1 || ns > 4 || len != 4 + 2 * ns) return FRCNN_E_ARG;
        if (ns != H->ncomp) return FRCNN_E_UNSUPPORTED;         // non-interleaved: several scans
        for (int c = 0; c < ns; ++c) {
          if (s[1 + 2 * c] != H->comp_id[c]) return FRCNN_E_UNSUPPORTED;
          H->comp_td[c] = s[2 + 2 * c] >> 4, H->comp_ta[c] = s[2 + 2 * c] & 15;
          if (H->comp_td[c] > 3 || H->comp_ta[c] > 3) return FRCNN_E_ARG;
        }
        if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return FRCNN_E_UNSUPPORTED;
        if (H->ncomp == 3) {
          if (H->adobe) return FRCNN_E_UNSUPPORTED;             // Adobe RGB / YCC by its transform flag
          if (H->comp_id[0] != 1 || H->comp_id[1] != 2 || H->comp_id[2] != 3) return FRCNN_E_UNSUPPORTED;
          if (H->comp_h[1] != 1 || H->comp_v[1] != 1 || H->comp_h[2] != 1 || H->comp_v[2] != 1) return FRCNN_E_UNSUPPORTED;
          H->hs = H->comp_h[0], H->vs = H->comp_v[0];
          if (!((H->hs == 1 && H->vs == 1) || (H->hs == 2 && H->vs == 1) || (H->hs == 2 && H->vs == 2))) return FRCNN_E_UNSUPPORTED;
        } else {
          H->hs = H->vs = 1;                                    // a single-component scan has one block per MCU whatever its factors
        }
        for (int c = 0; c < ns; ++c)
          if (!H->have_q[H->comp_tq[c]] || !H->dc[H->comp_td[c]].defined || !H->ac[H->comp_ta[c]].defined) return FRCNN_E_ARG;
        H->scan = p;
        return FRCNN_OK;
      }
      case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC8: case 0xC9: case 0xCA: case 0xCB: case 0xCC: case 0xCD:
      case 0xCE: case 0xCF: case 0xDC:                          // progressive, lossless, differential, arithmetic (+ DAC), DNL
        return FRCNN_E_UNSUPPORTED;
      default:                                                  // APPn, COM, reserved: skipped by their length
        break;
    }
  }
}

// MSB-first bit reader over the entropy-coded segment.  At a marker or the end of the data it stops consuming and appends zero bits,
// counted in `fake`: a decoder that has used one of them has run off the segment (checked after every block).
struct Bits {
  const unsigned char *p, *end;
  uint64_t acc;
  int n, fake;
  inline void fill() {
    while (n <= 56) {
      unsigned b = 0;
      if (p < end && *p != 0xFF) {
        b = *p++;
      } else if (p + 1 < end && p[1] == 0x00) {
        b = 0xFF;
        p += 2;
      } else {
        fake += 8;                                              // a marker (left in place), a lone trailing FF or the end
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1); }
  inline void skip(int k) { n -= k; }
  inline bool overrun() const { return n < fake; }
};

static inline int decode_symbol(Bits& b, const Huff& h) {
  const unsigned e = h.look[b.peek(LOOK)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  const int code16 = (int)b.peek(16);
  int len = LOOK + 1;
  while (len <= 16 && (code16 >> (16 - len)) > h.maxcode[len]) ++len;
  if (len > 16) return -1;
  b.skip(len);
  return h.vals[((code16 >> (16 - len)) + h.valoff[len]) & 255];
}

static inline int receive_extend(Bits& b, int s) {
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

static inline int decode_block(Bits& b, const Huff& dc, const Huff& ac, int* pred, int16_t* blk) {
  if (b.n < 32) b.fill();
  int s = decode_symbol(b, dc);
  if (s < 0 || s > 11) return FRCNN_E_ARG;
  if (s) *pred += receive_extend(b, s);
  if (*pred < -32768 || *pred > 32767) return FRCNN_E_ARG;
  blk[0] = (int16_t)*pred;
  for (int k = 1; k < 64;) {
    if (b.n < 32) b.fill();
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return FRCNN_E_ARG;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;                                       // EOB
      k += 16;
      if (k > 64) return FRCNN_E_ARG;
      continue;
    }
    k += r;
    if (k > 63 || s > 10) return FRCNN_E_ARG;
    blk[ZIGZAG[k++]] = (int16_t)receive_extend(b, s);
  }
  return b.overrun() ? FRCNN_E_ARG : FRCNN_OK;
}

static inline int info(const unsigned char* data, size_t n, int* out8) {
  if (!out8) return FRCNN_E_ARG;
  Header H;
  const int rc = parse_header(data, n, &H);
  if (rc != FRCNN_OK) return rc;
  JpegGeom g;
  if (!jpeg_geom(H.width, H.height, H.ncomp, H.hs, H.vs, &g)) return FRCNN_E_UNSUPPORTED;
  out8[0] = H.width, out8[1] = H.height, out8[2] = H.ncomp, out8[3] = H.hs, out8[4] = H.vs, out8[5] = H.restart_interval;
  out8[6] = H.sof, out8[7] = 0;
  return FRCNN_OK;
}

static inline int entropy_decode(const unsigned char* data, size_t n, void* coef_h, size_t coef_bytes) {
  if (!coef_h) return FRCNN_E_ARG;
  Header H;
  int rc = parse_header(data, n, &H);
  if (rc != FRCNN_OK) return rc;
  JpegGeom g;
  if (!jpeg_geom(H.width, H.height, H.ncomp, H.hs, H.vs, &g)) return FRCNN_E_UNSUPPORTED;
  if (coef_bytes < g.coef_bytes) return FRCNN_E_ARG;
  uint16_t* q = (uint16_t*)coef_h;
  for (int c = 0; c < 3; ++c)
    if (c < H.ncomp) memcpy(q + 64 * c, H.quant[H.comp_tq[c]], 128);
    else memset(q + 64 * c, 0, 128);
  int16_t* coef = (int16_t*)((char*)coef_h + 384);
  memset(coef, 0, (size_t)g.nblk * 128);
  Bits b = {data + H.scan, data + n, 0, 0, 0};
  int pred[3] = {0, 0, 0};
  const int mx = g.bx[0] / H.hs, my = g.by[0] / H.vs;
  long long done = 0;
  for (int y = 0; y < my; ++y)
    for (int x = 0; x < mx; ++x, ++done) {
      if (H.restart_interval && done && done % H.restart_interval == 0) {
        if (b.n - b.fake >= 8) return FRCNN_E_ARG;              // whole bytes of entropy data left before the marker
        const unsigned char* p = b.p;
        if (p >= b.end || *p != 0xFF) return FRCNN_E_ARG;
        while (p < b.end && *p == 0xFF) ++p;
        if (p >= b.end || *p != 0xD0 + (int)((done / H.restart_interval - 1) & 7)) return FRCNN_E_ARG;
        b.p = p + 1, b.acc = 0, b.n = 0, b.fake = 0;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < H.ncomp; ++c) {
        const int ch = c == 0 ? H.hs : 1, cv = c == 0 ? H.vs : 1;
        const Huff &dc = H.dc[H.comp_td[c]], &ac = H.ac[H.comp_ta[c]];
        for (int v = 0; v < cv; ++v)
          for (int h = 0; h < ch; ++h) {
            const size_t blk = (size_t)g.blk_base[c] + (size_t)(y * cv + v) * g.bx[c] + (size_t)(x * ch + h);
            rc = decode_block(b, dc, ac, &pred[c], coef + blk * 64);
            if (rc != FRCNN_OK) return rc;
          }
      }
    }
  return FRCNN_OK;
}

template <int MODE>
static inline void pixels_rows(const JpegGeom& g, const unsigned char* const* pl, unsigned char* bgr) {
  for (int y = 0; y < g.h; ++y)
    for (int x = 0; x < g.w; ++x) jpeg_pixel_bgr<MODE>(pl, g.pitch, g.cw, g.ch, x, y, bgr + ((size_t)y * g.w + x) * 3);
}

// planes: g.ws_bytes of scratch.  The host statement of frcnn_jpeg_pixels.
static inline int pixels_host(const void* coef_h, const JpegGeom& g, unsigned char* planes, unsigned char* bgr) {
  const uint16_t* q = (const uint16_t*)coef_h;
  const int16_t* coef = (const int16_t*)((const char*)coef_h + 384);
  const unsigned char* pl[3];
  for (int c = 0; c < 3; ++c) {
    pl[c] = planes + g.plane_off[c];
    for (int by = 0; by < g.by[c]; ++by)
      for (int bx = 0; bx < g.bx[c]; ++bx) {
        unsigned char out[64];
        jpeg_idct_block(coef + ((size_t)g.blk_base[c] + (size_t)by * g.bx[c] + bx) * 64, q + 64 * c, out);
        for (int r = 0; r < 8; ++r) memcpy(planes + g.plane_off[c] + (size_t)(by * 8 + r) * g.pitch[c] + bx * 8, out + r * 8, 8);
      }
  }
  switch (g.mode) {
    case JPEG_S11: pixels_rows<JPEG_S11>(g, pl, bgr); break;
    case JPEG_S21: pixels_rows<JPEG_S21>(g, pl, bgr); break;
    case JPEG_S22: pixels_rows<JPEG_S22>(g, pl, bgr); break;
    default: pixels_rows<JPEG_GREY>(g, pl, bgr); break;
  }
  return FRCNN_OK;
}

}  // namespace jpeg_host
