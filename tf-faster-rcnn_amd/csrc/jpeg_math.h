// The pixel arithmetic of a baseline JPEG after the entropy decoder, stated ONCE for the host (frcnn_jpeg_pixels_host, plain C++) and
// the kernels (csrc/jpeg_decode.hip): libjpeg's integer rules -- dequantisation, jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2), the
// "fancy" triangle chroma upsampling of h2v1 / h2v2 and the 16-bit fixed-point YCbCr -> RGB tables -- so that the result equals
// PIL.Image.open(...).convert("RGB") bit for bit.  No HIP includes: a host compiler reads this file as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

enum { JPEG_S11 = 0, JPEG_S21 = 1, JPEG_S22 = 2, JPEG_GREY = 3 };      // luma sampling 1x1 / 2x1 / 2x2 (chroma 1x1), one component

JPEG_HD int jpeg_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One 8-point pass of jpeg_idct_islow: out = (butterfly(in) + (1 << (shift - 1))) >> shift; shift = 11 for the column pass (inputs =
// dequantised coefficients), 18 for the row pass.  The sums are formed in uint32: the same bits as libjpeg's int32 wherever that does
// not overflow, and defined behaviour for whatever coefficients a damaged stream holds.
JPEG_HD void jpeg_idct_1d(const int* in, int* out, int shift) {
  typedef uint32_t u;
  const u in0 = (u)in[0], in1 = (u)in[1], in2 = (u)in[2], in3 = (u)in[3], in4 = (u)in[4], in5 = (u)in[5], in6 = (u)in[6], in7 = (u)in[7];
  u z1 = (in2 + in6) * 4433u;                                   // FIX_0_541196100
  const u tmp2 = z1 - in6 * 15137u;                             // FIX_1_847759065
  const u tmp3 = z1 + in2 * 6270u;                              // FIX_0_765366865
  const u tmp0 = (in0 + in4) << 13, tmp1 = (in0 - in4) << 13;
  const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  u t0 = in7, t1 = in5, t2 = in3, t3 = in1;
  z1 = t0 + t3;
  u z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const u z5 = (z3 + z4) * 9633u;                               // FIX_1_175875602
  t0 *= 2446u;                                                  // FIX_0_298631336
  t1 *= 16819u;                                                 // FIX_2_053119869
  t2 *= 25172u;                                                 // FIX_3_072711026
  t3 *= 12299u;                                                 // FIX_1_501321110
  z1 *= (u)-7373;                                               // -FIX_0_899976223
  z2 *= (u)-20995;                                              // -FIX_2_562915447
  z3 = z3 * (u)-16069 + z5;                                     // -FIX_1_961570560
  z4 = z4 * (u)-3196 + z5;                                      // -FIX_0_390180644
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  const u rnd = 1u << (shift - 1);
  out[0] = (int)(tmp10 + t3 + rnd) >> shift, out[7] = (int)(tmp10 - t3 + rnd) >> shift;
  out[1] = (int)(tmp11 + t2 + rnd) >> shift, out[6] = (int)(tmp11 - t2 + rnd) >> shift;
  out[2] = (int)(tmp12 + t1 + rnd) >> shift, out[5] = (int)(tmp12 - t1 + rnd) >> shift;
  out[3] = (int)(tmp13 + t0 + rnd) >> shift, out[4] = (int)(tmp13 - t0 + rnd) >> shift;
}

// A whole block: coef / quant [64] in natural order -> samples [64] (0..255).  The 8-lane kernel runs the same two passes with the
// block spread over 8 lanes; this form is the host's.
JPEG_HD void jpeg_idct_block(const int16_t* coef, const uint16_t* quant, unsigned char* out) {
  int ws[64];
  for (int c = 0; c < 8; ++c) {
    int in[8], o[8];
    for (int r = 0; r < 8; ++r) in[r] = (int)coef[r * 8 + c] * (int)quant[r * 8 + c];
    jpeg_idct_1d(in, o, 11);
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = o[r];
  }
  for (int r = 0; r < 8; ++r) {
    int o[8];
    jpeg_idct_1d(ws + r * 8, o, 18);
    for (int c = 0; c < 8; ++c) out[r * 8 + c] = (unsigned char)jpeg_clamp8(o[c] + 128);
  }
}

// The chroma sample of full-resolution pixel (x, y) from a subsampled plane (row pitch `pitch`) cropped to cw x ch samples; neighbour
// indices are clamped into the cropped plane.
template <int MODE>
JPEG_HD int jpeg_chroma_at(const unsigned char* p, int pitch, int cw, int ch, int x, int y) {
  if (MODE == JPEG_S11) return p[(size_t)y * pitch + x];
  const int i = x >> 1, odd = x & 1;
  const int in = odd ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
  if (MODE == JPEG_S21) {
    const unsigned char* row = p + (size_t)y * pitch;
    return (3 * row[i] + row[in] + (odd ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;
  const int rn = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
  const unsigned char *near = p + (size_t)r * pitch, *far = p + (size_t)rn * pitch;
  const int s = 3 * near[i] + far[i], sn = 3 * near[in] + far[in];
  return (3 * s + sn + (odd ? 7 : 8)) >> 4;
}

JPEG_HD void jpeg_ycc_to_bgr(int y, int cb, int cr, unsigned char* bgr) {
  cb -= 128, cr -= 128;
  bgr[0] = (unsigned char)jpeg_clamp8(y + ((116130 * cb + 32768) >> 16));
  bgr[1] = (unsigned char)jpeg_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  bgr[2] = (unsigned char)jpeg_clamp8(y + ((91881 * cr + 32768) >> 16));
}

// Pixel (x, y) of the image from the three sample planes (grey: pl[0] only).
template <int MODE>
JPEG_HD void jpeg_pixel_bgr(const unsigned char* const* pl, const int* pitch, int cw, int ch, int x, int y, unsigned char* bgr) {
  const int Y = pl[0][(size_t)y * pitch[0] + x];
  if (MODE == JPEG_GREY) {
    bgr[0] = bgr[1] = bgr[2] = (unsigned char)Y;
    return;
  }
  jpeg_ycc_to_bgr(Y, jpeg_chroma_at<MODE>(pl[1], pitch[1], cw, ch, x, y), jpeg_chroma_at<MODE>(pl[2], pitch[2], cw, ch, x, y), bgr);
}

// Geometry of a supported stream, derived from (width, height, ncomp, hs, vs) alone -- the scalars frcnn_jpeg_info reports.
struct JpegGeom {
  int w, h, ncomp, mode;
  int bx[3], by[3];          // blocks per row / column of each component, MCU padded
  int pitch[3];              // sample plane row pitch in bytes (a multiple of 16)
  int blk_base[3];           // index of the component's first block in the coefficient buffer
  int nblk;                  // blocks of all components
  int cw, ch;                // cropped chroma plane
  size_t plane_off[3];       // byte offset of each sample plane in the workspace (256-byte aligned)
  size_t ws_bytes, coef_bytes;
};

// false: not a geometry the decoder supports
JPEG_HD bool jpeg_geom(int w, int h, int ncomp, int hs, int vs, JpegGeom* g) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return false;
  if (ncomp == 1) {
    if (hs != 1 || vs != 1) return false;
    g->mode = JPEG_GREY;
  } else if (ncomp == 3) {
    if (hs == 1 && vs == 1) g->mode = JPEG_S11;
    else if (hs == 2 && vs == 1) g->mode = JPEG_S21;
    else if (hs == 2 && vs == 2) g->mode = JPEG_S22;
    else return false;
  } else {
    return false;
  }
  g->w = w, g->h = h, g->ncomp = ncomp;
  const int mx = (w + 8 * hs - 1) / (8 * hs), my = (h + 8 * vs - 1) / (8 * vs);
  g->cw = (w + hs - 1) / hs, g->ch = (h + vs - 1) / vs;
  size_t off = 0;
  long long nblk = 0;
  for (int c = 0; c < 3; ++c) {
    const bool on = c < ncomp;
    g->bx[c] = on ? (c == 0 ? mx * hs : mx) : 0;
    g->by[c] = on ? (c == 0 ? my * vs : my) : 0;
    g->pitch[c] = (g->bx[c] * 8 + 15) / 16 * 16;
    g->blk_base[c] = (int)nblk;
    nblk += (long long)g->bx[c] * g->by[c];
    g->plane_off[c] = off;
    off += ((size_t)g->pitch[c] * g->by[c] * 8 + 255) / 256 * 256;
  }
  if (nblk > 0x7fffffffLL / 8) return false;                    // (8 lanes per block in an int thread index; 65535^2 at 4:2:0 stays below)
  g->nblk = (int)nblk;
  g->ws_bytes = off;
  g->coef_bytes = 384 + (size_t)nblk * 128;
  return true;
}

// ---- the forward direction (csrc/jpeg_encode.hip, jpeg_host::coefs_host): BGR -> the same coefficient buffer, libjpeg's integer rules of
// jccolor / jcsample (no smoothing) / jfdctint / jcdctmgr, so that the coefficients equal those of PIL's own encoder bit for bit ----------

JPEG_HD void jpeg_bgr_to_ycc(int b, int g, int r, int* y, int* cb, int* cr) {
  *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// The padding order of libjpeg's preprocessing controller, as indices: the input pixels that make up sample (sx, sy) of component c's
// MCU-padded plane.  Columns are replicated on the INPUT out to the padded width; rows are replicated on the input up to a multiple of vs,
// and below that the DOWNSAMPLED last row is replicated -- so a chroma row below the cropped plane (ch rows) is row ch - 1 again, NOT the
// mean of two copies of the last input row (an 8 x 8 image at 4:2:0 shows the difference).  Luma rows are plain replication either way.
JPEG_HD int jpeg_src_col(int x, int w) { return x < w ? x : w - 1; }
JPEG_HD int jpeg_luma_src_row(int sy, int h) { return sy < h ? sy : h - 1; }
JPEG_HD int jpeg_chroma_src_row(int cy, int ch) { return cy < ch ? cy : ch - 1; }      // then rows vs * that + {0 .. vs - 1}, each clamped to h - 1

// h2v1: (a + b + bias) >> 1, bias 0, 1, 0, 1, ... along the row; h2v2: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ...
JPEG_HD int jpeg_down_h2v1(int a, int b, int cx) { return (a + b + (cx & 1)) >> 1; }
JPEG_HD int jpeg_down_h2v2(int a, int b, int c, int d, int cx) { return (a + b + c + d + 1 + (cx & 1)) >> 2; }

// One 8-point pass of jfdctint (CONST_BITS 13, PASS1_BITS 2).  FIRST: the row pass on samples - 128 (outputs 0 and 4 scaled up by 2 bits, the
// others descaled by 11); else the column pass (0 and 4 descaled by 2, the others by 15).  uint32 sums like jpeg_idct_1d.
template <bool FIRST>
JPEG_HD void jpeg_fdct_1d(const int* in, int* out) {
  typedef uint32_t u;
  const u d0 = (u)in[0], d1 = (u)in[1], d2 = (u)in[2], d3 = (u)in[3], d4 = (u)in[4], d5 = (u)in[5], d6 = (u)in[6], d7 = (u)in[7];
  const u tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
  const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int sh = FIRST ? 11 : 15;
  const u rnd = 1u << (sh - 1);
  if (FIRST) {
    out[0] = (int)((tmp10 + tmp11) << 2), out[4] = (int)((tmp10 - tmp11) << 2);
  } else {
    out[0] = (int)(tmp10 + tmp11 + 2u) >> 2, out[4] = (int)(tmp10 - tmp11 + 2u) >> 2;
  }
  u z1 = (tmp12 + tmp13) * 4433u;                               // FIX_0_541196100
  out[2] = (int)(z1 + tmp13 * 6270u + rnd) >> sh;               // FIX_0_765366865
  out[6] = (int)(z1 + tmp12 * (u)-15137 + rnd) >> sh;           // -FIX_1_847759065
  z1 = tmp4 + tmp7;
  u z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const u z5 = (z3 + z4) * 9633u;                               // FIX_1_175875602
  const u t4 = tmp4 * 2446u, t5 = tmp5 * 16819u, t6 = tmp6 * 25172u, t7 = tmp7 * 12299u;
  z1 *= (u)-7373, z2 *= (u)-20995;
  z3 = z3 * (u)-16069 + z5, z4 = z4 * (u)-3196 + z5;
  out[7] = (int)(t4 + z1 + z3 + rnd) >> sh, out[5] = (int)(t5 + z2 + z4 + rnd) >> sh;
  out[3] = (int)(t6 + z2 + z3 + rnd) >> sh, out[1] = (int)(t7 + z1 + z4 + rnd) >> sh;
}

// n / d, truncating, for 0 <= n < 2^22 and 1 <= d <= 2040 WITHOUT an integer divide (the device has no such instruction): the float
// quotient is within one of the true one (n, d and the quotient are all exact in 24 bits; one rounding in 1 / d, one in the product),
// and two comparisons settle it.  csrc/jpeg_encode_host_check.cc compares it with `/` for every n the DCT can produce and every d.
JPEG_HD int jpeg_div_trunc(int n, int d, float rd) {
  int q = (int)((float)n * rd);
  if (q * d > n) --q;
  if ((q + 1) * d <= n) ++q;
  return q;
}

// jcdctmgr's rounding division of a DCT output (scaled by 8) by qv = 8 q: symmetric about zero.
JPEG_HD int jpeg_quantise(int c, int q, float rd) {
  const int qv = q << 3, half = qv >> 1;
  return c >= 0 ? jpeg_div_trunc(c + half, qv, rd) : -jpeg_div_trunc(half - c, qv, rd);
}
JPEG_HD float jpeg_quant_rcp(int q) { return 1.0f / (float)(q << 3); }

// The host's form of a whole block: samples [8][pitch] -> quantised coefficients [64], natural order.
JPEG_HD void jpeg_fdct_block(const unsigned char* s, int pitch, const uint16_t* quant, int16_t* coef) {
  int ws[64];
  for (int r = 0; r < 8; ++r) {
    int in[8];
    for (int c = 0; c < 8; ++c) in[c] = (int)s[(size_t)r * pitch + c] - 128;
    jpeg_fdct_1d<true>(in, ws + r * 8);
  }
  for (int c = 0; c < 8; ++c) {
    int in[8], o[8];
    for (int r = 0; r < 8; ++r) in[r] = ws[r * 8 + c];
    jpeg_fdct_1d<false>(in, o);
    for (int r = 0; r < 8; ++r) coef[r * 8 + c] = (int16_t)jpeg_quantise(o[r], quant[r * 8 + c], jpeg_quant_rcp(quant[r * 8 + c]));
  }
}

// Luma blocks that pad an MCU beyond the component's real blocks (rbx x rby of them) carry no samples: all AC zero, DC that of the block
// before it in the MCU -- at the right edge the block to its left, in a bottom row the LAST block of the row above within the same MCU
// (itself possibly a right-edge dummy).  Every dummy therefore resolves to ONE real block; returns whether (brow, bcol) is a dummy and
// writes that block's position.  Chroma has no dummies (one block per MCU).
JPEG_HD bool jpeg_dummy_source(int brow, int bcol, int hs, int rbx, int rby, int* srow, int* scol) {
  int r = brow, c = bcol;
  if (r >= rby) r -= 1, c = (c / hs) * hs + hs - 1;
  if (c >= rbx) c -= 1;
  *srow = r, *scol = c;
  return r != brow || c != bcol;
}

// libjpeg's quality scaling (jpeg_quality_scaling + jpeg_add_quant_table, force_baseline) of the Annex K tables, natural order.
JPEG_HD int jpeg_quality_entry(int base, int quality) {
  quality = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (base * s + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}
