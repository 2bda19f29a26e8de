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
