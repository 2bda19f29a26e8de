// Baseline JPEG decode, hybrid: the serial Huffman stage on the host (csrc/jpeg_host.h, no GPU involved), everything per pixel here.
// The host hands over ONE buffer -- quantisation tables + un-dequantised int16 coefficients, 3 B per pixel at 4:2:0, what the BGR image
// would have cost over PCIe -- and two launches leave BGR uint8 [h][w][3] in HBM, the input of frcnn_prep_image / frcnn_prep_train_image:
//   k_jpeg_idct   coefficients -> uint8 sample planes in the workspace (MCU padded, row pitch a multiple of 16 B)
//   k_jpeg_color  planes -> fancy chroma upsampling + YCbCr -> BGR, 4 pixels (12 contiguous bytes, three dwords) per lane
// The arithmetic is csrc/jpeg_math.h, shared with frcnn_jpeg_pixels_host: libjpeg's integer rules, so the image equals PIL's bit for bit.
#include "common.h"
#include "jpeg_host.h"

#include <vector>

extern "C" int frcnn_jpeg_info(const unsigned char* data, size_t n, int* out8) { return jpeg_host::info(data, n, out8); }

extern "C" size_t frcnn_jpeg_coef_bytes(int width, int height, int ncomp, int hs, int vs) {
  JpegGeom g;
  return jpeg_geom(width, height, ncomp, hs, vs, &g) ? g.coef_bytes : 0;
}

extern "C" int frcnn_jpeg_entropy_decode(const unsigned char* data, size_t n, void* coef_h, size_t coef_bytes) {
  return jpeg_host::entropy_decode(data, n, coef_h, coef_bytes);
}

extern "C" int frcnn_jpeg_pixels_host(const void* coef_h, int width, int height, int ncomp, int hs, int vs, unsigned char* bgr_h) {
  JpegGeom g;
  if (!coef_h || !bgr_h) return FRCNN_E_ARG;
  if (!jpeg_geom(width, height, ncomp, hs, vs, &g)) return FRCNN_E_UNSUPPORTED;
  std::vector<unsigned char> planes(g.ws_bytes);
  return jpeg_host::pixels_host(coef_h, g, planes.data(), bgr_h);
}

extern "C" size_t frcnn_jpeg_workspace_bytes(int width, int height, int ncomp, int hs, int vs) {
  JpegGeom g;
  return jpeg_geom(width, height, ncomp, hs, vs, &g) ? g.ws_bytes : 0;
}

// 8 lanes per block, 32 blocks per workgroup.  Lane r of a block loads coefficient row r (16 B), dequantises, and the block is
// transposed through LDS so that the lane holds COLUMN r for the column pass; the pass results go back transposed, the lane picks up
// row r for the row pass and stores its 8 samples as one 8-byte store.  (A 375 x 500 image has ~4 500 blocks: one thread per block
// would launch 70 waves on 256 CUs.)
static constexpr int IDCT_THREADS = 256;

__global__ __launch_bounds__(IDCT_THREADS) void k_jpeg_idct(const unsigned char* __restrict__ coef_buf, JpegGeom g,
                                                             unsigned char* __restrict__ planes) {
  __shared__ int tile[IDCT_THREADS / 8][8][9];
  const int t = blockIdx.x * IDCT_THREADS + threadIdx.x;
  const int b = t >> 3, r = t & 7, lb = threadIdx.x >> 3;
  const bool on = b < g.nblk;
  const int c = (g.ncomp == 3 && b >= g.blk_base[1]) ? (b >= g.blk_base[2] ? 2 : 1) : 0;
  int v[8], o[8];
  if (on) {
    const uint16_t* q = reinterpret_cast<const uint16_t*>(coef_buf) + 64 * c + 8 * r;
    const int4 raw = *reinterpret_cast<const int4*>(coef_buf + 384 + ((size_t)b * 64 + (size_t)r * 8) * 2);
    const int w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = (int)(short)(w[j] & 0xffff) * (int)q[2 * j];
      v[2 * j + 1] = (w[j] >> 16) * (int)q[2 * j + 1];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[lb][r][j] = v[j];
  }
  __syncthreads();
  if (on) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[lb][j][r];
    jpeg_idct_1d(v, o, 11);
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[lb][j][r] = o[j];
  }
  __syncthreads();
  if (on) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[lb][r][j];
    jpeg_idct_1d(v, o, 18);
    const int local = b - g.blk_base[c];
    const int brow = local / g.bx[c], bcol = local - brow * g.bx[c];
    u32 lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo |= (u32)jpeg_clamp8(o[j] + 128) << (8 * j);
      hi |= (u32)jpeg_clamp8(o[4 + j] + 128) << (8 * j);
    }
    *reinterpret_cast<uint2*>(planes + g.plane_off[c] + (size_t)(brow * 8 + r) * g.pitch[c] + (size_t)bcol * 8) = make_uint2(lo, hi);
  }
}

// Pixels 4i .. 4i+3 of the image in raster order per lane: their 12 bytes start at byte 12i of bgr, dword aligned whatever the width.
// The chroma neighbours come straight from the planes (a few hundred KB, L2 resident).  The last lane of an image whose pixel count
// is no multiple of 4 stores bytes.
template <int MODE>
__global__ __launch_bounds__(256) void k_jpeg_color(const unsigned char* __restrict__ planes, JpegGeom g, unsigned char* __restrict__ bgr) {
  const size_t npix = (size_t)g.h * g.w;
  const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= npix) return;
  const unsigned char* pl[3] = {planes + g.plane_off[0], planes + g.plane_off[1], planes + g.plane_off[2]};
  const int pitch[3] = {g.pitch[0], g.pitch[1], g.pitch[2]};
  int y = (int)(p0 / (size_t)g.w), x = (int)(p0 - (size_t)y * g.w);
  const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
  unsigned char px[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < n) jpeg_pixel_bgr<MODE>(pl, pitch, g.cw, g.ch, x, y, px + 3 * i);
    else px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = 0;
    if (++x == g.w) x = 0, ++y;
  }
  unsigned char* o = bgr + p0 * 3;
  if (n == 4) {
    u32* o4 = reinterpret_cast<u32*>(o);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o4[j] = (u32)px[4 * j] | ((u32)px[4 * j + 1] << 8) | ((u32)px[4 * j + 2] << 16) | ((u32)px[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (j < 3 * n) o[j] = px[j];
  }
}

// coef_d: the buffer frcnn_jpeg_entropy_decode filled, on the device, 16-byte aligned.  bgr_d [h][w][3] uint8, 4-byte aligned.  ws:
// frcnn_jpeg_workspace_bytes() bytes, 16-byte aligned (the sample planes).  A workspace that is too small is FRCNN_E_ARG and nothing is
// launched.
extern "C" int frcnn_jpeg_pixels(const void* coef_d, int width, int height, int ncomp, int hs, int vs, unsigned char* bgr_d, void* ws,
                                 size_t ws_bytes, void* stream) {
  JpegGeom g;
  if (!coef_d || !bgr_d || !ws) return FRCNN_E_ARG;
  if (!jpeg_geom(width, height, ncomp, hs, vs, &g)) return FRCNN_E_UNSUPPORTED;
  if (ws_bytes < g.ws_bytes || ((size_t)coef_d & 15) || ((size_t)ws & 15) || ((size_t)bgr_d & 3)) return FRCNN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* coef = (const unsigned char*)coef_d;
  unsigned char* planes = (unsigned char*)ws;
  hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)(((size_t)g.nblk * 8 + IDCT_THREADS - 1) / IDCT_THREADS)), dim3(IDCT_THREADS), 0, st, coef, g,
                     planes);
  LAUNCH_CHECK();
  const dim3 grid((unsigned)(((size_t)g.h * g.w + 1023) / 1024)), block(256);
  switch (g.mode) {
    case JPEG_S11: hipLaunchKernelGGL(k_jpeg_color<JPEG_S11>, grid, block, 0, st, planes, g, bgr_d); break;
    case JPEG_S21: hipLaunchKernelGGL(k_jpeg_color<JPEG_S21>, grid, block, 0, st, planes, g, bgr_d); break;
    case JPEG_S22: hipLaunchKernelGGL(k_jpeg_color<JPEG_S22>, grid, block, 0, st, planes, g, bgr_d); break;
    default: hipLaunchKernelGGL(k_jpeg_color<JPEG_GREY>, grid, block, 0, st, planes, g, bgr_d); break;
  }
  LAUNCH_CHECK();
  return FRCNN_OK;
}
