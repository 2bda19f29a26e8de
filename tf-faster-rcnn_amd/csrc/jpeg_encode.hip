// Baseline JPEG encode, hybrid -- the mirror of csrc/jpeg_decode.hip: everything per pixel here, the serial Huffman stage on the host
// (csrc/jpeg_encode_host.h, no GPU involved).  Two launches turn BGR uint8 [h][w][3] in HBM into the SAME coefficient buffer the decoder
// reads -- quantisation tables + quantised int16 coefficients, 3 B per pixel at 4:2:0 -- which is what crosses PCIe:
//   k_jpeg_ycc    BGR -> YCbCr, edge replication and h2v1 / h2v2 downsampling -> uint8 sample planes in the workspace (the decoder's layout)
//   k_jpeg_fdct   planes -> jfdctint + quantisation, 8 lanes per block, one 16-byte store of coefficients per lane
// The arithmetic is csrc/jpeg_math.h, shared with frcnn_jpeg_coefs_host: libjpeg's integer rules, so the coefficients equal those of
// PIL's encoder bit for bit.
#include "common.h"
#include "jpeg_encode_host.h"

#include <vector>

extern "C" int frcnn_jpeg_quant_tables(int quality, unsigned short* out128) {
  if (!out128 || quality < 1 || quality > 100) return FRCNN_E_ARG;
  jpeg_host::quant_tables(quality, out128);
  return FRCNN_OK;
}

extern "C" size_t frcnn_jpeg_stream_bound(int width, int height, int hs, int vs) {
  JpegGeom g;
  return jpeg_geom(width, height, 3, hs, vs, &g) ? jpeg_host::stream_bound(g) : 0;
}

extern "C" long long frcnn_jpeg_entropy_encode(const void* coef_h, int width, int height, int hs, int vs, unsigned char* out, size_t cap) {
  JpegGeom g;
  if (!jpeg_geom(width, height, 3, hs, vs, &g)) return FRCNN_E_UNSUPPORTED;
  return jpeg_host::entropy_encode(coef_h, g, out, cap);
}

extern "C" int frcnn_jpeg_coefs_host(const unsigned char* bgr_h, int width, int height, int hs, int vs, int quality, void* coef_h) {
  JpegGeom g;
  if (!bgr_h || !coef_h || quality < 1 || quality > 100) return FRCNN_E_ARG;
  if (!jpeg_geom(width, height, 3, hs, vs, &g)) return FRCNN_E_UNSUPPORTED;
  std::vector<unsigned char> planes(g.ws_bytes);
  return jpeg_host::coefs_host(bgr_h, g, quality, planes.data(), coef_h);
}

struct JpegQuant {
  uint16_t q[2][64];
};

// N (1 or 2) pixels of row `row` from column x0, columns clamped to w - 1, as 3 N bytes.  Where both columns exist, the image starts on a
// dword boundary and the dwords that hold the bytes end inside the image, they come as two or three aligned dword loads (a pixel pair
// starts at any byte offset 0 .. 3 of a dword); else byte by byte.
template <int N>
__device__ __forceinline__ void load_pixels(const unsigned char* __restrict__ bgr, size_t nbytes, bool aligned, int w, int row, int x0,
                                            unsigned char* px) {
  const size_t a = ((size_t)row * w + x0) * 3, a0 = a & ~(size_t)3;
  if (aligned && x0 + N <= w && a0 + 12 <= nbytes) {
    const u32* p = reinterpret_cast<const u32*>(bgr + a0);
    const int k = (int)(a & 3);
    u64 v = (((u64)p[1] << 32) | p[0]) >> (8 * k);
    if (N == 2 && k == 3) v |= (u64)(p[2] & 255u) << 40;
#pragma unroll
    for (int j = 0; j < 3 * N; ++j) px[j] = (unsigned char)(v >> (8 * j));
    return;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const unsigned char* s = bgr + ((size_t)row * w + jpeg_src_col(x0 + i, w)) * 3;
    px[3 * i] = s[0], px[3 * i + 1] = s[1], px[3 * i + 2] = s[2];
  }
}

// One thread per hs x vs luma group = one sample of each chroma plane, over the MCU-padded planes (64 x 4 groups per workgroup).  The
// chroma rows below the cropped plane repeat its last row (jpeg_math.h, the padding order): only there does the thread load a second set
// of pixels.
template <int MODE>
__global__ __launch_bounds__(256) void k_jpeg_ycc(const unsigned char* __restrict__ bgr, JpegGeom g, int aligned, unsigned char* __restrict__ planes) {
  constexpr int HS = MODE == JPEG_S11 ? 1 : 2, VS = MODE == JPEG_S22 ? 2 : 1;
  const int cx = blockIdx.x * 64 + threadIdx.x, cy = blockIdx.y * 4 + threadIdx.y;
  if (cx >= g.bx[1] * 8 || cy >= g.by[1] * 8) return;
  const size_t nbytes = (size_t)g.h * g.w * 3;
  int sb[HS * VS], sr[HS * VS];
#pragma unroll
  for (int j = 0; j < VS; ++j) {
    const int sy = cy * VS + j;
    unsigned char px[3 * HS];
    load_pixels<HS>(bgr, nbytes, aligned != 0, g.w, jpeg_luma_src_row(sy, g.h), cx * HS, px);
    int y[HS];
#pragma unroll
    for (int i = 0; i < HS; ++i) jpeg_bgr_to_ycc(px[3 * i], px[3 * i + 1], px[3 * i + 2], &y[i], &sb[j * HS + i], &sr[j * HS + i]);
    unsigned char* o = planes + g.plane_off[0] + (size_t)sy * g.pitch[0] + (size_t)cx * HS;
    if (HS == 2) *reinterpret_cast<uint16_t*>(o) = (uint16_t)(y[0] | (y[1] << 8));
    else *o = (unsigned char)y[0];
  }
  if (cy >= g.ch) {
    const int r0 = jpeg_chroma_src_row(cy, g.ch) * VS;
#pragma unroll
    for (int j = 0; j < VS; ++j) {
      unsigned char px[3 * HS];
      int y;
      load_pixels<HS>(bgr, nbytes, aligned != 0, g.w, jpeg_luma_src_row(r0 + j, g.h), cx * HS, px);
#pragma unroll
      for (int i = 0; i < HS; ++i) jpeg_bgr_to_ycc(px[3 * i], px[3 * i + 1], px[3 * i + 2], &y, &sb[j * HS + i], &sr[j * HS + i]);
    }
  }
  int cb = sb[0], cr = sr[0];
  if (MODE == JPEG_S21) cb = jpeg_down_h2v1(sb[0], sb[HS - 1], cx), cr = jpeg_down_h2v1(sr[0], sr[HS - 1], cx);
  if (MODE == JPEG_S22)
    cb = jpeg_down_h2v2(sb[0], sb[HS - 1], sb[HS * (VS - 1)], sb[HS * VS - 1], cx), cr = jpeg_down_h2v2(sr[0], sr[HS - 1], sr[HS * (VS - 1)], sr[HS * VS - 1], cx);
  planes[g.plane_off[1] + (size_t)cy * g.pitch[1] + cx] = (unsigned char)cb;
  planes[g.plane_off[2] + (size_t)cy * g.pitch[2] + cx] = (unsigned char)cr;
}

// 8 lanes per block, 32 blocks per workgroup -- the mirror of k_jpeg_idct.  Lane r of a block loads sample row r (8 B) and runs the row
// pass in registers; the block is transposed through a padded LDS tile so that the lane holds COLUMN r for the column pass and the
// quantisation (entries r, 8 + r, ... of the table); the results go back through the tile (each lane rewrites exactly the words it read)
// and the lane stores coefficient row r as one 16-byte store.  A dummy block's lanes run the block it resolves to (jpeg_dummy_source) and
// keep the DC alone: no block waits for another.  The tables reach the buffer's head from the kernel arguments.
static constexpr int FDCT_THREADS = 256;

template <bool ALIGNED>
__global__ __launch_bounds__(FDCT_THREADS) void k_jpeg_fdct(const unsigned char* __restrict__ planes, JpegGeom g, JpegQuant Q, int hs,
                                                             unsigned char* __restrict__ coef_buf) {
  __shared__ int tile[FDCT_THREADS / 8][8][9];
  if (blockIdx.x == 0 && threadIdx.x < 192)
    reinterpret_cast<uint16_t*>(coef_buf)[threadIdx.x] = Q.q[threadIdx.x < 64 ? 0 : 1][threadIdx.x & 63];
  const int t = blockIdx.x * FDCT_THREADS + threadIdx.x;
  const int b = t >> 3, r = t & 7, lb = threadIdx.x >> 3;
  const bool on = b < g.nblk;
  const int c = b >= g.blk_base[1] ? (b >= g.blk_base[2] ? 2 : 1) : 0;
  bool dummy = false;
  int v[8], o[8];
  if (on) {
    const int local = b - g.blk_base[c];
    const int brow = local / g.bx[c], bcol = local - brow * g.bx[c];
    int srow = brow, scol = bcol;
    if (c == 0) dummy = jpeg_dummy_source(brow, bcol, hs, (g.w + 7) >> 3, (g.h + 7) >> 3, &srow, &scol);
    const uint2 raw = *reinterpret_cast<const uint2*>(planes + g.plane_off[c] + (size_t)(srow * 8 + r) * g.pitch[c] + (size_t)scol * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (int)((raw.x >> (8 * j)) & 255u) - 128;
      v[4 + j] = (int)((raw.y >> (8 * j)) & 255u) - 128;
    }
    jpeg_fdct_1d<true>(v, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[lb][r][j] = o[j];
  }
  __syncthreads();
  if (on) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[lb][j][r];
    jpeg_fdct_1d<false>(v, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = Q.q[c ? 1 : 0][j * 8 + r];
      tile[lb][j][r] = (dummy && (j | r)) ? 0 : jpeg_quantise(o[j], q, jpeg_quant_rcp(q));
    }
  }
  __syncthreads();
  if (on) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[lb][r][j];
    unsigned char* dst = coef_buf + 384 + ((size_t)b * 64 + (size_t)r * 8) * 2;
    if (ALIGNED) {
      int4 pk;
      pk.x = (v[0] & 0xffff) | (v[1] << 16), pk.y = (v[2] & 0xffff) | (v[3] << 16);
      pk.z = (v[4] & 0xffff) | (v[5] << 16), pk.w = (v[6] & 0xffff) | (v[7] << 16);
      *reinterpret_cast<int4*>(dst) = pk;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) reinterpret_cast<int16_t*>(dst)[j] = (int16_t)v[j];
    }
  }
}

// bgr_d [h][w][3] uint8 at any address (dword loads where it is 4-byte aligned).  coef_d: frcnn_jpeg_coef_bytes(width, height, 3, hs, vs)
// bytes, 2-byte aligned (16-byte stores where it is 16-byte aligned).  ws: frcnn_jpeg_workspace_bytes() bytes, 16-byte aligned (the sample
// planes).  A workspace that is too small is FRCNN_E_ARG and nothing is launched.
extern "C" int frcnn_jpeg_coefs(const unsigned char* bgr_d, int width, int height, int hs, int vs, int quality, void* coef_d, void* ws,
                                size_t ws_bytes, void* stream) {
  JpegGeom g;
  if (!bgr_d || !coef_d || !ws || quality < 1 || quality > 100) return FRCNN_E_ARG;
  if (!jpeg_geom(width, height, 3, hs, vs, &g)) return FRCNN_E_UNSUPPORTED;
  if (ws_bytes < g.ws_bytes || ((size_t)coef_d & 1) || ((size_t)ws & 15)) return FRCNN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* planes = (unsigned char*)ws;
  JpegQuant Q;
  jpeg_host::quant_tables(quality, &Q.q[0][0]);
  const int aligned = ((size_t)bgr_d & 3) == 0;
  const dim3 grid((unsigned)((g.bx[1] * 8 + 63) / 64), (unsigned)((g.by[1] * 8 + 3) / 4)), block(64, 4);
  switch (g.mode) {
    case JPEG_S11: hipLaunchKernelGGL(k_jpeg_ycc<JPEG_S11>, grid, block, 0, st, bgr_d, g, aligned, planes); break;
    case JPEG_S21: hipLaunchKernelGGL(k_jpeg_ycc<JPEG_S21>, grid, block, 0, st, bgr_d, g, aligned, planes); break;
    default: hipLaunchKernelGGL(k_jpeg_ycc<JPEG_S22>, grid, block, 0, st, bgr_d, g, aligned, planes); break;
  }
  LAUNCH_CHECK();
  const dim3 fgrid((unsigned)(((size_t)g.nblk * 8 + FDCT_THREADS - 1) / FDCT_THREADS));
  if (((size_t)coef_d & 15) == 0)
    hipLaunchKernelGGL(k_jpeg_fdct<true>, fgrid, dim3(FDCT_THREADS), 0, st, planes, g, Q, hs, (unsigned char*)coef_d);
  else
    hipLaunchKernelGGL(k_jpeg_fdct<false>, fgrid, dim3(FDCT_THREADS), 0, st, planes, g, Q, hs, (unsigned char*)coef_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}
