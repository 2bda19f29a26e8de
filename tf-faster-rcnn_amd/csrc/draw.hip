// Detections drawn on a BGR uint8 image in place, from the records and the DEVICE-RESIDENT count that Network.detect_device leaves: nothing
// is read back.  The rule is csrc/draw_math.h, shared with frcnn_draw_detections_host.
//
// A gather: each workgroup owns 1024 consecutive pixels in raster order (4 per lane: 12 contiguous bytes, three dwords, like k_jpeg_color).
// The records are staged 256 at a time, LAST chunk first: a lane prepares one record, the records that draw something and whose extent
// (box U label plate) meets the rows and columns of the workgroup's pixels are compacted in order into LDS by ballot, and every pixel walks
// the survivors from last to first and stops at the first primitive that covers it.  No two lanes write the same byte and no byte is
// written twice: the picture does not depend on scheduling.
#include "common.h"
#include "draw_math.h"

#include <vector>

static constexpr int DRAW_THREADS = 256;

__global__ __launch_bounds__(DRAW_THREADS) void k_draw_detections(unsigned char* __restrict__ bgr, DrawParams P, const float* __restrict__ dets,
                                                                  const int* __restrict__ cnt_d, const unsigned char* __restrict__ colours,
                                                                  const unsigned char* __restrict__ labels,
                                                                  const unsigned char* __restrict__ glyphs, int aligned) {
  __shared__ DrawRec recs[DRAW_THREADS];
  __shared__ int wave_n[DRAW_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t npix = (size_t)P.h * P.w;
  const size_t tp0 = (size_t)blockIdx.x * (DRAW_THREADS * 4), tp1 = (tp0 + DRAW_THREADS * 4 < npix ? tp0 + DRAW_THREADS * 4 : npix) - 1;
  const int ty0 = (int)(tp0 / (size_t)P.w), ty1 = (int)(tp1 / (size_t)P.w);
  const int tx0 = ty0 == ty1 ? (int)(tp0 - (size_t)ty0 * P.w) : 0, tx1 = ty0 == ty1 ? (int)(tp1 - (size_t)ty0 * P.w) : P.w - 1;
  const size_t p0 = tp0 + (size_t)tid * 4;
  const int n = p0 >= npix ? 0 : (npix - p0 < 4 ? (int)(npix - p0) : 4);
  int px[4], py[4];
  {
    int y = (int)((p0 < npix ? p0 : 0) / (size_t)P.w), x = (int)((p0 < npix ? p0 : 0) - (size_t)y * P.w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      px[i] = x, py[i] = y;
      if (++x == P.w) x = 0, ++y;
    }
  }
  unsigned todo = (1u << n) - 1, hit = 0;
  unsigned char col[12];
  int cnt = *cnt_d;
  cnt = cnt < 0 ? 0 : (cnt > P.max_dets ? P.max_dets : cnt);
  for (int base = cnt > 0 ? ((cnt - 1) / DRAW_THREADS) * DRAW_THREADS : -1; base >= 0; base -= DRAW_THREADS) {
    const int k = base + tid;
    DrawRec R;
    bool keep = k < cnt && draw_prepare(dets + (size_t)k * 6, P, labels, colours, &R);
    if (keep) {
      const int ex0 = R.x1 < R.px0 ? R.x1 : R.px0, ex1 = R.x2 > R.px1 - 1 ? R.x2 : R.px1 - 1;
      const int ey0 = R.y1 < R.py0 ? R.y1 : R.py0, ey1 = R.y2 > R.py1 - 1 ? R.y2 : R.py1 - 1;
      keep = !(ey1 < ty0 || ey0 > ty1 || ex1 < tx0 || ex0 > tx1);
    }
    const u64 mask = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int i = 0; i < DRAW_THREADS / 64; ++i) {
      off += i < wave ? wave_n[i] : 0;
      total += wave_n[i];
    }
    if (keep) recs[off + __popcll(mask & ((1ull << lane) - 1))] = R;
    __syncthreads();
    for (int i = total - 1; i >= 0 && todo; --i) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (((todo >> j) & 1) && draw_pixel(recs[i], P, labels, glyphs, px[j], py[j], col + 3 * j)) todo &= ~(1u << j), hit |= 1u << j;
    }
    __syncthreads();                                             // the next chunk overwrites recs and wave_n
  }
  if (!hit) return;
  unsigned char* o = bgr + p0 * 3;
  if (aligned && n == 4) {
    u32* o4 = reinterpret_cast<u32*>(o);
    unsigned char b[12];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const u32 d = o4[j];
      b[4 * j] = (unsigned char)d, b[4 * j + 1] = (unsigned char)(d >> 8), b[4 * j + 2] = (unsigned char)(d >> 16), b[4 * j + 3] = (unsigned char)(d >> 24);
    }
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if ((hit >> (j / 3)) & 1) b[j] = col[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) o4[j] = (u32)b[4 * j] | ((u32)b[4 * j + 1] << 8) | ((u32)b[4 * j + 2] << 16) | ((u32)b[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if ((hit >> (j / 3)) & 1) o[j] = col[j];
  }
}

// bgr_d [h][w][3] uint8, drawn in place (dword accesses where it is 4-byte aligned).  dets_d float32 [max_dets][6], cnt_d int32 [1]: the
// first min(*cnt_d, max_dets) records count.  colours_d uint8 [num_colours][3] BGR; labels_d uint8 [num_classes][label_stride], each name
// ending at its first NUL or at label_stride; glyphs_d uint8 [95][7], the 5 x 7 font of printable ASCII.
extern "C" int frcnn_draw_detections(unsigned char* bgr_d, int h, int w, const float* dets_d, const int* cnt_d, int max_dets, float conf,
                                     int thickness, int scale, const unsigned char* colours_d, int num_colours, const unsigned char* labels_d,
                                     int num_classes, int label_stride, const unsigned char* glyphs_d, void* stream) {
  const DrawParams P = {h, w, max_dets, thickness, scale, num_classes, label_stride, num_colours, conf};
  if (!bgr_d || !cnt_d || !colours_d || !labels_d || !glyphs_d || (!dets_d && max_dets > 0) || !draw_params_ok(P)) return FRCNN_E_ARG;
  if (max_dets == 0) return FRCNN_OK;
  const size_t npix = (size_t)h * w;
  hipLaunchKernelGGL(k_draw_detections, dim3((unsigned)((npix + DRAW_THREADS * 4 - 1) / (DRAW_THREADS * 4))), dim3(DRAW_THREADS), 0,
                     (hipStream_t)stream, bgr_d, P, dets_d, cnt_d, colours_d, labels_d, glyphs_d, ((size_t)bgr_d & 3) == 0 ? 1 : 0);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

// The host statement: the records in order, each painting the pixels of its extent that draw_pixel says it covers.
extern "C" int frcnn_draw_detections_host(unsigned char* bgr_h, int h, int w, const float* dets_h, int count, int max_dets, float conf,
                                          int thickness, int scale, const unsigned char* colours_h, int num_colours,
                                          const unsigned char* labels_h, int num_classes, int label_stride, const unsigned char* glyphs_h) {
  const DrawParams P = {h, w, max_dets, thickness, scale, num_classes, label_stride, num_colours, conf};
  if (!bgr_h || !colours_h || !labels_h || !glyphs_h || (!dets_h && max_dets > 0) || !draw_params_ok(P)) return FRCNN_E_ARG;
  const int cnt = count < 0 ? 0 : (count > max_dets ? max_dets : count);
  for (int k = 0; k < cnt; ++k) {
    DrawRec R;
    if (!draw_prepare(dets_h + (size_t)k * 6, P, labels_h, colours_h, &R)) continue;
    const int ex0 = R.x1 < R.px0 ? R.x1 : R.px0, ex1 = R.x2 > R.px1 - 1 ? R.x2 : R.px1 - 1;
    const int ey0 = R.y1 < R.py0 ? R.y1 : R.py0, ey1 = R.y2 > R.py1 - 1 ? R.y2 : R.py1 - 1;
    for (int y = ey0; y <= ey1; ++y)
      for (int x = ex0; x <= ex1; ++x) draw_pixel(R, P, labels_h, glyphs_h, x, y, bgr_h + ((size_t)y * w + x) * 3);
  }
  return FRCNN_OK;
}
