// Image preprocessing on device: the step right before the path -- lib/model/test.py:26-58
// (_get_image_blob) / lib/utils/blob.py:33-47 (prep_im_for_blob): BGR uint8 -> float32, minus PIXEL_MEANS, bilinear
// resize by im_scale with cv2.resize(..., fx, fy, INTER_LINEAR) semantics, written straight into the staged NHWC
// buffer the stem reads (C_out = 4 with a zero 4th channel, or 3).  One thread per output pixel, 3 B/pixel read
// (4 taps, L2-resident) and 16 B written: HBM-bound, 7.2 MB + 9.6 MB per 600x1000 image.
//
// cv2.resize is third-party code absent from the reference tree (OpenCV, unpinned): restated from OpenCV 3.x
// modules/imgproc/src/resize.cpp (resizeGeneric_ / HResizeLinear / VResizeLinear, 32f path):
//   scale = 1/fx (NOT src/dst);  dst size = cvRound(src * fx) (round half to even);
//   fx_d = (float)((dx + 0.5) * scale - 0.5); sx = floor(fx_d); fx_d -= sx;  sx < 0 -> (0, 0);  sx >= w-1 -> (w-1, 0)
//   rows: sy likewise but the WEIGHT is kept and the two row indices are clamped to [0, h-1]
//   value = (S[y0][x0]*(1-fx) + S[y0][x1]*fx) * (1-fy) + (S[y1][x0]*(1-fx) + S[y1][x1]*fx) * fy, every op rounded to f32
//   (columns right of the last interpolable one: S[y][x0] * 1.0f).
#include "common.h"

// np.round / cvRound: round half to even
static inline long long round_half_even(double v) { return (long long)nearbyint(v); }

extern "C" int frcnn_prep_image_shape(int h, int w, int target_size, int max_size, double* im_scale, int* out_h, int* out_w) {
  if (h <= 0 || w <= 0 || target_size <= 0 || max_size <= 0 || !im_scale || !out_h || !out_w) return FRCNN_E_ARG;
  const int smin = h < w ? h : w, smax = h < w ? w : h;
  double s = (double)target_size / (double)smin;                                       // test.py:45
  if ((double)round_half_even(s * (double)smax) > (double)max_size) s = (double)max_size / (double)smax;   // :47-48 (np.round)
  *im_scale = s;
  *out_h = (int)round_half_even((double)h * s);                                        // cv2: saturate_cast<int>(src * fx)
  *out_w = (int)round_half_even((double)w * s);
  return FRCNN_OK;
}

struct Mean3 { double b, g, r; };

// FLIP: the source is read mirrored (minibatch.py:63-64 `im[:, ::-1, :]` before anything else): mirrored column x is stored column
// w-1-x.  The tap arithmetic is unchanged, so a wave still reads its taps from the same few cache lines, in descending order.
// VEC4 (OC == 4 and a 16-byte aligned output, chosen by the launcher): one 16-byte store per lane, a wave writes 1 KiB contiguous.
// One output pixel (ox, oy) of one image: the arithmetic of k_prep_image and k_prep_image_batched, stated once.
template <typename SRC, bool FLIP, bool VEC4>
__device__ __forceinline__ void prep_pixel(const SRC* __restrict__ src, int h, int w, Mean3 mean, double scale_inv, int OW, int OC,
                                           int ox, int oy, float* __restrict__ out) {
  float fx = (float)(((double)ox + 0.5) * scale_inv - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  bool last = false;                         // dx >= xmax: the single-tap tail of HResizeLinear
  if (sx + 1 >= w) {
    last = true;
    if (sx >= w - 1) { fx = 0.f; sx = w - 1; }
  }
  float fy = (float)(((double)oy + 0.5) * scale_inv - 0.5);
  const int sy = (int)floorf(fy);
  fy -= (float)sy;
  const int y0 = min(max(sy, 0), h - 1), y1 = min(max(sy + 1, 0), h - 1);
  const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
  const int x1 = last ? sx : sx + 1;
  const int c0 = FLIP ? w - 1 - sx : sx, c1 = FLIP ? w - 1 - x1 : x1;      // stored columns of the two taps
  const double m[3] = {mean.b, mean.g, mean.r};
  float* o = out + ((size_t)oy * OW + ox) * OC;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // im.astype(float32) - PIXEL_MEANS (float64) assigned in place to float32: float64 subtraction, one rounding
    const float p00 = (float)((double)src[((size_t)y0 * w + c0) * 3 + c] - m[c]);
    const float p01 = (float)((double)src[((size_t)y0 * w + c1) * 3 + c] - m[c]);
    const float p10 = (float)((double)src[((size_t)y1 * w + c0) * 3 + c] - m[c]);
    const float p11 = (float)((double)src[((size_t)y1 * w + c1) * 3 + c] - m[c]);
    const float r0 = last ? p00 * 1.0f : p00 * a0 + p01 * a1;
    const float r1 = last ? p10 * 1.0f : p10 * a0 + p11 * a1;
    v[c] = r0 * b0 + r1 * b1;
  }
  if (VEC4) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], 0.f);
  } else {
    o[0] = v[0], o[1] = v[1], o[2] = v[2];
    if (OC == 4) o[3] = 0.f;
  }
}

template <typename SRC, bool FLIP, bool VEC4>
__global__ void k_prep_image(const SRC* __restrict__ src, int h, int w, Mean3 mean, double scale_inv, int OH, int OW, int OC,
                             float* __restrict__ out) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
  if (ox >= OW) return;
  prep_pixel<SRC, FLIP, VEC4>(src, h, w, mean, scale_inv, OW, OC, ox, oy, out);
}

// B same-size images in one launch: image b = blockIdx.z reads src[b][h][w][3] and writes out[b][OH][OW][OC].
template <typename SRC, bool VEC4>
__global__ void k_prep_image_batched(const SRC* __restrict__ src, int h, int w, Mean3 mean, double scale_inv, int OH, int OW, int OC,
                                     float* __restrict__ out) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y, b = blockIdx.z;
  if (ox >= OW) return;
  prep_pixel<SRC, false, VEC4>(src + (size_t)b * h * w * 3, h, w, mean, scale_inv, OW, OC, ox, oy, out + (size_t)b * OH * OW * OC);
}

template <typename SRC, bool FLIP>
static void launch_prep(const void* src_d, int h, int w, const double* pixel_means, double im_scale, float* out_d, int OH, int OW, int out_c,
                        hipStream_t stream) {
  const Mean3 mean = {pixel_means[0], pixel_means[1], pixel_means[2]};
  const dim3 grid((OW + 255) / 256, OH), block(256);
  if (out_c == 4 && ((size_t)out_d & 15) == 0)
    hipLaunchKernelGGL((k_prep_image<SRC, FLIP, true>), grid, block, 0, stream, (const SRC*)src_d, h, w, mean, 1.0 / im_scale, OH, OW, out_c, out_d);
  else
    hipLaunchKernelGGL((k_prep_image<SRC, FLIP, false>), grid, block, 0, stream, (const SRC*)src_d, h, w, mean, 1.0 / im_scale, OH, OW, out_c, out_d);
}

// src_d: BGR [h][w][3], uint8 (src_is_float = 0) or float32 (1).  pixel_means: HOST double[3] (B,G,R; config.py PIXEL_MEANS).
// out_d: float32 [OH][OW][out_c], out_c = 3 or 4 (4th channel zero), OH/OW from frcnn_prep_image_shape.
extern "C" int frcnn_prep_image(const void* src_d, int src_is_float, int h, int w, const double* pixel_means, double im_scale,
                                float* out_d, int OH, int OW, int out_c, void* stream) {
  if (!src_d || !pixel_means || !out_d || h <= 0 || w <= 0 || OH <= 0 || OW <= 0 || !(im_scale > 0)) return FRCNN_E_ARG;
  if (out_c != 3 && out_c != 4) return FRCNN_E_UNSUPPORTED;
  if (src_is_float)
    launch_prep<float, false>(src_d, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, (hipStream_t)stream);
  else
    launch_prep<unsigned char, false>(src_d, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, (hipStream_t)stream);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

template <typename SRC>
static void launch_prep_batched(const void* src_d, int B, int h, int w, const double* pixel_means, double im_scale, float* out_d, int OH,
                                int OW, int out_c, hipStream_t stream) {
  const Mean3 mean = {pixel_means[0], pixel_means[1], pixel_means[2]};
  const dim3 grid((OW + 255) / 256, OH, B), block(256);
  // a slot starts OH * OW * 16 bytes after the one before: every slot is 16-byte aligned iff the first is -- frcnn_prep_image's condition
  if (out_c == 4 && ((size_t)out_d & 15) == 0)
    hipLaunchKernelGGL((k_prep_image_batched<SRC, true>), grid, block, 0, stream, (const SRC*)src_d, h, w, mean, 1.0 / im_scale, OH, OW, out_c, out_d);
  else
    hipLaunchKernelGGL((k_prep_image_batched<SRC, false>), grid, block, 0, stream, (const SRC*)src_d, h, w, mean, 1.0 / im_scale, OH, OW, out_c, out_d);
}

// frcnn_prep_image of B same-size images in ONE launch (the image index on gridDim.z; B <= 65535, OH <= 65535: the grid's limits):
// src_d [B][h][w][3] -> out_d [B][OH][OW][out_c], slot b bit-identical to frcnn_prep_image of image b (both kernels call prep_pixel).
extern "C" int frcnn_prep_image_batched(const void* src_d, int src_is_float, int B, int h, int w, const double* pixel_means, double im_scale,
                                        float* out_d, int OH, int OW, int out_c, void* stream) {
  if (!src_d || !pixel_means || !out_d || B <= 0 || h <= 0 || w <= 0 || OH <= 0 || OW <= 0 || !(im_scale > 0)) return FRCNN_E_ARG;
  if (B > 65535 || OH > 65535) return FRCNN_E_ARG;
  if (out_c != 3 && out_c != 4) return FRCNN_E_UNSUPPORTED;
  if (src_is_float)
    launch_prep_batched<float>(src_d, B, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, (hipStream_t)stream);
  else
    launch_prep_batched<unsigned char>(src_d, B, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, (hipStream_t)stream);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

// The two views of the test-time flip ensemble (cfg.HIP.TEST_FLIP): slot 2b = prepared image b, slot 2b+1 = its columns x <-> OW-1-x.
// One thread per source pixel writes both; an exact permutation of the PREPARED image (not a second resize of the mirrored source).
__global__ void k_mirror_views(const float* __restrict__ in, int OH, int OW, int c, float* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= OW) return;
  const float* s = in + (((size_t)b * OH + y) * OW + x) * c;
  float* o0 = out + (((size_t)(2 * b) * OH + y) * OW + x) * c;
  float* o1 = out + (((size_t)(2 * b + 1) * OH + y) * OW + (OW - 1 - x)) * c;
  for (int k = 0; k < c; ++k) {
    const float v = s[k];
    o0[k] = v;
    o1[k] = v;
  }
}

// in_d [B][OH][OW][c] -> out_d [2B][OH][OW][c] (B <= 65535, OH <= 65535: the grid's limits; c >= 1); the buffers must not overlap
extern "C" int frcnn_mirror_views(const float* in_d, int B, int OH, int OW, int c, float* out_d, void* stream) {
  if (!in_d || !out_d || B <= 0 || OH <= 0 || OW <= 0 || c <= 0 || B > 65535 || OH > 65535) return FRCNN_E_ARG;
  hipLaunchKernelGGL(k_mirror_views, dim3((OW + 255) / 256, OH, B), dim3(256), 0, (hipStream_t)stream, in_d, OH, OW, c, out_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

// minibatch.py:44-46: gt_boxes[:, 0:4] = boxes (uint16) * im_scale (Python float) -> float64 product, rounded once into the float32 blob;
// gt_boxes[:, 4] = gt_classes (int32).  One thread per row.
__global__ void k_fill_gt(const unsigned short* __restrict__ boxes, const int* __restrict__ classes, int G, double im_scale,
                          float* __restrict__ gt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) gt[i * 5 + k] = (float)((double)boxes[i * 4 + k] * im_scale);
  gt[i * 5 + 4] = (float)classes[i];
}

// The training minibatch of ONE roidb entry (lib/roi_data_layer/minibatch.py:19-74 + lib/utils/blob.py:33-47) staged on device:
// frcnn_prep_image on the source mirrored iff `flipped`, and rows [0,G) of the static gt buffer gt_d [>=G][5] from the entry's
// boxes_d uint16 [G][4] / classes_d int32 [G] (a second tiny launch on the same stream; G = 0: skipped, pointers may be NULL).
extern "C" int frcnn_prep_train_image(const void* src_d, int src_is_float, int h, int w, int flipped, const double* pixel_means,
                                      double im_scale, float* out_d, int OH, int OW, int out_c, const unsigned short* boxes_d,
                                      const int* classes_d, int G, float* gt_d, void* stream) {
  if (!src_d || !pixel_means || !out_d || h <= 0 || w <= 0 || OH <= 0 || OW <= 0 || !(im_scale > 0) || G < 0) return FRCNN_E_ARG;
  if (G > 0 && (!boxes_d || !classes_d || !gt_d)) return FRCNN_E_ARG;
  if (out_c != 3 && out_c != 4) return FRCNN_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (src_is_float) {
    if (flipped) launch_prep<float, true>(src_d, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, st);
    else launch_prep<float, false>(src_d, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, st);
  } else {
    if (flipped) launch_prep<unsigned char, true>(src_d, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, st);
    else launch_prep<unsigned char, false>(src_d, h, w, pixel_means, im_scale, out_d, OH, OW, out_c, st);
  }
  LAUNCH_CHECK();
  if (G > 0) {
    hipLaunchKernelGGL(k_fill_gt, dim3((G + 63) / 64), dim3(64), 0, st, boxes_d, classes_d, G, im_scale, gt_d);
    LAUNCH_CHECK();
  }
  return FRCNN_OK;
}
