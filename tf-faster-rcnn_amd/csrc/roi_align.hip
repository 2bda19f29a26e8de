// RoIAlign pooling (cfg.POOLING_MODE = 'align'): forward gather, deterministic backward, and the host statements of both.
// The rule -- geometry, sample positions, taps, weights, operation order -- is csrc/roialign_math.h and nothing here restates it.
#include <stdlib.h>

#include "common.h"
#include "roialign_math.h"

// ------------------------------------------------------------------------------------------------
// Forward.  The work split of k_crop_and_resize_roi (csrc/detect_kernels.hip): one workgroup per (RoI, channel slab), lanes along the
// NHWC channel axis with float4 loads, the slab index the FASTEST block index so that XCD x only touches slab x of the map and every tap
// is served by that XCD's L2.  A RoI has P*S sample rows and P*S sample columns and each of the P*P*S*S samples is a (row, column)
// pair, so the workgroup derives the geometry and the 2*P*S axis taps ONCE into LDS (threads 0 .. 2*P*S-1, one coordinate each) and
// the P*P*C/4 outputs only read them: 2*S table reads (wave-wide broadcasts) and 4*S*S float4 taps per output.
// ITEMS outputs per thread are in flight together.
// ------------------------------------------------------------------------------------------------
template <int S, int ITEMS>
__global__ __launch_bounds__(256) void k_roi_align(const float4* __restrict__ feat_all, int NIMG, int H, int W, int C4, int nslab,
                                                   const float* __restrict__ rois, float scale, int pool,
                                                   const float4* __restrict__ bias, int act, float4* __restrict__ out) {
  __shared__ RoiAlignTap tab[2][ROIALIGN_MAX_AXIS];                    // [0]: sample rows, [1]: sample columns
  const int slab = blockIdx.x % nslab, r = blockIdx.x / nslab;
  const int SC4 = C4 / nslab, c40 = slab * SC4;
  const float* roi = rois + 5 * (size_t)r;
  float4* obase = out + (size_t)r * pool * pool * C4;
  const int total = pool * pool * SC4;
  const int img = roialign_image(roi[0], NIMG);
  if (img < 0) {                                                       // (uniform) not a valid image index: defined (zero) output
    for (int t = threadIdx.x; t < total; t += 256) obase[(size_t)(t / SC4) * C4 + c40 + t % SC4] = make_float4(0, 0, 0, 0);
    return;
  }
  const int PS = pool * S;                                             // <= ROIALIGN_MAX_AXIS (launch_align)
  if ((int)threadIdx.x < 2 * PS) {
    const RoiAlignGeom g = roialign_geom(roi, scale, pool);
    const int axis = (int)threadIdx.x >= PS, i = (int)threadIdx.x - axis * PS;
    tab[axis][i] = roialign_tap(roialign_coord(axis ? g.sx : g.sy, axis ? g.bin_w : g.bin_h, i / S, i % S, S), axis ? W : H);
  }
  __syncthreads();
  const float4* feat = feat_all + (size_t)img * H * W * C4;
  const float count = (float)(S * S);
  for (int t0 = threadIdx.x; t0 < total; t0 += 256 * ITEMS) {
    float4 v[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int t = t0 + k * 256;
      v[k] = make_float4(0, 0, 0, 0);
      if (t >= total) continue;
      const int pix = t / SC4, c4 = c40 + t % SC4;
      const int ph = pix / pool, pw = pix - ph * pool;
#pragma unroll
      for (int iy = 0; iy < S; ++iy) {
        const RoiAlignTap ty = tab[0][ph * S + iy];
        if (ty.kind & ROIALIGN_ZERO) continue;
        const float4* top = feat + (size_t)ty.lo * W * C4 + c4;
        const float4* bot = feat + (size_t)ty.hi * W * C4 + c4;
#pragma unroll
        for (int ix = 0; ix < S; ++ix) {
          const RoiAlignTap tx = tab[1][pw * S + ix];
          if (tx.kind & ROIALIGN_ZERO) continue;
          const float4 v1 = top[(size_t)tx.lo * C4], v2 = top[(size_t)tx.hi * C4];
          const float4 v3 = bot[(size_t)tx.lo * C4], v4 = bot[(size_t)tx.hi * C4];
          v[k].x += roialign_sample(ty.h, ty.l, tx.h, tx.l, v1.x, v2.x, v3.x, v4.x);
          v[k].y += roialign_sample(ty.h, ty.l, tx.h, tx.l, v1.y, v2.y, v3.y, v4.y);
          v[k].z += roialign_sample(ty.h, ty.l, tx.h, tx.l, v1.z, v2.z, v3.z, v4.z);
          v[k].w += roialign_sample(ty.h, ty.l, tx.h, tx.l, v1.w, v2.w, v3.w, v4.w);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int t = t0 + k * 256;
      if (t >= total) continue;
      const int pix = t / SC4, c4 = c40 + t % SC4;
      float4 o = make_float4(v[k].x / count, v[k].y / count, v[k].z / count, v[k].w / count);
      if (bias) {                     // the fused tail entry: conv1x1(align(F)) + b == align(conv1x1(F)) + b, the bias AFTER the pooling
        const float4 bv = bias[c4];
        o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
      }
      if (act == FRCNN_ACT_RELU) o = act_relu(o);
      obase[(size_t)pix * C4 + c4] = o;
    }
  }
}

int frcnn_detect_crop_slabs();        // csrc/detect_kernels.hip: frcnn_detect_set_tuning key 4 (-1 = automatic)

static bool align_args_ok(int H, int W, int C, int R, float feat_stride, int pool, int samples) {
  return H >= 1 && W >= 1 && C > 0 && R >= 0 && feat_stride > 0.0f && pool >= 1 && samples >= 1 && samples <= ROIALIGN_MAX_SAMPLES;
}

static int launch_align(const float* feat_d, int NIMG, int H, int W, int C, const float* rois_d, int R, float feat_stride, int pool,
                        int samples, const float* bias_d, int act, float* out_d, void* stream) {
  if (NIMG <= 0 || !align_args_ok(H, W, C, R, feat_stride, pool, samples) || (act != FRCNN_ACT_NONE && act != FRCNN_ACT_RELU))
    return FRCNN_E_ARG;
  if (R == 0) return FRCNN_OK;                          // empty in, empty out (pointers may be null)
  if (!feat_d || !rois_d || !out_d) return FRCNN_E_ARG;
  if (C % 4 || pool * samples > ROIALIGN_MAX_AXIS) return FRCNN_E_UNSUPPORTED;
  const int C4 = C / 4;
  // the slab rule of launch_crop's per-RoI form: >= 512-byte runs per slab, 4 slabs put slab s on XCDs s and s + 4
  int nslab = (C4 % 8 == 0 && C4 / 8 >= 16) ? 8 : 1;
  if (nslab == 8 && C4 / 8 < 32) nslab = 4;
  const int forced = frcnn_detect_crop_slabs();
  if (forced > 0 && C4 % forced == 0) nslab = forced;
  const long long blocks = (long long)R * nslab;
  if (blocks >= (1ll << 31)) return FRCNN_E_UNSUPPORTED;
  const float scale = 1.0f / feat_stride;
  hipStream_t st = (hipStream_t)stream;
#define ALIGN_LAUNCH(S, ITEMS)                                                                                                          \
  hipLaunchKernelGGL((k_roi_align<S, ITEMS>), dim3((unsigned)blocks), dim3(256), 0, st, (const float4*)feat_d, NIMG, H, W, C4, nslab, \
                     rois_d, scale, pool, (const float4*)bias_d, act, (float4*)out_d)
  if (samples == 1) ALIGN_LAUNCH(1, 4);
  else if (samples == 2) ALIGN_LAUNCH(2, 2);
  else if (samples == 3) ALIGN_LAUNCH(3, 1);
  else ALIGN_LAUNCH(4, 1);
#undef ALIGN_LAUNCH
  LAUNCH_CHECK();
  return FRCNN_OK;
}

extern "C" int frcnn_roi_align_batched(const float* feat_d, int N, int H, int W, int C, const float* rois_d, int R, float feat_stride,
                                       int pool, int samples, const float* bias_d, int act, float* out_d, void* stream) {
  return launch_align(feat_d, N, H, W, C, rois_d, R, feat_stride, pool, samples, bias_d, act, out_d, stream);
}

// ------------------------------------------------------------------------------------------------
// Backward w.r.t. the feature map, one image.  The deterministic GATHER form of k_crop_bwd_rows (csrc/backward_kernels.hip): one
// workgroup owns ONE feature row h and NT channels; (1) all threads scan the R * P * S sample rows and compact, in ascending
// (roi, ph, iy) order, those whose low or high tap row is h (wave ballots + a running prefix: the list is a function of the inputs
// only); (2) thread = channel walks the list and adds the taps into its own column of an LDS row buffer [W][NT] in
// (roi, ph, iy, pw, ix, tap) order; (3) the buffer is added to dfeat.  No atomics and a fixed order per element: the bits depend on
// neither NT nor the window size of the hit list.
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(NT) void k_roi_align_bwd_rows(const float* __restrict__ dout, int H, int W, int C,
                                                           const float* __restrict__ rois, int R, float scale, int pool, int S, int lcap,
                                                           float* __restrict__ dfeat) {
  extern __shared__ float align_lds[];
  float* acc = align_lds;                                  // [W][NT]
  int* list = (int*)(align_lds + (size_t)W * NT);          // [lcap] hits, ascending
  __shared__ int wcnt[NT / 64];
  __shared__ int total_s;
  const int h = blockIdx.x, tid = threadIdx.x, c = blockIdx.y * NT + tid;
  const int lane = tid & 63, wave = tid >> 6;
  const int PS = pool * S;
  const float count = (float)(S * S);
  for (int w = 0; w < W; ++w) acc[w * NT + tid] = 0.f;
  if (tid == 0) total_s = 0;
  __syncthreads();
  const int n = R * PS;
  const bool live = c < C;
  auto walk = [&](int hits) {                              // thread = channel: the listed sample rows into this thread's column of acc
    for (int k = 0; k < hits; ++k) {
      const int i = list[k];
      const int r = i / PS, rem = i - r * PS;
      const int ph = rem / S, iy = rem - ph * S;
      const RoiAlignGeom g = roialign_geom(rois + 5 * (size_t)r, scale, pool);
      const RoiAlignTap ty = roialign_tap(roialign_coord(g.sy, g.bin_h, ph, iy, S), H);
      const float* drow = dout + ((size_t)r * pool + ph) * pool * C;
      for (int pw = 0; pw < pool; ++pw) {
        const float gv = (live ? drow[(size_t)pw * C + c] : 0.f) / count;
        for (int ix = 0; ix < S; ++ix) {
          const RoiAlignTap tx = roialign_tap(roialign_coord(g.sx, g.bin_w, pw, ix, S), W);
          if (tx.kind & ROIALIGN_ZERO) continue;
          if (ty.lo == h) {
            acc[tx.lo * NT + tid] += gv * (ty.h * tx.h);
            acc[tx.hi * NT + tid] += gv * (ty.h * tx.l);
          }
          if (ty.hi == h) {
            acc[tx.lo * NT + tid] += gv * (ty.l * tx.h);
            acc[tx.hi * NT + tid] += gv * (ty.l * tx.l);
          }
        }
      }
    }
  };
  for (int base = 0; base < n; base += NT) {
    if (total_s + NT > lcap) {                             // (uniform) the window is full: walk it, then refill from here
      walk(total_s);
      __syncthreads();
      if (tid == 0) total_s = 0;
      __syncthreads();
    }
    const int i = base + tid;
    bool hit = false;
    if (i < n) {
      const int r = i / PS, rem = i - r * PS;
      const RoiAlignGeom g = roialign_geom(rois + 5 * (size_t)r, scale, pool);
      const RoiAlignTap ty = roialign_tap(roialign_coord(g.sy, g.bin_h, rem / S, rem % S, S), H);
      hit = !(ty.kind & ROIALIGN_ZERO) && (ty.lo == h || ty.hi == h);
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = total_s, all = 0;
    for (int q = 0; q < NT / 64; ++q) {
      if (q < wave) off += wcnt[q];
      all += wcnt[q];
    }
    if (hit) list[off + __popcll(m & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    if (tid == 0) total_s += all;
    __syncthreads();
  }
  walk(total_s);
  if (live) {
    float* drow = dfeat + (size_t)h * W * C + c;
    for (int w = 0; w < W; ++w) drow[(size_t)w * C] += acc[w * NT + tid];
  }
}

template <int NT>
static int launch_align_bwd(const float* dout_d, int H, int W, int C, const float* rois_d, int R, float scale, int pool, int samples, int lcap,
                            float* dfeat_d, hipStream_t st) {
  static KernelOnce once;
  HIP_TRY(kernel_once(once, (const void*)k_roi_align_bwd_rows<NT>, NT, 160 * 1024 - 64));
  hipLaunchKernelGGL(k_roi_align_bwd_rows<NT>, dim3(H, cdiv(C, NT)), dim3(NT), (size_t)W * NT * 4 + (size_t)lcap * 4, st, dout_d, H, W, C,
                     rois_d, R, scale, pool, samples, lcap, dfeat_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

// max_lds_bytes > 0: the LDS budget of the launch plan (tests force the narrow / windowed forms on small inputs); 0 = the CU's 160 KB.
// The plan of frcnn_crop_and_resize_bwd_plan over R * P * S sample rows.
extern "C" int frcnn_roi_align_bwd_plan(const float* dout_d, int H, int W, int C, const float* rois_d, int R, float feat_stride, int pool,
                                        int samples, float* dfeat_d, size_t max_lds_bytes, void* stream) {
  if (!align_args_ok(H, W, C, R, feat_stride, pool, samples)) return FRCNN_E_ARG;
  if (R == 0) return FRCNN_OK;
  if (!dout_d || !rois_d || !dfeat_d) return FRCNN_E_ARG;
  const long long n = (long long)R * pool * samples;
  if (n >= (1ll << 31) - 256) return FRCNN_E_UNSUPPORTED;
  const size_t budget = (max_lds_bytes > 0 && max_lds_bytes < 160 * 1024 - 64) ? max_lds_bytes : 160 * 1024 - 64;
  const float scale = 1.0f / feat_stride;
  for (int nt = 256; nt >= 64; nt >>= 1) {
    // widest channel slab whose row buffer leaves room for a hit window of at least 4 x NT entries (or the whole list)
    const size_t accb = (size_t)W * nt * 4;
    const long long want = (n + nt - 1) / nt * nt;
    if (accb + (size_t)min(want, (long long)4 * nt) * 4 > budget) continue;
    const int lcap = (int)min(want, (long long)((budget - accb) / 4 / nt * nt));
    hipStream_t st = (hipStream_t)stream;
    if (nt == 256) return launch_align_bwd<256>(dout_d, H, W, C, rois_d, R, scale, pool, samples, lcap, dfeat_d, st);
    if (nt == 128) return launch_align_bwd<128>(dout_d, H, W, C, rois_d, R, scale, pool, samples, lcap, dfeat_d, st);
    return launch_align_bwd<64>(dout_d, H, W, C, rois_d, R, scale, pool, samples, lcap, dfeat_d, st);
  }
  return FRCNN_E_UNSUPPORTED;             // W > ~600 feature columns (an image side of ~10 000 pixels at stride 16)
}
extern "C" int frcnn_roi_align_bwd(const float* dout_d, int H, int W, int C, const float* rois_d, int R, float feat_stride, int pool,
                                   int samples, float* dfeat_d, void* stream) {
  return frcnn_roi_align_bwd_plan(dout_d, H, W, C, rois_d, R, feat_stride, pool, samples, dfeat_d, 0, stream);
}

// ------------------------------------------------------------------------------------------------
// Host statements (no GPU involved): the bit-exact reference of the kernels above, over host pointers.
// ------------------------------------------------------------------------------------------------
extern "C" int frcnn_roi_align_host(const float* feat, int N, int H, int W, int C, const float* rois, int R, float feat_stride, int pool,
                                    int samples, const float* bias, int act, float* out) {
  if (N <= 0 || !align_args_ok(H, W, C, R, feat_stride, pool, samples) || (act != FRCNN_ACT_NONE && act != FRCNN_ACT_RELU)) return FRCNN_E_ARG;
  if (R == 0) return FRCNN_OK;
  if (!feat || !rois || !out) return FRCNN_E_ARG;
  roialign_fwd_host(feat, N, H, W, C, rois, R, feat_stride, pool, samples, bias, act == FRCNN_ACT_RELU, out);
  return FRCNN_OK;
}

extern "C" int frcnn_roi_align_bwd_host(const float* dout, int H, int W, int C, const float* rois, int R, float feat_stride, int pool,
                                        int samples, float* dfeat) {
  if (!align_args_ok(H, W, C, R, feat_stride, pool, samples)) return FRCNN_E_ARG;
  if (R == 0) return FRCNN_OK;
  if (!dout || !rois || !dfeat) return FRCNN_E_ARG;
  float* row = (float*)malloc(sizeof(float) * (size_t)W * C);
  if (!row) return FRCNN_E_ARG;
  roialign_bwd_host(dout, H, W, C, rois, R, feat_stride, pool, samples, dfeat, row);
  free(row);
  return FRCNN_OK;
}

// counts [R][4]: the zeroed, clamped-low, clamped-high and integer-coordinate samples of each RoI (the kinds of roialign_math.h)
extern "C" int frcnn_roi_align_classify_host(int H, int W, const float* rois, int R, float feat_stride, int pool, int samples,
                                             long long* counts) {
  if (!align_args_ok(H, W, 1, R, feat_stride, pool, samples)) return FRCNN_E_ARG;
  if (R == 0) return FRCNN_OK;
  if (!rois || !counts) return FRCNN_E_ARG;
  roialign_classify_host(H, W, rois, R, feat_stride, pool, samples, counts);
  return FRCNN_OK;
}
