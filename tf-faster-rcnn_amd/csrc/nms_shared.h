// What the proposal side (detect_kernels.hip) and the test-time post-processing (detect_post.hip) share: the NMS rule names and their
// overlap tests, the rule's threshold and range check, the radix-select bin pick and the in-LDS greedy reduce (with the chunk resolve it
// and the global-memory reduces of detect_kernels.hip are built on).  Included by exactly those two translation units.
#pragma once
#include "common.h"

#define NMS_RULE_CPU FRCNN_NMS_RULE_CPU    // (double)ovr >= thresh   lib/nms/cpu_nms.pyx:65
#define NMS_RULE_GPU FRCNN_NMS_RULE_GPU    // ovr > (float)thresh     lib/nms/nms_kernel.cu:71, lib/nms/py_cpu_nms.py:35
#define NMS_RULE_TF 2                      // tf.image.non_max_suppression (internal: frcnn_non_max_suppression / *_tf)

// One radix-select step over a 256-bin histogram: the bin that holds the k-th largest key and the number of keys in the bins
// above it.  Parallel suffix sum (shuffles inside the four 64-bin waves, then the wave totals); a serial walk by one thread
// costs ~10 us of dependent LDS round trips per pass.  Called by EVERY thread of the workgroup (barriers inside); k must not
// exceed the histogram total.
__device__ __forceinline__ void pick_bin(const int* hist, int k, int* wtot, int* out_bin, int* out_above) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int h = 0, x = 0;
  if (tid < 256) {
    h = hist[tid];
    x = h;
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_down(x, off, 64);
      if (lane + off < 64) x += y;                       // inclusive suffix sum inside the wave
    }
    if (lane == 0) wtot[wave] = x;
  }
  __syncthreads();
  if (tid < 256) {
    int above = 0;
    for (int w = wave + 1; w < 4; ++w) above += wtot[w];
    const int excl = x - h + above;                      // keys in bins > tid
    if (excl < k && k <= excl + h) { *out_bin = tid; *out_above = excl; }
  }
  __syncthreads();
}

template <int RULE>
__device__ __forceinline__ float rule_area(const float4 b) { return RULE == NMS_RULE_TF ? box_area_tf(b) : box_area(b); }
template <int RULE>
__device__ __forceinline__ bool rule_suppresses(const float4 a, float aa, const float4 b, float ab, float thr) {
  if (RULE == NMS_RULE_TF) return iou_suppresses_tf(a, aa, b, ab, thr);
  if (RULE == NMS_RULE_GPU) return iou_suppresses_gt(a, aa, b, ab, thr);
  return iou_suppresses(a, aa, b, ab, thr);
}

// `cur` (wave-uniform): bit b set = box b of the chunk is already removed (or past the end).  d: lane b holds the diagonal
// mask word of box b (bits > b only).  One iteration per KEPT box (not per box): next survivor = lowest clear bit.
__device__ __forceinline__ u64 resolve_chunk(u64 d, u64 cur) {
  u64 kept = 0;
  u64 avail = ~cur;
  while (avail) {
    const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)avail) - 1);
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)d, b);
    const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(d >> 32), b);
    kept |= (1ull << b);
    cur |= (((u64)hi << 32) | (u64)lo);
    avail = (b == 63) ? 0ull : (~cur & ((~0ull) << (b + 1)));
  }
  return kept;
}

// Greedy scan of a mask held in LDS (the per-class stage): one wave, mask rows `words` (<= 64) u64 wide; lane w owns the
// removed-bit word w.
template <typename Emit>
__device__ __forceinline__ int greedy_reduce_lds(const u64* mask, int K, int words, Emit emit) {
  const int lane = threadIdx.x & 63;
  u64 remv = 0ull;
  int total = 0;
  for (int c = 0; c < words; ++c) {
    const int i = c * 64 + lane;
    const u64 d = (i < K) ? mask[(size_t)i * words + c] : 0ull;
    const u64 sel = shfl_u64(remv, c);
    const u32 cur_lo = (u32)__builtin_amdgcn_readfirstlane((u32)sel);
    const u32 cur_hi = (u32)__builtin_amdgcn_readfirstlane((u32)(sel >> 32));
    u64 cur = ((u64)cur_hi << 32) | (u64)cur_lo;
    const int nvalid = min(64, K - c * 64);
    if (nvalid < 64) cur |= (~0ull) << nvalid;
    const u64 kept = resolve_chunk(d, cur);
    if ((kept >> lane) & 1ull) emit(total + __popcll(kept & ((1ull << lane) - 1ull)), i);
    total += __popcll(kept);
    if (lane > c && lane < words) {
      u64 acc = remv;
      u64 kk = kept;
      while (kk) {
        const int bq = __ffsll((long long)kk) - 1;
        kk &= kk - 1;
        acc |= mask[(size_t)(c * 64 + bq) * words + lane];
      }
      remv = acc;
    }
  }
  return total;
}

// threshold as the kernels compare it (f32): CPU rule `(double)ovr >= thresh` <=> ovr >= smallest f32 >= thresh;
// GPU rule `ovr > (float)thresh` (the reference passes a float, nms/gpu_nms.pyx:30); TF rule `iou > iou_threshold` (float attr).
static float rule_threshold(double thresh, int rule) { return rule == NMS_RULE_CPU ? thresh_to_f32(thresh) : (float)thresh; }
static bool rule_ok(int rule) { return rule == NMS_RULE_CPU || rule == NMS_RULE_GPU; }
