// IoU-family box regression losses for the device training step: frcnn_iou_loss and its host twin.  csrc/iouloss_math.h states the
// rule; here are its two launches on the caller's stream, nothing allocated, no atomics, no host synchronisation (legal in a recorded step):
//   k_iou_loss    one thread a slice, 256 a block: the slice in double, its four float32 gradients (every slice is written, active or
//                 not), and the block's partial sum -- the xor butterfly per wave, then the four waves in order by thread 0
//   k_iou_finish  one thread: the partials in order, times weight / mean_divisor, rounded once
// The same bits on every run, and the bits of frcnn_iou_loss_host.  Compiled with -ffp-contract=off.
#include "common.h"
#include "iouloss_math.h"

__global__ __launch_bounds__(IOULOSS_BLOCK) void k_iou_loss(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                            const float* __restrict__ in_w, const float* __restrict__ out_w, long long slices,
                                                            int K, const float* __restrict__ refs, int ref_cols, const IouLossNorm nm, int kind,
                                                            double scale, float* __restrict__ dpred, double* __restrict__ partial) {
  __shared__ double sh[IOULOSS_BLOCK / 64];
  const long long s = (long long)blockIdx.x * IOULOSS_BLOCK + threadIdx.x;
  double v = 0.0;
  if (s < slices) v = iouloss_at(s, K, pred, tgt, in_w, out_w, refs, ref_cols, nm, kind, scale, dpred);
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = 0.0;
    for (int w = 0; w < IOULOSS_BLOCK / 64; ++w) b = b + sh[w];
    partial[blockIdx.x] = b;
  }
}

__global__ void k_iou_finish(const double* __restrict__ partial, int nblocks, double scale, float* __restrict__ loss_out) {
  double s = 0.0;
  for (int i = 0; i < nblocks; ++i) s = s + partial[i];
  *loss_out = iouloss_f32(s * scale);
}

extern "C" size_t frcnn_iou_loss_workspace_bytes(long long slices) {
  const long long nb = (slices > 0 ? slices + IOULOSS_BLOCK - 1 : IOULOSS_BLOCK) / IOULOSS_BLOCK;
  return align_up((size_t)nb * sizeof(double), 256);
}

// E_ARG / E_UNSUPPORTED before anything is touched, the same for both entries
static int iou_loss_check(const void* const* ptrs, int nptrs, long long N, int K, int ref_cols, const float* means, const float* stds, int kind,
                          float weight, float mean_divisor) {
  for (int i = 0; i < nptrs; ++i)
    if (!ptrs[i]) return FRCNN_E_ARG;
  if (!iouloss_args_ok(N, K, ref_cols, means, stds, kind, weight, mean_divisor)) return FRCNN_E_ARG;
  if (N > IOULOSS_MAX_SLICES / K) return FRCNN_E_UNSUPPORTED;
  return FRCNN_OK;
}

extern "C" int frcnn_iou_loss(const float* pred_d, const float* targets_d, const float* inside_w_d, const float* outside_w_d, long long N, int K,
                              const float* refs_d, int ref_cols, const float* means, const float* stds, int kind, float weight,
                              float mean_divisor, float* loss_d, float* dpred_d, void* ws, size_t ws_bytes, void* stream) {
  const void* ptrs[] = {pred_d, targets_d, inside_w_d, outside_w_d, refs_d, means, stds, loss_d, dpred_d, ws};
  const int rc = iou_loss_check(ptrs, (int)(sizeof(ptrs) / sizeof(ptrs[0])), N, K, ref_cols, means, stds, kind, weight, mean_divisor);
  if (rc != FRCNN_OK) return rc;
  const long long slices = N * K;
  if (frcnn_iou_loss_workspace_bytes(slices) > ws_bytes) return FRCNN_E_WS;
  const int nb = (int)((slices + IOULOSS_BLOCK - 1) / IOULOSS_BLOCK);
  const double scale = iouloss_scale(weight, mean_divisor);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_iou_loss, dim3(nb), dim3(IOULOSS_BLOCK), 0, st, pred_d, targets_d, inside_w_d, outside_w_d, slices, K, refs_d, ref_cols,
                     iouloss_norm(means, stds), kind, scale, dpred_d, (double*)ws);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_iou_finish, dim3(1), dim3(1), 0, st, (const double*)ws, nb, scale, loss_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

extern "C" int frcnn_iou_loss_host(const float* pred, const float* targets, const float* inside_w, const float* outside_w, long long N, int K,
                                   const float* refs, int ref_cols, const float* means, const float* stds, int kind, float weight,
                                   float mean_divisor, float* loss, float* dpred) {
  const void* ptrs[] = {pred, targets, inside_w, outside_w, refs, means, stds, loss, dpred};
  const int rc = iou_loss_check(ptrs, (int)(sizeof(ptrs) / sizeof(ptrs[0])), N, K, ref_cols, means, stds, kind, weight, mean_divisor);
  if (rc != FRCNN_OK) return rc;
  iouloss_host(pred, targets, inside_w, outside_w, N, K, refs, ref_cols, means, stds, kind, weight, mean_divisor, loss, dpred);
  return FRCNN_OK;
}
