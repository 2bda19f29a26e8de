// Proposal recall, the per-image half of imdb.evaluate_recall (reference lib/datasets/imdb.py:126-214; csrc/recall_math.h states the
// rule): the IoU of every (candidate, gt) pair in float64 and the reference's G greedy picks, for many images in one launch.  Compiled
// with -ffp-contract=off: one rounding per operation, so every recorded IoU equals the reference's bit for bit.
//
// One workgroup of RECALL_THREADS per image.  The workgroup fills the image's n x G IoU matrix into its slice of the workspace,
// column-major (140 000 doubles at 2000 x 70: it stays in L2), and a wave per column takes the column's (maximum, first row).  That
// per-column state lives in LDS for G <= RECALL_LDS_COLS, else in the workspace.  A pick is two barriers: every thread proposes its best
// column, waves reduce with shuffles, the partials meet in LDS; then the picked row is overwritten with -1 in every column (the
// reference's `overlaps[box_ind, :] = -1`) and only the live columns whose first maximum WAS that row are scanned again -- retiring any
// other row cannot change a column's first maximum.  No atomics: every value has one writer and a fixed reduction order.
#include "common.h"
#include "recall_math.h"

#define RECALL_THREADS 512
#define RECALL_WAVES (RECALL_THREADS / 64)
#define RECALL_LDS_COLS 1024

// (value, index) maximum over the wave in numpy's argmax order; every lane returns the winner
__device__ __forceinline__ void recall_wave_best(double& v, long long& i) {
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) {
    const double ov = __shfl_xor(v, step, 64);
    const long long oi = (long long)shfl_u64((u64)i, (threadIdx.x & 63) ^ step);
    if (recall_better(ov, oi, v, i)) v = ov, i = oi;
  }
}

// maximum and first row of one column, by one wave; the row being retired in this pick reads as -1 whatever memory holds yet
__device__ __forceinline__ void recall_scan_column(const double* __restrict__ col, long long n, long long retired, int lane, double& v,
                                                   long long& a) {
  v = -3.0;
  a = 0x7fffffffffffffffll;
  for (long long r = lane; r < n; r += 64) {
    const double x = r == retired ? RECALL_RETIRED : col[r];
    if (x > v) v = x, a = r;                 // rows ascend within a lane: the first of equal values stays
  }
  recall_wave_best(v, a);
}

__global__ void __launch_bounds__(RECALL_THREADS) k_proposal_recall(
    const float* __restrict__ boxes, int stride, long long n_rows, const long long* __restrict__ start, const int* __restrict__ count,
    const float* __restrict__ scale, long long max_boxes, int limit, const double* __restrict__ gt, const long long* __restrict__ gt_off,
    long long n_gt_total, double* __restrict__ out, int* __restrict__ ran_out, double* __restrict__ ws) {
  __shared__ double s_cmax[RECALL_LDS_COLS];
  __shared__ long long s_carg[RECALL_LDS_COLS];
  __shared__ double s_pv[RECALL_WAVES];
  __shared__ long long s_pc[RECALL_WAVES];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long g0 = gt_off[img], G = gt_off[img + 1] - g0;
  if (tid == 0) ran_out[img] = 0;
  if (g0 < 0 || G <= 0 || g0 + G > n_gt_total) return;          // offsets the workspace was not sized for: nothing is written
  const long long first = start[img];
  const long long n = recall_rows(first, count[img], max_boxes, n_rows, limit);
  if (n == 0) return;                                           // imdb.py:174: the gts count in num_pos, nothing is recorded
  const float sc = scale[img];
  const double* q = gt + 4 * g0;
  double* m = ws + (size_t)max_boxes * (size_t)g0;              // [G][n], inside the slice [g0 * max_boxes, (g0 + G) * max_boxes)
  double* cmax = s_cmax;
  long long* carg = s_carg;
  if (G > RECALL_LDS_COLS) {
    cmax = ws + recall_matrix_doubles(max_boxes, n_gt_total) + g0;
    carg = (long long*)(ws + recall_matrix_doubles(max_boxes, n_gt_total) + n_gt_total) + g0;
  }

  for (long long r = tid; r < n; r += RECALL_THREADS) {
    const float* p = boxes + (size_t)(first + r) * stride + (stride - 4);
    const double b[4] = {recall_coord(p[0], sc), recall_coord(p[1], sc), recall_coord(p[2], sc), recall_coord(p[3], sc)};
    for (long long c = 0; c < G; ++c) m[(size_t)c * n + r] = recall_iou(b, q + 4 * c);
  }
  __threadfence_block();
  __syncthreads();
  for (long long c = wave; c < G; c += RECALL_WAVES) {
    double v;
    long long a;
    recall_scan_column(m + (size_t)c * n, n, -1, lane, v, a);
    if (lane == 0) cmax[c] = v, carg[c] = a;
  }
  __threadfence_block();
  __syncthreads();

  for (long long j = 0; j < G; ++j) {
    double v = -3.0;
    long long c_best = 0x7fffffffffffffffll;
    for (long long c = tid; c < G; c += RECALL_THREADS) {
      const double x = cmax[c];
      if (x > v) v = x, c_best = c;
    }
    recall_wave_best(v, c_best);
    if (lane == 0) s_pv[wave] = v, s_pc[wave] = c_best;
    __syncthreads();
    v = s_pv[0], c_best = s_pc[0];
#pragma unroll
    for (int w = 1; w < RECALL_WAVES; ++w)
      if (recall_better(s_pv[w], s_pc[w], v, c_best)) v = s_pv[w], c_best = s_pc[w];
    if (v < 0) {                                                // every live column holds only -1: the candidates ran out
      for (long long k = j + tid; k < G; k += RECALL_THREADS) out[g0 + k] = RECALL_RETIRED;
      if (tid == 0) ran_out[img] = 1;
      return;
    }
    const long long row = carg[c_best];
    __syncthreads();                                            // everyone has read the partials and the picked column's state
    if (tid == 0) out[g0 + j] = v, cmax[c_best] = RECALL_COL_USED;
    for (long long c = wave; c < G; c += RECALL_WAVES) {
      if (c == c_best || cmax[c] == RECALL_COL_USED) continue;  // (wave-uniform)
      if (lane == 0) m[(size_t)c * n + row] = RECALL_RETIRED;
      if (carg[c] != row) continue;
      double cv;
      long long ca;
      recall_scan_column(m + (size_t)c * n, n, row, lane, cv, ca);
      if (lane == 0) cmax[c] = cv, carg[c] = ca;
    }
    __threadfence_block();
    __syncthreads();
  }
}

extern "C" size_t frcnn_proposal_recall_workspace_bytes(int n_images, long long max_boxes, long long n_gt_total) {
  if (n_images < 0 || max_boxes < 0 || n_gt_total < 0) return 0;
  return recall_workspace_bytes(max_boxes, n_gt_total);
}

static int recall_check_args(const void* boxes, int box_stride, long long n_rows, const void* start, const void* count, const void* scale,
                             int n_images, long long max_boxes, const void* gt, const void* gt_off, long long n_gt_total, const void* out,
                             const void* ran_out, const void* ws, size_t ws_bytes) {
  if (n_images < 0 || n_rows < 0 || max_boxes < 0 || n_gt_total < 0 || (box_stride != 4 && box_stride != 5)) return FRCNN_E_ARG;
  if (n_images == 0) return FRCNN_OK;
  if (!start || !count || !scale || !gt_off || !ran_out) return FRCNN_E_ARG;
  if ((n_rows > 0 && !boxes) || (n_gt_total > 0 && (!gt || !out || !ws))) return FRCNN_E_ARG;
  if (ws_bytes < recall_workspace_bytes(max_boxes, n_gt_total)) return FRCNN_E_ARG;
  return FRCNN_OK;
}

extern "C" int frcnn_proposal_recall(const float* boxes_d, int box_stride, long long n_rows, const long long* start_d, const int* count_d,
                                     const float* scale_d, int n_images, long long max_boxes, int limit, const double* gt_d,
                                     const long long* gt_off_d, long long n_gt_total, double* gt_iou_d, int* ran_out_d, void* ws,
                                     size_t ws_bytes, void* stream) {
  const int rc = recall_check_args(boxes_d, box_stride, n_rows, start_d, count_d, scale_d, n_images, max_boxes, gt_d, gt_off_d, n_gt_total,
                                   gt_iou_d, ran_out_d, ws, ws_bytes);
  if (rc != FRCNN_OK || n_images == 0) return rc;
  hipLaunchKernelGGL(k_proposal_recall, dim3(n_images), dim3(RECALL_THREADS), 0, (hipStream_t)stream, boxes_d, box_stride, n_rows, start_d,
                     count_d, scale_d, max_boxes, limit, gt_d, gt_off_d, n_gt_total, gt_iou_d, ran_out_d, (double*)ws);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

// The same arguments as HOST pointers, the same workspace: csrc/recall_math.h's statement of the reference's loop, image after image.
// Here every value can be read, so what the kernel can only guard against is refused: a negative count, offsets that do not run from
// gt_off[0] >= 0 to n_gt_total without decreasing.
extern "C" int frcnn_proposal_recall_host(const float* boxes, int box_stride, long long n_rows, const long long* start, const int* count,
                                          const float* scale, int n_images, long long max_boxes, int limit, const double* gt,
                                          const long long* gt_off, long long n_gt_total, double* gt_iou, int* ran_out, void* ws,
                                          size_t ws_bytes) {
  const int rc = recall_check_args(boxes, box_stride, n_rows, start, count, scale, n_images, max_boxes, gt, gt_off, n_gt_total, gt_iou,
                                   ran_out, ws, ws_bytes);
  if (rc != FRCNN_OK || n_images == 0) return rc;
  if (gt_off[0] < 0 || gt_off[n_images] > n_gt_total) return FRCNN_E_ARG;
  for (int i = 0; i < n_images; ++i)
    if (count[i] < 0 || gt_off[i + 1] < gt_off[i] || start[i] < 0 || start[i] > n_rows) return FRCNN_E_ARG;
  for (int i = 0; i < n_images; ++i) {
    const long long g0 = gt_off[i], G = gt_off[i + 1] - g0;
    const long long n = recall_rows(start[i], count[i], max_boxes, n_rows, limit);
    ran_out[i] = 0;
    if (G == 0 || n == 0) continue;
    recall_match_image_host(boxes + (size_t)start[i] * box_stride, box_stride, n, scale[i], gt + 4 * g0, G,
                            (double*)ws + (size_t)max_boxes * (size_t)g0, gt_iou + g0, &ran_out[i]);
  }
  return FRCNN_OK;
}
