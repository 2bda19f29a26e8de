// Online hard example mining for the device training step: frcnn_ohem_select and its host twin.  csrc/ohem_math.h states the rule;
// here are its three launches, all on the caller's stream, nothing allocated, no host synchronisation (legal in a recorded step):
//   k_ohem_score   one thread a proposal row: label, targets and the loss of the read-only pass's cls_score / bbox_pred row -> OhemRow
//   k_ohem_select  ONE workgroup: the keys in LDS, a rank sort (keys are unique, so the order does not depend on the schedule), the
//                  greedy pass position by position -- every thread tests the later rows it owns against the kept box, which all of them
//                  read from the same address --, then two block scans: kept rows before suppressed ones, foreground before background
//   k_ohem_emit    one thread an output row of the target layer's seven outputs
// No float atomics (the integer counters in LDS are exact in any order): the same bits on every run.  Compiled with -ffp-contract=off.
#include "common.h"
#include "ohem_math.h"

#define OHEM_THREADS 1024
#define OHEM_PER_THREAD (OHEM_MAXN / OHEM_THREADS)

__global__ __launch_bounds__(256) void k_ohem_score(const float* __restrict__ rois, int N, const int* __restrict__ num_d,
                                                    const float* __restrict__ gt, int G, int C, const float* __restrict__ cls,
                                                    const float* __restrict__ pred, double fg_thresh, double bg_hi, double bg_lo,
                                                    const OhemNorm nm, OhemRow* __restrict__ rw, float* __restrict__ roi_loss) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const int n = max(0, min(*num_d, N));
  OhemRow o;
  o.key = 0, o.loss = 0.0f, o.kind = -1, o.assigned = 0;
  if (r < n)
    o = ohem_score_row(rois + 5 * (size_t)r, (u32)r, gt, G, C, cls + (size_t)r * C, pred + (size_t)r * 4 * C, fg_thresh, bg_hi, bg_lo, nm);
  rw[r] = o;
  roi_loss[r] = o.loss;
}

// inclusive scan of one int a thread over the workgroup; every thread gets its own prefix, *total the sum
__device__ __forceinline__ int ohem_block_scan(int v, int* sh, int* total) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < OHEM_THREADS; o <<= 1) {
    const int add = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  *total = sh[OHEM_THREADS - 1];
  return sh[tid];
}

__global__ __launch_bounds__(OHEM_THREADS) void k_ohem_select(const OhemRow* __restrict__ rw, const float* __restrict__ rois, int N, int B,
                                                              float thr, int nms, int rule, int* __restrict__ keep_inds,
                                                              int* __restrict__ counts) {
  __shared__ u64 key[OHEM_MAXN];                       // after the sort: P, the selection list (unsigned short)
  __shared__ unsigned short ord[OHEM_MAXN];
  __shared__ unsigned char flag[OHEM_MAXN];            // 1 = suppressed by a kept row
  __shared__ int sh[OHEM_THREADS];
  __shared__ int m_s, nfg_s, nbg_s;
  unsigned short* P = (unsigned short*)key;
  const int tid = threadIdx.x;
  if (tid == 0) m_s = 0, nfg_s = 0, nbg_s = 0;
  __syncthreads();
  for (int i = tid; i < N; i += OHEM_THREADS) {
    const u64 k = rw[i].key;
    key[i] = k, flag[i] = 0;
    if (k != 0) {
      atomicAdd(&m_s, 1);
      atomicAdd(rw[i].kind == 1 ? &nfg_s : &nbg_s, 1);
    }
  }
  __syncthreads();
  const int m = m_s;
  for (int i = tid; i < N; i += OHEM_THREADS) {
    const u64 k = key[i];
    if (k == 0) continue;
    int rank = 0;
    for (int j = 0; j < N; ++j) rank += key[j] > k ? 1 : 0;
    ord[rank] = (unsigned short)i;
  }
  int nkept = 0, p = 0;
  for (; p < m && nkept < B; ++p) {
    __syncthreads();                                   // the order, and the flags the rows before p wrote
    if (flag[p]) continue;
    ++nkept;
    if (!nms) continue;
    const float* a = rois + 5 * (size_t)ord[p] + 1;
    for (int j = p + 1 + tid; j < m; j += OHEM_THREADS)
      if (!flag[j] && ohem_suppresses(a, rois + 5 * (size_t)ord[j] + 1, thr, rule)) flag[j] = 1;
  }
  const int p_end = p;
  __syncthreads();                                     // nobody reads a key any more: P may be written
  // P = the kept rows in order, then the others in order; thread t owns the positions [OHEM_PER_THREAD t, OHEM_PER_THREAD (t + 1))
  const int p0 = OHEM_PER_THREAD * tid;
  bool kp[OHEM_PER_THREAD];
  int c = 0;
  for (int q = 0; q < OHEM_PER_THREAD; ++q) kp[q] = p0 + q < p_end && !flag[p0 + q], c += kp[q];
  unsigned short mine[OHEM_PER_THREAD];
  for (int q = 0; q < OHEM_PER_THREAD; ++q) mine[q] = p0 + q < m ? ord[p0 + q] : 0;
  int total = 0;
  int before = ohem_block_scan(c, sh, &total) - c;     // kept rows before p0
  for (int q = 0; q < OHEM_PER_THREAD; ++q) {
    const int pos = p0 + q;
    if (pos < m) P[kp[q] ? before : total + (pos - before)] = mine[q];
    before += kp[q];
  }
  __syncthreads();
  // the B selected rows P[i mod m], foreground first; thread t owns i in [OHEM_PER_THREAD t, OHEM_PER_THREAD (t + 1))
  int src[OHEM_PER_THREAD];
  bool fg[OHEM_PER_THREAD];
  c = 0;
  for (int q = 0; q < OHEM_PER_THREAD; ++q) {
    const int i = p0 + q;
    src[q] = (i < B && m > 0) ? (int)P[i % m] : -1;
    fg[q] = src[q] >= 0 && rw[src[q]].kind == 1;
    c += fg[q];
  }
  int sel_fg = 0;
  before = ohem_block_scan(c, sh, &sel_fg) - c;        // foreground rows before i = p0
  for (int q = 0; q < OHEM_PER_THREAD; ++q) {
    const int i = p0 + q;
    if (i < B) keep_inds[m > 0 ? (fg[q] ? before : sel_fg + (i - before)) : i] = src[q];
    before += fg[q];
  }
  if (tid == 0) counts[0] = sel_fg, counts[1] = m > 0 ? B - sel_fg : 0, counts[2] = nfg_s, counts[3] = nbg_s;
}

__global__ __launch_bounds__(256) void k_ohem_emit(const OhemRow* __restrict__ rw, const int* __restrict__ keep_inds, int B,
                                                   const float* __restrict__ rois, const float* __restrict__ scores, int N,
                                                   const float* __restrict__ gt, int C, const OhemNorm nm, float* __restrict__ out_rois,
                                                   float* __restrict__ out_scores, float* __restrict__ out_labels,
                                                   float* __restrict__ out_targets, float* __restrict__ out_inside,
                                                   float* __restrict__ out_outside) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= B) return;
  int src = keep_inds[s];
  if (src < 0 || src >= N) src = -1;
  ohem_emit_row(s, src, rw, rois, scores, gt, C, nm, out_rois, out_scores, out_labels, out_targets, out_inside, out_outside);
}

static OhemNorm ohem_norm(const double* means4, const double* stds4, const double* opts) {
  OhemNorm nm;
  for (int q = 0; q < 4; ++q) nm.mean[q] = means4[q], nm.std[q] = stds4[q], nm.inside[q] = opts ? (float)opts[1 + q] : 1.0f;
  return nm;
}

// E_ARG / E_UNSUPPORTED before anything is touched, the same for both entries
static int ohem_check(const void* const* ptrs, int nptrs, int N, int G, int C, int B, const double* opts, double nms_thresh, int rule) {
  for (int i = 0; i < nptrs; ++i)
    if (!ptrs[i]) return FRCNN_E_ARG;
  if (!ohem_args_ok(N, G, C, B, nms_thresh, rule)) return FRCNN_E_ARG;
  if (N > OHEM_MAXN || B > OHEM_MAXN || G > OHEM_MAXG || (opts && opts[0] != 0.0)) return FRCNN_E_UNSUPPORTED;     // opts[0]: TRAIN.USE_GT
  return FRCNN_OK;
}

extern "C" size_t frcnn_ohem_workspace_bytes(int max_rois, int num_classes) {
  (void)num_classes;
  return align_up(sizeof(OhemRow) * (size_t)(max_rois > 0 ? max_rois : 1), 256);
}

extern "C" int frcnn_ohem_select(const float* rpn_rois_d, const float* rpn_scores_d, int max_rois, const int* num_rois_d,
                                 const float* gt_boxes_d, int G, int num_classes, const float* cls_score_d, const float* bbox_pred_d,
                                 int batch_size, double fg_thresh, double bg_thresh_hi, double bg_thresh_lo, const double* means4,
                                 const double* stds4, const double* opts, double nms_thresh, int nms_rule, float* rois_d,
                                 float* roi_scores_d, float* labels_d, float* bbox_targets_d, float* inside_w_d, float* outside_w_d,
                                 int* counts_d, int* keep_inds_d, float* roi_loss_d, void* ws, size_t ws_bytes, void* stream) {
  const void* ptrs[] = {rpn_rois_d, rpn_scores_d, num_rois_d, gt_boxes_d, cls_score_d, bbox_pred_d, means4, stds4, rois_d, roi_scores_d,
                        labels_d, bbox_targets_d, inside_w_d, outside_w_d, counts_d, keep_inds_d, roi_loss_d, ws};
  const int N = max_rois, C = num_classes, B = batch_size;
  const int rc = ohem_check(ptrs, (int)(sizeof(ptrs) / sizeof(ptrs[0])), N, G, C, B, opts, nms_thresh, nms_rule);
  if (rc != FRCNN_OK) return rc;
  if (frcnn_ohem_workspace_bytes(N, C) > ws_bytes) return FRCNN_E_WS;
  hipStream_t st = (hipStream_t)stream;
  OhemRow* rw = (OhemRow*)ws;
  const OhemNorm nm = ohem_norm(means4, stds4, opts);
  hipLaunchKernelGGL(k_ohem_score, dim3(cdiv(N, 256)), dim3(256), 0, st, rpn_rois_d, N, num_rois_d, gt_boxes_d, G, C, cls_score_d,
                     bbox_pred_d, fg_thresh, bg_thresh_hi, bg_thresh_lo, nm, rw, roi_loss_d);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ohem_select, dim3(1), dim3(OHEM_THREADS), 0, st, rw, rpn_rois_d, N, B, softnms_thresh_f32(nms_thresh, nms_rule),
                     nms_thresh > 0.0 ? 1 : 0, nms_rule, keep_inds_d, counts_d);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ohem_emit, dim3(cdiv(B, 256)), dim3(256), 0, st, rw, keep_inds_d, B, rpn_rois_d, rpn_scores_d, N, gt_boxes_d, C, nm,
                     rois_d, roi_scores_d, labels_d, bbox_targets_d, inside_w_d, outside_w_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

extern "C" int frcnn_ohem_select_host(const float* rpn_rois, const float* rpn_scores, int max_rois, const int* num_rois,
                                      const float* gt_boxes, int G, int num_classes, const float* cls_score, const float* bbox_pred,
                                      int batch_size, double fg_thresh, double bg_thresh_hi, double bg_thresh_lo, const double* means4,
                                      const double* stds4, const double* opts, double nms_thresh, int nms_rule, float* rois,
                                      float* roi_scores, float* labels, float* bbox_targets, float* inside_w, float* outside_w,
                                      int* counts, int* keep_inds, float* roi_loss) {
  const void* ptrs[] = {rpn_rois, rpn_scores, num_rois, gt_boxes, cls_score, bbox_pred, means4, stds4, rois, roi_scores,
                        labels, bbox_targets, inside_w, outside_w, counts, keep_inds, roi_loss};
  const int N = max_rois, C = num_classes, B = batch_size;
  const int rc = ohem_check(ptrs, (int)(sizeof(ptrs) / sizeof(ptrs[0])), N, G, C, B, opts, nms_thresh, nms_rule);
  if (rc != FRCNN_OK) return rc;
  const OhemNorm nm = ohem_norm(means4, stds4, opts);
  const int n = *num_rois < 0 ? 0 : (*num_rois > N ? N : *num_rois);
  static thread_local OhemRow rw[OHEM_MAXN];
  static thread_local int order[OHEM_MAXN], P[OHEM_MAXN];
  static thread_local unsigned char kept[OHEM_MAXN];
  for (int r = 0; r < N; ++r) {
    OhemRow o;
    o.key = 0, o.loss = 0.0f, o.kind = -1, o.assigned = 0;
    if (r < n)
      o = ohem_score_row(rpn_rois + 5 * (size_t)r, (uint32_t)r, gt_boxes, G, C, cls_score + (size_t)r * C, bbox_pred + (size_t)r * 4 * C,
                         fg_thresh, bg_thresh_hi, bg_thresh_lo, nm);
    rw[r] = o, roi_loss[r] = o.loss;
  }
  ohem_select_rows(rw, rpn_rois, N, B, softnms_thresh_f32(nms_thresh, nms_rule), nms_thresh > 0.0, nms_rule, order, P, kept, keep_inds, counts);
  for (int s = 0; s < B; ++s)
    ohem_emit_row(s, keep_inds[s], rw, rpn_rois, rpn_scores, gt_boxes, C, nm, rois, roi_scores, labels, bbox_targets, inside_w, outside_w);
  return FRCNN_OK;
}
