// Proposal recall (lib/datasets/imdb.py:126-214 of the reference), the per-image matching rule as plain host + device C++:
// csrc/recall.hip (the kernel and the host entry frcnn_proposal_recall_host) and the stand-alone harness csrc/recall_host_check.cc
// include this one statement.
//
//   candidate coordinate  (double)(v / scale), the division in float32 (rois / im_scale of lib/model/test.py:95 is a float32 array
//                         over a scalar); scale 1.0 leaves the box as it is
//   IoU                   lib/utils/bbox.pyx:15-55: float64, "+1" widths, ua = candidate area + gt area - iw*ih, 0 unless iw > 0 and
//                         ih > 0; the expression order of k_bbox_overlaps (csrc/detect_kernels.hip), one rounding per operation
//   G picks               among unused gt columns and unused candidate rows every column's maximum and its FIRST row; the FIRST column
//                         of the largest maximum; record it, retire that row and that column.  A gt nothing overlaps records 0.0 and
//                         still retires the first unused row.  Once the rows run out every remaining pick sees only -1: the slots get
//                         -1.0 and the image's flag is set (the reference's `assert gt_ovr >= 0`).
//
// The IoU matrix of one image lives in the caller's workspace, COLUMN-major: m[c * n + r] (a column scan reads consecutive doubles).
// Boxes are finite (a NaN has no place in either order).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RECALL_HD __host__ __device__ __forceinline__
#else
#define RECALL_HD inline
#endif

#define RECALL_RETIRED (-1.0)                 // what the reference writes over a used row / column
#define RECALL_COL_USED (-2.0)                // a retired column's maximum in the per-column state: below every live value

RECALL_HD double recall_coord(float v, float scale) { return (double)(v / scale); }

// b = candidate, q = ground truth (bbox.pyx: boxes, query_boxes)
RECALL_HD double recall_iou(const double* b, const double* q) {
  const double box_area = (q[2] - q[0] + 1) * (q[3] - q[1] + 1);
  double o = 0.0;
  const double iw = (b[2] < q[2] ? b[2] : q[2]) - (b[0] > q[0] ? b[0] : q[0]) + 1;
  if (iw > 0) {
    const double ih = (b[3] < q[3] ? b[3] : q[3]) - (b[1] > q[1] ? b[1] : q[1]) + 1;
    if (ih > 0) {
      const double ua = (b[2] - b[0] + 1) * (b[3] - b[1] + 1) + box_area - iw * ih;
      o = iw * ih / ua;
    }
  }
  return o;
}

// numpy's argmax order: a larger value wins, an equal value at a lower index wins
RECALL_HD bool recall_better(double av, long long ai, double bv, long long bi) { return av > bv || (av == bv && ai < bi); }

// rows of an image that count: the count clamped to [0, max_boxes] and to the rows behind `start`, then the first `limit` (limit <= 0: all)
RECALL_HD long long recall_rows(long long start, long long count, long long max_boxes, long long n_rows, int limit) {
  long long n = count < max_boxes ? count : max_boxes;
  if (start < 0 || start > n_rows) return 0;
  if (n > n_rows - start) n = n_rows - start;
  if (limit > 0 && n > limit) n = limit;
  return n > 0 ? n : 0;
}

// the matrix slice of the image whose first gt is g0 starts max_boxes * g0 doubles into the workspace; the per-column state (one
// double + one int64 per gt, for images with more gts than the kernel keeps in LDS) follows all matrices
RECALL_HD size_t recall_matrix_doubles(long long max_boxes, long long n_gt_total) { return (size_t)max_boxes * (size_t)n_gt_total; }
RECALL_HD size_t recall_workspace_bytes(long long max_boxes, long long n_gt_total) {
  return (recall_matrix_doubles(max_boxes, n_gt_total) + 2 * (size_t)n_gt_total) * 8 + 256;
}

// One image, the reference's loop as written: every pick rescans every column (the kernel keeps per-column state instead; both are held
// to the recorded results of the reference's own method).  box: the image's first row, `stride` floats a row, coordinates in the last four.
inline void recall_match_image_host(const float* box, int stride, long long n, float scale, const double* gt, long long G, double* m,
                                    double* out, int* ran_out) {
  *ran_out = 0;
  if (n <= 0 || G <= 0) return;
  for (long long r = 0; r < n; ++r) {
    const float* p = box + (size_t)r * stride + (stride - 4);
    const double b[4] = {recall_coord(p[0], scale), recall_coord(p[1], scale), recall_coord(p[2], scale), recall_coord(p[3], scale)};
    for (long long c = 0; c < G; ++c) m[(size_t)c * n + r] = recall_iou(b, gt + 4 * c);
  }
  for (long long j = 0; j < G; ++j) {
    double best = -3.0;
    long long best_c = -1, best_r = -1;
    for (long long c = 0; c < G; ++c) {
      double v = -3.0;
      long long a = -1;
      for (long long r = 0; r < n; ++r)
        if (a < 0 || m[(size_t)c * n + r] > v) v = m[(size_t)c * n + r], a = r;
      if (best_c < 0 || v > best) best = v, best_c = c, best_r = a;
    }
    if (best < 0) {                           // only -1 is left: the reference's assertion
      for (; j < G; ++j) out[j] = RECALL_RETIRED;
      *ran_out = 1;
      return;
    }
    out[j] = best;
    for (long long c = 0; c < G; ++c) m[(size_t)c * n + best_r] = RECALL_RETIRED;
    for (long long r = 0; r < n; ++r) m[(size_t)best_c * n + r] = RECALL_RETIRED;
  }
}
