// Bounding-box voting (Gidaris & Komodakis 2015, "Object detection via a multi-region & semantic segmentation-aware CNN model";
// Detectron's TEST.BBOX_VOTE) and the merge of an image's two horizontal-flip views, as plain host + device C++: csrc/detect_post.hip
// (the kernels k_perclass_vote / k_box_vote / k_merge_flip_views and the host entries frcnn_box_vote_host / frcnn_merge_flip_views_host)
// and the stand-alone harness csrc/box_vote_host_check.cc include this one statement.
//
// Voting, per class and per image:
//   candidates   the n rows that entered the per-class stage (r < num_rois and score > score_thresh): decoded, clipped box x1,y1,x2,y2
//                (float32) and the ORIGINAL cls_prob score, in ascending input row r
//   kept         the m rows the per-class stage emitted (hard NMS, or Soft-NMS with its decayed scores), in emission order
//   for a kept d ov_c = the float32 IoU of d's box with candidate c: the arithmetic of iou_suppresses (csrc/common.h) -- "+1" widths,
//                rmax / rmin, one rounding per operation (every TU is built with -ffp-contract=off), IEEE division
//                c votes iff (double)ov_c >= vote_thresh
//                W = sum (double)s_c, X_k = sum (double)s_c * (double)box_c[k], k = 0..3: SEQUENTIAL sums over the voters in ascending
//                candidate row, in IEEE double (the product of two float32 values is exact in double, so fused or not is the same)
//                new box_k = (float)(X_k / W); the score, the class and the position in the list do not change
// Nothing is re-suppressed afterwards and the max_per_image cut sees the same scores as without voting.  d itself is a candidate with
// IoU 1, so W > 0 wherever the scores are positive; where W is not > 0 (a degenerate box with no "+1" area overlaps nothing, itself
// included; a one-class call whose kept row is no candidate) the box stays as it is.
// With vote_thresh = 1.0 and no two candidates sharing a box every box keeps its bits: (s * x) / s is exact.
//
// Merge of the flip views (image b: slot 2b as seen, slot 2b+1 mirrored; R rows a slot, R' = 2R rows out):
//   rows [0, n0)        view 0's rows, unchanged
//   rows [n0, n0 + n1)  view 1's rows with x1' = (im_w_scaled - 1) - x2 and x2' = (im_w_scaled - 1) - x1 (one float32 subtraction each
//                       from the float32 value im_w_scaled - 1), dx of EVERY class negated, dy, dw, dh, the scores and column 0 copied
//   the rest            zero;  num' = n0 + n1, with n0 / n1 the slots' counts clamped to [0, R]
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BOXVOTE_HD __host__ __device__ __forceinline__
#else
#define BOXVOTE_HD inline
#endif

#define BOXVOTE_MAX 1024                      // candidates and kept rows per class

BOXVOTE_HD float boxvote_rmax(float a, float b) { return a >= b ? a : b; }
BOXVOTE_HD float boxvote_rmin(float a, float b) { return a <= b ? a : b; }
BOXVOTE_HD float boxvote_area(float x1, float y1, float x2, float y2) { return ((x2 - x1) + 1.0f) * ((y2 - y1) + 1.0f); }
// a = the kept detection, b = the candidate; aa / ab their boxvote_area
BOXVOTE_HD float boxvote_iou(float ax1, float ay1, float ax2, float ay2, float aa, float bx1, float by1, float bx2, float by2, float ab) {
  const float xx1 = boxvote_rmax(ax1, bx1), yy1 = boxvote_rmax(ay1, by1);
  const float xx2 = boxvote_rmin(ax2, bx2), yy2 = boxvote_rmin(ay2, by2);
  const float w = boxvote_rmax(0.0f, (xx2 - xx1) + 1.0f);
  const float h = boxvote_rmax(0.0f, (yy2 - yy1) + 1.0f);
  const float inter = w * h;
  return inter / ((aa + ab) - inter);
}

struct BoxVoteAcc {
  double w, x[4];
};
BOXVOTE_HD void boxvote_clear(BoxVoteAcc& a) { a.w = a.x[0] = a.x[1] = a.x[2] = a.x[3] = 0.0; }
// one candidate (box b, score s) seen by the kept detection (box a, area aa): adds it where it votes
BOXVOTE_HD void boxvote_see(BoxVoteAcc& acc, float ax1, float ay1, float ax2, float ay2, float aa, float bx1, float by1, float bx2,
                            float by2, float s, double vote_thresh) {
  const float ov = boxvote_iou(ax1, ay1, ax2, ay2, aa, bx1, by1, bx2, by2, boxvote_area(bx1, by1, bx2, by2));
  if ((double)ov >= vote_thresh) {
    const double sd = (double)s;
    acc.w = acc.w + sd;
    acc.x[0] = acc.x[0] + sd * (double)bx1;
    acc.x[1] = acc.x[1] + sd * (double)by1;
    acc.x[2] = acc.x[2] + sd * (double)bx2;
    acc.x[3] = acc.x[3] + sd * (double)by2;
  }
}
// box [4]: the kept detection's own coordinates in, the voted ones out
BOXVOTE_HD void boxvote_finish(const BoxVoteAcc& acc, float* box) {
  if (acc.w > 0.0) {
    box[0] = (float)(acc.x[0] / acc.w);
    box[1] = (float)(acc.x[1] / acc.w);
    box[2] = (float)(acc.x[2] / acc.w);
    box[3] = (float)(acc.x[3] / acc.w);
  }
}

inline bool boxvote_thresh_ok(double vote_thresh) { return vote_thresh > 0.0 && vote_thresh <= 1.0; }      // false for a NaN

// The rule as written, one class on the host: kept [m,5], cands [n,5] = x1,y1,x2,y2,score -> out [m,5]
inline void boxvote_host(const float* kept, int m, const float* cands, int n, double vote_thresh, float* out) {
  for (int d = 0; d < m; ++d) {
    const float* a = kept + 5 * (size_t)d;
    const float aa = boxvote_area(a[0], a[1], a[2], a[3]);
    BoxVoteAcc acc;
    boxvote_clear(acc);
    for (int c = 0; c < n; ++c) {
      const float* b = cands + 5 * (size_t)c;
      boxvote_see(acc, a[0], a[1], a[2], a[3], aa, b[0], b[1], b[2], b[3], b[4], vote_thresh);
    }
    float* o = out + 5 * (size_t)d;
    o[0] = a[0], o[1] = a[1], o[2] = a[2], o[3] = a[3], o[4] = a[4];
    boxvote_finish(acc, o);
  }
}

// ---- the merge of two flip views ----------------------------------------------------------------------------------------------------
BOXVOTE_HD int boxvote_clamp_count(int n, int R) { return n < 0 ? 0 : n > R ? R : n; }
// Output row rp (0 <= rp < 2R) of an image whose slots hold n0 / n1 rows -> the source slot (0 / 1) and its row, or slot -1: a zero row
BOXVOTE_HD void boxvote_merge_source(int rp, int n0, int n1, int* view, int* row) {
  if (rp < n0) *view = 0, *row = rp;
  else if (rp < n0 + n1) *view = 1, *row = rp - n0;
  else *view = -1, *row = 0;
}
// element e of an output row: e in [0, C) cls_prob, [C, 5C) bbox_pred, [5C, 5C + 5) rois; src_* point at the source row
BOXVOTE_HD float boxvote_merge_prob(const float* src_prob, int view, int j) { return view < 0 ? 0.0f : src_prob[j]; }
BOXVOTE_HD float boxvote_merge_delta(const float* src_pred, int view, int k) {
  if (view < 0) return 0.0f;
  const float v = src_pred[k];
  return (view == 1 && (k & 3) == 0) ? -v : v;
}
BOXVOTE_HD float boxvote_merge_roi(const float* src_roi, int view, int k, float wm1) {
  if (view < 0) return 0.0f;
  if (view == 1 && k == 1) return wm1 - src_roi[3];
  if (view == 1 && k == 3) return wm1 - src_roi[1];
  return src_roi[k];
}

inline void boxvote_merge_host(const float* cls_prob, const float* bbox_pred, const float* rois, const int* num_rois, int B, int R, int C,
                               float im_w_scaled, float* out_prob, float* out_pred, float* out_rois, int* out_num) {
  const float wm1 = im_w_scaled - 1.0f;
  for (int b = 0; b < B; ++b) {
    const int n0 = num_rois ? boxvote_clamp_count(num_rois[2 * b], R) : R, n1 = num_rois ? boxvote_clamp_count(num_rois[2 * b + 1], R) : R;
    out_num[b] = n0 + n1;
    for (int rp = 0; rp < 2 * R; ++rp) {
      int view, row;
      boxvote_merge_source(rp, n0, n1, &view, &row);
      const size_t src = ((size_t)(2 * b + (view > 0 ? 1 : 0)) * R + row), dst = (size_t)b * 2 * R + rp;
      for (int j = 0; j < C; ++j) out_prob[dst * C + j] = boxvote_merge_prob(cls_prob + src * C, view, j);
      if (bbox_pred)
        for (int k = 0; k < 4 * C; ++k) out_pred[dst * 4 * C + k] = boxvote_merge_delta(bbox_pred + src * 4 * C, view, k);
      for (int k = 0; k < 5; ++k) out_rois[dst * 5 + k] = boxvote_merge_roi(rois + src * 5, view, k, wm1);
    }
  }
}
