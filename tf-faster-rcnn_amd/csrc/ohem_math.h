// Online hard example mining (Shrivastava, Gupta, Girshick, CVPR 2016, "Training Region-based Object Detectors with Online Hard Example
// Mining"): which BATCH_SIZE proposals a training step trains on, as plain host + device C++.  csrc/ohem.hip (the kernels and the host
// entry frcnn_ohem_select_host) and the stand-alone harness csrc/ohem_host_check.cc include this one statement.
//
//   candidates   the valid rows r < n = *num_rois of the padded proposal buffer [N,5] (N <= OHEM_MAXN) whose label rule below says
//                foreground or background; a row that is neither is no candidate.  TRAIN.USE_GT is refused.
//   labels       ohem_classify: ohem_iou_f64 -- the float64 arithmetic of utils/bbox.pyx, the ONE statement csrc/train_kernels.hip's
//                iou_f64 forwards to -- against every gt box, the FIRST arg-max, foreground where max >= FG_THRESH, background where
//                BG_THRESH_LO <= max < BG_THRESH_HI; label = the arg-max box's class for foreground, 0 for background
//   targets      ohem_encode: bbox_transform in float32, one rounding per operation, like encode_box of csrc/train_kernels.hip, EXCEPT
//                that log(gw / ew) is (float)ohem_log((double)(gw / ew)) -- logf is not the same function on host and device --, then
//                ohem_normalise: (float)(((double)t - mean) / std)
//   loss         ohem_row_loss, in double, rounded ONCE to float32:
//                  L = log(sum_c E(z_c - max z)) + max z - z_label                     c = 0 ... C-1 in this order, max = the first largest
//                    + [label > 0] sum_q out_w_q * smoothL1(in_w_q * (pred_q - t_q))   q = 0 ... 3 in this order, sigma = 1,
//                                                                                       out_w = in_w > 0, pred = bbox_pred[4 label + q]
//                the per-row terms of Network._add_losses before the mean.  A row with a logit, a prediction or a target that is not
//                finite has L = NaN (the canonical 0x7fc00000), as has a label outside [0, C).
//   E, log       E = softnms_exp_neg (csrc/softnms_math.h, x <= 0); ohem_log below for the sum in [1, C] and the width ratios: IEEE
//                double + - * / and integer bit operations only, so host and gfx950 return the same bits.  Against libm's log
//                (csrc/ohem_host_check.cc, x86-64 glibc): x = 1 + i (C - 1) / 2^20 for C = 81 and x = 2^(i / 2^16 - 8), i = 0 ... 2^20:
//                largest relative distance in double 4.7e-16; E over x = -i 40 / 2^20: 2.2e-16; float32 roundings that differ from
//                libm's: 0 of 3145731.
//   order        descending L, ties by ascending row (ohem_key: a non-finite L ranks before every finite one, ties again by row, so a
//                diverging run shows up in the step's loss and is not filtered away)
//   NMS          greedy over that order on the RoI boxes, the float32 IoU of softnms_iou (== iou_suppresses, "+1" areas): rule CPU
//                ov >= thresh_to_f32(thresh), rule GPU ov > (float)thresh.  thresh <= 0 skips the stage; thresh > 1 is refused.
//   selection    P = the kept candidates in order, then the suppressed ones in order (m rows in all); selected row i = P[i mod m],
//                i = 0 ... B-1 (fewer than B kept: suppressed rows follow in loss order; fewer than B candidates: they repeat)
//   output       the selected foreground rows first, then the background rows, each in selection order; keep_inds[B] = their rows;
//                counts = {fg selected, bg selected, fg candidates, bg candidates}; roi_loss[N] = L of every candidate, 0 elsewhere.
//   m = 0        what frcnn_proposal_target_layer_dn does when there is neither foreground nor background (the reference stops in
//                pdb there): counts {0, 0, 0, 0}, every output row zero, and keep_inds -1.
//
// The greedy pass may stop once B rows are kept: later rows cannot be selected.  Host and device both do.
#pragma once
#include "softnms_math.h"

#define OHEM_HD SOFTNMS_HD
#define OHEM_MAXN 3072                          // PT_MAXN of csrc/train_kernels.hip: rows of the proposal buffer, and of the batch
#define OHEM_MAXG 32767

OHEM_HD float ohem_nan() { return softnms_bits_f32(0x7fc00000u); }
OHEM_HD bool ohem_finite(double v) { return v - v == 0.0; }

// log(x) for a finite x > 0 that is a normal double: x = 2^e m with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(f), f = (m - 1) / (m + 1),
// |f| <= 0.1716: the odd series to f^23 by Horner in f^2 (the first dropped term is below 3e-21), e ln2 with ln2 split as in softnms_exp_neg.
OHEM_HD double ohem_log(double x) {
  if (!(x > 0.0) || !ohem_finite(x)) return (double)ohem_nan();
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  long long e = (long long)((b >> 52) & 0x7ff) - 1023;
  b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double m;
  __builtin_memcpy(&m, &b, 8);
  if (m > 1.41421356237309504880) m = m * 0.5, e += 1;
  const double f = (m - 1.0) / (m + 1.0), s = f * f;
  double p = 1.0 / 23.0;
  p = p * s + 1.0 / 21.0;
  p = p * s + 1.0 / 19.0;
  p = p * s + 1.0 / 17.0;
  p = p * s + 1.0 / 15.0;
  p = p * s + 1.0 / 13.0;
  p = p * s + 1.0 / 11.0;
  p = p * s + 1.0 / 9.0;
  p = p * s + 1.0 / 7.0;
  p = p * s + 1.0 / 5.0;
  p = p * s + 1.0 / 3.0;
  p = p * s + 1.0;
  const double ed = (double)e;
  return ed * 6.93147180369123816490e-01 + (ed * 1.90821492927058770002e-10 + 2.0 * f * p);
}

// utils/bbox.pyx:28-54 for one (box, query box) pair, float64
OHEM_HD double ohem_iou_f64(double b0, double b1, double b2, double b3, const float* q) {
  const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  const double box_area = (q2 - q0 + 1) * (q3 - q1 + 1);
  const double iw = (b2 < q2 ? b2 : q2) - (b0 > q0 ? b0 : q0) + 1;
  if (iw > 0) {
    const double ih = (b3 < q3 ? b3 : q3) - (b1 > q1 ? b1 : q1) + 1;
    if (ih > 0) {
      const double ua = (b2 - b0 + 1) * (b3 - b1 + 1) + box_area - iw * ih;
      return iw * ih / ua;
    }
  }
  return 0.0;
}

// box = x1,y1,x2,y2; gt [G,5].  -> 1 foreground, 0 background, -1 neither; *assigned = the first arg-max gt box
OHEM_HD int ohem_classify(const float* box, const float* gt, int G, double fg_thresh, double bg_hi, double bg_lo, int* assigned) {
  double best = -1.0;
  int bi = 0;
  for (int g = 0; g < G; ++g) {
    const double o = ohem_iou_f64(box[0], box[1], box[2], box[3], gt + 5 * (size_t)g);
    if (o > best) best = o, bi = g;
  }
  *assigned = bi;
  if (best >= fg_thresh) return 1;
  return (best < bg_hi && best >= bg_lo) ? 0 : -1;
}

OHEM_HD void ohem_encode(const float* ex, const float* gt, float* t) {
  const float ew = (ex[2] - ex[0]) + 1.0f, eh = (ex[3] - ex[1]) + 1.0f;
  const float ecx = ex[0] + 0.5f * ew, ecy = ex[1] + 0.5f * eh;
  const float gw = (gt[2] - gt[0]) + 1.0f, gh = (gt[3] - gt[1]) + 1.0f;
  const float gcx = gt[0] + 0.5f * gw, gcy = gt[1] + 0.5f * gh;
  t[0] = (gcx - ecx) / ew, t[1] = (gcy - ecy) / eh;
  t[2] = (float)ohem_log((double)(gw / ew)), t[3] = (float)ohem_log((double)(gh / eh));
}
OHEM_HD float ohem_normalise(float t, double mean, double std) { return (float)(((double)t - mean) / std); }

// cls [C] logits, pred [4C]; tgt [4] the normalised targets of the label's four columns, in_w [4].  label 0 = background.
OHEM_HD float ohem_row_loss(const float* cls, const float* pred, int C, int label, const float* tgt, const float* in_w) {
  if (label < 0 || label >= C) return ohem_nan();
  bool ok = true;
  int am = 0;
  for (int c = 0; c < C; ++c) {
    ok = ok && ohem_finite((double)cls[c]);
    if (cls[c] > cls[am]) am = c;
  }
  if (!ok) return ohem_nan();
  const double mx = (double)cls[am];
  double s = 0.0;
  for (int c = 0; c < C; ++c) s = s + softnms_exp_neg((double)cls[c] - mx);
  double L = ohem_log(s) + mx - (double)cls[label];
  if (label > 0) {
    double box = 0.0;
    for (int q = 0; q < 4; ++q) {
      const double d = (double)in_w[q] * ((double)pred[4 * label + q] - (double)tgt[q]);
      const double ad = d < 0.0 ? -d : d;
      const double f = ad < 1.0 ? 0.5 * (d * d) : ad - 0.5;
      box = box + (in_w[q] > 0.0f ? 1.0 : 0.0) * f;
    }
    L = L + box;
  }
  return ohem_finite(L) ? (float)L : ohem_nan();
}

// (L descending, row ascending) <=> key descending; a non-finite L before every finite one; never 0
OHEM_HD uint64_t ohem_key(float L, uint32_t r) {
  const uint32_t hi = ohem_finite((double)L) ? softnms_sortable(L) : 0xffffffffu;
  return ((uint64_t)hi << 32) | (uint64_t)(0xffffffffu - r);
}
OHEM_HD uint32_t ohem_key_row(uint64_t key) { return 0xffffffffu - (uint32_t)(key & 0xffffffffu); }

// a = a kept RoI box, b = a later one
OHEM_HD bool ohem_suppresses(const float* a, const float* b, float thr, int rule) {
  const float ov = softnms_iou(a[0], a[1], a[2], a[3], softnms_area(a[0], a[1], a[2], a[3]), b[0], b[1], b[2], b[3],
                               softnms_area(b[0], b[1], b[2], b[3]));
  return rule == SOFTNMS_RULE_CPU ? ov >= thr : ov > thr;
}

inline bool ohem_args_ok(int N, int G, int C, int B, double nms_thresh, int rule) {
  return N > 0 && G > 0 && C >= 2 && B > 0 && nms_thresh == nms_thresh && !(nms_thresh > 1.0) &&
         (rule == SOFTNMS_RULE_CPU || rule == SOFTNMS_RULE_GPU);
}

// What one row of the proposal buffer is to the selection: its key (0 = no candidate), loss, kind and gt box.
struct OhemRow {
  uint64_t key;
  float loss;
  short kind, assigned;
};
struct OhemNorm { double mean[4], std[4]; float inside[4]; };

// row r (< n) of rois [N,5] with its cls [C] / pred [4C] rows
OHEM_HD OhemRow ohem_score_row(const float* roi, uint32_t r, const float* gt, int G, int C, const float* cls, const float* pred,
                               double fg_thresh, double bg_hi, double bg_lo, const OhemNorm& nm) {
  OhemRow o;
  int assigned = 0;
  const int kind = ohem_classify(roi + 1, gt, G, fg_thresh, bg_hi, bg_lo, &assigned);
  o.kind = (short)kind, o.assigned = (short)assigned, o.key = 0, o.loss = 0.0f;
  if (kind < 0) return o;
  float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int label = 0;
  if (kind == 1) {
    const float* g = gt + 5 * (size_t)assigned;
    label = g[4] >= 0.0f && g[4] < (float)C ? (int)g[4] : -1;
    ohem_encode(roi + 1, g, t);
    for (int q = 0; q < 4; ++q) t[q] = ohem_normalise(t[q], nm.mean[q], nm.std[q]);
  }
  o.loss = ohem_row_loss(cls, pred, C, label, t, nm.inside);
  o.key = ohem_key(o.loss, r);
  return o;
}

// One output row s of the target layer's seven outputs: src = the selected proposal row (-1: a zero row), rw its OhemRow.
OHEM_HD void ohem_emit_row(int s, int src, const OhemRow* rw, const float* rois, const float* scores, const float* gt, int C,
                           const OhemNorm& nm, float* out_rois, float* out_scores, float* out_labels, float* out_targets,
                           float* out_inside, float* out_outside) {
  float* orow = out_rois + 5 * (size_t)s;
  float* trow = out_targets + (size_t)s * 4 * C;
  float* irow = out_inside + (size_t)s * 4 * C;
  float* urow = out_outside + (size_t)s * 4 * C;
  for (int c = 0; c < 4 * C; ++c) trow[c] = 0.0f, irow[c] = 0.0f, urow[c] = 0.0f;
  if (src < 0) {
    orow[0] = orow[1] = orow[2] = orow[3] = orow[4] = 0.0f, out_scores[s] = 0.0f, out_labels[s] = 0.0f;
    return;
  }
  const float* roi = rois + 5 * (size_t)src;
  for (int q = 0; q < 5; ++q) orow[q] = roi[q];
  out_scores[s] = scores[src];
  const float* g = gt + 5 * (size_t)rw[src].assigned;
  const float label = rw[src].kind == 1 ? g[4] : 0.0f;
  out_labels[s] = label;
  if (label > 0.0f && label < (float)C) {
    float t[4];
    ohem_encode(roi + 1, g, t);
    const int c4 = 4 * (int)label;
    for (int q = 0; q < 4; ++q) {
      trow[c4 + q] = ohem_normalise(t[q], nm.mean[q], nm.std[q]);
      irow[c4 + q] = nm.inside[q];
      urow[c4 + q] = nm.inside[q] > 0.0f ? 1.0f : 0.0f;
    }
  }
}

// The order, the greedy pass and the selection on the host.  rw [N] (rows >= n have key 0); order / P [N] scratch, kept [N] scratch.
// -> keep_inds [B] (fg rows first), counts [4].
inline void ohem_select_rows(const OhemRow* rw, const float* rois, int N, int B, float thr, bool nms, int rule, int* order, int* P,
                             unsigned char* kept, int* keep_inds, int* counts) {
  int m = 0, nfg = 0, nbg = 0;
  for (int i = 0; i < N; ++i) {
    if (rw[i].key == 0) continue;
    ++m, nfg += rw[i].kind == 1, nbg += rw[i].kind == 0;
  }
  for (int i = 0; i < N; ++i) {
    if (rw[i].key == 0) continue;
    int rank = 0;
    for (int j = 0; j < N; ++j) rank += rw[j].key > rw[i].key;
    order[rank] = i;
  }
  int nkept = 0;
  for (int p = 0; p < m; ++p) kept[p] = 0;
  for (int p = 0; p < m && nkept < B; ++p) {
    bool sup = false;
    for (int q = 0; q < p && nms && !sup; ++q)
      sup = kept[q] && ohem_suppresses(rois + 5 * (size_t)order[q] + 1, rois + 5 * (size_t)order[p] + 1, thr, rule);
    kept[p] = !sup, nkept += !sup;
  }
  int k = 0;
  for (int p = 0; p < m; ++p)
    if (kept[p]) P[k++] = order[p];
  for (int p = 0; p < m; ++p)
    if (!kept[p]) P[k++] = order[p];
  int sel_fg = 0, w = 0;
  for (int i = 0; i < B && m > 0; ++i) sel_fg += rw[P[i % m]].kind == 1;
  for (int i = 0; i < B; ++i) keep_inds[i] = -1;
  for (int pass = 1; pass >= 0 && m > 0; --pass)
    for (int i = 0; i < B; ++i)
      if ((int)rw[P[i % m]].kind == pass) keep_inds[w++] = P[i % m];
  counts[0] = sel_fg, counts[1] = m > 0 ? B - sel_fg : 0, counts[2] = nfg, counts[3] = nbg;
}
