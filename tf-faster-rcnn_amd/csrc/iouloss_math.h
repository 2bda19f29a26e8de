// IoU-family box regression losses on the DECODED boxes -- IoU, GIoU (Rezatofighi et al., CVPR 2019), DIoU and CIoU (Zheng et al., AAAI
// 2020) -- as plain host + device C++.  csrc/iou_loss.hip (the kernels and the host entry frcnn_iou_loss_host) and the stand-alone
// harness csrc/iou_loss_host_check.cc include this one statement.
//
//   slice        four consecutive columns 4k .. 4k+3 of row r of pred, targets, inside_w and outside_w, all [N, 4K]; slice s = r K + k
//                starts at element 4 s.  RCNN head: N = rows of the RoI minibatch, K = num_classes.  RPN: the [1,H,W,4A] tensors read as
//                [H W A, 4], K = 1, row (h W + w) A + a = anchor a at (h, w).
//   active       a slice is active iff any of its four inside weights is non-zero (a NaN is non-zero).  The inside weights are not read
//                otherwise: an IoU loss has no per-coordinate weight.  The slice's weight is ow = outside_w[r, 4k].
//   decode       d = pred * std + mean and d = targets * std + mean, through bbox_transform_inv on the row's reference box a (RoI columns
//                1..4 with ref_cols 5, the anchor with ref_cols 4):  w = a.x2 - a.x1 + 1, h likewise, cx = a.x1 + 0.5 w, cy likewise;
//                pcx = dx w + cx, pcy = dy h + cy, pw = E(min(dw, log(1000 / 16))) w, ph likewise -- a coordinate above the clamp has
//                gradient 0 --; box = (pcx - 0.5 pw, pcy - 0.5 ph, pcx + 0.5 pw, pcy + 0.5 ph).
//   loss         of the predicted box P against the target box T, plain areas (x2 - x1)(y2 - y1), eps = 1e-7, as torchvision's
//                *_box_iou_loss:  inter = iw ih where iw > 0 and ih > 0, else 0;  iou = inter / (union + eps)
//                  kind 1 iou    L = 1 - iou
//                  kind 2 giou   L = 1 - iou + (areaC - union) / (areaC + eps)             C = the enclosing box
//                  kind 3 diou   L = 1 - iou + rho2 / (c2 + eps)                           rho2 = squared centre distance, c2 = squared diagonal of C
//                  kind 4 ciou   L = diou's L + alpha v,  v = (4 / pi^2)(A(wT / hT) - A(wP / hP))^2,  alpha = v / (1 - iou + v + eps)
//                alpha is a CONSTANT in the gradient (the paper's and torchvision's convention).  Where a max or min of a coordinate of P
//                and one of T ties, the value is T's and P's coordinate gets no gradient through it.
//   result       loss = weight / mean_divisor * sum over the active slices of ow L;  dpred[slice] = weight / mean_divisor * ow * dL/dpred,
//                the chain through the decode including the factor std;  every element of an inactive slice gets +0.
//   non-finite   an active slice with a pred, target, outside weight or reference coordinate that is not finite has L = NaN and four NaN
//                gradients; no other slice's gradient changes.  An inactive slice's values are never read beyond the inside weights.
//   arithmetic   every active slice in double from the float32 inputs, the gradient rounded to float32 ONCE; the slice losses are summed in
//                double in a fixed order: per 64 slices the xor butterfly 32, 16 ... 1, the four waves of a block in order, then the blocks
//                in order (iouloss_host below adds in exactly that order), times weight / mean_divisor, rounded once.
//   E, A         iouloss_exp and iouloss_atan below: IEEE double + - * / and integer bit operations only, no exp() / atan() on either
//                side, so host and gfx950 return the same bits (every TU is built with -ffp-contract=off).  Against libm
//                (csrc/iou_loss_host_check.cc, x86-64 glibc): E over x = -12 + i 16.2 / 2^20, A over x = 2^(i / 2^16 - 8), i = 0 ... 2^20,
//                both signs: largest relative distance in double 2.2e-16 (E) and 2.8e-16 (A); the harness prints both and holds them below 1e-15.
#pragma once
#include "softnms_math.h"

#define IOULOSS_HD SOFTNMS_HD
#define IOULOSS_IOU 1
#define IOULOSS_GIOU 2
#define IOULOSS_DIOU 3
#define IOULOSS_CIOU 4
#define IOULOSS_EPS 1e-7
#define IOULOSS_CLIP 4.135166556742356          // log(1000 / 16), BBOX_XFORM_CLIP of Detectron / torchvision
#define IOULOSS_BLOCK 256                       // slices per block partial
#define IOULOSS_MAX_SLICES 0x7fffffffll

IOULOSS_HD float iouloss_nan() { return softnms_bits_f32(0x7fc00000u); }
IOULOSS_HD bool iouloss_finite(double v) { return v - v == 0.0; }
IOULOSS_HD float iouloss_f32(double v) { return v == v ? (float)v : iouloss_nan(); }      // the ONE rounding; every NaN leaves as 0x7fc00000

// exp(x) for a finite x: 0 below -700, +inf above 709; else x = k ln2 + r, k = round(x / ln2), |r| <= 0.35, the Taylor polynomial of
// degree 13 by Horner (softnms_exp_neg's, first dropped term below 4e-18), times 2^k built from its exponent bits (normal in this range).
IOULOSS_HD double iouloss_exp(double x) {
  if (x < -700.0) return 0.0;
  if (x > 709.0) return (double)softnms_bits_f32(0x7f800000u);
  const double t = x * 1.4426950408889634074;
  const long long k = t < 0.0 ? (long long)(t - 0.5) : (long long)(t + 0.5);
  const double kd = (double)k;
  const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const uint64_t bits = (uint64_t)(1023 + k) << 52;
  double s;
  __builtin_memcpy(&s, &bits, 8);
  return p * s;
}

// atan(x) for a finite x: odd; |x| > 1 -> pi/2 - atan(1 / |x|); t in [0, 1] is moved to u = (t - c) / (1 + t c) around c = 0, tan(pi/8)
// or 1 (atan c = 0, pi/8, pi/4), |u| <= tan(pi/16) = 0.1989; the odd series to u^27 by Horner in u^2 (the first dropped term is below 2e-22).
IOULOSS_HD double iouloss_atan(double x) {
  const bool neg = x < 0.0;
  double t = neg ? -x : x;
  const bool inv = t > 1.0;
  if (inv) t = 1.0 / t;
  double base = 0.0, u = t;
  if (t > 0.66817863791929891999) base = 0.78539816339744830962, u = (t - 1.0) / (1.0 + t);
  else if (t > 0.19891236737965800691) base = 0.39269908169872415481, u = (t - 0.41421356237309504880) / (1.0 + t * 0.41421356237309504880);
  const double s = u * u;
  double p = 1.0 / 27.0;
  p = 1.0 / 25.0 - p * s;
  p = 1.0 / 23.0 - p * s;
  p = 1.0 / 21.0 - p * s;
  p = 1.0 / 19.0 - p * s;
  p = 1.0 / 17.0 - p * s;
  p = 1.0 / 15.0 - p * s;
  p = 1.0 / 13.0 - p * s;
  p = 1.0 / 11.0 - p * s;
  p = 1.0 / 9.0 - p * s;
  p = 1.0 / 7.0 - p * s;
  p = 1.0 / 5.0 - p * s;
  p = 1.0 / 3.0 - p * s;
  p = 1.0 - p * s;
  double a = base + u * p;
  if (inv) a = 1.57079632679489661923 - a;
  return neg ? -a : a;
}

struct IouLossNorm { double mean[4], std[4]; };
struct IouLossBox { double x1, y1, x2, y2; bool clamp_w, clamp_h; double w, h; };      // w, h: the decoded width and height (pw, ph)

// bbox_transform_inv of one slice: a = the reference box x1,y1,x2,y2; v = the four raw values (pred or targets)
IOULOSS_HD IouLossBox iouloss_decode(const float* a, const float* v, const IouLossNorm& nm) {
  const double w = (double)a[2] - (double)a[0] + 1.0, h = (double)a[3] - (double)a[1] + 1.0;
  const double cx = (double)a[0] + 0.5 * w, cy = (double)a[1] + 0.5 * h;
  const double dx = (double)v[0] * nm.std[0] + nm.mean[0], dy = (double)v[1] * nm.std[1] + nm.mean[1];
  const double dw = (double)v[2] * nm.std[2] + nm.mean[2], dh = (double)v[3] * nm.std[3] + nm.mean[3];
  IouLossBox b;
  b.clamp_w = dw > IOULOSS_CLIP, b.clamp_h = dh > IOULOSS_CLIP;
  const double pcx = dx * w + cx, pcy = dy * h + cy;
  b.w = iouloss_exp(b.clamp_w ? IOULOSS_CLIP : dw) * w, b.h = iouloss_exp(b.clamp_h ? IOULOSS_CLIP : dh) * h;
  b.x1 = pcx - 0.5 * b.w, b.y1 = pcy - 0.5 * b.h, b.x2 = pcx + 0.5 * b.w, b.y2 = pcy + 0.5 * b.h;
  return b;
}

// One slice: a = its reference box, p / t / iw its four pred / targets / inside weights, ow its outside weight, scale = weight /
// mean_divisor.  -> ow L (0 for an inactive slice), g[4] = the float32 gradient of scale * ow * L.
IOULOSS_HD double iouloss_slice(const float* a, const float* p, const float* t, const float* iw, float ow, const IouLossNorm& nm, int kind,
                                double scale, float* g) {
  if (!(iw[0] != 0.0f || iw[1] != 0.0f || iw[2] != 0.0f || iw[3] != 0.0f)) {
    g[0] = g[1] = g[2] = g[3] = 0.0f;
    return 0.0;
  }
  bool ok = iouloss_finite((double)ow);
  for (int q = 0; q < 4; ++q) ok = ok && iouloss_finite((double)p[q]) && iouloss_finite((double)t[q]) && iouloss_finite((double)a[q]);
  if (!ok) {
    g[0] = g[1] = g[2] = g[3] = iouloss_nan();
    return (double)iouloss_nan();
  }
  const IouLossBox P = iouloss_decode(a, p, nm), T = iouloss_decode(a, t, nm);
  // intersection and union; gx1 ... gy2 collect dL / d(P's corners)
  const bool tx1 = P.x1 > T.x1, ty1 = P.y1 > T.y1, tx2 = P.x2 < T.x2, ty2 = P.y2 < T.y2;       // P's coordinate bounds the intersection
  const double ix1 = tx1 ? P.x1 : T.x1, iy1 = ty1 ? P.y1 : T.y1, ix2 = tx2 ? P.x2 : T.x2, iy2 = ty2 ? P.y2 : T.y2;
  const double iwd = ix2 - ix1, ihd = iy2 - iy1;
  const bool hit = iwd > 0.0 && ihd > 0.0;
  const double inter = hit ? iwd * ihd : 0.0;
  const double pw = P.x2 - P.x1, ph = P.y2 - P.y1;
  const double uni = pw * ph + (T.x2 - T.x1) * (T.y2 - T.y1) - inter;
  const double ue = uni + IOULOSS_EPS;
  const double iou = inter / ue;
  double L = 1.0 - iou;
  // d inter / d corner, d union / d corner = d areaP - d inter
  const double i_x1 = hit && tx1 ? -ihd : 0.0, i_y1 = hit && ty1 ? -iwd : 0.0, i_x2 = hit && tx2 ? ihd : 0.0, i_y2 = hit && ty2 ? iwd : 0.0;
  const double u_x1 = -ph - i_x1, u_y1 = -pw - i_y1, u_x2 = ph - i_x2, u_y2 = pw - i_y2;
  const double di = -1.0 / ue, du = inter / (ue * ue);                                            // dL / d inter, dL / d union so far
  double gx1 = di * i_x1 + du * u_x1, gy1 = di * i_y1 + du * u_y1, gx2 = di * i_x2 + du * u_x2, gy2 = di * i_y2 + du * u_y2;
  if (kind != IOULOSS_IOU) {
    const bool ex1 = P.x1 < T.x1, ey1 = P.y1 < T.y1, ex2 = P.x2 > T.x2, ey2 = P.y2 > T.y2;     // P's coordinate bounds the enclosing box
    const double cw = (ex2 ? P.x2 : T.x2) - (ex1 ? P.x1 : T.x1), ch = (ey2 ? P.y2 : T.y2) - (ey1 ? P.y1 : T.y1);
    if (kind == IOULOSS_GIOU) {
      const double ac = cw * ch, ae = ac + IOULOSS_EPS;
      L = L + (ac - uni) / ae;
      const double dc = ue / (ae * ae), dun = -1.0 / ae;                                        // d term / d areaC, d term / d union
      gx1 = gx1 + (dc * (ex1 ? -ch : 0.0) + dun * u_x1), gy1 = gy1 + (dc * (ey1 ? -cw : 0.0) + dun * u_y1);
      gx2 = gx2 + (dc * (ex2 ? ch : 0.0) + dun * u_x2), gy2 = gy2 + (dc * (ey2 ? cw : 0.0) + dun * u_y2);
    } else {
      const double c2 = cw * cw + ch * ch, ce = c2 + IOULOSS_EPS;
      const double ddx = (P.x1 + P.x2) * 0.5 - (T.x1 + T.x2) * 0.5, ddy = (P.y1 + P.y2) * 0.5 - (T.y1 + T.y2) * 0.5;
      const double rho2 = ddx * ddx + ddy * ddy;
      L = L + rho2 / ce;
      const double dr = 1.0 / ce, dc = -rho2 / (ce * ce);                                       // d term / d rho2, d term / d c2
      gx1 = gx1 + (dr * ddx + dc * (ex1 ? -2.0 * cw : 0.0)), gy1 = gy1 + (dr * ddy + dc * (ey1 ? -2.0 * ch : 0.0));
      gx2 = gx2 + (dr * ddx + dc * (ex2 ? 2.0 * cw : 0.0)), gy2 = gy2 + (dr * ddy + dc * (ey2 ? 2.0 * ch : 0.0));
      if (kind == IOULOSS_CIOU) {
        const double tw = T.x2 - T.x1, th = T.y2 - T.y1;
        const double da = iouloss_atan(tw / th) - iouloss_atan(pw / ph);
        const double v = 0.40528473456935108578 * (da * da);
        const double alpha = v / (1.0 - iou + v + IOULOSS_EPS);
        L = L + alpha * v;
        const double q = pw * pw + ph * ph;
        const double v_w = -0.81056946913870217155 * da * (ph / q), v_h = 0.81056946913870217155 * da * (pw / q);      // dv / d pw, dv / d ph
        gx1 = gx1 - alpha * v_w, gx2 = gx2 + alpha * v_w, gy1 = gy1 - alpha * v_h, gy2 = gy2 + alpha * v_h;
      }
    }
  }
  // corners -> centre and size -> the decoded deltas -> pred
  const double a_w = (double)a[2] - (double)a[0] + 1.0, a_h = (double)a[3] - (double)a[1] + 1.0;
  const double s = scale * (double)ow;
  g[0] = iouloss_f32(s * ((gx1 + gx2) * a_w * nm.std[0]));
  g[1] = iouloss_f32(s * ((gy1 + gy2) * a_h * nm.std[1]));
  g[2] = P.clamp_w ? 0.0f : iouloss_f32(s * (0.5 * (gx2 - gx1) * P.w * nm.std[2]));
  g[3] = P.clamp_h ? 0.0f : iouloss_f32(s * (0.5 * (gy2 - gy1) * P.h * nm.std[3]));
  return (double)ow * L;
}

inline bool iouloss_args_ok(long long N, int K, int ref_cols, const float* means, const float* stds, int kind, float weight, float mean_divisor) {
  if (N <= 0 || K <= 0 || (ref_cols != 4 && ref_cols != 5) || kind < IOULOSS_IOU || kind > IOULOSS_CIOU || !means || !stds) return false;
  for (int q = 0; q < 4; ++q)
    if (!(stds[q] > 0.0f) || !iouloss_finite((double)stds[q]) || !iouloss_finite((double)means[q])) return false;
  return mean_divisor > 0.0f && iouloss_finite((double)mean_divisor) && iouloss_finite((double)weight);
}
inline IouLossNorm iouloss_norm(const float* means, const float* stds) {
  IouLossNorm nm;
  for (int q = 0; q < 4; ++q) nm.mean[q] = (double)means[q], nm.std[q] = (double)stds[q];
  return nm;
}
IOULOSS_HD double iouloss_scale(float weight, float mean_divisor) { return (double)weight / (double)mean_divisor; }

// slice s of the [N, 4K] tensors with refs [N, ref_cols]
IOULOSS_HD double iouloss_at(long long s, int K, const float* pred, const float* tgt, const float* in_w, const float* out_w, const float* refs,
                             int ref_cols, const IouLossNorm& nm, int kind, double scale, float* dpred) {
  const long long r = s / K;
  const size_t e = 4 * (size_t)s;
  return iouloss_slice(refs + (size_t)r * ref_cols + (ref_cols == 5 ? 1 : 0), pred + e, tgt + e, in_w + e, out_w[e], nm, kind, scale, dpred + e);
}

// The whole op on the host in the device's order of additions.  Arguments as frcnn_iou_loss_host; the caller has checked them.
inline void iouloss_host(const float* pred, const float* tgt, const float* in_w, const float* out_w, long long N, int K, const float* refs,
                         int ref_cols, const float* means, const float* stds, int kind, float weight, float mean_divisor, float* loss,
                         float* dpred) {
  const IouLossNorm nm = iouloss_norm(means, stds);
  const double scale = iouloss_scale(weight, mean_divisor);
  const long long slices = N * K;
  double total = 0.0;
  for (long long b0 = 0; b0 < slices; b0 += IOULOSS_BLOCK) {
    double block = 0.0;
    for (int w0 = 0; w0 < IOULOSS_BLOCK; w0 += 64) {
      double v[64], n[64];
      for (int l = 0; l < 64; ++l) {
        const long long s = b0 + w0 + l;
        v[l] = s < slices ? iouloss_at(s, K, pred, tgt, in_w, out_w, refs, ref_cols, nm, kind, scale, dpred) : 0.0;
      }
      for (int o = 32; o; o >>= 1) {
        for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ o];
        for (int l = 0; l < 64; ++l) v[l] = n[l];
      }
      block = block + v[0];
    }
    total = total + block;
  }
  *loss = iouloss_f32(total * scale);
}
