"""Second statements of RoIAlign (tf-faster-rcnn_amd/csrc/roialign_math.h), numpy and torch only.

  align_f32        float32, the header's operation order: expected to equal frcnn_roi_align_host bit for bit
  align_f64        the same float32 sample coordinates, everything after them (weights, products, sums, the mean) in float64
  roi_align_torch  differentiable in `feat` like oracle/dense_ref.py:crop_and_resize_torch (NCHW in, [R,C,P,P] out): float64 autograd
  AlignTrainRef    oracle/dense_ref.py:TrainRef with the RoI pooling replaced (ResNet tail)
  weight_sum       the closed form of sum(backward(ones)): the sum of all tap weights / S^2, in float64

Rule: scale = 1/stride; start = x1*scale, end = x2*scale; extent = max(end - start, 1); bin = extent / P;
coordinate of sample i of bin p = (start + p*bin) + ((i + 0.5)*bin) / S; outside [-1, n]: the sample is zero; else v = max(v, 0),
low = (int)v; low >= n-1: low = high = n-1 and v = low; else high = low+1; l = v - low, h = 1 - l;
sample = ((hy*hx*v1 + hy*lx*v2) + ly*hx*v3) + ly*lx*v4; out = (sum of the S*S samples in (iy, ix) order) / (S*S)."""
import os
import sys

import numpy as np

f32 = np.float32

# the edge inputs of tests/test_roi_align_*.py: a 5 x 6 map at stride 16 (two images)
EDGE_H, EDGE_W, EDGE_STRIDE = 5, 6, 16.0
EDGE_ROIS = np.array([[0, 8, 8, 70, 60],            # interior only
                      [0, -40, -40, 30, 30],        # zeroed + clamped-low samples
                      [0, 60, 50, 140, 120],        # zeroed + clamped-high samples + samples on integer coordinates
                      [0, 50, 50, 40, 40],          # degenerate: widened to 1
                      [0, 0, 0, 95, 79],            # the whole map
                      [1, 16, 16, 48, 48]],         # the second image
                     dtype=np.float32)
# (zeroed, clamped-low, clamped-high, integer-coordinate) samples of each edge RoI at P = 7, S = 2
EDGE_KINDS_7_2 = [(0, 0, 0, None), (115, 45, 0, None), (160, 0, 27, 6), (0, 0, 28, None), (0, 0, 64, None), (0, 0, 0, None)]


def axis_taps(start, extent_end, scale, n, P, S):
    """float32 coordinates of the P*S samples of one axis for every RoI -> dict(v, valid, lo, hi) with v the clamped coordinate."""
    s = start.astype(f32) * f32(scale)
    e = extent_end.astype(f32) * f32(scale)
    ext = e - s
    ext = np.where(ext >= f32(1), ext, f32(1)).astype(f32)
    bin_ = ext / f32(P)
    p = np.repeat(np.arange(P), S).astype(f32)[None, :]
    i = np.tile(np.arange(S), P).astype(f32)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        v = (s[:, None] + p * bin_[:, None]) + ((i + f32(0.5)) * bin_[:, None]) / f32(S)
        assert v.dtype == np.float32
        valid = (v >= f32(-1)) & (v <= f32(n))
    v = np.where(valid, v, f32(0))
    v = np.where(v < 0, f32(0), v).astype(f32)
    lo = v.astype(np.int64)
    high = lo >= n - 1
    lo = np.where(high, n - 1, lo)
    hi = np.where(high, n - 1, lo + 1)
    v = np.where(high, lo.astype(f32), v).astype(f32)
    return dict(v=v, valid=valid, lo=lo, hi=hi)


def _taps(rois, stride, H, W, P, S):
    r = np.asarray(rois, dtype=np.float32).reshape(-1, 5)
    scale = f32(1) / f32(stride)
    return r, axis_taps(r[:, 2], r[:, 4], scale, H, P, S), axis_taps(r[:, 1], r[:, 3], scale, W, P, S)


def _image_index(r, N):
    with np.errstate(invalid="ignore"):
        ok = (r[:, 0] > -1) & (r[:, 0] < N)
    return np.where(ok, np.where(ok, r[:, 0], 0).astype(np.int64), -1)


def _align(feat, rois, stride, P, S, dt):
    feat = np.asarray(feat, dtype=np.float32)
    if feat.ndim == 3:
        feat = feat[None]
    N, H, W, C = feat.shape
    r, ty, tx = _taps(rois, stride, H, W, P, S)
    img = _image_index(r, N)
    R = r.shape[0]
    out = np.zeros((R, P, P, C), dtype=dt)
    one = dt(1)
    for k in range(R):
        if img[k] < 0:
            continue
        f = feat[img[k]].astype(dt)
        ly = ty["v"][k].astype(dt) - ty["lo"][k].astype(dt)
        lx = tx["v"][k].astype(dt) - tx["lo"][k].astype(dt)
        hy, hx = one - ly, one - lx
        acc = np.zeros((P, P, C), dtype=dt)
        for iy in range(S):
            a = np.arange(P) * S + iy
            for ix in range(S):
                b = np.arange(P) * S + ix
                yl, yh, xl, xh = ty["lo"][k][a][:, None], ty["hi"][k][a][:, None], tx["lo"][k][b][None, :], tx["hi"][k][b][None, :]
                wy_h, wy_l = hy[a][:, None, None], ly[a][:, None, None]
                wx_h, wx_l = hx[b][None, :, None], lx[b][None, :, None]
                smp = (((wy_h * wx_h) * f[yl, xl] + (wy_h * wx_l) * f[yl, xh]) + (wy_l * wx_h) * f[yh, xl]) + (wy_l * wx_l) * f[yh, xh]
                ok = (ty["valid"][k][a][:, None] & tx["valid"][k][b][None, :])[:, :, None]
                acc = np.where(ok, acc + smp, acc)
        assert acc.dtype == dt
        out[k] = acc / dt(S * S)
    return out


def align_f32(feat, rois, stride, P, S):
    return _align(feat, rois, stride, P, S, np.float32)


def align_f64(feat, rois, stride, P, S):
    return _align(feat, rois, stride, P, S, np.float64)


def tap_magnitude(feat, rois, stride, P, S):
    """[R,P,P,C] float64: sum over an output's samples of sum over taps of weight * |tap value|, / S^2 -- what the rounding errors of
    the float32 statement scale with."""
    return align_f64(np.abs(np.asarray(feat, dtype=np.float32)), rois, stride, P, S)


def weight_sum(rois, stride, H, W, P, S):
    """float64 sum over all valid samples of the four tap weights, / S^2 (each valid sample's weights sum to (hy+ly)*(hx+lx))."""
    r, ty, tx = _taps(rois, stride, H, W, P, S)
    total = 0.0
    for k in range(r.shape[0]):
        ly = ty["v"][k].astype(np.float64) - ty["lo"][k]
        lx = tx["v"][k].astype(np.float64) - tx["lo"][k]
        wy = np.where(ty["valid"][k], (1.0 - ly) + ly, 0.0)
        wx = np.where(tx["valid"][k], (1.0 - lx) + lx, 0.0)
        total += float(wy.sum() * wx.sum())
    return total / float(S * S)


def valid_samples(rois, stride, H, W, P, S):
    """int [R,P,P]: how many of a bin's S*S samples are not zeroed."""
    r, ty, tx = _taps(rois, stride, H, W, P, S)
    vy = ty["valid"].reshape(-1, P, S).sum(axis=2)
    vx = tx["valid"].reshape(-1, P, S).sum(axis=2)
    return vy[:, :, None] * vx[:, None, :]


def roi_align_torch(feat, rois, stride, P, S):
    """feat [N,C,H,W] (torch, any float dtype, may require grad); rois [R,5] -> [R,C,P,P].  Sample coordinates in float32 exactly as
    the header takes them, weights and sums in feat's dtype; taps by gather, so autograd gives the gradient w.r.t. feat."""
    import torch
    N, C, H, W = feat.shape
    r, ty, tx = _taps(rois, stride, H, W, P, S)
    img = _image_index(r, N)
    R = r.shape[0]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ly = tt(ty["v"].astype(np.float64) - ty["lo"]).to(feat.dtype)[:, :, None, None]           # [R,PS,1,1]
    lx = tt(tx["v"].astype(np.float64) - tx["lo"]).to(feat.dtype)[:, None, :, None]           # [R,1,PS,1]
    hy, hx = 1.0 - ly, 1.0 - lx
    f = feat.permute(0, 2, 3, 1)                                                              # [N,H,W,C]
    n = tt(np.maximum(img, 0))[:, None, None]
    yl, yh = tt(ty["lo"])[:, :, None], tt(ty["hi"])[:, :, None]
    xl, xh = tt(tx["lo"])[:, None, :], tt(tx["hi"])[:, None, :]
    smp = hy * hx * f[n, yl, xl] + hy * lx * f[n, yl, xh] + ly * hx * f[n, yh, xl] + ly * lx * f[n, yh, xh]       # [R,PS,PS,C]
    ok = ty["valid"][:, :, None] & tx["valid"][:, None, :] & (img >= 0)[:, None, None]
    smp = smp * tt(ok.astype(np.float64)).to(feat.dtype)[..., None]
    out = smp.reshape(R, P, S, P, S, C).sum(dim=(2, 4)) / float(S * S)
    return out.permute(0, 3, 1, 2)


def align_train_ref():
    """-> the TrainRef subclass whose train_tail pools with roi_align_torch (needs oracle/ on sys.path)."""
    here = os.path.dirname(os.path.abspath(__file__))
    ora = os.path.join(os.path.dirname(here), "oracle")
    if ora not in sys.path:
        sys.path.insert(0, ora)
    from dense_ref import TrainRef

    class AlignTrainRef(TrainRef):
        samples = 2

        def train_tail(self, feat, rois):
            pool5 = roi_align_torch(feat, rois, 16.0, 7, self.samples)
            return self.run_blocks(pool5, self.blocks[3:]).mean(dim=(2, 3))

    return AlignTrainRef
