"""TEST INFRASTRUCTURE ONLY -- the IoU-family box regression losses (frcnn_iou_loss / frcnn_iou_loss_host) as an independent float64
statement: the forward in numpy, the gradient by torch CPU float64 autograd over the same forward (one function, `forward`, written
against the few array operations numpy and torch share), NOT by the hand-derived formulas of csrc/iouloss_math.h.

The rule (csrc/iouloss_math.h has the full text): pred / targets / inside / outside are [N, 4K]; a slice is four consecutive columns; it
is active iff any inside weight is non-zero; its weight is outside[r, 4k].  d = v * std + mean (std, mean float32 values) is decoded on
the row's reference box as bbox_transform_inv does, widths clamped at log(1000 / 16) with gradient 0 above the clamp; plain areas,
eps 1e-7; alpha of CIoU is a constant in the gradient; where a max / min of a coordinate of P and one of T ties, T's is taken.
loss = weight / divisor * sum(ow * L).  An active slice with a non-finite pred, target, outside weight or reference coordinate has
L = NaN and four NaN gradients.

MUTANTS are deliberately wrong variants of the statement; tests/test_iou_loss_cpu.py shows that the cases tell each from the statement."""
import numpy as np
import torch

KINDS = ("iou", "giou", "diou", "ciou")
EPS = 1e-7
CLIP = float(np.log(1000.0 / 16.0))
MUTANTS = ("alpha_grad", "plus_one", "no_clamp", "no_std", "inside_w")


def _decode(xp, a, v, mean, std, mutant, inside, is_pred):
    detach = (lambda x: x.detach()) if xp is torch else (lambda x: x)
    if mutant == "inside_w" and is_pred:
        v = inside * v
    d = v * std + mean
    if mutant == "no_std":
        d = detach(d) + (v - detach(v))                      # the same value, the chain without std
    w, h = a[:, 2] - a[:, 0] + 1.0, a[:, 3] - a[:, 1] + 1.0
    cx, cy = a[:, 0] + 0.5 * w, a[:, 1] + 0.5 * h
    dw, dh = d[:, 2], d[:, 3]
    if mutant != "no_clamp":
        dw = xp.where(dw > CLIP, xp.zeros_like(dw) + CLIP, dw)
        dh = xp.where(dh > CLIP, xp.zeros_like(dh) + CLIP, dh)
    pcx, pcy, pw, ph = d[:, 0] * w + cx, d[:, 1] * h + cy, xp.exp(dw) * w, xp.exp(dh) * h
    return pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph


def forward(xp, a, p, t, inside, mean, std, kind, mutant=None, alpha=None, want_alpha=False):
    """Per-slice loss L [S] of S active, finite slices: a [S,4] reference boxes, p / t / inside [S,4], mean / std [4] (float64 arrays of xp).
    alpha: CIoU's alpha [S] held at given values (what a finite difference must do to see the gradient the convention defines);
    want_alpha: return CIoU's alpha instead of L."""
    detach = (lambda x: x.detach()) if xp is torch else (lambda x: x)
    one = 1.0 if mutant == "plus_one" else 0.0
    px1, py1, px2, py2 = _decode(xp, a, p, mean, std, mutant, inside, True)
    tx1, ty1, tx2, ty2 = _decode(xp, a, t, mean, std, mutant, inside, False)
    ix1, iy1 = xp.where(px1 > tx1, px1, tx1), xp.where(py1 > ty1, py1, ty1)
    ix2, iy2 = xp.where(px2 < tx2, px2, tx2), xp.where(py2 < ty2, py2, ty2)
    iw, ih = ix2 - ix1 + one, iy2 - iy1 + one
    inter = xp.where((iw > 0) & (ih > 0), iw * ih, xp.zeros_like(iw))
    union = (px2 - px1 + one) * (py2 - py1 + one) + (tx2 - tx1 + one) * (ty2 - ty1 + one) - inter
    iou = inter / (union + EPS)
    L = 1.0 - iou
    if kind == "iou":
        return L
    cx1, cy1 = xp.where(px1 < tx1, px1, tx1), xp.where(py1 < ty1, py1, ty1)
    cx2, cy2 = xp.where(px2 > tx2, px2, tx2), xp.where(py2 > ty2, py2, ty2)
    if kind == "giou":
        area_c = (cx2 - cx1 + one) * (cy2 - cy1 + one)
        return L + (area_c - union) / (area_c + EPS)
    diag = (cx2 - cx1) ** 2 + (cy2 - cy1) ** 2
    rho = ((px1 + px2) / 2 - (tx1 + tx2) / 2) ** 2 + ((py1 + py2) / 2 - (ty1 + ty2) / 2) ** 2
    L = L + rho / (diag + EPS)
    if kind == "diou":
        return L
    v = (4.0 / np.pi ** 2) * (xp.arctan((tx2 - tx1) / (ty2 - ty1)) - xp.arctan((px2 - px1) / (py2 - py1))) ** 2
    alpha = v / (1.0 - iou + v + EPS) if alpha is None else alpha
    if want_alpha:
        return alpha
    if mutant != "alpha_grad":
        alpha = detach(alpha)
    return L + alpha * v


def _slices(pred, targets, inside, outside, refs, K):
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    p, t, iw, ow = (f64(x).reshape(-1, 4) for x in (pred, targets, inside, outside))
    refs = f64(refs)
    a = np.repeat(refs[:, -4:], K, axis=0)
    assert a.shape[0] == p.shape[0], "refs must have one row per row of pred"
    active = (iw != 0).any(axis=1)
    finite = np.isfinite(p).all(1) & np.isfinite(t).all(1) & np.isfinite(ow[:, 0]) & np.isfinite(a).all(1)
    return p, t, iw, ow[:, 0], a, active, finite


def loss_and_grad(pred, targets, inside, outside, refs, means, stds, kind, weight, divisor, K, mutant=None):
    """-> dict(loss float64, grad float64 like pred, slice_loss [N K] (0 inactive, NaN non-finite), active [N K] bool)"""
    p, t, iw, ow, a, active, finite = _slices(pred, targets, inside, outside, refs, K)
    mean, std = np.asarray(means, np.float32).astype(np.float64), np.asarray(stds, np.float32).astype(np.float64)
    scale = float(np.float32(weight)) / float(np.float32(divisor))
    sel = np.where(active & finite)[0]
    bad = np.where(active & ~finite)[0]
    L = np.zeros(p.shape[0])
    grad = np.zeros(p.shape)
    if sel.size:
        L[sel] = forward(np, a[sel], p[sel], t[sel], iw[sel], mean, std, kind, mutant)
        tt = lambda x: torch.from_numpy(np.ascontiguousarray(x))
        leaf = tt(p[sel]).requires_grad_(True)
        Lt = forward(torch, tt(a[sel]), leaf, tt(t[sel]), tt(iw[sel]), tt(mean), tt(std), kind, mutant)
        assert np.array_equal(Lt.detach().numpy(), L[sel]) or np.allclose(Lt.detach().numpy(), L[sel], rtol=1e-13, atol=1e-15)
        (scale * (tt(ow[sel]) * Lt).sum()).backward()
        grad[sel] = leaf.grad.numpy()
    L[bad], grad[bad] = np.nan, np.nan
    loss = scale * float(np.sum(ow[active] * L[active])) if active.any() else 0.0
    return dict(loss=np.float64(loss), grad=grad.reshape(np.asarray(pred).shape), slice_loss=L, active=active)


def loss_only(pred, targets, inside, outside, refs, means, stds, kind, weight, divisor, K, alpha_at=None):
    """The numpy forward alone on float64 inputs (no float32 conversion of pred): what the finite-difference witness differentiates.
    alpha_at: the pred at which CIoU's alpha is taken and held (the convention: alpha is a constant in the gradient)."""
    p, t, iw, ow, a, active, finite = _slices(pred, targets, inside, outside, refs, K)
    mean, std = np.asarray(means, np.float32).astype(np.float64), np.asarray(stds, np.float32).astype(np.float64)
    sel = np.where(active & finite)[0]
    alpha = None
    if kind == "ciou" and alpha_at is not None:
        p0 = np.asarray(alpha_at, dtype=np.float64).reshape(-1, 4)
        alpha = forward(np, a[sel], p0[sel], t[sel], iw[sel], mean, std, kind, want_alpha=True)
    L = forward(np, a[sel], p[sel], t[sel], iw[sel], mean, std, kind, alpha=alpha)
    return float(np.float32(weight)) / float(np.float32(divisor)) * float(np.sum(ow[sel] * L))


def ulps(got, want):
    """float32 ulp distance, elementwise, between float32 `got` and float64 `want` rounded to float32: 0 for equal values (-0 == +0) and
    for two NaNs, a huge number where only one is NaN."""
    g, w = np.asarray(got, dtype=np.float32).ravel(), np.asarray(want, dtype=np.float64).astype(np.float32).ravel()

    def key(x):
        b = x.view(np.int32).astype(np.int64)
        return np.where(b < 0, -(b & 0x7fffffff), b)
    d = np.abs(key(g) - key(w))
    gn, wn = np.isnan(g), np.isnan(w)
    d = np.where(gn & wn, 0, d)
    return np.where(gn ^ wn, np.int64(1) << 40, d)
