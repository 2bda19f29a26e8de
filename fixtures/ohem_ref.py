"""TEST INFRASTRUCTURE ONLY -- online hard example mining as a numpy float64 statement, written independently of csrc/ohem_math.h:
libm's exp / log, a plain argsort and a loop.  select() returns what frcnn_ohem_select[_host] must return, plus the margins the
fixture generator asserts (fixtures/gen_golden_ohem.py)."""
import numpy as np

f32, f64 = np.float32, np.float64


def overlaps_f64(boxes, query):
    """utils/bbox.pyx:28-54 -> [n, k] float64 (boxes, query: x1,y1,x2,y2)"""
    b, q = boxes.astype(f64), query.astype(f64)
    out = np.zeros((b.shape[0], q.shape[0]), dtype=f64)
    for k in range(q.shape[0]):
        area = (q[k, 2] - q[k, 0] + 1) * (q[k, 3] - q[k, 1] + 1)
        iw = np.minimum(b[:, 2], q[k, 2]) - np.maximum(b[:, 0], q[k, 0]) + 1
        ih = np.minimum(b[:, 3], q[k, 3]) - np.maximum(b[:, 1], q[k, 1]) + 1
        ua = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1) + area - iw * ih
        ok = (iw > 0) & (ih > 0)
        out[ok, k] = (iw * ih)[ok] / ua[ok]
    return out


def targets_f32(ex, gt, means, stds):
    """model/bbox_transform.py:14-32 on float32 rows with a correctly rounded logarithm, then (t - means) / stds in float64 (proposal_target_layer.py:83-96) -> float32"""
    ex, gt = ex.astype(f32), gt.astype(f32)
    ew, eh = ex[:, 2] - ex[:, 0] + f32(1), ex[:, 3] - ex[:, 1] + f32(1)
    ecx, ecy = ex[:, 0] + f32(0.5) * ew, ex[:, 1] + f32(0.5) * eh
    gw, gh = gt[:, 2] - gt[:, 0] + f32(1), gt[:, 3] - gt[:, 1] + f32(1)
    gcx, gcy = gt[:, 0] + f32(0.5) * gw, gt[:, 1] + f32(0.5) * gh
    # (the logarithm in float64, rounded once: numpy's float32 log is a SIMD routine good to a few ulps whose bits depend on the CPU)
    t = np.stack([(gcx - ecx) / ew, (gcy - ecy) / eh, np.log((gw / ew).astype(f64)).astype(f32), np.log((gh / eh).astype(f64)).astype(f32)], axis=1)
    return ((t.astype(f64) - np.asarray(means, f64)) / np.asarray(stds, f64)).astype(f32)


def row_loss(cls, pred, label, tgt, in_w):
    """cross entropy + [label > 0] SmoothL1 (sigma 1) of one row, float64 with libm"""
    z = cls.astype(f64)
    if not np.all(np.isfinite(z)):
        return np.nan
    mx = z.max()
    L = np.log(np.sum(np.exp(z - mx))) + mx - z[label]
    if label > 0:
        d = np.asarray(in_w, f64) * (pred[4 * label:4 * label + 4].astype(f64) - tgt.astype(f64))
        ad = np.abs(d)
        L = L + np.sum((np.asarray(in_w) > 0) * np.where(ad < 1.0, 0.5 * d * d, ad - 0.5))
    return L if np.isfinite(L) else np.nan


def nms_iou_f64(a, b):
    """the "+1" IoU of lib/nms/cpu_nms.pyx on two boxes, in float64"""
    a, b = a.astype(f64), b.astype(f64)
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1)
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    inter = w * h
    return inter / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter)


def select(rois, scores, n, gt, C, cls, pred, B, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.1, means=(0, 0, 0, 0), stds=(0.1, 0.1, 0.2, 0.2),
           inside=(1, 1, 1, 1), nms_thresh=0.7, rule=0):
    """-> dict: rois [B,5], scores [B], labels [B,1], targets / inside / outside [B,4C], counts [4], keep_inds [B], roi_loss [N] (float64;
    NaN = a non-finite loss) and the margins: loss_gap (smallest relative gap between two DISTINCT candidate losses), label_gap (smallest
    |max IoU - threshold| over the valid rows), nms_gap (smallest |IoU - nms_thresh| the greedy pass met)."""
    N = rois.shape[0]
    L = np.zeros(N, dtype=f64)
    kind = np.full(N, -1)
    assign = np.zeros(N, dtype=np.int64)
    label_gap = np.inf
    if n:
        ov = overlaps_f64(rois[:n, 1:5], gt[:, :4])
        assign[:n] = ov.argmax(axis=1)
        mx = ov.max(axis=1)
        kind[:n] = np.where(mx >= fg_thresh, 1, np.where((mx < bg_hi) & (mx >= bg_lo), 0, -1))
        label_gap = min(np.abs(mx - t).min() for t in (fg_thresh, bg_hi, bg_lo))
    tg = targets_f32(rois[:, 1:5], gt[assign, :4], means, stds)
    cand = [r for r in range(n) if kind[r] >= 0]
    for r in cand:
        L[r] = row_loss(cls[r], pred[r], int(gt[assign[r], 4]) if kind[r] == 1 else 0, tg[r], inside)
    key = np.where(np.isnan(L[cand]), np.inf, L[cand]) if cand else np.zeros(0)
    order = [cand[i] for i in np.argsort(-key, kind="stable")]                      # descending loss, ties by ascending row, NaN first
    fin = np.unique(key[np.isfinite(key)])
    loss_gap = np.min(np.diff(fin) / np.maximum(np.abs(fin[1:]), 1e-300)) if fin.size > 1 else np.inf
    kept, sup, nms_gap = [], [], np.inf
    for r in order:
        hit = False
        if nms_thresh > 0 and len(kept) < B:
            for k in kept:
                o = nms_iou_f64(rois[k, 1:5], rois[r, 1:5])
                nms_gap = min(nms_gap, abs(o - nms_thresh))
                if (o >= nms_thresh) if rule == 0 else (o > f64(f32(nms_thresh))):
                    hit = True
                    break
        (sup if hit or len(kept) >= B else kept).append(r)
    P = kept + sup
    sel = [P[i % len(P)] for i in range(B)] if P else []
    keep = [r for r in sel if kind[r] == 1] + [r for r in sel if kind[r] == 0]
    out = dict(rois=np.zeros((B, 5), f32), scores=np.zeros(B, f32), labels=np.zeros((B, 1), f32), targets=np.zeros((B, 4 * C), f32),
               inside=np.zeros((B, 4 * C), f32), outside=np.zeros((B, 4 * C), f32), keep_inds=np.full(B, -1, np.int32), roi_loss=L,
               counts=np.array([sum(kind[r] == 1 for r in sel), sum(kind[r] == 0 for r in sel), int((kind == 1).sum()), int((kind == 0).sum())], np.int32),
               loss_gap=f64(loss_gap), label_gap=f64(label_gap), nms_gap=f64(nms_gap), n_kept=np.int64(len(kept)))
    for s, r in enumerate(keep):
        out["keep_inds"][s], out["rois"][s], out["scores"][s] = r, rois[r], scores[r]
        if kind[r] == 1:
            c = int(gt[assign[r], 4])
            out["labels"][s, 0] = c
            out["targets"][s, 4 * c:4 * c + 4] = tg[r]
            out["inside"][s, 4 * c:4 * c + 4] = inside
            out["outside"][s, 4 * c:4 * c + 4] = np.asarray(inside) > 0
    return out
