"""TEST INFRASTRUCTURE ONLY -- bounding-box voting and the merge of two flip views as plain numpy, the second statement of the rules that
tf-faster-rcnn_amd/csrc/boxvote_math.h holds for the kernels and the host entries.  Written from the rules' text, not from that header:

    voting     per kept detection d: ov_c = the float32 IoU of d's box with candidate c ("+1" widths, one numpy operation = one rounding
               per step, the order of cpu_nms.pyx:57-64); c votes iff float64(ov_c) >= vote_thresh; W = sum of float64(s_c) and
               X_k = sum of float64(s_c) * float64(box_c[k]) over the voters IN ASCENDING CANDIDATE ROW, one Python float (IEEE double)
               addition at a time -- numpy.sum reduces pairwise and does not state the rule --; the new box is float32(X_k / W); the
               score and the position stay.  No voter with W > 0: the box stays.
    merge      image b of B has the views 2b (as seen) and 2b+1 (mirrored), R rows each, n0 / n1 of them valid: 2R rows out, view 0's
               n0 rows, then view 1's n1 rows with x1' = (w - 1) - x2, x2' = (w - 1) - x1 in float32 and the dx of every class negated,
               then zeros; the count is n0 + n1.

Besides the boxes, vote() reports per kept detection the number of voters, which the fixture generator and the tests assert on."""
import numpy as np

import soft_nms_ref

F = np.float32
clustered = soft_nms_ref.clustered
iou = soft_nms_ref.iou                      # a float32 [4], b float32 [n,4] -> float32 [n]


def vote(kept, cands, vote_thresh):
    """kept float32 [m,5], cands float32 [n,5] -> (out float32 [m,5], voters int32 [m])"""
    kept = np.ascontiguousarray(kept, dtype=np.float32).reshape(-1, 5)
    cands = np.ascontiguousarray(cands, dtype=np.float32).reshape(-1, 5)
    out, voters = kept.copy(), np.zeros(len(kept), dtype=np.int32)
    t = float(vote_thresh)
    for d in range(len(kept)):
        if len(cands) == 0:
            continue
        ov = iou(kept[d, :4], cands[:, :4])
        w, x = 0.0, [0.0, 0.0, 0.0, 0.0]
        for c in np.flatnonzero(ov.astype(np.float64) >= t):            # ascending candidate row
            s = float(cands[c, 4])
            w = w + s
            for k in range(4):
                x[k] = x[k] + s * float(cands[c, k])
            voters[d] += 1
        if w > 0.0:
            for k in range(4):
                out[d, k] = F(x[k] / w)
    return out, voters


def count_voters(kept, cands, vote_thresh):
    """the voters of every kept detection at once (the same float32 operations, broadcast over kept x cands) -> int32 [m]"""
    a, b = np.asarray(kept, dtype=np.float32)[:, None, :4], np.asarray(cands, dtype=np.float32)[None, :, :4]
    aa = ((a[..., 2] - a[..., 0]) + F(1)) * ((a[..., 3] - a[..., 1]) + F(1))
    ab = ((b[..., 2] - b[..., 0]) + F(1)) * ((b[..., 3] - b[..., 1]) + F(1))
    w = np.maximum(F(0), (np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])) + F(1))
    h = np.maximum(F(0), (np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])) + F(1))
    inter = w * h
    ov = inter / ((aa + ab) - inter)
    assert ov.dtype == np.float32
    return (ov.astype(np.float64) >= float(vote_thresh)).sum(axis=1).astype(np.int32)


def hard_nms(dets, thresh, rule=0):
    """greedy NMS of one class (cpu_nms.pyx / nms_kernel.cu rule) -> the kept rows in emission order"""
    dets = np.ascontiguousarray(dets, dtype=np.float32)
    order = np.lexsort((np.arange(len(dets)), -dets[:, 4].astype(np.float64)))
    alive = np.ones(len(dets), dtype=bool)
    keep = []
    for i in order:
        if not alive[i]:
            continue
        keep.append(i)
        alive[i] = False
        rest = np.flatnonzero(alive)
        if rest.size:
            ov = iou(dets[i, :4], dets[rest, :4])
            alive[rest[(ov.astype(np.float64) >= float(thresh)) if rule == 0 else (ov > F(thresh))]] = False
    return np.array(keep, dtype=np.int64)


def merge_flip_views(cls_prob, bbox_pred, rois, num_rois, im_w_scaled, B):
    """cls_prob [2B*R,C], bbox_pred [2B*R,4C] or None, rois [2B*R,5], num_rois [2B] or None -> the same four for B images of 2R rows"""
    rows, C = cls_prob.shape
    R = rows // (2 * B)
    o_prob, o_rois = np.zeros((rows, C), dtype=np.float32), np.zeros((rows, 5), dtype=np.float32)
    o_pred = None if bbox_pred is None else np.zeros((rows, 4 * C), dtype=np.float32)
    o_num = np.zeros(B, dtype=np.int32)
    wm1 = F(im_w_scaled) - F(1)
    for b in range(B):
        n0, n1 = (R, R) if num_rois is None else (min(max(int(num_rois[2 * b]), 0), R), min(max(int(num_rois[2 * b + 1]), 0), R))
        s0, s1, d = 2 * b * R, (2 * b + 1) * R, 2 * b * R
        o_prob[d:d + n0], o_rois[d:d + n0] = cls_prob[s0:s0 + n0], rois[s0:s0 + n0]
        o_prob[d + n0:d + n0 + n1] = cls_prob[s1:s1 + n1]
        r1 = rois[s1:s1 + n1].copy()
        r1[:, 1], r1[:, 3] = wm1 - rois[s1:s1 + n1, 3], wm1 - rois[s1:s1 + n1, 1]
        o_rois[d + n0:d + n0 + n1] = r1
        if bbox_pred is not None:
            o_pred[d:d + n0] = bbox_pred[s0:s0 + n0]
            p1 = bbox_pred[s1:s1 + n1].copy()
            p1[:, 0::4] = -p1[:, 0::4]
            o_pred[d + n0:d + n0 + n1] = p1
        o_num[b] = n0 + n1
    assert o_rois.dtype == np.float32
    return o_prob, o_pred, o_rois, o_num
