"""TEST INFRASTRUCTURE ONLY -- the ordering machinery of csrc/detect_kernels.hip (proposal side) and csrc/detect_post.hip
(k_perclass_nms, k_final_select) restated in plain numpy on uint64 keys, step by step as the kernels do it (NOT as a sort): key construction (make_key), the 8-pass radix select of k_select_topk with its LDS-list
gather as a flag, the `>= cut` compaction, the counting rank of k_rank, the score recovery of k_scatter_sorted, the rank sort of
k_perclass_nms, and the 4-pass select + class-major compaction of k_final_select.

Its purpose is the `mutant` argument: each name below plants ONE mistake of the kind such code can carry.  tests/test_select_cpu.py
shows that the unmutated restatement equals oracle/frcnn_oracle.py, that every mutant is invisible on the inputs the suite had
before oracle/score_cases.py existed (the proof of the gap), and which of the new cases catch it.

   cut_hi32         (a) the cut compares only the upper 32 bits of the key (the last four radix passes are skipped)
   gather_4097      (b) the bucket is gathered when it holds <= 4097 keys, into a list of 4096: the last one is lost
   ties_desc        (c) ties ordered index-descending (the index half of the key holds the index, not its complement)
   signed_zero_key  (d) the key this project had: -0.0 below +0.0
   nan_key          (e) the key this project had: NaN by sign and payload (+NaN above +inf, -NaN below -inf)
   rank_ge          (f) the rank counts `>=` on the score half (minus the row itself): tied rows share a rank and collide.  (On the
                        whole, unique key `>=` is `>` plus the row itself -- a constant nobody could miss; the mistake that unique
                        scores hide is the comparison of scores.)
   final_gt         (g) k_final_select drops ties at the cut: every row `>` the cut and of the rows AT it only the first ones in slot
                        order, up to max_per_image in all -- an exact top-K where the reference keeps every row `>=` the cut
   wave_order       (h) compaction in wave-arrival order instead of index order.  k_select_topk compacts exactly so (one atomicAdd
                        a wave) and may: stage 2b ranks the keys, so the order of its K compacted keys is FREE -- this restatement
                        emits them in index order and the mutant in another, with the same result everywhere.  The order is
                        visible only in k_final_select, whose rows are the output; there the mutant lets the waves of a
                        1024-thread trip arrive last wave first.
"""
import ctypes

import numpy as np

import frcnn_oracle as ora

f32 = np.float32
u32 = np.uint32
u64 = np.uint64
SEL_LIST = 4096
MUTANTS = ("cut_hi32", "gather_4097", "ties_desc", "signed_zero_key", "nan_key", "rank_ge", "final_gt", "wave_order")
QNAN = np.array([0x7fc00000], dtype=u32).view(f32)[0]


# ----------------------------------------------------------------------------------------------------- keys
def sortable_u32(scores, mutant=None):
    """csrc/common.h sortable_u32: larger score <=> larger uint; -0.0 == +0.0; every NaN 0xffffffff"""
    b = np.ascontiguousarray(scores, dtype=f32).view(u32).copy()
    nan = (b & u32(0x7fffffff)) > u32(0x7f800000)
    if mutant != "signed_zero_key":
        b[b == u32(0x80000000)] = u32(0)
    out = np.where(b & u32(0x80000000), ~b, b | u32(0x80000000)).astype(u32)
    if mutant != "nan_key":
        out[nan] = u32(0xffffffff)
    return out


def make_key(scores, mutant=None):
    """(sortable << 32) | ((0x7fffffff - index) << 1) | (the score is -0.0): unique by the index alone"""
    s = np.ascontiguousarray(scores, dtype=f32)
    idx = np.arange(s.size, dtype=u64)
    low = idx if mutant == "ties_desc" else u64(0x7fffffff) - idx
    negzero = (s.view(u32) == u32(0x80000000)).astype(u64)
    return (sortable_u32(s, mutant).astype(u64) << u64(32)) | (low << u64(1)) | negzero


def key_index(keys, mutant=None):
    low = (keys & u64(0xffffffff)) >> u64(1)
    return (low if mutant == "ties_desc" else u64(0x7fffffff) - low).astype(np.int64)


def key_score(keys):
    """the input's bits, a zero's sign included; a NaN comes back as the quiet NaN"""
    hi = (keys >> u64(32)).astype(u32)
    bits = np.where(hi & u32(0x80000000), hi & u32(0x7fffffff), ~hi).astype(u32)
    bits = np.where(hi == u32(0x80000000), ((keys & u64(1)) << u64(31)).astype(u32), bits)
    bits = np.where(hi == u32(0xffffffff), u32(0x7fc00000), bits).astype(u32)
    return bits.view(f32)


# ----------------------------------------------------------------------------------------------------- radix select
def pick_bin(hist, k, prev):
    """the bin that holds the k-th largest key and the number of keys in the bins above it; no such bin (k exceeds the total):
    the device leaves the previous pass's pair in place"""
    above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])
    hit = np.flatnonzero((above < k) & (k <= above + hist))
    return (int(hit[0]), int(above[hit[0]])) if hit.size else prev


def radix_select(keys, K, bits=64, mutant=None, info=None):
    """The K-th largest of `keys` (0 < K < n) by 8-bit passes from the top.  bits = 64: k_select_topk -- after the pass at shift
    48 a bucket of <= SEL_LIST keys is gathered into the LDS list and the later passes read the list.  bits = 32: k_final_select."""
    n = keys.size
    assert 0 < K < n
    one = keys.dtype.type
    prefix, mask, k, lst, pick = one(0), one(0), int(K), None, (0, 0)
    last = 32 if (mutant == "cut_hi32" and bits == 64) else 0
    for shift in range(bits - 8, last - 8, -8):
        src = keys if lst is None else lst
        live = src[(src & mask) == prefix]
        hist = np.bincount(((live >> one(shift)) & one(255)).astype(np.int64), minlength=256)
        pick = pick_bin(hist, k, pick)
        k -= pick[1]
        prefix = prefix | (one(pick[0]) << one(shift))
        mask = mask | (one(255) << one(shift))
        if bits == 64 and shift == 48:
            limit = SEL_LIST + 1 if mutant == "gather_4097" else SEL_LIST
            if hist[pick[0]] <= limit:
                lst = keys[(keys & mask) == prefix][:SEL_LIST]           # a set: the order inside the list is free
            if info is not None:
                info["bucket"], info["gathered"] = int(hist[pick[0]]), lst is not None
    return prefix


def select_topk(keys, K, mutant=None, info=None):
    """k_select_topk: the min(K, n) keys >= the K-th largest, compacted in an order that is FREE (see the module docstring)"""
    n = keys.size
    cut = u64(0) if K >= n else radix_select(keys, K, 64, mutant, info)
    sel = keys[keys >= cut]
    if mutant in ("wave_order", "cut_hi32"):
        # cut_hi32 selects MORE than K keys and the device would keep whichever K arrive first; index order would coincide with the
        # tie rule (lower index first) and hide the mistake, so the mutant keeps them from the far end
        sel = sel[::-1]
    return sel[:min(K, n)]


def rank_scatter(ckeys, mutant=None):
    """k_rank + k_scatter_sorted: rank = how many keys are greater; (index, score) written at the rank.  Slots no key claims
    stay 0, as in the zero-initialised restatement of a scratch buffer; of two keys on one slot the later one stays."""
    K = ckeys.size
    if mutant == "rank_ge":
        hi = ckeys >> u64(32)
        rank = K - np.searchsorted(np.sort(hi), hi, side="left") - 1
    else:
        rank = K - np.searchsorted(np.sort(ckeys), ckeys, side="right")
    sidx, sscores = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=f32)
    sidx[rank] = key_index(ckeys, mutant)
    sscores[rank] = key_score(ckeys)
    return sidx, sscores


def sort_topk(scores, K, mutant=None, info=None):
    """launch_topk_sort: -> (sidx [min(K, n)], sscores) = `order = scores.argsort()[::-1][:K]` and scores[order]"""
    return rank_scatter(select_topk(make_key(scores, mutant), K, mutant, info), mutant)


def same_scores(a, b):
    """bit for bit, except that any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, dtype=f32).reshape(-1), np.ascontiguousarray(b, dtype=f32).reshape(-1)
    return a.shape == b.shape and bool(np.all((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))))


# ----------------------------------------------------------------------------------------------------- layers on top
def nms_in_order(dets, thresh):
    """cpu_nms on rows ALREADY in their order (oracle_c.c:oracle_cpu_nms with the identity order): no second sort that could
    repair a wrong one"""
    dets = np.ascontiguousarray(dets, dtype=f32)
    k = dets.shape[0]
    if k == 0:
        return []
    order, keep = np.arange(k, dtype=np.int64), np.empty(k, dtype=np.int64)
    n = ora._lib().oracle_cpu_nms(ora._p(dets), ctypes.c_int(k), ora._p(order), ctypes.c_double(float(thresh)), ora._p(keep))
    return keep[:n].tolist()


def proposal_layer(rpn_cls_prob, rpn_bbox_pred, im_info, anchors, num_anchors, pre_nms_topN, post_nms_topN, nms_thresh, mutant=None):
    """frcnn_proposal_layer: decode + clip every anchor, launch_topk_sort, NMS in that order, the first post_nms_topN"""
    scores = np.ascontiguousarray(rpn_cls_prob[:, :, :, num_anchors:]).reshape(-1)
    props = ora.clip_boxes(ora.bbox_transform_inv(anchors, rpn_bbox_pred.reshape(-1, 4)), im_info[:2])
    K = pre_nms_topN if 0 < pre_nms_topN < scores.size else scores.size
    sidx, ss = sort_topk(scores, K, mutant)
    keep = nms_in_order(np.hstack((props[sidx], ss.reshape(-1, 1))), nms_thresh)[:post_nms_topN]
    blob = np.hstack((np.zeros((len(keep), 1), dtype=f32), props[sidx][keep].astype(f32, copy=False)))
    return blob, ss[keep].reshape(-1, 1)


def proposal_top_layer(rpn_cls_prob, rpn_bbox_pred, im_info, anchors, num_anchors, rpn_top_n, mutant=None):
    scores = np.ascontiguousarray(rpn_cls_prob[:, :, :, num_anchors:]).reshape(-1)
    props = ora.clip_boxes(ora.bbox_transform_inv(anchors, rpn_bbox_pred.reshape(-1, 4)), im_info[:2])
    sidx, ss = sort_topk(scores, rpn_top_n, mutant)
    return np.hstack((np.zeros((sidx.size, 1), dtype=f32), props[sidx].astype(f32, copy=False))), ss.reshape(-1, 1)


# ----------------------------------------------------------------------------------------------------- test-time post-processing
def perclass_nms(scores, boxes, j, nms_thresh, thresh, mutant=None):
    """k_perclass_nms for class j: `scores > thresh` (drops NaN), rank sort on make_key(score, row), NMS -> [n,5]"""
    s = np.ascontiguousarray(scores[:, j], dtype=f32)
    with np.errstate(invalid="ignore"):
        valid = np.flatnonzero(s > f32(thresh))
    keys = make_key(s, mutant)[valid]
    if keys.size == 0:
        return np.zeros((0, 5), dtype=f32)
    sidx, ss = rank_scatter(keys, mutant)
    dets = np.hstack((boxes[sidx, j * 4:(j + 1) * 4], ss.reshape(-1, 1))).astype(f32, copy=False)
    return dets[nms_in_order(dets, nms_thresh), :]


def final_select(per_class, R, max_per_image, max_out, mutant=None):
    """k_final_select on the per-class lists (class c's n_c rows sit at slots c * R + p): the max_per_image-th largest score by a
    4-pass radix select when there are more rows than that, every row `>=` it, compacted class-major in slot order, at most
    max_out rows written.  -> (records [min(count, max_out), 6], count)"""
    slot = np.concatenate([c * R + np.arange(d.shape[0]) for c, d in enumerate(per_class)]).astype(np.int64)
    rows = np.vstack([np.hstack((d, np.full((d.shape[0], 1), c + 1, dtype=f32))) for c, d in enumerate(per_class)]).astype(f32)
    keys = sortable_u32(rows[:, 4], mutant)
    cut = u32(0)
    if max_per_image > 0 and rows.shape[0] > max_per_image:
        cut = radix_select(keys, max_per_image, 32, mutant)
    keep = keys >= cut
    if mutant == "final_gt" and cut:
        at = np.flatnonzero(keys == cut)
        keep[at[max(0, max_per_image - int((keys > cut).sum())):]] = False
    if mutant == "wave_order":
        trip, wave = slot // 1024, (slot % 1024) // 64
        order = np.lexsort((slot, -wave, trip))                          # inside a trip the last wave arrives first
    else:
        order = np.arange(slot.size)
    order = order[keep[order]]
    return rows[order][:max_out], int(order.size)


def detect_post(scores, boxes, num_classes, nms_thresh=0.3, max_per_image=100, thresh=0.0, max_out=128, mutant=None):
    """frcnn_detect_post from the decoded boxes on: -> (records [min(count, max_out), 6], count)"""
    per_class = [perclass_nms(scores, boxes, j, nms_thresh, thresh, mutant) for j in range(1, num_classes)]
    return final_select(per_class, scores.shape[0], max_per_image, max_out, mutant)
