"""Tensor-level wrappers over the C ABI.  torch is plumbing here: device buffers, streams.

Every function takes/returns torch CUDA tensors (float32, contiguous, NHWC) and launches on the
CURRENT torch stream (so torch.cuda.Event / torch.cuda.synchronize see the work).  Outputs may be
passed in (`out=`) so a captured hipGraph can reuse static buffers.
"""
import ctypes

import numpy as np
import torch

import frcnn_hip as _binding
from . import ACT_NONE, NMS_RULE_CPU, call, check, lib

_ws_cache = {}
ws_scope = "default"     # set by callers that run several independent chains concurrently (one scope per stream)

# The entered buffer scopes, innermost last: (owner, key, store) -- Session.shape_scope pushes (the session, the shape's key, that shape's
# buffer dict), see the comment there.  The bottom entry, and unscoped()'s, is "no scope".  One stack per process, not per thread, like
# stream_pin, arena, ws_scope and frcnn_hip.recorder: a step is single-threaded by design.
_scope_stack = [(None, None, None)]


def active_store(owner, default=None):
    """The innermost entered scope's store if `owner` entered it (owner = None: whoever did); `default` otherwise and outside every scope."""
    o, _, store = _scope_stack[-1]
    return store if store is not None and (owner is None or o is owner) else default


def scope_depth():
    return len(_scope_stack) - 1


class unscoped(object):
    """`with unscoped():` -- buffers allocated inside belong to the session, not to the image shape being built (filter images, solver state)."""

    def __enter__(self):
        _scope_stack.append(_scope_stack[0])

    def __exit__(self, *exc):
        _scope_stack.pop()


stream_pin = None        # a ctypes stream handle: every launch of this module goes there instead of torch's current stream (see pinned_stream)


def _stream():
    return stream_pin if stream_pin is not None else ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class pinned_stream(object):
    """`with pinned_stream(s):` -- the launches of this module go to torch stream `s` without the per-call current_stream() lookup
    and without making `s` torch's current stream (a `with torch.cuda.stream(...)` costs ~10 us of host time per entry; the reverse
    sweep switches streams ~200 times a step).  Only for regions whose torch-level ops, if any, belong on torch's current stream."""

    def __init__(self, stream):
        self.handle = ctypes.c_void_p(stream.cuda_stream)

    def __enter__(self):
        global stream_pin
        self.prev, stream_pin = stream_pin, self.handle
        return self

    def __exit__(self, *exc):
        global stream_pin
        stream_pin = self.prev
        return False


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


# ---- a training step as a replayable launch list (frcnn_hip/replay.py) ------------------------------------------------------------------
# `arena`: while set, the result tensors these wrappers allocate themselves are static session buffers (same address every step).
# `_binding.recorder`: while set, every call() and every stream-level operation below is appended to the recording of the step.
arena = None


def _empty(shape, dtype=torch.float32, device=None):
    if arena is not None:
        return arena.take(shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,), dtype, device)
    return torch.empty(shape, dtype=dtype, device=device)


def _zeros(shape, dtype=torch.float32, device=None):
    if arena is not None:
        return t_zero(arena.take(shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,), dtype, device))
    return torch.zeros(shape, dtype=dtype, device=device)


def t_zero(t):
    """t.zero_() on torch's current stream (recorded as an operation of the step)"""
    t.zero_()
    R = _binding.recorder
    if R is not None:
        R.add_op(lambda rec, t=t: t.zero_())
    return t


def t_copy(dst, src):
    """dst.copy_(src) on torch's current stream"""
    dst.copy_(src)
    R = _binding.recorder
    if R is not None:
        R.add_op(lambda rec, dst=dst, src=src: dst.copy_(src))
    return dst


def ev_record(ev, stream):
    ev.record(stream)
    R = _binding.recorder
    if R is not None:
        s = R.slot(stream)
        R.add_op(lambda rec, ev=ev, s=s: ev.record(rec.bound[s]))


def st_wait_event(stream, ev):
    stream.wait_event(ev)
    R = _binding.recorder
    if R is not None:
        s = R.slot(stream)
        R.add_op(lambda rec, ev=ev, s=s: rec.bound[s].wait_event(ev))


def st_wait_stream(stream, other):
    """stream.wait_stream(other)"""
    R = _binding.recorder
    if R is None:
        stream.wait_stream(other)
        return
    ev = torch.cuda.Event()                     # (torch's wait_stream makes a fresh event per call; a recording owns one per site)
    R.keep.append(ev)
    ev_record(ev, other)
    st_wait_event(stream, ev)


def host_op(fn):
    """fn(): host code that enqueues work through torch (a collective, a tensor expression): run now and, while a step is being
    recorded, again at every replay.  fn may take one argument -- None now, the Recording at replay (rec.bound[slot] is the stream
    bound to a slot that was looked up with recorder.slot(stream) at record time)."""
    import inspect
    takes = len(inspect.signature(fn).parameters) > 0
    out = fn(None) if takes else fn()
    R = _binding.recorder
    if R is not None:
        R.add_op(fn if takes else (lambda rec, fn=fn: fn()))
    return out


def _chk(t, dtype=torch.float32):
    if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype):
        raise ValueError("expected a contiguous CUDA %s tensor, got %s %s contiguous=%s" %
                         (dtype, t.device, t.dtype, t.is_contiguous()))
    return t


def workspace(nbytes, device, tag="default"):
    """Grow-only scratch buffer per (device, tag); never reallocated inside a captured region
    as long as the first (warm-up) call already saw the largest request."""
    # scratch follows the INNERMOST entered scope, whoever owns it (there is no session in hand here; every Network entry point --
    # forward_device, extract_head, detect_device, train_step_async -- enters its own session's scope before its first launch): it belongs to
    # that shape and is freed with it; a buffer a captured graph may still address is retired INTO the same store, i.e. lives as long as it
    store = active_store(None, _ws_cache)
    key = ("ws", str(device), tag, ws_scope)
    buf = store.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            store.setdefault(("ws_retired",), []).append(buf)
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        store[key] = buf
    return buf


# ------------------------------------------------------------------------------------------ anchors
def generate_anchors(base_size=16, ratios=(0.5, 1, 2), scales=(8, 16, 32)):
    """HOST float64 [A,4] base anchors (lib/layer_utils/generate_anchors.py:41-52)."""
    r = np.ascontiguousarray(ratios, dtype=np.float64)
    s = np.ascontiguousarray(scales, dtype=np.float64)
    out = np.empty((r.size * s.size, 4), dtype=np.float64)
    call("frcnn_generate_anchors", int(base_size), r.ctypes.data_as(ctypes.c_void_p), r.size,
         s.ctypes.data_as(ctypes.c_void_p), s.size, out.ctypes.data_as(ctypes.c_void_p))
    return out


def generate_anchors_pre(height, width, feat_stride, base_d, out=None):
    """DEVICE f32 [H*W*A,4] (lib/layer_utils/snippets.py:14-30).  base_d: float64 CUDA [A,4]."""
    A = base_d.shape[0]
    _chk(base_d, torch.float64)
    if out is None:
        out = _empty((height * width * A, 4), dtype=torch.float32, device=base_d.device)
    call("frcnn_generate_anchors_pre", height, width, int(feat_stride), _ptr(base_d), A, _ptr(out), _stream())
    return out


# ------------------------------------------------------------------------------------------ NMS
def nms(dets, thresh, max_keep=None, keep=None, num=None, rule=NMS_RULE_CPU):
    """cpu_nms (rule NMS_RULE_CPU) / gpu_nms (NMS_RULE_GPU) semantics on device.  dets f32 [k,5] any order ->
    (keep int32 [max_keep], num int32 [1])."""
    _chk(dets)
    k = dets.shape[0]
    max_keep = k if max_keep is None else min(max_keep, k)
    dev = dets.device
    keep = _empty((max(max_keep, 1),), dtype=torch.int32, device=dev) if keep is None else keep
    num = _zeros((1,), dtype=torch.int32, device=dev) if num is None else num
    nb = lib().frcnn_nms_workspace_bytes(max(k, 1))
    ws = workspace(nb, dev, "nms")
    call("frcnn_nms_rule", _ptr(dets), k, float(thresh), int(rule), max_keep, _ptr(keep), _ptr(num), _ptr(ws), ws.numel(), _stream())
    return keep, num


def nms_sorted(boxes, thresh, max_keep=None, rule=NMS_RULE_CPU):
    """Device-pointer form of `_nms`: boxes f32 [k, >=4] sorted by descending score."""
    _chk(boxes)
    k, stride = boxes.shape
    max_keep = k if max_keep is None else min(max_keep, k)
    dev = boxes.device
    keep = _empty((max(max_keep, 1),), dtype=torch.int32, device=dev)
    num = _zeros((1,), dtype=torch.int32, device=dev)
    nb = lib().frcnn_nms_workspace_bytes(max(k, 1))
    ws = workspace(nb, dev, "nms")
    call("frcnn_nms_sorted_rule", _ptr(boxes), k, stride, float(thresh), int(rule), max_keep, _ptr(keep), _ptr(num), _ptr(ws),
         ws.numel(), _stream())
    return keep, num


def non_max_suppression(boxes, scores, max_output_size, iou_threshold, selected=None, num=None):
    """tf.image.non_max_suppression(boxes [k,4], scores [k], max_output_size, iou_threshold) on device (the NMS of the
    reference's USE_E2E_TF graph, proposal_layer.py:72).  -> (selected int32 [max_output_size], num int32 [1])."""
    _chk(boxes), _chk(scores)
    k = boxes.shape[0]
    assert boxes.shape == (k, 4) and scores.numel() == k
    m = min(int(max_output_size), k)
    dev = boxes.device
    selected = _empty((max(m, 1),), dtype=torch.int32, device=dev) if selected is None else selected
    num = _zeros((1,), dtype=torch.int32, device=dev) if num is None else num
    nb = lib().frcnn_nms_workspace_bytes(max(k, 1))
    ws = workspace(nb, dev, "nms")
    call("frcnn_non_max_suppression", _ptr(boxes), _ptr(scores), k, m, float(iou_threshold), _ptr(selected), _ptr(num),
         _ptr(ws), ws.numel(), _stream())
    return selected, num


def bbox_overlaps(boxes, query):
    _chk(boxes, torch.float64), _chk(query, torch.float64)
    out = _empty((boxes.shape[0], query.shape[0]), dtype=torch.float64, device=boxes.device)
    call("frcnn_bbox_overlaps", _ptr(boxes), boxes.shape[0], _ptr(query), query.shape[0], _ptr(out), _stream())
    return out


def coco_match(det_xywh, det_off, gt_xywh, gt_area, gt_crowd, gt_off, iou_thrs, area_rng, want_iou=False):
    """COCO bbox matching of every (image, category) group (frcnn_coco_match): device tensors det_xywh [n_det,4] f64 (per group sorted
    by -score, cut to max_det), gt_xywh [n_gt,4] f64, gt_area [n_gt] f64, gt_crowd [n_gt] u8, iou_thrs [T] f64, area_rng [A,2] f64; the CSR
    offsets det_off / gt_off [n_groups+1] are HOST int64 arrays: they are checked against the tensors here (non-decreasing from 0, totals
    = n_det / n_gt), the pair total and the workspace size follow from them, and they are uploaded for the kernel -- so no caller can
    hand the entry a workspace sized for other totals.  Returns (det_matched [A,T,n_det] u8, det_ignored [A,T,n_det] u8, gt_ignored
    [A,n_gt] u8, iou [n_pairs] f64 or None) on the current stream, zero where no group covers an element."""
    for t, dt in ((det_xywh, torch.float64), (gt_xywh, torch.float64), (gt_area, torch.float64), (iou_thrs, torch.float64),
                  (area_rng, torch.float64), (gt_crowd, torch.uint8)):
        _chk(t, dt)
    det_off, gt_off = (np.ascontiguousarray(o, dtype=np.int64).reshape(-1) for o in (det_off, gt_off))
    n_groups, n_det, n_gt, T, A = det_off.size - 1, det_xywh.shape[0], gt_xywh.shape[0], iou_thrs.numel(), area_rng.shape[0]
    if n_groups < 0 or gt_off.size != n_groups + 1 or gt_area.numel() != n_gt or gt_crowd.numel() != n_gt or area_rng.numel() != 2 * A:
        raise ValueError("coco_match: inconsistent sizes")
    for off, total in ((det_off, n_det), (gt_off, n_gt)):
        if off[0] != 0 or off[-1] != total or np.any(np.diff(off) < 0):
            raise ValueError("coco_match: offsets must run from 0 to the number of rows without decreasing")
    n_pairs = int(np.sum(np.diff(det_off) * np.diff(gt_off)))
    dev = det_xywh.device
    det_off_d, gt_off_d = torch.from_numpy(det_off).to(dev), torch.from_numpy(gt_off).to(dev)
    matched = _zeros((A, T, n_det), dtype=torch.uint8, device=dev)
    ignored = _zeros((A, T, n_det), dtype=torch.uint8, device=dev)
    gt_ignored = _zeros((A, n_gt), dtype=torch.uint8, device=dev)
    iou = _empty((n_pairs,), dtype=torch.float64, device=dev) if want_iou else None
    nbytes = lib().frcnn_coco_match_workspace_bytes(n_groups, n_det, n_gt, n_pairs)
    ws = workspace(nbytes, dev, "coco_match")
    call("frcnn_coco_match", _ptr(det_xywh), _ptr(det_off_d), _ptr(gt_xywh), _ptr(gt_area), _ptr(gt_crowd), _ptr(gt_off_d), n_groups,
         _ptr(iou_thrs), T, _ptr(area_rng), A, _ptr(matched), _ptr(ignored), _ptr(gt_ignored), _ptr(iou), _ptr(ws), nbytes, _stream())
    return matched, ignored, gt_ignored, iou


def proposal_recall(boxes, start, count, scale, gt, gt_off, max_boxes, limit=None, out=None, ran_out=None):
    """The matching loop of imdb.evaluate_recall for n_images images in one launch (frcnn_proposal_recall, csrc/recall.hip).  DEVICE
    tensors: boxes f32 [n_rows, 4 | 5] (5: the `rois` layout), start int64 [n_images] (first row of every image), count int32
    [n_images] (read by the kernel: a forward's num_rois goes in as it is), scale f32 [n_images], gt f64 [n_gt,4], gt_off int64
    [n_images+1]; max_boxes bounds every count.  limit None or <= 0: every row counts.  -> (gt_iou f64 [n_gt], ran_out int32
    [n_images]) on the current stream: slot gt_off[i] + j is image i's j-th pick; the slots of an image without candidates keep what
    `out` held (zeros when it is allocated here)."""
    _chk(boxes), _chk(start, torch.int64), _chk(count, torch.int32), _chk(scale), _chk(gt, torch.float64), _chk(gt_off, torch.int64)
    n_images, n_gt, dev = count.numel(), gt.shape[0], boxes.device
    if boxes.dim() != 2 or start.numel() != n_images or scale.numel() != n_images or gt_off.numel() != n_images + 1 or gt.shape[1:] != (4,):
        raise ValueError("proposal_recall: inconsistent sizes")
    out = _zeros((n_gt,), dtype=torch.float64, device=dev) if out is None else _chk(out, torch.float64)
    ran_out = _empty((n_images,), dtype=torch.int32, device=dev) if ran_out is None else _chk(ran_out, torch.int32)
    if out.numel() != n_gt or ran_out.numel() != n_images:
        raise ValueError("proposal_recall: inconsistent sizes")
    nbytes = lib().frcnn_proposal_recall_workspace_bytes(n_images, int(max_boxes), n_gt)
    ws = workspace(nbytes, dev, "proposal_recall")
    call("frcnn_proposal_recall", _ptr(boxes), boxes.shape[1], boxes.shape[0], _ptr(start), _ptr(count), _ptr(scale), n_images, int(max_boxes),
         0 if limit is None else int(limit), _ptr(gt), _ptr(gt_off), n_gt, _ptr(out), _ptr(ran_out), _ptr(ws), nbytes, _stream())
    return out, ran_out


def proposal_recall_host(boxes, start, count, scale, gt, gt_off, max_boxes, limit=None):
    """frcnn_proposal_recall_host: the same on HOST numpy arrays, no GPU needed -> (gt_iou f64 [n_gt] zero-filled, ran_out int32)."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    start, gt_off = np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(gt_off, dtype=np.int64)
    count, scale = np.ascontiguousarray(count, dtype=np.int32), np.ascontiguousarray(scale, dtype=np.float32)
    gt = np.ascontiguousarray(gt, dtype=np.float64).reshape(-1, 4)
    n_images, n_gt = count.size, gt.shape[0]
    if boxes.ndim != 2 or start.size != n_images or scale.size != n_images or gt_off.size != n_images + 1:
        raise ValueError("proposal_recall_host: inconsistent sizes")
    out, ran_out = np.zeros(n_gt, dtype=np.float64), np.zeros(n_images, dtype=np.int32)
    nbytes = lib().frcnn_proposal_recall_workspace_bytes(n_images, int(max_boxes), n_gt)
    ws = np.empty(nbytes, dtype=np.uint8)
    check(lib().frcnn_proposal_recall_host(boxes.ctypes.data, boxes.shape[1], boxes.shape[0], start.ctypes.data, count.ctypes.data,
                                           scale.ctypes.data, n_images, int(max_boxes), 0 if limit is None else int(limit), gt.ctypes.data,
                                           gt_off.ctypes.data, n_gt, out.ctypes.data, ran_out.ctypes.data, ws.ctypes.data, nbytes),
          "frcnn_proposal_recall_host")
    return out, ran_out


def bbox_transform_inv(boxes, deltas, out=None):
    """lib/model/bbox_transform.py:35-65 on device: boxes [N,4], deltas [N,4k] -> [N,4k]."""
    _chk(boxes), _chk(deltas)
    N, k = boxes.shape[0], deltas.shape[1] // 4
    out = _empty((N, 4 * k), dtype=torch.float32, device=boxes.device) if out is None else out
    call("frcnn_bbox_transform_inv", _ptr(boxes), _ptr(deltas), N, k, _ptr(out), _stream())
    return out


def clip_boxes(boxes, im_h, im_w):
    """lib/model/bbox_transform.py:68-81 in place: boxes [N,4k]."""
    _chk(boxes)
    call("frcnn_clip_boxes", _ptr(boxes), boxes.shape[0], boxes.shape[1] // 4, float(im_h), float(im_w), _stream())
    return boxes


def bbox_transform(ex_rois, gt_rois):
    """lib/model/bbox_transform.py:14-32 on device: [N,4] x [N,4] -> targets [N,4]."""
    _chk(ex_rois), _chk(gt_rois)
    out = _empty((ex_rois.shape[0], 4), dtype=torch.float32, device=ex_rois.device)
    call("frcnn_bbox_transform", _ptr(ex_rois), _ptr(gt_rois), ex_rois.shape[0], _ptr(out), _stream())
    return out


# ------------------------------------------------------------------------------------------ proposals
def proposal_layer(rpn_cls_prob, rpn_bbox_pred, im_h, im_w, feat_stride, base_d, pre_nms_topn, post_nms_topn,
                   nms_thresh, rois=None, scores=None, num=None, rule=NMS_RULE_CPU):
    """lib/layer_utils/proposal_layer.py:16-53 on device, for the B images of rpn_cls_prob [B,H,W,2A] in one set of launches.
    Returns (rois [B*post,5] with rois[:,0] = image index, scores [B*post,1], num [B])."""
    _chk(rpn_cls_prob), _chk(rpn_bbox_pred), _chk(base_d, torch.float64)
    B, H, W, A2 = rpn_cls_prob.shape
    A = A2 // 2
    dev = rpn_cls_prob.device
    rois = _empty((B * post_nms_topn, 5), dtype=torch.float32, device=dev) if rois is None else rois
    scores = _empty((B * post_nms_topn, 1), dtype=torch.float32, device=dev) if scores is None else scores
    num = _zeros((B,), dtype=torch.int32, device=dev) if num is None else num
    nb = lib().frcnn_proposal_batched_workspace_bytes(B, H, W, A, int(pre_nms_topn))
    ws = workspace(nb, dev, "proposal")
    call("frcnn_proposal_layer_batched", _ptr(rpn_cls_prob), _ptr(rpn_bbox_pred), B, float(im_h), float(im_w), H, W, A,
         int(feat_stride), _ptr(base_d), int(pre_nms_topn), int(post_nms_topn), float(nms_thresh), int(rule), _ptr(rois),
         _ptr(scores), _ptr(num), _ptr(ws), ws.numel(), _stream())
    return rois, scores, num


def proposal_layer_tf(rpn_cls_prob, rpn_bbox_pred, im_h, im_w, feat_stride, base_d, post_nms_topn, nms_thresh, rois=None,
                      scores=None, num=None):
    """lib/layer_utils/proposal_layer.py:56-84 (USE_E2E_TF): NMS with tf.image.non_max_suppression semantics over ALL
    anchors, no pre-NMS top-N, B images per launch.  Returns (rois [B*post,5] zero padded, scores [B*post,1], num [B])."""
    _chk(rpn_cls_prob), _chk(rpn_bbox_pred), _chk(base_d, torch.float64)
    B, H, W, A2 = rpn_cls_prob.shape
    A = A2 // 2
    dev = rpn_cls_prob.device
    rois = _empty((B * post_nms_topn, 5), dtype=torch.float32, device=dev) if rois is None else rois
    scores = _empty((B * post_nms_topn, 1), dtype=torch.float32, device=dev) if scores is None else scores
    num = _zeros((B,), dtype=torch.int32, device=dev) if num is None else num
    nb = lib().frcnn_proposal_batched_workspace_bytes(B, H, W, A, 0)
    ws = workspace(nb, dev, "proposal")
    call("frcnn_proposal_layer_tf_batched", _ptr(rpn_cls_prob), _ptr(rpn_bbox_pred), B, float(im_h), float(im_w), H, W, A,
         int(feat_stride), _ptr(base_d), int(post_nms_topn), float(nms_thresh), _ptr(rois), _ptr(scores), _ptr(num),
         _ptr(ws), ws.numel(), _stream())
    return rois, scores, num


def proposal_top_layer_inds(rpn_cls_prob, rpn_bbox_pred, im_h, im_w, feat_stride, base_d, top_inds, rois=None, scores=None):
    """proposal_top_layer.py:30-33,46-55 for caller-chosen anchor indices (int32 device tensor): decode + clip those."""
    _chk(rpn_cls_prob), _chk(rpn_bbox_pred), _chk(base_d, torch.float64), _chk(top_inds, torch.int32)
    _, H, W, A2 = rpn_cls_prob.shape
    n = top_inds.numel()
    dev = rpn_cls_prob.device
    rois = _empty((n, 5), dtype=torch.float32, device=dev) if rois is None else rois
    scores = _empty((n, 1), dtype=torch.float32, device=dev) if scores is None else scores
    call("frcnn_proposal_top_layer_inds", _ptr(rpn_cls_prob), _ptr(rpn_bbox_pred), float(im_h), float(im_w), H, W, A2 // 2,
         int(feat_stride), _ptr(base_d), _ptr(top_inds), n, _ptr(rois), _ptr(scores), _stream())
    return rois, scores


def proposal_top_layer(rpn_cls_prob, rpn_bbox_pred, im_h, im_w, feat_stride, base_d, rpn_top_n, rois=None, scores=None):
    _chk(rpn_cls_prob), _chk(rpn_bbox_pred), _chk(base_d, torch.float64)
    _, H, W, A2 = rpn_cls_prob.shape
    A = A2 // 2
    dev = rpn_cls_prob.device
    rois = _empty((rpn_top_n, 5), dtype=torch.float32, device=dev) if rois is None else rois
    scores = _empty((rpn_top_n, 1), dtype=torch.float32, device=dev) if scores is None else scores
    nb = lib().frcnn_proposal_workspace_bytes(H, W, A, int(rpn_top_n))
    ws = workspace(nb, dev, "proposal")
    call("frcnn_proposal_top_layer", _ptr(rpn_cls_prob), _ptr(rpn_bbox_pred), float(im_h), float(im_w), H, W, A,
         int(feat_stride), _ptr(base_d), int(rpn_top_n), _ptr(rois), _ptr(scores), _ptr(ws), ws.numel(), _stream())
    return rois, scores


def crop_and_resize(feat, rois, feat_stride, pool, max_pool=False, out=None):
    """feat [N,H,W,C] or [H,W,C]; rois [R,5] with rois[:,0] = image index (the box_ind of tf.image.crop_and_resize,
    network.py:143) -> [R,pool,pool,C] (TF crop_and_resize semantics)."""
    _chk(feat), _chk(rois)
    H, W, C = feat.shape[-3:]
    N = feat.shape[0] if feat.dim() == 4 else 1
    R = rois.shape[0]
    out = _empty((R, pool, pool, C), dtype=torch.float32, device=feat.device) if out is None else out
    call("frcnn_crop_and_resize_batched", _ptr(feat), N, H, W, C, _ptr(rois), R, float(feat_stride), int(pool),
         1 if max_pool else 0, _ptr(out), _stream())
    return out


def crop_and_resize_bias_act(feat, rois, feat_stride, pool, bias, act, out=None):
    """act(crop_and_resize(feat) + bias): see frcnn_crop_and_resize_bias_act."""
    _chk(feat), _chk(rois)
    H, W, C = feat.shape[-3:]
    N = feat.shape[0] if feat.dim() == 4 else 1
    R = rois.shape[0]
    out = _empty((R, pool, pool, C), dtype=torch.float32, device=feat.device) if out is None else out
    call("frcnn_crop_and_resize_bias_act", _ptr(feat), N, H, W, C, _ptr(rois), R, float(feat_stride), int(pool), _ptr(bias),
         int(act), _ptr(out), _stream())
    return out


def roi_align(feat, rois, feat_stride, pool, samples, out=None):
    """RoIAlign (csrc/roialign_math.h): feat [N,H,W,C] or [H,W,C]; rois [R,5] with rois[:,0] = image index -> [R,pool,pool,C], the mean
    of samples x samples bilinear samples per bin."""
    return roi_align_bias_act(feat, rois, feat_stride, pool, samples, None, ACT_NONE, out=out)


def roi_align_bias_act(feat, rois, feat_stride, pool, samples, bias, act, out=None):
    """act(roi_align(feat) + bias): see frcnn_roi_align_batched."""
    _chk(feat), _chk(rois)
    H, W, C = feat.shape[-3:]
    N = feat.shape[0] if feat.dim() == 4 else 1
    R = rois.shape[0]
    out = _empty((R, pool, pool, C), dtype=torch.float32, device=feat.device) if out is None else out
    call("frcnn_roi_align_batched", _ptr(feat), N, H, W, C, _ptr(rois), R, float(feat_stride), int(pool), int(samples), _ptr(bias),
         int(act), _ptr(out), _stream())
    return out


def _host_f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


def roi_align_host(feat, rois, feat_stride, pool, samples, bias=None, act=ACT_NONE):
    """frcnn_roi_align_host: the same on HOST numpy arrays, no GPU needed -> f32 [R,pool,pool,C], the device's bits."""
    feat, rois = _host_f32(feat), _host_f32(rois, (-1, 5))
    if feat.ndim == 3:
        feat = feat[None]
    N, H, W, C = feat.shape
    R = rois.shape[0]
    bias = None if bias is None else _host_f32(bias, (C,))
    out = np.empty((R, pool, pool, C), dtype=np.float32)
    check(lib().frcnn_roi_align_host(feat.ctypes.data, N, H, W, C, rois.ctypes.data if R else None, R, float(feat_stride), int(pool),
                                     int(samples), None if bias is None else bias.ctypes.data, int(act), out.ctypes.data if R else None),
          "frcnn_roi_align_host")
    return out


def roi_align_bwd_host(dout, rois, feat_stride, samples, dfeat):
    """frcnn_roi_align_bwd_host: dfeat (numpy f32 [H,W,C], contiguous, modified in place) += the gradient of dout [R,P,P,C]."""
    dout, rois = _host_f32(dout), _host_f32(rois, (-1, 5))
    if not (isinstance(dfeat, np.ndarray) and dfeat.dtype == np.float32 and dfeat.flags.c_contiguous and dfeat.ndim == 3):
        raise ValueError("roi_align_bwd_host: dfeat must be a contiguous float32 [H,W,C] array")
    R, P, _, C = dout.shape
    H, W = dfeat.shape[0], dfeat.shape[1]
    if dfeat.shape[2] != C or rois.shape[0] != R:
        raise ValueError("roi_align_bwd_host: shapes disagree")
    check(lib().frcnn_roi_align_bwd_host(dout.ctypes.data if R else None, H, W, C, rois.ctypes.data if R else None, R, float(feat_stride),
                                         int(P), int(samples), dfeat.ctypes.data), "frcnn_roi_align_bwd_host")
    return dfeat


def roi_align_classify_host(H, W, rois, feat_stride, pool, samples):
    """-> int64 [R,4]: a RoI's zeroed, clamped-low, clamped-high and integer-coordinate samples (the kinds of csrc/roialign_math.h)."""
    rois = _host_f32(rois, (-1, 5))
    counts = np.zeros((rois.shape[0], 4), dtype=np.int64)
    if rois.shape[0]:
        check(lib().frcnn_roi_align_classify_host(int(H), int(W), rois.ctypes.data, rois.shape[0], float(feat_stride), int(pool), int(samples),
                                                  counts.ctypes.data), "frcnn_roi_align_classify_host")
    return counts


def detect_post(cls_prob, bbox_pred, rois, num_rois, im_scale, im_h, im_w, nms_thresh=0.3, score_thresh=0.0,
                max_per_image=100, max_out=None, out=None, count=None, batch=1, rule=NMS_RULE_CPU, soft=0, sigma=0.5, min_score=0.001,
                vote=0.0):
    """lib/model/test.py:95-102 + :162-180 on device.  batch = 1: (dets [max_out,6], count [1]).  batch = B: cls_prob
    [B*R,C] (R rows per image), num_rois [B] -> (dets [B,max_out,6], count [B]), one launch pair for all images.
    bbox_pred = None: cfg.TEST.BBOX_REG False (the rois themselves, un-regressed and un-clipped, test.py:103-105).
    soft = 0: hard per-class NMS (exactly the call it always made).  soft = 1 (linear) / 2 (Gaussian with `sigma`): Soft-NMS
    (frcnn_detect_post_soft_batched, csrc/softnms_math.h) -- a class's neighbours keep a decayed score, rows whose score falls below
    `min_score` are dropped, and the max_per_image cut sees the decayed scores.
    vote = 0: off (the calls above, untouched).  0 < vote <= 1: bounding-box voting (frcnn_detect_post_vote_batched, csrc/boxvote_math.h)
    between the per-class stage and the cut -- every kept box becomes the score-weighted mean of the class's candidates whose IoU with it
    is >= vote; scores, classes and order stay."""
    if soft not in (0, 1, 2):
        raise ValueError("detect_post: soft must be 0 (hard), 1 (linear) or 2 (Gaussian), got %r" % (soft,))
    if not (vote == 0 or 0.0 < vote <= 1.0):
        raise ValueError("detect_post: vote must be 0 (off) or a threshold in (0, 1], got %r" % (vote,))
    _chk(cls_prob), _chk(rois)
    if bbox_pred is not None:
        _chk(bbox_pred)
    B = int(batch)
    R, C = cls_prob.shape[0] // B, cls_prob.shape[1]
    if cls_prob.shape[0] != B * R or rois.shape[0] != B * R:
        raise ValueError("detect_post: %d rows do not split into %d images" % (cls_prob.shape[0], B))
    dev = cls_prob.device
    max_out = (max_per_image + 28 if max_per_image > 0 else R * (C - 1)) if max_out is None else max_out
    shape = (max_out, 6) if B == 1 else (B, max_out, 6)
    out = _empty(shape, dtype=torch.float32, device=dev) if out is None else out
    count = _zeros((B,), dtype=torch.int32, device=dev) if count is None else count
    # a batched record may be a strided view (per-image slices contiguous, frcnn_hip.parallel.new_record)
    if out.dtype != torch.float32 or out.shape[-1] != 6 or out.stride(-1) != 1 or out.stride(-2) != 6 or out.shape[-2] < max_out:
        raise ValueError("detect_post: `out` must be float32 [.., >=max_out, 6] with contiguous images")
    out_stride = out.stride(0) if out.dim() == 3 else 0
    nb = lib().frcnn_detect_post_batched_workspace_bytes(B, R, C)
    ws = workspace(nb, dev, "detect_post")
    # the three entries share their leading and trailing arguments; between them: nothing / the Soft-NMS triple / that and the vote threshold
    head = (_ptr(cls_prob), _ptr(bbox_pred), _ptr(rois), _ptr(num_rois), B, R, C, float(im_scale), int(im_h), int(im_w),
            float(nms_thresh), int(rule), float(score_thresh), int(max_per_image))
    tail = (_ptr(out), _ptr(count), int(max_out), int(out_stride), _ptr(ws), ws.numel(), _stream())
    soft_args = (int(soft), float(sigma), float(min_score))
    if vote:
        call("frcnn_detect_post_vote_batched", *head, *soft_args, float(vote), *tail)
    elif soft:
        call("frcnn_detect_post_soft_batched", *head, *soft_args, *tail)
    else:
        call("frcnn_detect_post_batched", *head, *tail)
    return out, count


SOFT_NMS_METHODS = {"linear": 1, "gaussian": 2}


def soft_nms(dets, nms_thresh=0.3, rule=NMS_RULE_CPU, method=1, sigma=0.5, min_score=0.001):
    """Soft-NMS of one class on the device (frcnn_soft_nms): dets f32 [k,5] = x1,y1,x2,y2,score, k <= 1024 -> (out [k,5]: the emitted
    rows in emission order with their decayed scores, the rest 0; index int32 [k]: their input rows, the rest -1; count int32 [1])."""
    _chk(dets)
    if dets.dim() != 2 or dets.shape[1] != 5:
        raise ValueError("soft_nms: dets must be [k,5]")
    k, dev = dets.shape[0], dets.device
    out = _empty((max(k, 1), 5), dtype=torch.float32, device=dev)
    index = _empty((max(k, 1),), dtype=torch.int32, device=dev)
    count = _zeros((1,), dtype=torch.int32, device=dev)
    call("frcnn_soft_nms", _ptr(dets if k else out), k, float(nms_thresh), int(rule), int(method), float(sigma), float(min_score), _ptr(out),
         _ptr(index), _ptr(count), _stream())
    return out[:k], index[:k], count


def soft_nms_host(dets, nms_thresh=0.3, rule=NMS_RULE_CPU, method=1, sigma=0.5, min_score=0.001):
    """frcnn_soft_nms_host: the same on a HOST numpy array, no GPU needed -> (out f32 [n,5], index int32 [n]) of the n emitted rows."""
    dets = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 5)
    k = dets.shape[0]
    out, index, count = np.zeros((max(k, 1), 5), dtype=np.float32), np.full(max(k, 1), -1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    check(lib().frcnn_soft_nms_host((dets if k else out).ctypes.data, k, float(nms_thresh), int(rule), int(method), float(sigma),
                                    float(min_score), out.ctypes.data, index.ctypes.data, count.ctypes.data), "frcnn_soft_nms_host")
    n = int(count[0])
    return out[:n], index[:n]


def box_vote(kept, cands, vote_thresh=0.8):
    """Bounding-box voting of one class on the device (frcnn_box_vote, csrc/boxvote_math.h): kept f32 [m,5], cands f32 [n,5] =
    x1,y1,x2,y2,score, m, n <= 1024 -> out [m,5]: every kept box replaced by the score-weighted mean of the candidates whose IoU with it
    is >= vote_thresh (sequential double sums in candidate order); scores and order as in `kept`."""
    _chk(kept), _chk(cands)
    if kept.dim() != 2 or kept.shape[1] != 5 or cands.dim() != 2 or cands.shape[1] != 5:
        raise ValueError("box_vote: kept and cands must be [m,5] and [n,5]")
    m, n, dev = kept.shape[0], cands.shape[0], kept.device
    out = _empty((max(m, 1), 5), dtype=torch.float32, device=dev)
    call("frcnn_box_vote", _ptr(kept if m else out), m, _ptr(cands if n else out), n, float(vote_thresh), _ptr(out), _stream())
    return out[:m]


def box_vote_host(kept, cands, vote_thresh=0.8):
    """frcnn_box_vote_host: the same on HOST numpy arrays, no GPU needed -> out f32 [m,5], the device's bits."""
    kept = np.ascontiguousarray(kept, dtype=np.float32).reshape(-1, 5)
    cands = np.ascontiguousarray(cands, dtype=np.float32).reshape(-1, 5)
    m, n = kept.shape[0], cands.shape[0]
    out = np.zeros((max(m, 1), 5), dtype=np.float32)
    check(lib().frcnn_box_vote_host((kept if m else out).ctypes.data, m, (cands if n else out).ctypes.data, n, float(vote_thresh),
                                    out.ctypes.data), "frcnn_box_vote_host")
    return out[:m]


def mirror_views(image, out=None):
    """The two views of the test-time flip ensemble (frcnn_mirror_views): prepared input [B,OH,OW,c] -> [2B,OH,OW,c], slot 2b image b as
    it is, slot 2b+1 its columns mirrored (an exact permutation)."""
    _chk(image)
    if image.dim() != 4:
        raise ValueError("mirror_views: image must be [B,OH,OW,c]")
    B, OH, OW, c = image.shape
    out = _empty((2 * B, OH, OW, c), dtype=torch.float32, device=image.device) if out is None else out
    if tuple(out.shape) != (2 * B, OH, OW, c) or out.dtype != torch.float32 or not out.is_contiguous() or out.data_ptr() == image.data_ptr():
        raise ValueError("mirror_views: `out` must be a float32 contiguous [2B,OH,OW,c] buffer of its own")
    call("frcnn_mirror_views", _ptr(image), B, OH, OW, c, _ptr(out), _stream())
    return out


def merge_flip_views(cls_prob, bbox_pred, rois, num_rois, im_w_scaled, batch=1, out=None):
    """The outputs of the 2B views of mirror_views as B images of 2R rows (frcnn_merge_flip_views): cls_prob [2B*R,C], bbox_pred
    [2B*R,4C] or None, rois [2B*R,5], num_rois int32 [2B] or None -> (cls_prob [B*2R,C], bbox_pred [B*2R,4C] or None, rois [B*2R,5],
    num_rois int32 [B]).  Per image: view 0's rows, then view 1's with their x mirrored back about the prepared width im_w_scaled
    (= im_info[1]) and dx negated, then zeros.  The counts are read on the device.  out = the four result buffers, to reuse them."""
    _chk(cls_prob), _chk(rois)
    if bbox_pred is not None:
        _chk(bbox_pred)
    B = int(batch)
    rows, C = cls_prob.shape
    R = rows // (2 * B)
    if rows != 2 * B * R or R == 0 or rois.shape[0] != rows or (bbox_pred is not None and tuple(bbox_pred.shape) != (rows, 4 * C)):
        raise ValueError("merge_flip_views: %d rows do not split into 2 views of %d images" % (rows, B))
    dev = cls_prob.device
    if out is None:
        out = (_empty((rows, C), dtype=torch.float32, device=dev),
               None if bbox_pred is None else _empty((rows, 4 * C), dtype=torch.float32, device=dev),
               _empty((rows, 5), dtype=torch.float32, device=dev), _empty((B,), dtype=torch.int32, device=dev))
    o_prob, o_pred, o_rois, o_num = out
    call("frcnn_merge_flip_views", _ptr(cls_prob), _ptr(bbox_pred), _ptr(rois), _ptr(num_rois), B, R, C, float(im_w_scaled), _ptr(o_prob),
         _ptr(o_pred if bbox_pred is not None else None), _ptr(o_rois), _ptr(o_num), _stream())
    return o_prob, (o_pred if bbox_pred is not None else None), o_rois, o_num


def merge_flip_views_host(cls_prob, bbox_pred, rois, num_rois, im_w_scaled, batch=1):
    """frcnn_merge_flip_views_host: merge_flip_views on HOST numpy arrays, no GPU needed."""
    cls_prob = np.ascontiguousarray(cls_prob, dtype=np.float32)
    rois = np.ascontiguousarray(rois, dtype=np.float32)
    bbox_pred = None if bbox_pred is None else np.ascontiguousarray(bbox_pred, dtype=np.float32)
    num_rois = None if num_rois is None else np.ascontiguousarray(num_rois, dtype=np.int32)
    B = int(batch)
    rows, C = cls_prob.shape
    R = rows // (2 * B)
    if rows != 2 * B * R or R == 0 or rois.shape != (rows, 5) or (bbox_pred is not None and bbox_pred.shape != (rows, 4 * C)) or \
            (num_rois is not None and num_rois.shape != (2 * B,)):
        raise ValueError("merge_flip_views_host: %d rows do not split into 2 views of %d images" % (rows, B))
    o_prob, o_rois, o_num = np.empty((rows, C), np.float32), np.empty((rows, 5), np.float32), np.empty((B,), np.int32)
    o_pred = None if bbox_pred is None else np.empty((rows, 4 * C), np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    check(lib().frcnn_merge_flip_views_host(p(cls_prob), p(bbox_pred), p(rois), p(num_rois), B, R, C, float(im_w_scaled), p(o_prob),
                                            p(o_pred), p(o_rois), p(o_num)), "frcnn_merge_flip_views_host")
    return o_prob, o_pred, o_rois, o_num


def im_detect_boxes(rois, bbox_pred, im_scale, im_h, im_w, num_classes=None):
    """lib/model/test.py:95-105 on device: -> pred_boxes [R,4C].  bbox_pred = None (cfg.TEST.BBOX_REG False): np.tile(boxes, (1, C))."""
    _chk(rois)
    if bbox_pred is None:
        R, C4 = rois.shape[0], 4 * int(num_classes)
    else:
        _chk(bbox_pred)
        R, C4 = bbox_pred.shape
    out = _empty((R, C4), dtype=torch.float32, device=rois.device)
    call("frcnn_im_detect_boxes", _ptr(rois), _ptr(bbox_pred), R, C4 // 4, float(im_scale), int(im_h), int(im_w), _ptr(out),
         _stream())
    return out


# ------------------------------------------------------------------------------------------ dense
def pack_filter_hwio(w_hwio, scale=None):
    """HOST numpy HWIO -> packed [Cout][KH][KW][Cin] (folding a per-output-channel scale)."""
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    KH, KW, Cin, Cout = w.shape
    out = np.empty((Cout, KH, KW, Cin), dtype=np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    call("frcnn_pack_filter_hwio", w.ctypes.data_as(ctypes.c_void_p), KH, KW, Cin, Cout,
         None if sc is None else sc.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out


def pack_filter_foldw(w_hwio, scale=None):
    """HOST: stem filter HWIO [KH,KW<=8,Cin<=4,Cout] -> [Cout][KH][8][4] (zero padded) for the
    fold_w mode of frcnn_conv2d_nhwc: the kw taps become part of the contiguous channel run of the
    4-channel-padded image, so the 7x7x3 stem runs on the MFMA pipe with K = KH*32."""
    w = np.asarray(w_hwio, dtype=np.float32)
    KH, KW, Cin, Cout = w.shape
    assert KW <= 8 and Cin <= 4
    if scale is not None:
        w = w * np.asarray(scale, dtype=np.float32)[None, None, None, :]
    out = np.zeros((Cout, KH, 8, 4), dtype=np.float32)
    out[:, :, :KW, :Cin] = np.transpose(w, (3, 0, 1, 2))
    return out


def conv_out_size(n, k, stride, pad_lo, pad_hi):
    return (n + pad_lo + pad_hi - k) // stride + 1


split_k = True      # module switch: allow split-K launches (frcnn_conv2d_nhwc_ws) where the library's plan asks for them


def conv2d(x, w_packed, bias, KH, KW, stride=1, pad=(0, 0, 0, 0), act=ACT_NONE, residual=None, res_stride=1,
           fold_w=False, out=None, mask=None):
    """x [N,H,W,Cin]; w_packed [Cout,KH,KW,Cin] (fold_w: [Cout,KH,8,4]); pad = (top, bottom, left, right).
    mask (training, a float32 tensor of the result's shape): out = mask > 0 ? out : 0 inside the launch (frcnn_conv2d_nhwc_masked_ws)."""
    _chk(x), _chk(w_packed)
    N, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    OH = conv_out_size(H, KH, stride, pad[0], pad[1])
    OW = conv_out_size(W, KW, stride, pad[2], pad[3])
    out = _empty((N, OH, OW, Cout), dtype=torch.float32, device=x.device) if out is None else out
    RH = RW = 0
    if residual is not None:
        _chk(residual)
        RH, RW = residual.shape[1], residual.shape[2]
    nb = lib().frcnn_conv2d_workspace_bytes(N, OH, OW, Cout, KH, KW, Cin, 1 if fold_w else 0) if split_k else 0
    if mask is not None:
        _chk(mask)
        assert not fold_w and mask.numel() == out.numel()
        ws = workspace(nb, x.device, "conv_splitk") if nb else None
        call("frcnn_conv2d_nhwc_masked_ws", _ptr(x), N, H, W, Cin, _ptr(w_packed), _ptr(bias), _ptr(residual), RH, RW,
             int(res_stride), _ptr(out), OH, OW, Cout, KH, KW, int(stride), int(pad[0]), int(pad[2]), int(act), _ptr(mask),
             _ptr(ws), ws.numel() if nb else 0, _stream())
        return out
    if nb:                                  # under-filled launch: split-K through a per-chain scratch buffer
        ws = workspace(nb, x.device, "conv_splitk")
        call("frcnn_conv2d_nhwc_ws", _ptr(x), N, H, W, Cin, _ptr(w_packed), _ptr(bias), _ptr(residual), RH, RW,
             int(res_stride), _ptr(out), OH, OW, Cout, KH, KW, int(stride), int(pad[0]), int(pad[2]), int(act),
             1 if fold_w else 0, _ptr(ws), ws.numel(), _stream())
        return out
    call("frcnn_conv2d_nhwc", _ptr(x), N, H, W, Cin, _ptr(w_packed), _ptr(bias), _ptr(residual), RH, RW,
         int(res_stride), _ptr(out), OH, OW, Cout, KH, KW, int(stride), int(pad[0]), int(pad[2]), int(act),
         1 if fold_w else 0, _stream())
    return out


def prep_image_shape(h, w, target_size, max_size):
    """HOST: (im_scale, OH, OW) of _get_image_blob / prep_im_for_blob for an h x w image."""
    sc, oh, ow = ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
    call("frcnn_prep_image_shape", int(h), int(w), int(target_size), int(max_size), ctypes.byref(sc), ctypes.byref(oh),
         ctypes.byref(ow))
    return sc.value, oh.value, ow.value


def prep_image(im_d, pixel_means, im_scale, out_hw, out=None, out_c=4):
    """im_d: BGR uint8 or float32 [h,w,3] on device -> float32 [1,OH,OW,out_c] = resize(im - PIXEL_MEANS) (cv2 INTER_LINEAR)."""
    assert im_d.is_cuda and im_d.is_contiguous() and im_d.dim() == 3 and im_d.shape[2] == 3
    assert im_d.dtype in (torch.uint8, torch.float32)
    h, w = im_d.shape[:2]
    OH, OW = out_hw
    out = _empty((1, OH, OW, out_c), dtype=torch.float32, device=im_d.device) if out is None else out
    assert out.shape == (1, OH, OW, out_c)
    means = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pixel_means, dtype=np.float64).reshape(-1)[:3]])
    call("frcnn_prep_image", _ptr(im_d), 1 if im_d.dtype == torch.float32 else 0, h, w, means, float(im_scale), _ptr(out), OH, OW,
         int(out_c), _stream())
    return out


def prep_image_batched(ims_d, pixel_means, im_scale, out_hw, out=None, out_c=4):
    """ims_d: B same-size BGR images, uint8 or float32 [B,h,w,3] on device -> float32 [B,OH,OW,out_c] in one launch; slot b holds the bits
    of prep_image(ims_d[b])."""
    assert ims_d.is_cuda and ims_d.is_contiguous() and ims_d.dim() == 4 and ims_d.shape[3] == 3 and ims_d.shape[0] >= 1
    assert ims_d.dtype in (torch.uint8, torch.float32)
    B, h, w = ims_d.shape[:3]
    OH, OW = out_hw
    out = _empty((B, OH, OW, out_c), dtype=torch.float32, device=ims_d.device) if out is None else out
    assert out.shape == (B, OH, OW, out_c) and out.is_contiguous() and out.dtype == torch.float32
    means = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pixel_means, dtype=np.float64).reshape(-1)[:3]])
    call("frcnn_prep_image_batched", _ptr(ims_d), 1 if ims_d.dtype == torch.float32 else 0, B, h, w, means, float(im_scale), _ptr(out), OH,
         OW, int(out_c), _stream())
    return out


def prep_train_image(im_d, flipped, pixel_means, im_scale, out_hw, out=None, out_c=4, boxes=None, classes=None, gt_out=None):
    """One roidb entry's minibatch on device (roi_data_layer/minibatch.py): prep_image of the image mirrored first iff `flipped`, and --
    boxes uint16 [G,4] / classes int32 [G] / gt_out float32 [>=G,5] given -- gt_out[:G] = (boxes * im_scale, classes)."""
    assert im_d.is_cuda and im_d.is_contiguous() and im_d.dim() == 3 and im_d.shape[2] == 3
    assert im_d.dtype in (torch.uint8, torch.float32)
    h, w = im_d.shape[:2]
    OH, OW = out_hw
    out = _empty((1, OH, OW, out_c), dtype=torch.float32, device=im_d.device) if out is None else out
    assert out.shape == (1, OH, OW, out_c) and out.is_contiguous() and out.dtype == torch.float32
    G = 0 if boxes is None else int(boxes.shape[0])
    if G:
        assert boxes.dtype == torch.uint16 and boxes.shape == (G, 4) and boxes.is_cuda and boxes.is_contiguous()
        assert classes.dtype == torch.int32 and classes.shape == (G,) and classes.is_cuda and classes.is_contiguous()
        assert gt_out.dtype == torch.float32 and gt_out.dim() == 2 and gt_out.shape[0] >= G and gt_out.shape[1] == 5 and gt_out.is_contiguous()
    means = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pixel_means, dtype=np.float64).reshape(-1)[:3]])
    call("frcnn_prep_train_image", _ptr(im_d), 1 if im_d.dtype == torch.float32 else 0, h, w, 1 if flipped else 0, means, float(im_scale),
         _ptr(out), OH, OW, int(out_c), _ptr(boxes if G else None), _ptr(classes if G else None), G, _ptr(gt_out if G else None), _stream())
    return out


# ---- baseline JPEG decode: host Huffman stage, device IDCT + colour (csrc/jpeg_host.h, csrc/jpeg_decode.hip) ---------------------------
JPEG_OK, JPEG_E_ARG, JPEG_E_UNSUPPORTED = 0, -1, -3


class JpegError(_binding.FrcnnHipError):
    """rc = JPEG_E_UNSUPPORTED (a stream outside the decoder's list, or no JPEG at all) or JPEG_E_ARG (a damaged stream)."""

    def __init__(self, what, rc):
        _binding.FrcnnHipError.__init__(self, "%s: %s" % (what, {JPEG_E_ARG: "damaged stream or bad argument",
                                                                 JPEG_E_UNSUPPORTED: "not a supported baseline JPEG"}.get(rc, "error %d" % rc)))
        self.rc = rc


def _jpeg_bytes(data):
    """bytes-like -> (object that keeps the memory alive, address, length) without a copy for bytes / numpy uint8"""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data, dtype=np.uint8)
        return a, a.ctypes.data, a.size
    data = bytes(data) if not isinstance(data, bytes) else data
    return data, ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, len(data)


def jpeg_info(data):
    """HOST: geometry (width, height, ncomp, hs, vs, restart_interval, sof, 0) of a supported stream; JpegError otherwise."""
    keep, addr, n = _jpeg_bytes(data)
    out = (ctypes.c_int * 8)()
    rc = lib().frcnn_jpeg_info(addr, n, out)
    if rc != 0:
        raise JpegError("frcnn_jpeg_info", rc)
    return tuple(out)


def jpeg_coef_bytes(geom):
    return int(lib().frcnn_jpeg_coef_bytes(*[int(v) for v in geom[:5]]))


def jpeg_entropy_decode(data, out=None, geom=None):
    """HOST: the Huffman stage -> the coefficient buffer as a host uint8 tensor (its first jpeg_coef_bytes(geom) bytes when `out`, e.g. a
    pinned ring slot, is larger).  ctypes releases the GIL for the call, so several threads decode side by side."""
    keep, addr, n = _jpeg_bytes(data)
    geom = jpeg_info(data) if geom is None else geom
    nbytes = jpeg_coef_bytes(geom)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and not out.is_cuda
    rc = lib().frcnn_jpeg_entropy_decode(addr, n, out.data_ptr(), out.numel())
    if rc != 0:
        raise JpegError("frcnn_jpeg_entropy_decode", rc)
    return out[:nbytes]


def jpeg_pixels_host(coef, geom):
    """HOST statement of jpeg_pixels: coefficient buffer -> BGR uint8 numpy [h,w,3] (the arithmetic header the kernels compile)."""
    w, h = int(geom[0]), int(geom[1])
    assert not coef.is_cuda and coef.dtype == torch.uint8 and coef.is_contiguous() and coef.numel() >= jpeg_coef_bytes(geom)
    out = np.empty((h, w, 3), dtype=np.uint8)
    rc = lib().frcnn_jpeg_pixels_host(coef.data_ptr(), w, h, int(geom[2]), int(geom[3]), int(geom[4]), out.ctypes.data)
    if rc != 0:
        raise JpegError("frcnn_jpeg_pixels_host", rc)
    return out


def jpeg_pixels(coef_d, geom, out=None):
    """coef_d: the coefficient buffer on the device (uint8) -> BGR uint8 [h,w,3] on the device: IDCT into sample planes, then chroma
    upsampling + colour conversion, on the current stream."""
    w, h = int(geom[0]), int(geom[1])
    assert coef_d.is_cuda and coef_d.dtype == torch.uint8 and coef_d.is_contiguous() and coef_d.numel() >= jpeg_coef_bytes(geom)
    out = _empty((h, w, 3), dtype=torch.uint8, device=coef_d.device) if out is None else out
    assert out.shape == (h, w, 3) and out.dtype == torch.uint8 and out.is_contiguous() and out.is_cuda
    ws = workspace(int(lib().frcnn_jpeg_workspace_bytes(w, h, int(geom[2]), int(geom[3]), int(geom[4]))), coef_d.device, tag="jpeg")
    call("frcnn_jpeg_pixels", _ptr(coef_d), w, h, int(geom[2]), int(geom[3]), int(geom[4]), _ptr(out), _ptr(ws), ws.numel(), _stream())
    return out


# ---- baseline JPEG encode, the mirror: device colour + downsampling + DCT, host Huffman stage (csrc/jpeg_encode.hip, csrc/jpeg_encode_host.h)
JPEG_SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}            # PIL's `subsampling` -> luma (hs, vs)


def jpeg_encode_geom(h, w, subsampling=2):
    """(width, height, 3, hs, vs): the geometry tuple of a BGR [h,w,3] image encoded at PIL's `subsampling` 0 / 1 / 2"""
    hs, vs = JPEG_SAMPLING[int(subsampling)]
    return (int(w), int(h), 3, hs, vs)


def jpeg_quant_tables(quality):
    """HOST: uint16 [2,64], luminance then chrominance in natural order, libjpeg's scaling of the Annex K tables"""
    out = np.empty((2, 64), dtype=np.uint16)
    check(lib().frcnn_jpeg_quant_tables(int(quality), out.ctypes.data), "frcnn_jpeg_quant_tables")
    return out


def _coef_geom(geom):
    n = jpeg_coef_bytes(geom)
    if n == 0:
        raise JpegError("frcnn_jpeg_coef_bytes", JPEG_E_UNSUPPORTED)
    return n


def jpeg_coefs_host(im, quality=90, subsampling=2, out=None):
    """HOST statement of jpeg_coefs: BGR uint8 [h,w,3] (numpy or CPU tensor) -> the coefficient buffer, a host uint8 tensor."""
    a = np.ascontiguousarray(im.numpy() if torch.is_tensor(im) else im, dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3
    geom = jpeg_encode_geom(a.shape[0], a.shape[1], subsampling)
    n = _coef_geom(geom)
    out = torch.empty(n, dtype=torch.uint8) if out is None else out
    assert out.dtype == torch.uint8 and out.is_contiguous() and not out.is_cuda and out.numel() >= n
    rc = lib().frcnn_jpeg_coefs_host(a.ctypes.data, geom[0], geom[1], geom[3], geom[4], int(quality), out.data_ptr())
    if rc != 0:
        raise JpegError("frcnn_jpeg_coefs_host", rc)
    return out[:n]


def jpeg_coefs(im_d, quality=90, subsampling=2, out=None):
    """BGR uint8 [h,w,3] on the device -> the coefficient buffer on the device (uint8; `out`: at least jpeg_coef_bytes bytes at an even
    address), two launches on the current stream."""
    assert im_d.is_cuda and im_d.dtype == torch.uint8 and im_d.is_contiguous() and im_d.dim() == 3 and im_d.shape[2] == 3
    geom = jpeg_encode_geom(im_d.shape[0], im_d.shape[1], subsampling)
    n = _coef_geom(geom)
    out = _empty((n,), dtype=torch.uint8, device=im_d.device) if out is None else out
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n
    ws = workspace(int(lib().frcnn_jpeg_workspace_bytes(*geom)), im_d.device, tag="jpeg_enc")
    call("frcnn_jpeg_coefs", _ptr(im_d), geom[0], geom[1], geom[3], geom[4], int(quality), _ptr(out), _ptr(ws), ws.numel(), _stream())
    return out[:n]


def jpeg_stream_bound(geom):
    return int(lib().frcnn_jpeg_stream_bound(int(geom[0]), int(geom[1]), int(geom[3]), int(geom[4])))


def jpeg_entropy_encode(coef, geom, out=None):
    """HOST: the Huffman stage of the encoder, coefficient buffer (host uint8 tensor) -> the bytes of a complete baseline JPEG file.  `out`: a
    numpy uint8 scratch array of at least jpeg_stream_bound(geom) bytes (e.g. one per worker thread).  ctypes releases the GIL for the call."""
    assert not coef.is_cuda and coef.dtype == torch.uint8 and coef.is_contiguous() and coef.numel() >= _coef_geom(geom)
    cap = jpeg_stream_bound(geom)
    out = np.empty(cap, dtype=np.uint8) if out is None else out
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= cap
    n = lib().frcnn_jpeg_entropy_encode(coef.data_ptr(), int(geom[0]), int(geom[1]), int(geom[3]), int(geom[4]), out.ctypes.data, out.size)
    if n < 0:
        raise JpegError("frcnn_jpeg_entropy_encode", int(n))
    return out[:n].tobytes()


# ---- detections drawn on the image (csrc/draw_math.h, csrc/draw.hip) ------------------------------------------------------------------
def _draw_tables_ok(colours, labels, glyphs):
    assert colours.dtype == torch.uint8 and colours.dim() == 2 and colours.shape[1] == 3 and colours.is_contiguous()
    assert labels.dtype == torch.uint8 and labels.dim() == 2 and labels.is_contiguous()
    assert glyphs.dtype == torch.uint8 and tuple(glyphs.shape) == (95, 7) and glyphs.is_contiguous()


def draw_detections(im_d, dets_d, cnt_d, conf, thickness, scale, colours_d, labels_d, glyphs_d):
    """In place on im_d (BGR uint8 [h,w,3], device): the records dets_d [max_dets,6] and their device-resident count cnt_d [1] int32, as
    detect_post leaves them.  colours_d [n,3] BGR, labels_d [num_classes,stride] NUL-padded names, glyphs_d [95,7]: uint8 device tensors."""
    assert im_d.is_cuda and im_d.dtype == torch.uint8 and im_d.is_contiguous() and im_d.dim() == 3 and im_d.shape[2] == 3
    assert dets_d.is_cuda and dets_d.dtype == torch.float32 and dets_d.dim() == 2 and dets_d.shape[1] == 6 and dets_d.is_contiguous()
    assert cnt_d.is_cuda and cnt_d.dtype == torch.int32 and cnt_d.numel() >= 1
    _draw_tables_ok(colours_d, labels_d, glyphs_d)
    assert colours_d.is_cuda and labels_d.is_cuda and glyphs_d.is_cuda
    call("frcnn_draw_detections", _ptr(im_d), int(im_d.shape[0]), int(im_d.shape[1]), _ptr(dets_d), _ptr(cnt_d), int(dets_d.shape[0]),
         float(conf), int(thickness), int(scale), _ptr(colours_d), int(colours_d.shape[0]), _ptr(labels_d), int(labels_d.shape[0]),
         int(labels_d.shape[1]), _ptr(glyphs_d), _stream())
    return im_d


def draw_detections_host(im, dets, count, conf, thickness, scale, colours, labels, glyphs):
    """HOST statement of draw_detections, in place on the numpy uint8 [h,w,3] image `im`; dets float32 [max_dets,6] numpy, count an int;
    the tables CPU uint8 tensors."""
    assert isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.flags["C_CONTIGUOUS"]
    dets = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
    _draw_tables_ok(colours, labels, glyphs)
    assert not (colours.is_cuda or labels.is_cuda or glyphs.is_cuda)
    check(lib().frcnn_draw_detections_host(im.ctypes.data, im.shape[0], im.shape[1], dets.ctypes.data, int(count), dets.shape[0], float(conf),
                                           int(thickness), int(scale), colours.data_ptr(), colours.shape[0], labels.data_ptr(),
                                           labels.shape[0], labels.shape[1], glyphs.data_ptr()), "frcnn_draw_detections_host")
    return im


def winograd_filter_transform(w_hwio, scale=None, m=2):
    """HOST: 3x3 HWIO filter -> U [(m+2)^2, Cout, Cin] (F(m x m,3x3), optional folded per-output scale)."""
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    assert w.shape[0] == 3 and w.shape[1] == 3
    Cin, Cout = w.shape[2], w.shape[3]
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    if m == 7:                               # the mixed F(4,3)+F(3,3) scheme for 7x7 maps: 121 points
        out = np.empty((121, Cout, Cin), dtype=np.float32)
        call("frcnn_winograd7_filter_transform", w.ctypes.data_as(ctypes.c_void_p), Cin, Cout,
             None if sc is None else sc.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        return out
    out = np.empty(((m + 2) ** 2, Cout, Cin), dtype=np.float32)
    call("frcnn_winograd_filter_transform", w.ctypes.data_as(ctypes.c_void_p), Cin, Cout,
         None if sc is None else sc.ctypes.data_as(ctypes.c_void_p), int(m), out.ctypes.data_as(ctypes.c_void_p))
    return out


def winograd_filter_transform_device(w_packed, m=4, transpose_flip=False, out=None):
    """Packed filter [Cout,3,3,Cin] on device -> U [(m+2)^2,Cout,Cin] (or, transpose_flip, the dgrad filter [(m+2)^2,Cin,Cout])."""
    _chk(w_packed)
    O, kh, kw, C = w_packed.shape
    assert kh == 3 and kw == 3
    G = winograd_points(m)
    shape = (G, C, O) if transpose_flip else (G, O, C)
    out = _empty(shape, dtype=torch.float32, device=w_packed.device) if out is None else out
    assert out.numel() == G * O * C
    if m == 7:
        call("frcnn_winograd7_filter_transform_device", _ptr(w_packed), O, C, 1 if transpose_flip else 0, _ptr(out), _stream())
    else:
        call("frcnn_winograd_filter_transform_device", _ptr(w_packed), O, C, int(m), 1 if transpose_flip else 0, _ptr(out), _stream())
    return out.view(shape)


def winograd_points(m):
    """GEMMs per layer: (m+2)^2 for F(m x m,3x3); 121 for the mixed 7x7 scheme (m == 7)."""
    return 121 if m == 7 else (m + 2) ** 2


def winograd_tiles(N, H, W, m):
    if m == 7:
        assert H == 7 and W == 7
        return N
    return N * ((H + m - 1) // m) * ((W + m - 1) // m)


def winograd_input_transform(x, v, m=2):
    _chk(x), _chk(v)
    N, H, W, C = x.shape
    assert v.numel() == winograd_points(m) * winograd_tiles(N, H, W, m) * C
    if m == 7:
        call("frcnn_winograd7_input_transform", _ptr(x), N, C, _ptr(v), _stream())
    else:
        call("frcnn_winograd_input_transform", _ptr(x), N, H, W, C, int(m), _ptr(v), _stream())
    return v


def gemm_batched_nt(x, w, y):
    """y[g] = x[g] @ w[g]^T for x [G,M,K], w [G,N,K], y [G,M,N] in one launch of the f32-MFMA kernel."""
    _chk(x), _chk(w), _chk(y)
    G, M, K = x.shape
    N = w.shape[1]
    assert w.shape == (G, N, K) and y.shape == (G, M, N)
    call("frcnn_gemm_batched_nt", _ptr(x), _ptr(w), _ptr(y), G, M, N, K, _stream())
    return y


def winograd_output_transform(mm, bias, act, out, m=2):
    _chk(mm), _chk(out)
    N, H, W, C = out.shape
    assert mm.numel() == winograd_points(m) * winograd_tiles(N, H, W, m) * C
    if m == 7:
        call("frcnn_winograd7_output_transform", _ptr(mm), N, C, _ptr(bias), int(act), _ptr(out), _stream())
    else:
        call("frcnn_winograd_output_transform", _ptr(mm), N, H, W, C, int(m), _ptr(bias), int(act), _ptr(out), _stream())
    return out


def winograd2_conv_x3(x, planes, bias, act, out):
    """out = act(conv3x3(x, stride 1, SAME) + bias) for x, out [N,H,W,64] as F(2x2,3x3) in one launch (frcnn_winograd2_conv_x3);
    planes = gemm_x3_pack(U [16,64,64]) of the m = 2 filter transform.  Bit for bit winograd_input_transform -> gemm_x3 ->
    winograd_output_transform."""
    N, H, W, C = x.shape
    if C != 64 or tuple(out.shape) != (N, H, W, 64) or planes.numel() * planes.element_size() != 16 * 3 * 64 * 64 * 2:
        check(-3, "frcnn_winograd2_conv_x3")            # FRCNN_E_UNSUPPORTED: the entry takes no channel count, so it is refused here
    _chk(x), _chk(out)
    call("frcnn_winograd2_conv_x3", _ptr(x), N, H, W, _ptr(planes), _ptr(bias), int(act), _ptr(out), _stream())
    return out


def winograd_output_transform_masked(mm, mask, out, m, out_planes=None):
    """Training: out = mask > 0 ? A^T M A : 0 (no bias, no activation) as float32 `out` [N,H,W,C] and, with `out_planes` (an H2 of
    [N*H*W, C]), as the operand planes of the next data-gradient GEMM too.  m in (4, 7)."""
    _chk(mm), _chk(mask), _chk(out)
    N, H, W, C = out.shape
    assert mm.numel() == winograd_points(m) * winograd_tiles(N, H, W, m) * C and mask.numel() == out.numel()
    if out_planes is not None:
        assert isinstance(out_planes, H2) and out_planes.rows == N * H * W and out_planes.K == C
    pl, inv = (None, None) if out_planes is None else (out_planes.planes, out_planes.inv)
    if m == 7:
        call("frcnn_winograd7_output_transform_masked", _ptr(mm), N, C, _ptr(mask), _ptr(out), _ptr(pl), _ptr(inv), _stream())
    else:
        call("frcnn_winograd_output_transform_masked", _ptr(mm), N, H, W, C, int(m), _ptr(mask), _ptr(out), _ptr(pl), _ptr(inv), _stream())
    return out


def conv3x3_winograd(x, u, bias, act=ACT_NONE, out=None, v_buf=None, m_buf=None, u_planes=None, v_planes=None, mask=None, out_planes=None):
    """3x3 / stride 1 / pad 1 convolution as Winograd F(m x m,3x3): x [N,H,W,Cin], u [(m+2)^2,Cout,Cin] -> [N,H,W,Cout].
    u_planes = h2_pack_w(u) and v_planes (an H2 of [points * tiles, Cin]): the input transform emits V as operand planes and the
    products run in frcnn_gemm_h2 instead of the f32-MFMA batched GEMM.
    mask / out_planes (training, m in (4, 7), no bias / activation): winograd_output_transform_masked."""
    N, H, W, Cin = x.shape
    G, Cout = u.shape[0], u.shape[1]
    m = {16: 2, 36: 4, 121: 7}[G]
    T = winograd_tiles(N, H, W, m)
    dev = x.device
    mm = _empty((G, T, Cout), dtype=torch.float32, device=dev) if m_buf is None else m_buf
    out = _empty((N, H, W, Cout), dtype=torch.float32, device=dev) if out is None else out
    if u_planes is not None:
        v_planes = H2.empty(G * T, Cin, dev) if v_planes is None else v_planes
        winograd_input_transform_h2(x, v_planes, m)
        gemm_h2(v_planes, u_planes, G, T, Cout, Cin, out=mm.view(G * T, Cout))
    else:
        v = _empty((G, T, Cin), dtype=torch.float32, device=dev) if v_buf is None else v_buf
        winograd_input_transform(x, v, m)
        gemm_batched_nt(v, u, mm)
    if mask is not None:
        assert bias is None and act == ACT_NONE
        return winograd_output_transform_masked(mm, mask, out, m, out_planes)
    if out_planes is not None:              # float32 result + the operand planes of the convolution that follows (training forward)
        winograd_output_transform_h2(mm, bias, act, tuple(out.shape), m, out_planes, out)
        return out
    return winograd_output_transform(mm, bias, act, out, m)


def maxpool(x, k, stride, pad=(0, 0, 0, 0), out=None):
    _chk(x)
    N, H, W, C = x.shape
    OH = conv_out_size(H, k, stride, pad[0], pad[1])
    OW = conv_out_size(W, k, stride, pad[2], pad[3])
    out = _empty((N, OH, OW, C), dtype=torch.float32, device=x.device) if out is None else out
    call("frcnn_maxpool_nhwc", _ptr(x), N, H, W, C, int(k), int(stride), int(pad[0]), int(pad[2]), _ptr(out), OH, OW,
         _stream())
    return out


def dwconv3x3(x, w, bias, stride=1, pad=(1, 1, 1, 1), act=ACT_NONE, out=None, out_planes=None, want_f32=True):
    """Depthwise 3x3 (+ folded BN bias, activation).  out_planes: an H2 of [N*OH*OW, C] that receives the result as frcnn_gemm_h2
    operand planes (frcnn_dwconv3x3_nhwc_h2); want_f32 = False then skips the float32 tensor (returns None for it)."""
    _chk(x), _chk(w)
    N, H, W, C = x.shape
    OH = conv_out_size(H, 3, stride, pad[0], pad[1])
    OW = conv_out_size(W, 3, stride, pad[2], pad[3])
    if out_planes is None:
        out = _empty((N, OH, OW, C), dtype=torch.float32, device=x.device) if out is None else out
        call("frcnn_dwconv3x3_nhwc", _ptr(x), N, H, W, C, _ptr(w), _ptr(bias), _ptr(out), OH, OW, int(stride),
             int(pad[0]), int(pad[2]), int(act), _stream())
        return out
    assert isinstance(out_planes, H2) and out_planes.rows == N * OH * OW and out_planes.K == C
    if want_f32 and out is None:
        out = _empty((N, OH, OW, C), dtype=torch.float32, device=x.device)
    call("frcnn_dwconv3x3_nhwc_h2", _ptr(x), N, H, W, C, _ptr(w), _ptr(bias), _ptr(out if want_f32 else None), _ptr(out_planes.planes),
         _ptr(out_planes.inv), OH, OW, int(stride), int(pad[0]), int(pad[2]), int(act), _stream())
    return out if want_f32 else None


def spatial_mean(x, out=None):
    _chk(x)
    N, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * C)
    out = _empty((N, C), dtype=torch.float32, device=x.device) if out is None else out
    call("frcnn_spatial_mean", _ptr(x), N, HW, C, _ptr(out), _stream())
    return out


def softmax_rows(x, C=None, out=None):
    _chk(x)
    R, ld = x.shape
    C = ld if C is None else C
    out = _empty((R, C), dtype=torch.float32, device=x.device) if out is None else out
    call("frcnn_softmax_rows", _ptr(x), R, C, ld, _ptr(out), _stream())
    return out


def rpn_softmax(score, A, out=None):
    """score [1,H,W,ld] (first 2A channels = bg|fg scores) -> prob [1,H,W,2A]."""
    _chk(score)
    N, H, W, ld = score.shape
    out = _empty((N, H, W, 2 * A), dtype=torch.float32, device=score.device) if out is None else out
    call("frcnn_rpn_softmax", _ptr(score), N * H * W, A, ld, _ptr(out), _stream())
    return out


def copy_cols(src, col0, cols, out=None):
    _chk(src)
    ld = src.shape[-1]
    R = src.numel() // ld
    out = _empty(tuple(src.shape[:-1]) + (cols,), dtype=torch.float32, device=src.device) if out is None else out
    call("frcnn_copy_cols", _ptr(src), R, ld, int(col0), int(cols), _ptr(out), cols, _stream())
    return out


# ------------------------------------------------------------------------------------------ training
def _host_doubles(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    if _binding.recorder is not None:
        _binding.recorder.keep.append(a)         # (a recorded launch keeps the pointer)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def rpn_target_opts(clobber_positives=False, positive_weight=-1.0, inside_weights=(1.0, 1.0, 1.0, 1.0)):
    """opts block of frcnn_anchor_target_layer*: TRAIN.RPN_CLOBBER_POSITIVES, TRAIN.RPN_POSITIVE_WEIGHT, TRAIN.RPN_BBOX_INSIDE_WEIGHTS."""
    return [1.0 if clobber_positives else 0.0, float(positive_weight)] + [float(v) for v in inside_weights]


def roi_target_opts(use_gt=False, inside_weights=(1.0, 1.0, 1.0, 1.0)):
    """opts block of frcnn_proposal_target_layer*: TRAIN.USE_GT, TRAIN.BBOX_INSIDE_WEIGHTS."""
    return [1.0 if use_gt else 0.0] + [float(v) for v in inside_weights]


def anchor_target_layer(gt_boxes, im_h, im_w, H, W, base_d, feat_stride=16, rpn_batchsize=256, fg_fraction=0.5,
                        pos_overlap=0.7, neg_overlap=0.3, seed=0, opts=None):
    """lib/layer_utils/anchor_target_layer.py:18-138 on device -> (labels [1,1,A*H,W], targets, inside, outside [1,H,W,4A]).
    opts: rpn_target_opts(...) or None (reference defaults)."""
    _chk(gt_boxes), _chk(base_d, torch.float64)
    A, G, dev = base_d.shape[0], gt_boxes.shape[0], gt_boxes.device
    labels = _empty((1, 1, A * H, W), dtype=torch.float32, device=dev)
    tg, iw, ow = (_empty((1, H, W, 4 * A), dtype=torch.float32, device=dev) for _ in range(3))
    # (sized for every box count the tensor's storage can hold: a recorded step is replayed with the next image's G)
    Gcap = max(G, (gt_boxes.untyped_storage().nbytes() - 4 * gt_boxes.storage_offset()) // 20)
    ws = workspace(lib().frcnn_anchor_target_workspace_bytes(H, W, A, Gcap), dev, "anchor_target")
    o = _host_doubles(opts) if opts is not None else (None, None)
    call("frcnn_anchor_target_layer", _ptr(gt_boxes), G, float(im_h), float(im_w), H, W, A, int(feat_stride), _ptr(base_d),
         int(rpn_batchsize), float(fg_fraction), float(pos_overlap), float(neg_overlap), int(seed), o[1], _ptr(labels), _ptr(tg),
         _ptr(iw), _ptr(ow), _ptr(ws), ws.numel(), _stream())
    if _binding.recorder is not None:
        _binding.recorder.patch_last(1, var="gt")    # the image's box count (gt_boxes: the first G rows of a static buffer)
        if int(seed) >= 0:
            _binding.recorder.patch_last(13)         # the sampling seed advances with the step (Network._sample_seed)
    return labels, tg, iw, ow


def anchor_target_layer_inject(gt_boxes, im_h, im_w, H, W, base_d, disable, feat_stride=16, rpn_batchsize=256, fg_fraction=0.5,
                               pos_overlap=0.7, neg_overlap=0.3, opts=None):
    """anchor_target_layer with the reference's host-drawn `disable_inds` (int32 device tensor of ALL-anchor indices, may be
    empty): see frcnn_anchor_target_layer_inject."""
    _chk(gt_boxes), _chk(base_d, torch.float64), _chk(disable, torch.int32)
    A, G, dev = base_d.shape[0], gt_boxes.shape[0], gt_boxes.device
    labels = _empty((1, 1, A * H, W), dtype=torch.float32, device=dev)
    tg, iw, ow = (_empty((1, H, W, 4 * A), dtype=torch.float32, device=dev) for _ in range(3))
    ws = workspace(lib().frcnn_anchor_target_workspace_bytes(H, W, A, G), dev, "anchor_target")
    o = _host_doubles(opts) if opts is not None else (None, None)
    call("frcnn_anchor_target_layer_inject", _ptr(gt_boxes), G, float(im_h), float(im_w), H, W, A, int(feat_stride), _ptr(base_d),
         int(rpn_batchsize), float(fg_fraction), float(pos_overlap), float(neg_overlap), _ptr(disable) if disable.numel() else None,
         int(disable.numel()), o[1], _ptr(labels), _ptr(tg), _ptr(iw), _ptr(ow), _ptr(ws), ws.numel(), _stream())
    return labels, tg, iw, ow


def proposal_target_layer_inject(rpn_rois, rpn_scores, gt_boxes, num_classes, keep_inds, n_fg, means=(0.0, 0.0, 0.0, 0.0),
                                 stds=(0.1, 0.1, 0.2, 0.2), opts=None):
    """proposal_target_layer for host-drawn keep_inds (int32 device [batch], fg rows first): frcnn_proposal_target_layer_inject.
    opts: roi_target_opts(...) or None."""
    _chk(rpn_rois), _chk(rpn_scores), _chk(gt_boxes), _chk(keep_inds, torch.int32)
    dev, N, G, B, C = rpn_rois.device, rpn_rois.shape[0], gt_boxes.shape[0], keep_inds.numel(), int(num_classes)
    rois = _empty((B, 5), dtype=torch.float32, device=dev)
    sc = _empty((B,), dtype=torch.float32, device=dev)
    labels = _empty((B, 1), dtype=torch.float32, device=dev)
    tg, iw, ow = (_empty((B, 4 * C), dtype=torch.float32, device=dev) for _ in range(3))
    m, s, o = _host_doubles(means), _host_doubles(stds), (_host_doubles(opts) if opts is not None else (None, None))
    call("frcnn_proposal_target_layer_inject", _ptr(rpn_rois), _ptr(rpn_scores), N, _ptr(gt_boxes), G, C, B, _ptr(keep_inds), int(n_fg),
         m[1], s[1], o[1], _ptr(rois), _ptr(sc), _ptr(labels), _ptr(tg), _ptr(iw), _ptr(ow), _stream())
    return rois, sc, labels, tg, iw, ow


def proposal_target_layer(rpn_rois, rpn_scores, gt_boxes, num_classes, batch_size=256, fg_fraction=0.25, fg_thresh=0.5,
                          bg_hi=0.5, bg_lo=0.0, means=(0.0, 0.0, 0.0, 0.0), stds=(0.1, 0.1, 0.2, 0.2), seed=0, num=None, opts=None):
    """lib/layer_utils/proposal_target_layer.py:18-152 on device.  num: int32 [1] device tensor = valid rows of rpn_rois
    (the proposal layer's count); without it every row is a proposal.  opts: roi_target_opts(...) or None."""
    _chk(rpn_rois), _chk(rpn_scores), _chk(gt_boxes)
    dev, N, G, B, C = rpn_rois.device, rpn_rois.shape[0], gt_boxes.shape[0], int(batch_size), int(num_classes)
    rois = _empty((B, 5), dtype=torch.float32, device=dev)
    sc = _empty((B,), dtype=torch.float32, device=dev)
    labels = _empty((B, 1), dtype=torch.float32, device=dev)
    tg, iw, ow = (_empty((B, 4 * C), dtype=torch.float32, device=dev) for _ in range(3))
    counts = _zeros((4,), dtype=torch.int32, device=dev)
    m, s, o = _host_doubles(means), _host_doubles(stds), (_host_doubles(opts) if opts is not None else (None, None))
    if num is not None:
        call("frcnn_proposal_target_layer_dn", _ptr(rpn_rois), _ptr(rpn_scores), N, _ptr(num), _ptr(gt_boxes), G, C, B,
             float(fg_fraction), float(fg_thresh), float(bg_hi), float(bg_lo), m[1], s[1], int(seed), o[1], _ptr(rois), _ptr(sc),
             _ptr(labels), _ptr(tg), _ptr(iw), _ptr(ow), _ptr(counts), _stream())
        if _binding.recorder is not None:
            _binding.recorder.patch_last(5, var="gt")
            _binding.recorder.patch_last(14)
        return rois, sc, labels, tg, iw, ow, counts
    call("frcnn_proposal_target_layer", _ptr(rpn_rois), _ptr(rpn_scores), N, _ptr(gt_boxes), G, C, B, float(fg_fraction),
         float(fg_thresh), float(bg_hi), float(bg_lo), m[1], s[1], int(seed), o[1], _ptr(rois), _ptr(sc), _ptr(labels), _ptr(tg),
         _ptr(iw), _ptr(ow), _ptr(counts), _stream())
    if _binding.recorder is not None:
        _binding.recorder.patch_last(4, var="gt")
        _binding.recorder.patch_last(13)
    return rois, sc, labels, tg, iw, ow, counts


def ohem_select(rpn_rois, rpn_scores, num, gt_boxes, num_classes, cls_score, bbox_pred, batch_size=256, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.0,
                means=(0.0, 0.0, 0.0, 0.0), stds=(0.1, 0.1, 0.2, 0.2), opts=None, nms_thresh=0.7, rule=NMS_RULE_CPU):
    """Online hard example mining on the device (frcnn_ohem_select, csrc/ohem_math.h): the padded proposal buffer rpn_rois [N,5] /
    rpn_scores [N] with num (int32 [1], device) valid rows, and cls_score [N,C] / bbox_pred [N,4C] of a read-only pass over those rows
    -> (rois [B,5], scores [B], labels [B,1], targets, inside, outside [B,4C], counts int32 [4], keep_inds int32 [B], roi_loss [N])."""
    _chk(rpn_rois), _chk(rpn_scores), _chk(gt_boxes), _chk(cls_score), _chk(bbox_pred), _chk(num, torch.int32)
    dev, N, G, B, C = rpn_rois.device, rpn_rois.shape[0], gt_boxes.shape[0], int(batch_size), int(num_classes)
    if tuple(cls_score.shape) != (N, C) or tuple(bbox_pred.shape) != (N, 4 * C) or rpn_scores.numel() != N:
        raise ValueError("ohem_select: cls_score / bbox_pred / rpn_scores must have one row per row of rpn_rois")
    rois = _empty((B, 5), dtype=torch.float32, device=dev)
    sc = _empty((B,), dtype=torch.float32, device=dev)
    labels = _empty((B, 1), dtype=torch.float32, device=dev)
    tg, iw, ow = (_empty((B, 4 * C), dtype=torch.float32, device=dev) for _ in range(3))
    counts = _empty((4,), dtype=torch.int32, device=dev)
    keep = _empty((B,), dtype=torch.int32, device=dev)
    loss = _empty((N,), dtype=torch.float32, device=dev)
    ws = workspace(lib().frcnn_ohem_workspace_bytes(N, C), dev, "ohem")
    m, s, o = _host_doubles(means), _host_doubles(stds), (_host_doubles(opts) if opts is not None else (None, None))
    call("frcnn_ohem_select", _ptr(rpn_rois), _ptr(rpn_scores), N, _ptr(num), _ptr(gt_boxes), G, C, _ptr(cls_score), _ptr(bbox_pred), B,
         float(fg_thresh), float(bg_hi), float(bg_lo), m[1], s[1], o[1], float(nms_thresh), int(rule), _ptr(rois), _ptr(sc), _ptr(labels),
         _ptr(tg), _ptr(iw), _ptr(ow), _ptr(counts), _ptr(keep), _ptr(loss), _ptr(ws), ws.numel(), _stream())
    if _binding.recorder is not None:
        _binding.recorder.patch_last(5, var="gt")    # the image's box count (gt_boxes: the first G rows of a static buffer)
    return rois, sc, labels, tg, iw, ow, counts, keep, loss


def ohem_select_host(rpn_rois, rpn_scores, num, gt_boxes, num_classes, cls_score, bbox_pred, batch_size=256, fg_thresh=0.5, bg_hi=0.5,
                     bg_lo=0.0, means=(0.0, 0.0, 0.0, 0.0), stds=(0.1, 0.1, 0.2, 0.2), opts=None, nms_thresh=0.7, rule=NMS_RULE_CPU):
    """frcnn_ohem_select_host: the same on HOST numpy arrays, no GPU needed; num an int.  -> the same nine results as numpy arrays."""
    f32 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
    C, B = int(num_classes), int(batch_size)
    rpn_rois = f32(rpn_rois, (-1, 5))
    N = rpn_rois.shape[0]
    rpn_scores, gt_boxes, cls_score, bbox_pred = f32(rpn_scores, (N,)), f32(gt_boxes, (-1, 5)), f32(cls_score, (N, C)), f32(bbox_pred, (N, 4 * C))
    nb = max(B, 1)
    rois, sc, labels = np.zeros((nb, 5), np.float32), np.zeros(nb, np.float32), np.zeros((nb, 1), np.float32)
    tg, iw, ow = (np.zeros((nb, 4 * C), np.float32) for _ in range(3))
    counts, keep, loss = np.zeros(4, np.int32), np.zeros(nb, np.int32), np.zeros(max(N, 1), np.float32)
    n = np.array([int(num)], dtype=np.int32)
    m, s = np.ascontiguousarray(means, dtype=np.float64), np.ascontiguousarray(stds, dtype=np.float64)
    o = None if opts is None else np.ascontiguousarray(opts, dtype=np.float64)
    check(lib().frcnn_ohem_select_host(rpn_rois.ctypes.data, rpn_scores.ctypes.data, N, n.ctypes.data, gt_boxes.ctypes.data, gt_boxes.shape[0], C,
                                       cls_score.ctypes.data, bbox_pred.ctypes.data, B, float(fg_thresh), float(bg_hi), float(bg_lo),
                                       m.ctypes.data, s.ctypes.data, None if o is None else o.ctypes.data, float(nms_thresh), int(rule),
                                       rois.ctypes.data, sc.ctypes.data, labels.ctypes.data, tg.ctypes.data, iw.ctypes.data, ow.ctypes.data,
                                       counts.ctypes.data, keep.ctypes.data, loss.ctypes.data), "frcnn_ohem_select_host")
    return rois, sc, labels, tg, iw, ow, counts, keep, loss


def softmax_ce_loss(logits, labels, rpn_shape=None):
    """-> (loss [1], dlogits like logits).  rpn_shape=(A,H,W): logits [1,H,W,2A] with labels [1,1,A*H,W]."""
    _chk(logits), _chk(labels)
    dev = logits.device
    if rpn_shape is None:
        R, C, A, H, W = logits.shape[0], logits.shape[1], 0, 0, 0
    else:
        A, H, W = rpn_shape
        R, C = A * H * W, 2
    loss = _zeros((1,), dtype=torch.float32, device=dev)
    grad = _zeros(tuple(logits.shape), dtype=logits.dtype, device=logits.device)
    ws = workspace(lib().frcnn_loss_workspace_bytes(R), dev, "loss")
    call("frcnn_softmax_ce_loss", _ptr(logits), _ptr(labels), R, C, A, H, W, _ptr(loss), _ptr(grad), _ptr(ws), ws.numel(), _stream())
    return loss, grad


def smooth_l1_loss(pred, targets, inside_w, outside_w, sigma, mean_divisor):
    _chk(pred), _chk(targets), _chk(inside_w), _chk(outside_w)
    dev, n = pred.device, pred.numel()
    loss = _zeros((1,), dtype=torch.float32, device=dev)
    grad = _empty(tuple(pred.shape), dtype=pred.dtype, device=pred.device)
    ws = workspace(lib().frcnn_loss_workspace_bytes(n), dev, "loss")
    call("frcnn_smooth_l1_loss", _ptr(pred), _ptr(targets), _ptr(inside_w), _ptr(outside_w), n, float(sigma), float(mean_divisor),
         _ptr(loss), _ptr(grad), _ptr(ws), ws.numel(), _stream())
    return loss, grad


IOU_LOSS_KINDS = {"iou": 1, "giou": 2, "diou": 3, "ciou": 4}      # IOULOSS_* of csrc/iouloss_math.h


def _iou_loss_kind(kind):
    if kind in IOU_LOSS_KINDS:
        return IOU_LOSS_KINDS[kind]
    if isinstance(kind, str):
        raise ValueError("iou_loss: kind %r is none of %s" % (kind, sorted(IOU_LOSS_KINDS)))
    return int(kind)


def _host_floats(values):
    a = np.ascontiguousarray(values, dtype=np.float32)
    if _binding.recorder is not None:
        _binding.recorder.keep.append(a)         # (a recorded launch keeps the pointer)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def iou_loss(pred, targets, inside_w, outside_w, refs, means, stds, kind, weight, mean_divisor, K):
    """IoU / GIoU / DIoU / CIoU loss on the decoded boxes (frcnn_iou_loss, csrc/iouloss_math.h): pred, targets, inside_w, outside_w of one
    shape with 4 K N elements, read as [N, 4K]; refs [N,4] (anchors) or [N,5] (RoIs); means / stds four floats each; kind a name of
    IOU_LOSS_KINDS or its number.  -> (loss [1], grad like pred, every element written)."""
    _chk(pred), _chk(targets), _chk(inside_w), _chk(outside_w), _chk(refs)
    dev, K = pred.device, int(K)
    if K <= 0 or pred.numel() % (4 * K) or not (targets.numel() == inside_w.numel() == outside_w.numel() == pred.numel()):
        raise ValueError("iou_loss: pred, targets and the weights must have the same number of elements, a multiple of 4 K")
    N = pred.numel() // (4 * K)
    if refs.dim() != 2 or refs.shape[0] != N or len(means) != 4 or len(stds) != 4:
        raise ValueError("iou_loss: refs must have one row per row of pred (%d), means and stds four values" % N)
    loss = _zeros((1,), dtype=torch.float32, device=dev)
    grad = _empty(tuple(pred.shape), dtype=pred.dtype, device=dev)
    ws = workspace(lib().frcnn_iou_loss_workspace_bytes(N * K), dev, "iou_loss")
    m, s = _host_floats(means), _host_floats(stds)
    call("frcnn_iou_loss", _ptr(pred), _ptr(targets), _ptr(inside_w), _ptr(outside_w), N, K, _ptr(refs), int(refs.shape[1]), m[1], s[1],
         _iou_loss_kind(kind), float(weight), float(mean_divisor), _ptr(loss), _ptr(grad), _ptr(ws), ws.numel(), _stream())
    return loss, grad


def iou_loss_host(pred, targets, inside_w, outside_w, refs, means, stds, kind, weight, mean_divisor, K):
    """frcnn_iou_loss_host: the same on HOST numpy arrays, no GPU needed.  -> (loss [1], grad like pred) as numpy arrays."""
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    pred, targets, inside_w, outside_w, refs = f32(pred), f32(targets), f32(inside_w), f32(outside_w), f32(refs)
    K = int(K)
    if K <= 0 or pred.size % (4 * K) or not (targets.size == inside_w.size == outside_w.size == pred.size):
        raise ValueError("iou_loss_host: pred, targets and the weights must have the same number of elements, a multiple of 4 K")
    N = pred.size // (4 * K)
    if refs.ndim != 2 or refs.shape[0] != N or len(means) != 4 or len(stds) != 4:
        raise ValueError("iou_loss_host: refs must have one row per row of pred (%d), means and stds four values" % N)
    m, s = f32(means), f32(stds)
    loss, grad = np.zeros(1, np.float32), np.empty(pred.shape, np.float32)
    check(lib().frcnn_iou_loss_host(pred.ctypes.data, targets.ctypes.data, inside_w.ctypes.data, outside_w.ctypes.data, N, K, refs.ctypes.data,
                                    int(refs.shape[1]), m.ctypes.data, s.ctypes.data, _iou_loss_kind(kind), float(weight), float(mean_divisor),
                                    loss.ctypes.data, grad.ctypes.data), "frcnn_iou_loss_host")
    return loss, grad


# ------------------------------------------------------------------------------------------ backward
def transpose_pad(x2d, Mp, out=None):
    """x2d [M,C] -> [C,Mp] (zero padded)."""
    _chk(x2d)
    M, C = x2d.shape
    out = _empty((C, Mp), dtype=torch.float32, device=x2d.device) if out is None else out
    call("frcnn_transpose_pad", _ptr(x2d), M, C, _ptr(out), int(Mp), _stream())
    return out


def im2col_t(x, KH, KW, stride, pad, OH, OW, Mp, out=None):
    _chk(x)
    N, H, W, Cin = x.shape
    out = _empty((KH * KW * Cin, Mp), dtype=torch.float32, device=x.device) if out is None else out
    call("frcnn_im2col_t", _ptr(x), N, H, W, Cin, OH, OW, KH, KW, int(stride), int(pad[0]), int(pad[2]), _ptr(out), int(Mp), _stream())
    return out


def flip_transpose_filter(w_packed, out=None):
    _chk(w_packed)
    Cout, KH, KW, Cin = w_packed.shape
    out = _empty((Cin, KH, KW, Cout), dtype=torch.float32, device=w_packed.device) if out is None else out
    call("frcnn_flip_transpose_filter", _ptr(w_packed), Cout, KH, KW, Cin, _ptr(out), _stream())
    return out


def conv2d_dgrad_strided(dy, w_packed, stride, pad, H, W, dx, accumulate):
    _chk(dy), _chk(w_packed), _chk(dx)
    N, OH, OW, Cout = dy.shape
    _, KH, KW, Cin = w_packed.shape
    call("frcnn_conv2d_dgrad_strided", _ptr(dy), N, OH, OW, Cout, _ptr(w_packed), KH, KW, Cin, int(stride), int(pad[0]), int(pad[2]),
         _ptr(dx), int(H), int(W), 1 if accumulate else 0, _stream())
    return dx


def conv2d_wgrad_supported(Cin, Cout):
    return bool(lib().frcnn_conv2d_wgrad_supported(int(Cin), int(Cout)))


def conv2d_wgrad(dy, x, KH, KW, stride, pad, out, h2=False):
    """dW [Cout, KH, KW, Cin] of a convolution from dY [N,OH,OW,Cout] and its input X [N,H,W,Cin], both read as they lie; pad =
    (top, bottom, left, right).  Cin % 64 == 0 and Cout % 64 == 0 (conv2d_wgrad_supported).  h2 False: f32 matrix pipe
    (csrc/wgrad_tn.hip); True: two-piece fp16 operands split in registers, fp16 matrix pipe (csrc/wgrad_h2.hip)."""
    _chk(dy), _chk(x), _chk(out)
    N, OH, OW, Cout = dy.shape
    _, H, W, Cin = x.shape
    if out.numel() != Cout * KH * KW * Cin:
        raise ValueError("conv2d_wgrad: out has %d elements, the filter %d" % (out.numel(), Cout * KH * KW * Cin))
    name = "frcnn_conv2d_wgrad_h2" if h2 else "frcnn_conv2d_wgrad"
    nb = getattr(lib(), name + "_workspace_bytes")(N, OH, OW, Cin, Cout, int(KH), int(KW))
    ws = workspace(nb, x.device, "conv_wgrad") if nb else None
    call(name, _ptr(dy), _ptr(x), N, H, W, Cin, OH, OW, Cout, int(KH), int(KW), int(stride), int(pad[0]), int(pad[2]),
         _ptr(out), _ptr(ws), int(nb), _stream())
    return out


def relu_bwd(grad, y):
    _chk(grad), _chk(y)
    call("frcnn_relu_bwd", _ptr(grad), _ptr(y), grad.numel(), _stream())
    return grad


def gemm_x3_pack(w, planes=None):
    """bf16 planes [G][3][N][K] of a filter bank w [G,N,K] or [N,...K] (frcnn_gemm_x3_pack); `planes`: re-split into an existing buffer."""
    _chk(w)
    G, N, K = (w.shape[0], w.shape[1], w.shape[2]) if w.dim() == 3 else (1, w.shape[0], w[0].numel())
    if planes is None:
        planes = torch.empty(lib().frcnn_gemm_x3_pack_bytes(G, N, K), dtype=torch.uint8, device=w.device)
    call("frcnn_gemm_x3_pack", _ptr(w), G, N, K, _ptr(planes), _stream())
    return planes


def gemm_x3(x, planes, G, M, N, K, bias=None, residual=None, act=ACT_NONE, out=None, cfg=-1, terms=6):
    """out[g] = act(x[g] W[g]^T + bias + residual[g]) through frcnn_gemm_x3 (products on the bf16 pipe as exact 3-way splits).
    cfg: -1 = tiles by shape; terms: 6 (default) or 9 (all cross terms: every f32 product exact)."""
    _chk(x)
    out = _empty((G, M, N) if G > 1 else (M, N), dtype=torch.float32, device=x.device) if out is None else out
    call("frcnn_gemm_x3", _ptr(x), _ptr(planes), _ptr(bias), _ptr(residual), _ptr(out), int(G), int(M), int(N), int(K), int(act),
         int(cfg), int(terms), _stream())
    return out


class H2(object):
    """A float32 tensor [rows, K] held as frcnn_gemm_h2 operand planes: `planes` uint8 buffer = fp16 [2][rows][K] (H then L) and
    `inv` f32 [K/128][rows] = the exact power-of-two block scales 2^-e (csrc/gemm_h2.hip)."""
    __slots__ = ("planes", "inv", "rows", "K")

    def __init__(self, planes, inv, rows, K):
        self.planes, self.inv, self.rows, self.K = planes, inv, int(rows), int(K)

    @staticmethod
    def empty(rows, K, device):
        assert K % 128 == 0
        return H2(torch.empty(lib().frcnn_h2_planes_bytes(int(rows), int(K)), dtype=torch.uint8, device=device),
                  torch.empty((K // 128, rows), dtype=torch.float32, device=device), rows, K)

    def to_float(self):
        """(h + l) * 2^-e as float32 [rows, K] (tests / debugging: host-side torch arithmetic, not a product path)."""
        hl = self.planes.view(torch.float16).view(2, self.rows, self.K).float()
        inv = self.inv.t().repeat_interleave(128, dim=1)
        return (hl[0] + hl[1]) * inv


def h2_split(x, out=None):
    """frcnn_h2_split: x f32 [..., K] (K % 128 == 0) -> H2 planes of its rows."""
    _chk(x)
    K = x.shape[-1]
    rows = x.numel() // K
    out = H2.empty(rows, K, x.device) if out is None else out
    assert out.rows == rows and out.K == K
    call("frcnn_h2_split", _ptr(x), rows, K, _ptr(out.planes), _ptr(out.inv), _stream())
    return out


def h2_pack_w(w, out=None):
    """frcnn_h2_pack_w: filter bank w [G,N,K] or [N,...K] f32 -> (planes uint8 [G][2][N][K] fp16, w_inv f32 [G,N])."""
    _chk(w)
    G, N, K = (w.shape[0], w.shape[1], w.shape[2]) if w.dim() == 3 else (1, w.shape[0], w[0].numel())
    if out is None:
        out = (torch.empty(lib().frcnn_h2_planes_bytes(G * N, K), dtype=torch.uint8, device=w.device),
               torch.empty((G, N), dtype=torch.float32, device=w.device))
    call("frcnn_h2_pack_w", _ptr(w), G, N, K, _ptr(out[0]), _ptr(out[1]), _stream())
    return out


def gemm_h2(x, wp, G, M, N, K, bias=None, residual=None, act=ACT_NONE, out=None, out_planes=None, want_f32=True, cfg=-1, mask=None):
    """out[g] = act(x[g] W[g]^T + bias + residual[g]) through frcnn_gemm_h2.  x: H2 of [G*M, K]; wp = h2_pack_w(W [G,N,K]).
    residual: f32 [G*M, N] or an H2 of [G*M, N] (read as (h + l) * 2^-e).  out: f32 [G*M, N] (allocated when want_f32 and out is None);
    out_planes: an H2 of [G*M, N] to ALSO receive the result as the next GEMM's operand (emitted from the epilogue).
    mask (training; float32 [G*M, N]): result = mask > 0 ? result : 0 in the tile epilogue (frcnn_gemm_h2_masked; float32 residual only).
    Returns (out or None, out_planes or None)."""
    assert isinstance(x, H2) and x.rows == G * M and x.K == K
    if out is None and want_f32:
        out = _empty((G * M, N), dtype=torch.float32, device=x.planes.device)
    if out_planes is not None:
        assert out_planes.rows == G * M and out_planes.K == N
    rp = residual if isinstance(residual, H2) else None
    if rp is not None:
        assert rp.rows == G * M and rp.K == N
    if mask is not None:
        _chk(mask)
        assert rp is None and mask.numel() == G * M * N
        call("frcnn_gemm_h2_masked", _ptr(x.planes), _ptr(x.inv), _ptr(wp[0]), _ptr(wp[1]), _ptr(bias), _ptr(residual), _ptr(mask), _ptr(out),
             _ptr(None if out_planes is None else out_planes.planes), _ptr(None if out_planes is None else out_planes.inv),
             int(G), int(M), int(N), int(K), int(act), int(cfg), _stream())
        return out, out_planes
    call("frcnn_gemm_h2", _ptr(x.planes), _ptr(x.inv), _ptr(wp[0]), _ptr(wp[1]), _ptr(bias), _ptr(None if rp is not None else residual),
         _ptr(None if rp is None else rp.planes), _ptr(None if rp is None else rp.inv), _ptr(out),
         _ptr(None if out_planes is None else out_planes.planes), _ptr(None if out_planes is None else out_planes.inv),
         int(G), int(M), int(N), int(K), int(act), int(cfg), _stream())
    return out, out_planes


def gemm_h2_mean(x, wp, G, M, N, K, bias, residual, act, rows, out=None, cfg=-1):
    """frcnn_gemm_h2_mean: [G * M / rows, N] = mean over each group of `rows` consecutive rows of act(x[g] W^T + bias + residual[g]); one
    batch entry per image (the reduction order is then independent of the batch slot).  residual: f32 [G*M, N], an H2, or None."""
    assert isinstance(x, H2) and x.rows == G * M and x.K == K and M % rows == 0
    if out is None:
        out = _empty((G * (M // rows), N), dtype=torch.float32, device=x.planes.device)
    rp = residual if isinstance(residual, H2) else None
    ws = workspace(lib().frcnn_gemm_h2_mean_workspace_bytes(int(G), int(M), int(N)), x.planes.device, "h2_mean")
    call("frcnn_gemm_h2_mean", _ptr(x.planes), _ptr(x.inv), _ptr(wp[0]), _ptr(wp[1]), _ptr(bias), _ptr(None if rp is not None else residual),
         _ptr(None if rp is None else rp.planes), _ptr(None if rp is None else rp.inv), int(G), int(M), int(N), int(K), int(act), int(rows),
         _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), int(cfg), _stream())
    return out


def winograd_input_transform_h2(x, v, m):
    """x [N,H,W,C] f32 -> V as H2 planes of [points * tiles, C] (frcnn_winograd[7]_input_transform_h2)."""
    _chk(x)
    N, H, W, C = x.shape
    assert isinstance(v, H2) and v.K == C and v.rows == winograd_points(m) * winograd_tiles(N, H, W, m)
    if m == 7:
        call("frcnn_winograd7_input_transform_h2", _ptr(x), N, C, _ptr(v.planes), _ptr(v.inv), _stream())
    else:
        call("frcnn_winograd_input_transform_h2", _ptr(x), N, H, W, C, int(m), _ptr(v.planes), _ptr(v.inv), _stream())
    return v


def winograd_output_transform_h2(mm, bias, act, shape, m, out_planes, out=None):
    """mm [(points), tiles, C] f32 -> act(A^T M A + bias) of shape [N,H,W,C] as H2 planes (`out_planes`, rows = N*H*W) and, when `out`
    is given, as the float32 tensor too."""
    _chk(mm)
    N, H, W, C = shape
    assert isinstance(out_planes, H2) and out_planes.rows == N * H * W and out_planes.K == C
    assert mm.numel() == winograd_points(m) * winograd_tiles(N, H, W, m) * C
    if out is not None:
        _chk(out)
        assert tuple(out.shape) == tuple(shape)
    if m == 7:
        call("frcnn_winograd7_output_transform_h2", _ptr(mm), N, C, _ptr(bias), int(act), _ptr(out), _ptr(out_planes.planes),
             _ptr(out_planes.inv), _stream())
    else:
        call("frcnn_winograd_output_transform_h2", _ptr(mm), N, H, W, C, int(m), _ptr(bias), int(act), _ptr(out), _ptr(out_planes.planes),
             _ptr(out_planes.inv), _stream())
    return out_planes


def relu6_bwd(grad, y):
    _chk(grad), _chk(y)
    call("frcnn_relu6_bwd", _ptr(grad), _ptr(y), grad.numel(), _stream())
    return grad


def maxpool_bwd(x, y, dy, k, stride, dx):
    """gradient of maxpool(x) (padding bottom / right only) into dx (written)."""
    _chk(x), _chk(y), _chk(dy), _chk(dx)
    N, H, W, C = x.shape
    call("frcnn_maxpool_bwd", _ptr(x), N, H, W, C, int(k), int(stride), _ptr(y), _ptr(dy), y.shape[1], y.shape[2], _ptr(dx), _stream())
    return dx


def dropout(x, seed, keep_prob, out=None, step_mult=0):
    """tf.nn.dropout with a counter-based mask of (seed, element index); the same call on a gradient is the backward pass.
    step_mult: seed = step_mult * (the step's sampling seed) + const -- tells a recorded training step how to advance it."""
    _chk(x)
    out = _empty(tuple(x.shape), dtype=x.dtype, device=x.device) if out is None else out
    call("frcnn_dropout", _ptr(x), x.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, float(keep_prob), _ptr(out), _stream())
    if _binding.recorder is not None and step_mult:
        _binding.recorder.patch_last(2, step_mult)
    return out


def dwconv3x3_dgrad(g, w, stride, pad, dx, accumulate=False):
    _chk(g), _chk(w), _chk(dx)
    N, OH, OW, C = g.shape
    call("frcnn_dwconv3x3_dgrad", _ptr(g), N, OH, OW, C, _ptr(w), _ptr(dx), dx.shape[1], dx.shape[2], int(stride), int(pad[0]), int(pad[2]),
         1 if accumulate else 0, _stream())
    return dx


def dwconv3x3_wgrad(g, x, stride, pad, scale, dw):
    _chk(g), _chk(x), _chk(dw)
    N, OH, OW, C = g.shape
    ws = workspace(lib().frcnn_dwconv3x3_wgrad_workspace_bytes(N, OH, OW, C), g.device, "dw_wgrad")
    call("frcnn_dwconv3x3_wgrad", _ptr(g), _ptr(x), N, x.shape[1], x.shape[2], C, OH, OW, int(stride), int(pad[0]), int(pad[2]), _ptr(scale),
         _ptr(dw), _ptr(ws), ws.numel(), _stream())
    return dw


def dwconv3x3_refold(w, scale, wf):
    _chk(w), _chk(scale), _chk(wf)
    call("frcnn_dwconv3x3_refold", _ptr(w), _ptr(scale), w.shape[-1], _ptr(wf), _stream())
    return wf


def add_strided(src, dst, stride, accumulate):
    _chk(src), _chk(dst)
    N, OH, OW, C = src.shape
    call("frcnn_add_strided", _ptr(src), N, OH, OW, C, _ptr(dst), dst.shape[1], dst.shape[2], int(stride), 1 if accumulate else 0, _stream())
    return dst


def spatial_mean_bwd(dy, HW, out):
    _chk(dy), _chk(out)
    call("frcnn_spatial_mean_bwd", _ptr(dy), dy.shape[0], int(HW), dy.shape[1], _ptr(out), _stream())
    return out


def colsum(dy2d, out):
    _chk(dy2d), _chk(out)
    call("frcnn_colsum", _ptr(dy2d), dy2d.shape[0], dy2d.shape[1], _ptr(out), _stream())
    return out


def crop_and_resize_bwd(dout, rois, feat_stride, dfeat, max_lds=0):
    """dfeat += gradient of crop_and_resize w.r.t. the feature map.  max_lds (bytes; tests): the LDS budget of the launch plan."""
    _chk(dout), _chk(rois), _chk(dfeat)
    R, P, _, C = dout.shape
    H, W = dfeat.shape[-3], dfeat.shape[-2]
    if max_lds:
        call("frcnn_crop_and_resize_bwd_plan", _ptr(dout), H, W, C, _ptr(rois), R, float(feat_stride), P, _ptr(dfeat), int(max_lds), _stream())
    else:
        call("frcnn_crop_and_resize_bwd", _ptr(dout), H, W, C, _ptr(rois), R, float(feat_stride), P, _ptr(dfeat), _stream())
    return dfeat


def roi_align_bwd(dout, rois, feat_stride, samples, dfeat, max_lds=0):
    """dfeat += gradient of roi_align w.r.t. the feature map (one image).  max_lds (bytes; tests): the LDS budget of the launch plan."""
    _chk(dout), _chk(rois), _chk(dfeat)
    R, P, _, C = dout.shape
    H, W = dfeat.shape[-3], dfeat.shape[-2]
    if max_lds:
        call("frcnn_roi_align_bwd_plan", _ptr(dout), H, W, C, _ptr(rois), R, float(feat_stride), P, int(samples), _ptr(dfeat), int(max_lds),
             _stream())
    else:
        call("frcnn_roi_align_bwd", _ptr(dout), H, W, C, _ptr(rois), R, float(feat_stride), P, int(samples), _ptr(dfeat), _stream())
    return dfeat


def sgd_momentum(w, acc, w_folded, grad, scale, K, lr, momentum, weight_decay, grad_scale=1.0):
    call("frcnn_sgd_momentum", _ptr(w), _ptr(acc), _ptr(w_folded), _ptr(grad), _ptr(scale), w.numel(), int(K), float(lr),
         float(momentum), float(weight_decay), float(grad_scale), _stream())


def sgd_desc_table(entries, device):
    """entries: list of (w, acc, w_folded or None, grad, scale or None, K, lr_mult, weight_decay) tensors / numbers ->
    uint8 device tensor holding the SgdDesc array of frcnn_sgd_momentum_multi."""
    import struct
    nb = lib().frcnn_sgd_desc_bytes()
    assert nb == 64, nb
    raw = bytearray()
    for w, acc, wf, grad, scale, K, lr_mult, wd in entries:
        raw += struct.pack("<QQQQQqiffi", w.data_ptr(), acc.data_ptr(), 0 if wf is None else wf.data_ptr(), grad.data_ptr(),
                           0 if scale is None else scale.data_ptr(), int(w.numel()), int(K), float(lr_mult), float(wd), 0)
    return torch.frombuffer(raw, dtype=torch.uint8).clone().to(device)


def sgd_momentum_multi(table, count, lr, momentum, grad_scale=1.0):
    call("frcnn_sgd_momentum_multi", _ptr(table), int(count), float(lr), float(momentum), float(grad_scale), _stream())


def sgd_momentum_range(table, first, count, lr, momentum, grad_scale=1.0):
    """frcnn_sgd_momentum_multi for the descriptors [first, first + count) of `table`."""
    call("frcnn_sgd_momentum_range", _ptr(table), int(first), int(count), float(lr), float(momentum), float(grad_scale), _stream())


def sumsq(w, scale, out, accumulate):
    ws = workspace(4096, w.device, "sumsq")
    call("frcnn_sumsq", _ptr(w), w.numel(), float(scale), _ptr(out), 1 if accumulate else 0, _ptr(ws), ws.numel(), _stream())


def sumsq_multi(ptr_table, sizes, scale, out, accumulate=False):
    """ptr_table int64 [count] (device pointers of float tensors), sizes int64 [count], both on device."""
    count = ptr_table.numel()
    ws = workspace(8 * 64 * count, out.device, "sumsq")
    call("frcnn_sumsq_multi", _ptr(ptr_table), _ptr(sizes), count, float(scale), _ptr(out), 1 if accumulate else 0, _ptr(ws), ws.numel(),
         _stream())
    return out


# ------------------------------------------------------------------------------------------ summary statistics
SUMMARY_BUCKETS, SUMMARY_RECORD = 1551, 1560          # include/frcnn_hip.h FRCNN_SUMMARY_*: words 1551.. = num, n_zero, n_nonfinite, min, max, sum, sum_squares
_summary_limits = None


def summary_limits():
    """HOST float64 [1551]: TensorFlow's default histogram bucket limits, the table the device kernel uses (frcnn_summary_limits)."""
    global _summary_limits
    if _summary_limits is None:
        out = np.empty((SUMMARY_BUCKETS,), dtype=np.float64)
        call("frcnn_summary_limits", out.ctypes.data_as(ctypes.c_void_p))
        out.setflags(write=False)
        _summary_limits = out
    return _summary_limits


class SummaryPlan(object):
    """frcnn_summary_stats over a fixed list of device tensors (float32, contiguous; views at any float offset): the (pointer, count)
    table, the record buffer and the scratch are made once, `launch()` is the three enqueues on the current stream, `read()` the one
    read-back.  The plan holds addresses, not tensors: it is valid while the caller keeps them where they are (static step buffers, solver
    state)."""

    def __init__(self, tensors):
        tensors = [_chk(t) for t in tensors]
        self.count = len(tensors)
        dev = tensors[0].device if tensors else None
        if self.count:
            self.table = torch.tensor([[t.data_ptr(), t.numel()] for t in tensors], dtype=torch.int64).to(dev)
            self.out = torch.empty((self.count, SUMMARY_RECORD), dtype=torch.int64, device=dev)
            self.ws = torch.empty((int(lib().frcnn_summary_stats_workspace_bytes(self.count)),), dtype=torch.uint8, device=dev)

    def launch(self):
        if self.count:
            call("frcnn_summary_stats", _ptr(self.table), self.count, _ptr(self.out), _ptr(self.ws), self.ws.numel(), _stream())
        return self

    def read(self):
        """list of dict(counts int64 [1551], num, n_zero, n_nonfinite, min, max, sum, sum_squares), one per tensor (waits for the launch)"""
        if not self.count:
            return []
        raw = self.out.cpu().numpy()
        f = raw.view(np.float64)
        return [dict(counts=raw[i, :SUMMARY_BUCKETS].copy(), num=int(raw[i, 1551]), n_zero=int(raw[i, 1552]), n_nonfinite=int(raw[i, 1553]),
                     min=float(f[i, 1554]), max=float(f[i, 1555]), sum=float(f[i, 1556]), sum_squares=float(f[i, 1557]))
                for i in range(self.count)]


def summary_stats(tensors):
    """Histogram + moments of every tensor of the list in one launch sequence (csrc/summary_stats.hip) -> list of dict, see
    SummaryPlan.read.  A non-finite value is counted in n_nonfinite only."""
    tensors = list(tensors)                                  # (alive until the read-back)
    return SummaryPlan(tensors).launch().read()


class Graph:
    """One captured hipGraph (frcnn_graph_* in the C ABI)."""

    def __init__(self):
        self.handle = None

    def capture(self, fn):
        st = torch.cuda.current_stream()
        if st.cuda_stream == 0:
            raise RuntimeError("capture needs a non-default stream (use torch.cuda.stream(torch.cuda.Stream()))")
        call("frcnn_graph_begin", ctypes.c_void_p(st.cuda_stream))
        try:
            fn()
        finally:
            h = ctypes.c_void_p()
            call("frcnn_graph_end", ctypes.c_void_p(st.cuda_stream), ctypes.byref(h))
        self.handle = h
        return self

    def launch(self):
        call("frcnn_graph_launch", self.handle, _stream())

    def __del__(self):
        try:
            if self.handle:
                call("frcnn_graph_destroy", self.handle)
        except Exception:
            pass
