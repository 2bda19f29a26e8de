"""model.test -- the test loop of the reference (lib/model/test.py) on the device chain.

`im_detect` / `test_net` keep the reference's names and return conventions.  `im_detect` / `detect` take the ALREADY
SCALED, mean-subtracted blob plus its scale; `_get_image_blob` (test.py:26-58) is provided ON DEVICE
(`frcnn_prep_image`: uint8 BGR in HBM -> mean-subtracted, cv2.INTER_LINEAR-resized, staged stem input), and
`im_detect_bgr` / `detect_bgr` are the raw-image forms (the reference's `im_detect(sess, net, im)` signature)."""
import numpy as np
import torch

from frcnn_hip import ops
from frcnn_hip.runtime import Timer
from model.config import cfg


def im_detect(sess, net, blob, im_scale, im_shape):
    """blob [1,H,W,3] f32 (BGR - PIXEL_MEANS, scaled by im_scale), im_shape = original (h, w[, c]).
    Returns (scores [R,C], pred_boxes [R,4C]) like lib/model/test.py:86-107 -- decode + clip of the
    per-class boxes included -- computed from the device tensors."""
    im_info = np.array([blob.shape[1], blob.shape[2], im_scale], dtype=np.float32)
    img = net._stage_image(sess, blob, im_info)
    p = net.forward_device(sess, img, im_info)
    n = p["rois"].shape[0] if net._num_rois is None else int(net._num_rois.item())
    rois, bbox_pred = p["rois"][:n].contiguous(), (p["bbox_pred"][:n].contiguous() if cfg.TEST.BBOX_REG else None)
    pred_boxes = ops.im_detect_boxes(rois, bbox_pred, im_scale, im_shape[0], im_shape[1], net._num_classes)      # test.py:95-105
    return p["cls_prob"][:n].cpu().numpy(), pred_boxes.cpu().numpy()


def _get_image_blob(sess, net, im):
    """test.py:26-58 on device for cfg.TEST.SCALES[0]: im = BGR uint8 (or float32) [h,w,3], numpy or device tensor.
    Returns (staged image [1,H,W,4] on device -- zero 4th channel, what forward_device takes --, im_scale)."""
    if isinstance(im, np.ndarray):
        im = torch.from_numpy(np.ascontiguousarray(im)).to(sess.device, non_blocking=True)     # 3 B/pixel over PCIe
    im_scale, OH, OW = ops.prep_image_shape(im.shape[0], im.shape[1], cfg.TEST.SCALES[0], cfg.TEST.MAX_SIZE)
    with net.shape_scope(sess, (1, OH, OW, 4), (OH, OW)):        # the staged image belongs to its shape's scope (freed with the shape's graph)
        out = sess.buf(net._tag + "/image", (1, OH, OW, 4))
    ops.prep_image(im, cfg.PIXEL_MEANS, im_scale, (OH, OW), out=out, out_c=4)
    return out, im_scale


def im_detect_bgr(sess, net, im):
    """The reference's `im_detect(sess, net, im)` (test.py:86-107): raw BGR image in, (scores, pred_boxes) out."""
    img, im_scale = _get_image_blob(sess, net, im)
    im_info = np.array([img.shape[1], img.shape[2], im_scale], dtype=np.float32)
    p = net.forward_device(sess, img, im_info)
    n = p["rois"].shape[0] if net._num_rois is None else int(net._num_rois.item())
    pred_boxes = ops.im_detect_boxes(p["rois"][:n].contiguous(), p["bbox_pred"][:n].contiguous() if cfg.TEST.BBOX_REG else None, im_scale,
                                     im.shape[0], im.shape[1], net._num_classes)
    return p["cls_prob"][:n].cpu().numpy(), pred_boxes.cpu().numpy()


def detect_bgr(sess, net, im, max_per_image=100, thresh=0.):
    """Raw BGR image -> per-class detections, everything after the (optional) H2D copy on the GPU."""
    img, im_scale = _get_image_blob(sess, net, im)
    im_info = np.array([img.shape[1], img.shape[2], im_scale], dtype=np.float32)
    dets, cnt = net.detect_device(sess, img, im_info, im.shape[:2], max_per_image=max_per_image, thresh=thresh)
    n = min(int(cnt.item()), dets.shape[0])
    return _per_class(dets[:n].cpu().numpy(), net._num_classes)


def _per_class(rec, num_classes):
    """detection records [n,6] (x1,y1,x2,y2,score,class) -> the per-class list of detect_bgr and detect_bgr_batch"""
    return [np.zeros((0, 5), dtype=np.float32)] + [rec[rec[:, 5] == j, :5] for j in range(1, num_classes)]


class _PinnedRing(object):
    """`depth` pinned host buffers handed out in turn; one is handed out again only after the event recorded behind the copy that last
    used it has completed (mark).  The batched loop keeps one batch in flight, so with two buffers that wait never blocks."""

    def __init__(self, depth=2):
        self._bufs, self._evs, self._k = [None] * depth, [None] * depth, 0

    def take(self, nbytes):
        k = self._k = (self._k + 1) % len(self._bufs)
        if self._evs[k] is not None:
            self._evs[k].synchronize()
        if self._bufs[k] is None or self._bufs[k].numel() < nbytes:
            self._bufs[k] = torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=True)
        return self._bufs[k][:nbytes], k

    def mark(self, k):
        if self._evs[k] is None:
            self._evs[k] = torch.cuda.Event()
        self._evs[k].record(torch.cuda.current_stream())
        return self._evs[k]


class _Pending(object):
    """one enqueued batch: its pinned record (detections of every slot, then the counts) and the event behind the copy that fills it"""
    __slots__ = ("host", "ev", "B", "n_valid", "max_out", "num_classes")


def _check_max_per_image(max_per_image):
    if max_per_image <= 0:
        raise ValueError("the batched loop reads back a fixed-size record per image (max_per_image + 28 rows, detect_bgr's): max_per_image "
                         "must be > 0; the unlimited form (max_per_image <= 0) is the one-by-one loop's")


def _enqueue_batch(sess, net, stage, n_valid, max_per_image, thresh, ring):
    """stage: B same-size BGR images [B,h,w,3] on the device.  Preprocessing (one launch), the chain, the post-processing and ONE
    non-blocking copy of the batch's record into pinned memory are enqueued; nothing waits.  -> _Pending"""
    B, h, w = int(stage.shape[0]), int(stage.shape[1]), int(stage.shape[2])
    im_scale, OH, OW = ops.prep_image_shape(h, w, cfg.TEST.SCALES[0], cfg.TEST.MAX_SIZE)
    with net.shape_scope(sess, (B, OH, OW, 4), (OH, OW)):        # the staged batch belongs to its (batch, shape) scope, like detect_bgr's image
        img = sess.buf(net._tag + "/image", (B, OH, OW, 4))
    ops.prep_image_batched(stage, cfg.PIXEL_MEANS, im_scale, (OH, OW), out=img, out_c=4)
    _check_max_per_image(max_per_image)
    max_out = max_per_image + 28
    im_info = np.array([OH, OW, im_scale], dtype=np.float32)
    # the record of THIS batch: a later batch of the same shape writes its own, so a deferred read-back never sees another batch's rows
    rec = torch.empty((B * max_out * 6 + B,), dtype=torch.float32, device=stage.device)
    net.detect_device(sess, img, im_info, (h, w), max_per_image=max_per_image, thresh=thresh,
                      out=rec[:B * max_out * 6].view(B, max_out, 6), count=rec[B * max_out * 6:].view(torch.int32))
    p = _Pending()
    host, k = ring.take(rec.numel() * 4)
    p.host = host.view(torch.float32)
    p.host.copy_(rec, non_blocking=True)
    p.ev = ring.mark(k)
    p.B, p.n_valid, p.max_out, p.num_classes = B, int(n_valid), max_out, net._num_classes
    return p


def _finish_batch(p):
    """waits for the batch's record and returns the per-class lists of its first n_valid images (padded slots are dropped here)"""
    p.ev.synchronize()
    a = p.host.numpy()
    dets = a[:p.B * p.max_out * 6].reshape(p.B, p.max_out, 6)
    cnt = a[p.B * p.max_out * 6:].view(np.int32)
    return [_per_class(dets[b, :min(int(cnt[b]), p.max_out)], p.num_classes) for b in range(p.n_valid)]


def _stage_batch(sess, ims):
    """B same-size BGR images -> one [B,h,w,3] device tensor: a device batch as it is, a numpy batch or a list of numpy images in one
    stacked H2D copy, a list of device images stacked on the device."""
    if torch.is_tensor(ims):
        return ims.contiguous()
    if isinstance(ims, np.ndarray) or isinstance(ims[0], np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(np.stack(ims))).to(sess.device, non_blocking=True)
    return torch.stack(list(ims))


def detect_bgr_batch(sess, net, ims, n_valid=None, max_per_image=100, thresh=0.):
    """detect_bgr of B same-size raw BGR images (uint8 or float32; [B,h,w,3] or a list of [h,w,3], numpy or device) in ONE chain: one
    preprocessing launch (frcnn_prep_image_batched), one batched forward + post-processing (Network.detect_device), one read-back.
    The first n_valid images count (the rest pad the batch to a size whose graph exists); returns their per-class lists, each identical
    to detect_bgr of that image alone.  One synchronous batch (it allocates its pinned record and waits for it): a loop over many batches
    is detect_paths_batched, which reuses two pinned records and keeps a batch in flight."""
    _check_max_per_image(max_per_image)
    stage = _stage_batch(sess, ims)
    assert stage.dim() == 4 and stage.shape[3] == 3
    n_valid = int(stage.shape[0]) if n_valid is None else int(n_valid)
    assert 1 <= n_valid <= stage.shape[0]
    return _finish_batch(_enqueue_batch(sess, net, stage, n_valid, max_per_image, thresh, _PinnedRing(1)))


def plan_batches(sizes, batch):
    """sizes: the source (h, w) of every image, by image index.  -> ordered list of (indices, pad): the images of one launch and how many
    times the last of them is repeated to fill it.  Images are grouped by exact source size (equal size = equal im_scale, blob shape and
    im_info, what a batch needs), groups in order of first appearance, indices ascending inside a group.  A group gives len // batch full
    batches; a remainder of r images is one batch padded to `batch` if 2 r >= batch, else r single images -- so a shape captures at most
    two graphs, (batch, shape) and (1, shape), and all work of one shape is contiguous (cfg.HIP.GRAPH_CACHE_SHAPES keeps 4).
    batch = 1: one single-image entry per image in the original order."""
    batch = int(batch)
    assert batch >= 1
    if batch == 1:
        return [([i], 0) for i in range(len(sizes))]
    groups = {}
    for i, (h, w) in enumerate(sizes):
        groups.setdefault((int(h), int(w)), []).append(i)
    plan = []
    for idx in groups.values():
        full = len(idx) // batch * batch
        plan += [(idx[k:k + batch], 0) for k in range(0, full, batch)]
        rem = idx[full:]
        if rem and 2 * len(rem) >= batch:
            plan.append((rem, batch - len(rem)))
        else:
            plan += [([i], 0) for i in rem]
    return plan


def detect(sess, net, blob, im_scale, im_shape, max_per_image=100, thresh=0.):
    """Whole per-image body of test_net (test.py:156-180) on the GPU -> all_boxes-style list over
    classes of [n,5] arrays (x1,y1,x2,y2,score)."""
    im_info = np.array([blob.shape[1], blob.shape[2], im_scale], dtype=np.float32)
    img = net._stage_image(sess, blob, im_info)
    dets, cnt = net.detect_device(sess, img, im_info, im_shape, max_per_image=max_per_image, thresh=thresh)
    n = min(int(cnt.item()), dets.shape[0])
    rec = dets[:n].cpu().numpy()
    out = [np.zeros((0, 5), dtype=np.float32) for _ in range(net._num_classes)]
    for j in range(1, net._num_classes):
        out[j] = rec[rec[:, 5] == j, :5]
    return out


def apply_nms(all_boxes, thresh):
    """test.py:109-135: non-maximum suppression (the device NMS behind model.nms_wrapper.nms) on every all_boxes[cls][image]
    of a finished test_net run; degenerate boxes (x2 <= x1 or y2 <= y1) are dropped first.  Returns a new nested list."""
    from model.nms_wrapper import nms
    num_classes, num_images = len(all_boxes), len(all_boxes[0])
    nms_boxes = [[[] for _ in range(num_images)] for _ in range(num_classes)]
    for c in range(num_classes):
        for i in range(num_images):
            dets = all_boxes[c][i]
            if isinstance(dets, list) or len(dets) == 0:
                continue
            dets = np.asarray(dets, dtype=np.float32)
            dets = dets[(dets[:, 2] > dets[:, 0]) & (dets[:, 3] > dets[:, 1])]
            if dets.shape[0] == 0:
                continue
            keep = nms(dets, thresh)
            if len(keep) == 0:
                continue
            nms_boxes[c][i] = dets[keep, :].copy()
    return nms_boxes


def imdb_images(imdb):
    """BGR uint8 images of an imdb (datasets.pascal_voc), decoded with PIL (cv2 is not available here; both wrap libjpeg, the
    decoded pixels may differ in the last bit from cv2.imread's).  cfg.HIP.JPEG_DEVICE: the same pixels as device tensors from a
    frcnn_hip.jpeg.JpegPrefetcher (host Huffman stage on worker threads, IDCT + colour on the device; detect_bgr takes either)."""
    if cfg.HIP.JPEG_DEVICE:
        from frcnn_hip.jpeg import JpegPrefetcher
        for im in JpegPrefetcher([imdb.image_path_at(i) for i in range(imdb.num_images)], torch.device("cuda", torch.cuda.current_device())):
            yield im
        return
    from PIL import Image
    for i in range(imdb.num_images):
        yield np.ascontiguousarray(np.asarray(Image.open(imdb.image_path_at(i)).convert("RGB"))[:, :, ::-1])


def image_sizes(paths):
    """source (h, w) of every file from its header, nothing decoded"""
    from PIL import Image
    sizes = []
    for p in paths:
        with Image.open(p) as im:
            sizes.append((im.size[1], im.size[0]))
    return sizes


def detect_paths_batched(sess, net, paths, batch, max_per_image=100, thresh=0., on_image=None, on_start=None):
    """detect_bgr of every image file of `paths`, same-size images `batch` at a time (plan_batches) -> per-class lists by index into
    `paths`, the bits of the one-by-one loop.  The files are decoded in plan order -- a JpegPrefetcher writing each image straight into
    its slot of the batch's device buffer under cfg.HIP.JPEG_DEVICE, PIL into a pinned buffer and one copy per batch otherwise.  One
    batch stays in flight: a batch's record is read after the NEXT batch has been enqueued, so the host never waits on the batch it has
    just launched; the last read-back is the only wait with nothing behind it.  on_image(i): called once per finished image; on_start(): called once, after
    the pass over the file headers and before the first image is decoded.  max_per_image must be > 0 (checked before any work)."""
    _check_max_per_image(max_per_image)
    return run_paths_batched(sess, paths, batch, lambda stage, idx, n, ring: _enqueue_batch(sess, net, stage, n, max_per_image, thresh, ring),
                             _finish_batch, on_image, on_start)


def run_paths_batched(sess, paths, batch, enqueue, finish, on_image=None, on_start=None):
    """The loop of detect_paths_batched for any per-batch work (tools/rpn_recall.py runs the RPN and the recall matcher through it):
    enqueue(stage [B,h,w,3] uint8 on the device, idx, n_valid, ring) enqueues a batch's launches and ONE non-blocking copy of its record
    into a pinned buffer taken from `ring` (a _PinnedRing) and returns a pending object without waiting; finish(pending) waits for that
    record and returns one result per valid image.  -> the results by index into `paths`."""
    sizes = image_sizes(paths)
    plan = plan_batches(sizes, batch)
    order = [i for idx, _ in plan for i in idx]
    results = [None] * len(paths)
    records, stages = _PinnedRing(2), _PinnedRing(2)
    on_device = bool(cfg.HIP.JPEG_DEVICE)
    if on_device:
        from frcnn_hip.jpeg import JpegPrefetcher
        source = JpegPrefetcher([paths[i] for i in order], sess.device, depth=max(8, 2 * int(batch)))
    else:
        from frcnn_hip.jpeg import pil_bgr
        source = (pil_bgr(paths[i]) for i in order)

    def consume(idx, pending):
        for i, per_class in zip(idx, finish(pending)):
            results[i] = per_class
            if on_image is not None:
                on_image(i)

    try:
        prev = None
        if on_start is not None:
            on_start()
        for idx, pad in plan:
            n, B = len(idx), len(idx) + pad
            if on_device:
                stage = torch.empty((B,) + tuple(sizes[idx[0]]) + (3,), dtype=torch.uint8, device=sess.device)
                for k in range(n):
                    source.read_into(stage[k])
            else:
                ims = [next(source) for _ in range(n)]
                host, slot = stages.take(B * ims[0].size)
                host = host.view((B,) + ims[0].shape)
                for k in range(n):
                    host[k].copy_(torch.from_numpy(ims[k]))
                stage = torch.empty(host.shape, dtype=torch.uint8, device=sess.device)
                stage[:n].copy_(host[:n], non_blocking=True)
                stages.mark(slot)
            for k in range(n, B):
                stage[k].copy_(stage[n - 1])                 # padding: the last image again, device to device
            pending = enqueue(stage, idx, n, records)
            if prev is not None:
                consume(*prev)
            prev = (idx, pending)
        if prev is not None:
            consume(*prev)
    finally:
        if hasattr(source, "close"):
            source.close()
    return results


def test_net_imdb(sess, net, imdb, output_dir, max_per_image=100, thresh=0.):
    """The reference's test_net(sess, net, imdb, weights_filename) (test.py:139-192): every image of the imdb through the
    raw-image device path, then detections.pkl + imdb.evaluate_detections.  cfg.HIP.TEST_BATCH_IMAGES > 1: same-size images that many
    at a time (detect_paths_batched); all_boxes is the same, array for array.  max_per_image <= 0 (no limit per image: a record of
    any length) keeps the one-by-one loop whatever the switch says."""
    import os
    import pickle
    all_boxes = [[[] for _ in range(imdb.num_images)] for _ in range(imdb.num_classes)]
    _t = {'im_detect': Timer(), 'misc': Timer()}
    if int(cfg.HIP.TEST_BATCH_IMAGES) > 1 and max_per_image > 0:
        done = [0]

        def on_image(i):
            done[0] += 1
            _t['im_detect'].toc()                        # time since the last finished image: the average is the loop's time per image
            _t['im_detect'].tic()
            print('im_detect: {:d}/{:d} {:.3f}s {:.3f}s'.format(done[0], imdb.num_images, _t['im_detect'].average_time, _t['misc'].average_time))
        per_image = detect_paths_batched(sess, net, [imdb.image_path_at(i) for i in range(imdb.num_images)], int(cfg.HIP.TEST_BATCH_IMAGES),
                                         max_per_image, thresh, on_image, on_start=_t['im_detect'].tic)
        for i, per_class in enumerate(per_image):
            for j in range(1, imdb.num_classes):
                all_boxes[j][i] = per_class[j]
    else:
        for i, im in enumerate(imdb_images(imdb)):
            _t['im_detect'].tic()
            per_class = detect_bgr(sess, net, im, max_per_image, thresh)
            _t['im_detect'].toc()
            for j in range(1, imdb.num_classes):
                all_boxes[j][i] = per_class[j]
            print('im_detect: {:d}/{:d} {:.3f}s {:.3f}s'.format(i + 1, imdb.num_images, _t['im_detect'].average_time, _t['misc'].average_time))
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'detections.pkl'), 'wb') as f:
        pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)
    print('Evaluating detections')
    imdb.evaluate_detections(all_boxes, output_dir)
    return all_boxes


def test_net(sess, net, images, num_classes=None, max_per_image=100, thresh=0., imdb=None, output_dir=None):
    """images: iterable of (blob, im_scale, im_shape).  Returns all_boxes[cls][image] like the
    reference; prints the same per-image timing line (test.py:183-185).  With an imdb (datasets.pascal_voc) the
    detections are written and evaluated as at test.py:187-192: `detections.pkl` + imdb.evaluate_detections."""
    images = list(images)
    num_classes = net._num_classes if num_classes is None else num_classes
    all_boxes = [[[] for _ in range(len(images))] for _ in range(num_classes)]
    _t = {'im_detect': Timer(), 'misc': Timer()}
    for i, (blob, im_scale, im_shape) in enumerate(images):
        _t['im_detect'].tic()
        per_class = detect(sess, net, blob, im_scale, im_shape, max_per_image, thresh)
        torch.cuda.synchronize()
        _t['im_detect'].toc()
        _t['misc'].tic()
        for j in range(1, num_classes):
            all_boxes[j][i] = per_class[j]
        _t['misc'].toc()
        print('im_detect: {:d}/{:d} {:.3f}s {:.3f}s'.format(i + 1, len(images), _t['im_detect'].average_time,
                                                            _t['misc'].average_time))
    if imdb is not None and output_dir is not None:
        import os
        import pickle
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, 'detections.pkl'), 'wb') as f:
            pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)
        print('Evaluating detections')
        imdb.evaluate_detections(all_boxes, output_dir)
    return all_boxes
