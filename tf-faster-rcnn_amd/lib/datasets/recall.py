"""datasets.recall -- proposal recall, the reference's imdb.evaluate_recall (lib/datasets/imdb.py:126-214) in three parts:

select_gt   host numpy on one roidb entry: the ground-truth rows that count (gt_classes > 0, max gt_overlaps == 1 -- which drops crowd
            rows --, seg_areas inside one of the reference's eight inclusive ranges);
match_*     the greedy matching of every image, `frcnn_proposal_recall` on the device (match_device) or the C host statement of the
            same rule through ctypes (match_host, what runs on a machine without a GPU); csrc/recall_math.h states the rule;
summarise   the sorted overlaps, the recall per IoU threshold and their mean, as the reference returns them.

Per image the reference repeats, once per ground-truth box: among the unused gts and unused candidates take every gt's best candidate
(the first of equal ones), then the best-covered gt (the first of equal ones); record that IoU; retire both.  A gt nothing overlaps is
recorded as 0.0 and still retires a candidate; with fewer candidates than gts the reference's `assert gt_ovr >= 0` fires, and so do
match_host / match_device (AssertionError).  An image without candidates records nothing; its gts still count in num_pos."""
import numpy as np

AREAS = {'all': 0, 'small': 1, 'medium': 2, 'large': 3, '96-128': 4, '128-256': 5, '256-512': 6, '512-inf': 7}
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2], [96 ** 2, 128 ** 2], [128 ** 2, 256 ** 2],
               [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]]


def default_thresholds():
    return np.arange(0.5, 0.95 + 1e-5, 0.05)


def select_gt(roidb_entry, area='all'):
    """Row indices of the entry's ground truth inside the area range (imdb.py:157-164), ascending."""
    assert area in AREAS, 'unknown area range: {}'.format(area)
    lo, hi = AREA_RANGES[AREAS[area]]
    ov = roidb_entry['gt_overlaps']
    ov = ov.toarray() if hasattr(ov, 'toarray') else np.asarray(ov)
    max_ov = ov.max(axis=1) if ov.shape[0] else np.zeros(0)
    gt_inds = np.where((np.asarray(roidb_entry['gt_classes']) > 0) & (max_ov == 1))[0]
    areas = np.asarray(roidb_entry['seg_areas'])[gt_inds]
    return gt_inds[(areas >= lo) & (areas <= hi)]


def pack(candidates, gt_boxes, limit=None):
    """Lists over images of [n,4] candidates and [g,4] ground truth -> the arrays of one frcnn_proposal_recall call: dict(boxes f32
    [N,4], start int64, count int32, scale f32 (ones), gt f64 [G,4], gt_off int64, max_boxes, limit)."""
    assert len(candidates) == len(gt_boxes)
    cands = [np.asarray(c, dtype=np.float32).reshape(-1, 4) for c in candidates]
    gts = [np.asarray(g).astype(np.float64).reshape(-1, 4) for g in gt_boxes]
    count = np.array([c.shape[0] for c in cands], dtype=np.int32)
    return dict(boxes=np.concatenate(cands) if cands else np.zeros((0, 4), dtype=np.float32),
                start=(np.cumsum(count, dtype=np.int64) - count).astype(np.int64), count=count, scale=np.ones(len(cands), dtype=np.float32),
                gt=np.concatenate(gts) if gts else np.zeros((0, 4)), gt_off=np.concatenate([[0], np.cumsum([g.shape[0] for g in gts])]).astype(np.int64),
                max_boxes=int(count.max()) if count.size else 0, limit=limit)


def _collect(p, gt_iou, ran_out):
    """the recorded slots of the images that had candidates, image after image (what the reference hstacks), and num_pos"""
    assert not np.any(ran_out), 'gt_ovr >= 0: image(s) %s have fewer candidates than ground-truth boxes' % np.nonzero(ran_out)[0].tolist()
    off = p['gt_off']
    keep = [gt_iou[off[i]:off[i + 1]] for i in range(len(p['count'])) if p['count'][i] > 0]
    return (np.concatenate(keep) if keep else np.zeros(0)), int(off[-1] - off[0])


def match_host(candidates, gt_boxes, limit=None):
    """-> (gt_overlaps float64, unsorted: the picks of every image with candidates in image order; num_pos).  The C host statement."""
    from frcnn_hip import ops
    p = pack(candidates, gt_boxes, limit)
    return _collect(p, *ops.proposal_recall_host(p['boxes'], p['start'], p['count'], p['scale'], p['gt'], p['gt_off'], p['max_boxes'], limit))


def match_device(candidates, gt_boxes, limit=None, device=None):
    """The same from frcnn_proposal_recall (csrc/recall.hip); no fallback: without the library or a GPU this raises."""
    import torch
    from frcnn_hip import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    p = pack(candidates, gt_boxes, limit)
    t = {k: torch.from_numpy(p[k]).to(dev) for k in ('boxes', 'start', 'count', 'scale', 'gt', 'gt_off')}
    gt_iou, ran_out = ops.proposal_recall(t['boxes'], t['start'], t['count'], t['scale'], t['gt'], t['gt_off'], p['max_boxes'], limit)
    torch.cuda.current_stream().synchronize()
    return _collect(p, gt_iou.cpu().numpy(), ran_out.cpu().numpy())


def summarise(gt_overlaps, num_pos, thresholds=None):
    """imdb.py:203-214: {'ar', 'recalls', 'thresholds', 'gt_overlaps' (sorted)}; num_pos == 0 divides by zero as the reference does."""
    gt_overlaps = np.sort(np.asarray(gt_overlaps, dtype=np.float64))
    if thresholds is None:
        thresholds = default_thresholds()
    recalls = np.zeros_like(thresholds)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i, t in enumerate(thresholds):
            recalls[i] = (gt_overlaps >= t).sum() / float(num_pos)
    return {'ar': recalls.mean(), 'recalls': recalls, 'thresholds': thresholds, 'gt_overlaps': gt_overlaps}


def evaluate(roidb, candidate_boxes=None, thresholds=None, area='all', limit=None, match=None):
    """imdb.evaluate_recall on a roidb list; match 'device' / 'host' / None (device when CUDA is available, as COCOeval chooses)."""
    if match is None:
        import torch
        match = 'device' if torch.cuda.is_available() else 'host'
    assert match in ('device', 'host'), match
    assert area in AREAS, 'unknown area range: {}'.format(area)
    cands, gts = [], []
    for i, e in enumerate(roidb):
        gts.append(np.asarray(e['boxes'])[select_gt(e, area), :])
        if candidate_boxes is None:                      # imdb.py:167-171: the non-ground-truth boxes of this roidb
            cands.append(np.asarray(e['boxes'])[np.where(np.asarray(e['gt_classes']) == 0)[0], :])
        else:
            cands.append(candidate_boxes[i])
    gt_overlaps, num_pos = (match_device if match == 'device' else match_host)(cands, gts, limit)
    return summarise(gt_overlaps, num_pos, thresholds)
