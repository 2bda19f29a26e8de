"""datasets.coco_eval -- the COCO bbox evaluator (evaluate -> accumulate -> summarize) the reference reaches through
`pycocotools.cocoeval.COCOeval` (lib/datasets/coco.py:218-229).  pycocotools is not installable here, so the published protocol is
restated from its description (parity with the published evaluator is UNPINNED in this project's sense, like TensorFlow and cv2;
fixtures/coco_eval_ref.py is the independent second statement the tests compare with).

Protocol.  iouThrs = linspace(.5, .95, 10), recThrs = linspace(0, 1, 101), maxDets = [1, 10, 100], areaRng = all / small / medium /
large with both ends inclusive, one evaluation per category.  Per (image, category) group the detections are stable-sorted by -score
and cut to maxDets[-1]; IoU on xywh boxes in float64 without "+1", i / (crowd ? det area : det area + gt area - i), 0 unless both
overlaps are positive.  Per area range a gt is ignored if it is a crowd or its annotation area lies outside the range; gts are visited
non-ignored first, each class in file order.  Per threshold t a detection (in score order) starts with best = min(t, 1 - 1e-10) and
walks the gts: skip one already matched at t unless it is a crowd; stop once a non-ignored match is held and the ignored gts begin; skip
if iou < best; else take it.  A matched detection inherits its gt's ignore flag, an unmatched one is ignored if its own w*h lies outside
the range.  Accumulate and summarize are the usual cumulative tp / fp -> precision envelope at 101 recall points -> 12 means over the
cells > -1.

The grouping into a CSR layout and accumulate / summarize are host numpy in float64; IoU + matching is `frcnn_coco_match` on the device
(match="device") or the numpy statement below (match="host", what tools/reval.py uses on a machine without a GPU)."""
import numpy as np


class Params(object):
    def __init__(self):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = 'bbox'


def build_groups(gt_anns, dt_anns, img_ids, cat_ids, max_det):
    """The non-empty (category, image) groups, category-major, as CSR arrays: detections per group stable-sorted by -score and cut to
    max_det, gts in file order.  Returns a dict of numpy arrays (see the keys below)."""
    I = len(img_ids)
    img_pos, cat_pos = {v: i for i, v in enumerate(img_ids)}, {v: i for i, v in enumerate(cat_ids)}
    gt_anns = [a for a in gt_anns if a['image_id'] in img_pos and a['category_id'] in cat_pos]
    dt_anns = [a for a in dt_anns if a['image_id'] in img_pos and a['category_id'] in cat_pos]

    def keys(anns):
        return np.array([cat_pos[a['category_id']] * I + img_pos[a['image_id']] for a in anns], dtype=np.int64).reshape(-1)

    def boxes(anns):
        return np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(-1, 4)
    kg, kd = keys(gt_anns), keys(dt_anns)
    score = np.array([a['score'] for a in dt_anns], dtype=np.float64).reshape(-1)
    og = np.argsort(kg, kind='stable')
    od = np.lexsort((-score, kd))                                  # by group, then -score; stable: ties keep the results' order
    kd_s = kd[od]
    rank = np.arange(len(od)) - np.searchsorted(kd_s, kd_s, side='left')
    od = od[rank < max_det]
    kg, kd = kg[og], kd[od]
    groups = np.union1d(kg, kd)
    gt_xywh = boxes(gt_anns)[og]
    return dict(group=groups, n_images=I,
                det_off=np.searchsorted(kd, np.append(groups, np.iinfo(np.int64).max), side='left').astype(np.int64),
                gt_off=np.searchsorted(kg, np.append(groups, np.iinfo(np.int64).max), side='left').astype(np.int64),
                det_xywh=np.ascontiguousarray(boxes(dt_anns)[od]), det_score=score[od], det_id=np.array([dt_anns[i]['id'] for i in od], dtype=np.int64),
                gt_xywh=np.ascontiguousarray(gt_xywh), gt_area=np.array([gt_anns[i]['area'] for i in og], dtype=np.float64).reshape(-1),
                gt_crowd=np.array([1 if gt_anns[i].get('iscrowd', 0) else 0 for i in og], dtype=np.uint8).reshape(-1),
                gt_id=np.array([gt_anns[i]['id'] for i in og], dtype=np.int64))


def n_pairs(csr):
    return int(np.sum(np.diff(csr['det_off']) * np.diff(csr['gt_off'])))


def iou_xywh(d, g, crowd):
    """[D,4] x [G,4] -> [D,G] float64; the operation order of csrc/coco_eval.hip (bit-equal)."""
    dx2, dy2, gx2, gy2 = d[:, 0] + d[:, 2], d[:, 1] + d[:, 3], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    iw = np.minimum(dx2[:, None], gx2[None, :]) - np.maximum(d[:, None, 0], g[None, :, 0])
    ih = np.minimum(dy2[:, None], gy2[None, :]) - np.maximum(d[:, None, 1], g[None, :, 1])
    inter = iw * ih
    da = (d[:, 2] * d[:, 3])[:, None]
    union = np.where(crowd[None, :] != 0, da, (da + (g[:, 2] * g[:, 3])[None, :]) - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where((iw <= 0) | (ih <= 0), 0.0, inter / union)


def _last_argmax(v):
    return v.shape[-1] - 1 - np.argmax(v[..., ::-1], axis=-1)


def match_host(csr, iou_thrs, area_rng, want_iou=False):
    """The numpy matcher: (det_matched [A,T,n_det] u8, det_ignored [A,T,n_det] u8, gt_ignored [A,n_gt] u8, iou [n_pairs] f64 | None),
    the outputs of frcnn_hip.ops.coco_match.  Within one class of gts (ignored or not) the sequential walk keeps the LAST gt of maximal
    IoU >= the threshold among those still available, and an ignored gt is only reached when no non-ignored one qualified: that is
    what the array expressions below select, for all (area, threshold) pairs at once, detection after detection."""
    iou_thrs, area_rng = np.asarray(iou_thrs, dtype=np.float64), np.asarray(area_rng, dtype=np.float64).reshape(-1, 2)
    A, T = area_rng.shape[0], iou_thrs.shape[0]
    det_off, gt_off = csr['det_off'], csr['gt_off']
    n_det, n_gt = int(det_off[-1]), int(gt_off[-1])
    matched, ignored = np.zeros((A, T, n_det), dtype=np.uint8), np.zeros((A, T, n_det), dtype=np.uint8)
    lo, hi = area_rng[:, 0:1], area_rng[:, 1:2]
    gt_ignored = ((csr['gt_crowd'][None, :] != 0) | (csr['gt_area'][None, :] < lo) | (csr['gt_area'][None, :] > hi)).astype(np.uint8)
    det_area = csr['det_xywh'][:, 2] * csr['det_xywh'][:, 3]
    det_out = (det_area[None, :] < lo) | (det_area[None, :] > hi)                                    # [A, n_det]
    thr = np.minimum(iou_thrs, 1 - 1e-10)[None, :, None]
    ious = []
    ai, ti = np.meshgrid(np.arange(A), np.arange(T), indexing='ij')
    for k in range(len(det_off) - 1):
        d0, d1, g0, g1 = det_off[k], det_off[k + 1], gt_off[k], gt_off[k + 1]
        D, G = d1 - d0, g1 - g0
        if D == 0 or G == 0:
            ignored[:, :, d0:d1] = det_out[:, None, d0:d1]
            continue
        crowd = csr['gt_crowd'][g0:g1] != 0
        iou = iou_xywh(csr['det_xywh'][d0:d1], csr['gt_xywh'][g0:g1], crowd)
        if want_iou:
            ious.append(iou.reshape(-1))
        ign = gt_ignored[:, None, g0:g1] != 0                      # [A,1,G]
        taken = np.zeros((A, T, G), dtype=bool)
        for d in range(D):
            cand = (~taken | crowd[None, None, :]) & (iou[d][None, None, :] >= thr)
            v1 = np.where(cand & ~ign, iou[d][None, None, :], -1.0)
            v2 = np.where(cand & ign, iou[d][None, None, :], -1.0)
            has1, has2 = v1.max(axis=-1) >= 0, v2.max(axis=-1) >= 0
            m = np.where(has1, _last_argmax(v1), _last_argmax(v2))
            has = has1 | has2
            matched[:, :, d0 + d] = has
            ignored[:, :, d0 + d] = np.where(has, gt_ignored[ai, g0 + m], det_out[:, None, d0 + d])
            taken[ai[has], ti[has], m[has]] = True
    return matched, ignored, gt_ignored, (np.concatenate(ious) if ious else np.zeros(0)) if want_iou else None


def match_device(csr, iou_thrs, area_rng, want_iou=False, device=None):
    """The same outputs from frcnn_coco_match (csrc/coco_eval.hip); no fallback: without the library or a GPU this raises."""
    import torch
    from frcnn_hip import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    out = ops.coco_match(up(csr['det_xywh'], np.float64), csr['det_off'], up(csr['gt_xywh'], np.float64),
                         up(csr['gt_area'], np.float64), up(csr['gt_crowd'], np.uint8), csr['gt_off'],
                         up(iou_thrs, np.float64), up(np.asarray(area_rng, dtype=np.float64).reshape(-1, 2), np.float64), want_iou)
    torch.cuda.current_stream().synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


class COCOeval(object):
    """`COCOeval(cocoGt, cocoDt[, match])`: cocoGt a datasets.coco_api.COCO, cocoDt its loadRes(...); evaluate(), accumulate(),
    summarize() as in the published tool; results in .eval ('precision' [T,R,K,A,M], 'recall' [T,K,A,M]) and .stats [12]."""

    def __init__(self, cocoGt, cocoDt, iouType='bbox', match=None):
        assert iouType == 'bbox', 'only bbox evaluation is provided'
        if match is None:
            import torch
            match = 'device' if torch.cuda.is_available() else 'host'
        assert match in ('device', 'host'), match
        self.cocoGt, self.cocoDt, self.match = cocoGt, cocoDt, match
        self.params = Params()
        self.params.imgIds, self.params.catIds = sorted(cocoGt.getImgIds()), sorted(cocoGt.getCatIds())
        self.eval, self.stats, self.csr = {}, [], None

    def evaluate(self):
        p = self.params
        p.imgIds, p.catIds, p.maxDets = list(np.unique(p.imgIds)), list(np.unique(p.catIds)), sorted(p.maxDets)
        self.csr = build_groups(self.cocoGt.dataset.get('annotations', []), self.cocoDt.dataset.get('annotations', []), p.imgIds, p.catIds, p.maxDets[-1])
        fn = match_device if self.match == 'device' else match_host
        self.det_matched, self.det_ignored, self.gt_ignored, _ = fn(self.csr, p.iouThrs, p.areaRng)

    def accumulate(self):
        p, c = self.params, self.csr
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
        det_off, gt_off = c['det_off'], c['gt_off']
        det_rank = np.arange(int(det_off[-1])) - np.repeat(det_off[:-1], np.diff(det_off))
        # groups are category-major: the groups, detections and gts of category k are contiguous
        first = np.searchsorted(c['group'], np.arange(K + 1) * c['n_images'], side='left')
        for k in range(K):
            d0, d1, g0, g1 = det_off[first[k]], det_off[first[k + 1]], gt_off[first[k]], gt_off[first[k + 1]]
            if first[k] == first[k + 1]:
                continue
            for a in range(A):
                npig = int(np.count_nonzero(self.gt_ignored[a, g0:g1] == 0))
                if npig == 0:
                    continue
                for m, max_det in enumerate(p.maxDets):
                    sel = np.nonzero(det_rank[d0:d1] < max_det)[0] + d0
                    sel = sel[np.argsort(-c['det_score'][sel], kind='mergesort')]
                    dtm, dtig = self.det_matched[a][:, sel] != 0, self.det_ignored[a][:, sel] != 0
                    tps = np.cumsum(dtm & ~dtig, axis=1).astype(np.float64)
                    fps = np.cumsum(~dtm & ~dtig, axis=1).astype(np.float64)
                    for t in range(T):
                        tp, fp = tps[t], fps[t]
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        q = np.zeros(R)
                        if nd:
                            pr = np.maximum.accumulate(pr[::-1])[::-1]          # non-increasing from the right
                            inds = np.searchsorted(rc, p.recThrs, side='left')
                            ok = inds < nd
                            q[ok] = pr[inds[ok]]
                        precision[t, :, k, a, m] = q
        self.eval = {'params': p, 'counts': [T, R, K, A, M], 'precision': precision, 'recall': recall}

    def _summarize(self, ap=1, iouThr=None, areaRng='all', maxDets=100, verbose=True):
        p = self.params
        iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        titleStr, typeStr = ('Average Precision', '(AP)') if ap == 1 else ('Average Recall', '(AR)')
        iouStr = '{:0.2f}:{:0.2f}'.format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
        aind = [i for i, lbl in enumerate(p.areaRngLbl) if lbl == areaRng]
        mind = [i for i, md in enumerate(p.maxDets) if md == maxDets]
        s = self.eval['precision'] if ap == 1 else self.eval['recall']
        if iouThr is not None:
            s = s[np.where(iouThr == p.iouThrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        if verbose:
            print(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
        return mean_s

    def summarize(self, verbose=True):
        assert self.eval, 'Please run accumulate() first'
        md = self.params.maxDets
        rows = [(1, None, 'all', md[2]), (1, .5, 'all', md[2]), (1, .75, 'all', md[2]), (1, None, 'small', md[2]), (1, None, 'medium', md[2]),
                (1, None, 'large', md[2]), (0, None, 'all', md[0]), (0, None, 'all', md[1]), (0, None, 'all', md[2]), (0, None, 'small', md[2]),
                (0, None, 'medium', md[2]), (0, None, 'large', md[2])]
        self.stats = np.array([self._summarize(ap, iouThr=t, areaRng=a, maxDets=m, verbose=verbose) for ap, t, a, m in rows], dtype=np.float64)
        return self.stats
