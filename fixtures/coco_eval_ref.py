"""TEST INFRASTRUCTURE ONLY -- a second statement of the COCO bbox evaluation protocol (tf-faster-rcnn_amd/lib/datasets/coco_eval.py
states it in its docstring), written as plain per-group Python loops over Python floats.  It shares no code with coco_eval.py and exists
so that the host matcher, the device kernel and the accumulate step have something independent to be compared with.

The published evaluator (pycocotools) is not installable where this project is built and is not part of the reference tree, so neither
statement could be run against it: parity with the published tool is UNPINNED in this project's sense (as for TensorFlow and cv2,
DESIGN.md); what the tests pin is that two independently written statements of the protocol, and the kernel, agree exactly, plus
hand-derivable known answers."""
import numpy as np

IOU_THRS = [float(v) for v in np.linspace(.5, 0.95, 10)]
REC_THRS = [float(v) for v in np.linspace(.0, 1.00, 101)]
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]]


def iou_one(d, g, crowd):
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    da = d[2] * d[3]
    return inter / (da if crowd else (da + g[2] * g[3]) - inter)


def evaluate_group(gts, dts, iou_thrs=IOU_THRS, area_rng=AREA_RNG, max_det=100):
    """gts: [{'bbox', 'area', 'iscrowd'}] in file order, dts: [{'bbox', 'score'}] in results order -> dict with `order` (indices into dts:
    stable by -score, cut), `iou` [D][G], and per area range `matched` [T][D], `ignored` [T][D], `gt_ignored` [G] (file order)."""
    order = sorted(range(len(dts)), key=lambda i: -dts[i]['score'])[:max_det]          # sorted() is stable
    D, G = len(order), len(gts)
    iou = [[iou_one(dts[i]['bbox'], g['bbox'], bool(g['iscrowd'])) for g in gts] for i in order]
    out = dict(order=order, iou=iou, matched=[], ignored=[], gt_ignored=[])
    for lo, hi in area_rng:
        gt_ig = [bool(g['iscrowd']) or g['area'] < lo or g['area'] > hi for g in gts]
        visit = [j for j in range(G) if not gt_ig[j]] + [j for j in range(G) if gt_ig[j]]
        matched, ignored = [], []
        for t in iou_thrs:
            taken = [False] * G
            row_m, row_i = [], []
            for d in range(D):
                best, m = min(t, 1 - 1e-10), -1
                for j in visit:
                    if taken[j] and not gts[j]['iscrowd']:
                        continue
                    if m > -1 and not gt_ig[m] and gt_ig[j]:
                        break
                    if iou[d][j] < best:
                        continue
                    best, m = iou[d][j], j
                if m > -1:
                    taken[m] = True
                    row_m.append(True)
                    row_i.append(gt_ig[m])
                else:
                    bb = dts[order[d]]['bbox']
                    area = bb[2] * bb[3]
                    row_m.append(False)
                    row_i.append(area < lo or area > hi)
            matched.append(row_m)
            ignored.append(row_i)
        out['matched'].append(matched)
        out['ignored'].append(ignored)
        out['gt_ignored'].append(gt_ig)
    return out


def evaluate(gt_anns, dt_anns, img_ids, cat_ids):
    """{(k, i): evaluate_group(...)} over category index k, image index i; groups with neither gts nor dets are absent."""
    groups, by_gt, by_dt = {}, {}, {}
    for a in gt_anns:                                              # buckets keep the file / results order
        by_gt.setdefault((a['image_id'], a['category_id']), []).append(a)
    for a in dt_anns:
        by_dt.setdefault((a['image_id'], a['category_id']), []).append(a)
    for k, c in enumerate(cat_ids):
        for i, im in enumerate(img_ids):
            gts, dts = by_gt.get((im, c), []), by_dt.get((im, c), [])
            if gts or dts:
                groups[(k, i)] = dict(evaluate_group(gts, dts), scores=None)
                groups[(k, i)]['scores'] = [dts[j]['score'] for j in groups[(k, i)]['order']]
    return groups


def accumulate(groups, n_images, n_cats):
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision, recall = -np.ones((T, R, n_cats, A, M)), -np.ones((T, n_cats, A, M))
    for k in range(n_cats):
        E = [groups[(k, i)] for i in range(n_images) if (k, i) in groups]
        if not E:
            continue
        for a in range(A):
            npig = sum(1 for e in E for ig in e['gt_ignored'][a] if not ig)
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                scores = [s for e in E for s in e['scores'][:max_det]]
                inds = sorted(range(len(scores)), key=lambda j: -scores[j])
                for t in range(T):
                    dm = [v for e in E for v in e['matched'][a][t][:max_det]]
                    di = [v for e in E for v in e['ignored'][a][t][:max_det]]
                    tp = fp = 0
                    rc, pr = [], []
                    for j in inds:
                        tp += 1 if (dm[j] and not di[j]) else 0
                        fp += 1 if (not dm[j] and not di[j]) else 0
                        rc.append(float(tp) / npig)
                        pr.append(float(tp) / (float(fp) + float(tp) + float(np.spacing(1))))
                    recall[t, k, a, m] = rc[-1] if rc else 0
                    for j in range(len(pr) - 1, 0, -1):
                        if pr[j] > pr[j - 1]:
                            pr[j - 1] = pr[j]
                    q = [0.0] * R
                    j = 0
                    for r, thr in enumerate(REC_THRS):              # first position with rc >= thr (rc is non-decreasing)
                        while j < len(rc) and rc[j] < thr:
                            j += 1
                        if j < len(rc):
                            q[r] = pr[j]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall):
    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    t50, t75 = 0, 5
    return np.array([mean(precision[:, :, :, 0, 2]), mean(precision[t50, :, :, 0, 2]), mean(precision[t75, :, :, 0, 2]),
                     mean(precision[:, :, :, 1, 2]), mean(precision[:, :, :, 2, 2]), mean(precision[:, :, :, 3, 2]),
                     mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
                     mean(recall[:, :, 1, 2]), mean(recall[:, :, 2, 2]), mean(recall[:, :, 3, 2])], dtype=np.float64)
