"""TEST INFRASTRUCTURE ONLY -- inputs for the COCO evaluator tests (tests/test_coco_cpu.py, tests/test_coco_gpu.py): a seeded random
annotation / result set with crowds, tied scores and areas on the range boundaries, the hand-derivable known-answer cases, and the
layout of fixtures/coco_eval_ref.py's per-group results in the CSR order of datasets.coco_eval.build_groups."""
import numpy as np


def dataset(images, cats, anns):
    """A datasets.coco_api.COCO over in-memory lists."""
    from datasets.coco_api import COCO
    c = COCO()
    c.dataset = dict(images=[dict(id=i, width=640, height=480) for i in images], categories=[dict(id=k, name="c%d" % k) for k in cats],
                     annotations=[dict(a, id=n + 1) for n, a in enumerate(anns)])
    c.createIndex()
    return c


def gt(image, cat, bbox, area=None, crowd=0):
    return dict(image_id=image, category_id=cat, bbox=[float(v) for v in bbox], area=float(bbox[2] * bbox[3] if area is None else area), iscrowd=crowd)


def det(image, cat, bbox, score):
    return dict(image_id=image, category_id=cat, bbox=[float(v) for v in bbox], score=float(score))


def random_set(seed=0, n_images=40, n_cats=12, max_det=130, max_gt=40, crowd_frac=0.15, fill=0.35):
    """(image ids, category ids (gapped), gt annotations, results).  Per (image, category): with probability `fill` 0..max_gt gts and
    0..max_det detections (sizes skewed to small, a few at the maximum), else nothing or only one of the two kinds.  Detections are
    jittered copies of gts or clutter; scores come from a grid of 50 values, so ties are the rule; some gt areas and detection boxes sit
    exactly on 32^2 and 96^2."""
    rng = np.random.RandomState(seed)
    images = [int(v) for v in np.sort(rng.choice(10 ** 5, n_images, replace=False))]
    cats = [int(v) for v in np.sort(rng.choice(np.arange(1, 91), n_cats, replace=False))]
    gts, dts = [], []

    def size(mx):
        u = rng.rand()
        return mx if u < 0.06 else int(mx * rng.rand() ** 3)
    for c in cats:
        for im in images:
            u = rng.rand()
            G = size(max_gt) if u < fill + 0.1 else 0
            D = size(max_det) if (u < fill or u > 0.9) else 0
            boxes = []
            for _ in range(G):
                w, h = rng.choice([32.0, 96.0, 16.0, 64.0, float(np.round(rng.uniform(4, 200), 1))]), float(np.round(rng.uniform(4, 200), 1))
                if rng.rand() < 0.2:
                    h = w                                          # 32 x 32 and 96 x 96: areas exactly on the boundaries
                x, y = float(np.round(rng.uniform(0, 400), 1)), float(np.round(rng.uniform(0, 300), 1))
                boxes.append([x, y, float(w), h])
                gts.append(gt(im, c, boxes[-1], area=w * h if rng.rand() < 0.5 else float(np.round(w * h * rng.uniform(0.3, 1.0), 2)),
                              crowd=int(rng.rand() < crowd_frac)))
            for _ in range(D):
                if boxes and rng.rand() < 0.7:
                    b = list(boxes[rng.randint(len(boxes))])
                    if rng.rand() < 0.6:
                        b = [b[0] + rng.randint(-3, 4) * 2.0, b[1] + rng.randint(-3, 4) * 2.0, max(1.0, b[2] + rng.randint(-2, 3) * 4.0),
                             max(1.0, b[3] + rng.randint(-2, 3) * 4.0)]
                else:
                    b = [float(np.round(rng.uniform(0, 400), 1)), float(np.round(rng.uniform(0, 300), 1)), float(rng.choice([32.0, 96.0, 50.5])),
                         float(rng.choice([32.0, 96.0, 20.25]))]
                dts.append(det(im, c, b, rng.randint(1, 51) / 50.0))
    perm = rng.permutation(len(dts))                               # results arrive in no particular order
    return images, cats, gts, [dts[i] for i in perm]


def ref_flags(groups, csr, n_area=4, n_thr=10):
    """fixtures/coco_eval_ref.evaluate()'s per-group lists laid out like ops.coco_match's outputs for the CSR `csr`."""
    n_det, n_gt = int(csr['det_off'][-1]), int(csr['gt_off'][-1])
    matched, ignored = np.zeros((n_area, n_thr, n_det), dtype=np.uint8), np.zeros((n_area, n_thr, n_det), dtype=np.uint8)
    gt_ignored, iou = np.zeros((n_area, n_gt), dtype=np.uint8), []
    assert len(groups) == len(csr['group'])
    for n, key in enumerate(csr['group']):
        e = groups[(int(key) // csr['n_images'], int(key) % csr['n_images'])]
        d0, d1, g0, g1 = csr['det_off'][n], csr['det_off'][n + 1], csr['gt_off'][n], csr['gt_off'][n + 1]
        assert d1 - d0 == len(e['order']) and g1 - g0 == len(e['gt_ignored'][0])
        for a in range(n_area):
            gt_ignored[a, g0:g1] = e['gt_ignored'][a]
            if d1 > d0:
                matched[a, :, d0:d1] = np.array(e['matched'][a], dtype=np.uint8).reshape(n_thr, -1)
                ignored[a, :, d0:d1] = np.array(e['ignored'][a], dtype=np.uint8).reshape(n_thr, -1)
        iou.extend(v for row in e['iou'] for v in row)
    return matched, ignored, gt_ignored, np.array(iou, dtype=np.float64)
