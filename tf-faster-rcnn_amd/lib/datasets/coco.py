"""datasets.coco -- the `coco(image_set, year)` imdb of the reference (lib/datasets/coco.py:27-312) without pycocotools: the annotation
index is datasets.coco_api.COCO, the bbox evaluation datasets.coco_eval.COCOeval (IoU + matching on the device).  Training side:
`gt_roidb` from the instances json -- boxes sanitised as at coco.py:138-145, crowd rows with gt_overlaps = -1 for every class, `width` /
`height` / `seg_areas` kept by the subclass's own append_flipped_images.  As with pascal_voc here there is no pickle cache of the roidb
(it is keyed by the dataset name only and goes stale with the data under it).  Selective-search / MCG proposal files are not provided."""
import os
import pickle
import uuid

import numpy as np
import scipy.sparse

from datasets import results
from datasets.coco_api import COCO
from datasets.coco_eval import COCOeval
from datasets.imdb import imdb

VIEW_MAP = {'minival2014': 'val2014',              # 5k val2014 subset
            'valminusminival2014': 'val2014',      # val2014 \ minival2014
            'test-dev2015': 'test2015'}


def ann_file(image_set, year, data_dir=None):
    """<data_dir>/coco/annotations/{instances|image_info}_<set><year>.json (coco.py:65-69)"""
    if data_dir is None:
        from model.config import cfg
        data_dir = cfg.DATA_DIR
    prefix = 'instances' if image_set.find('test') == -1 else 'image_info'
    return os.path.join(data_dir, 'coco', 'annotations', prefix + '_' + image_set + year + '.json')


class coco(imdb):
    def __init__(self, image_set, year, match=None):
        imdb.__init__(self, 'coco_' + year + '_' + image_set)
        from model.config import cfg
        self.config = {'use_salt': True, 'cleanup': True}
        self._year, self._image_set = year, image_set
        self._data_path = os.path.join(cfg.DATA_DIR, 'coco')
        self._match = match                                        # COCOeval's matcher: None = the device when there is one
        self._COCO = COCO(self._get_ann_file())
        cats = self._COCO.loadCats(self._COCO.getCatIds())
        self._classes = tuple(['__background__'] + [c['name'] for c in cats])
        self._class_to_ind = dict(zip(self.classes, range(self.num_classes)))
        self._class_to_coco_cat_id = dict(zip([c['name'] for c in cats], self._COCO.getCatIds()))
        self._coco_cat_id_to_class_ind = dict((self._class_to_coco_cat_id[cls], self._class_to_ind[cls]) for cls in self._classes[1:])
        self._image_index = self._COCO.getImgIds()
        self.set_proposal_method('gt')
        self.competition_mode(False)
        coco_name = image_set + year                               # e.g. "val2014"; some sets are views (subsets) into others
        self._view_map = dict(VIEW_MAP)
        self._data_name = self._view_map.get(coco_name, coco_name)
        self._gt_splits = ('train', 'val', 'minival')              # (test splits carry no annotations)

    def _get_ann_file(self):
        return ann_file(self._image_set, self._year, os.path.dirname(self._data_path))

    def image_path_at(self, i):
        return self.image_path_from_index(self._image_index[i])

    def image_path_from_index(self, index):
        # images/train2014/COCO_train2014_000000119993.jpg
        file_name = 'COCO_' + self._data_name + '_' + str(index).zfill(12) + '.jpg'
        image_path = os.path.join(self._data_path, 'images', self._data_name, file_name)
        assert os.path.exists(image_path), 'Path does not exist: {}'.format(image_path)
        return image_path

    def gt_roidb(self):
        """coco.py:103-121 without the pickle cache (see the module docstring): one entry per image of the set."""
        return [self._load_coco_annotation(index) for index in self._image_index]

    def _load_coco_annotation(self, index):
        """coco.py:123-179: boxes uint16 [n,4], gt_classes int32 [n], gt_overlaps csr float32 [n,classes] (crowd rows -1 everywhere, so
        they are excluded from training), seg_areas float32 [n], width, height.  Annotations without area or with an empty clipped box
        are dropped."""
        info = self._COCO.loadImgs(index)[0]
        width, height = info['width'], info['height']
        rows = []                                                  # (box, class index, area, is a crowd) of every annotation that is kept
        for ann in self._COCO.loadAnns(self._COCO.getAnnIds(imgIds=index, iscrowd=None)):
            # xywh -> inclusive corners: the origin clamped into the image, the far corner w-1 / h-1 beyond it, clamped to the last pixel
            x, y, w, h = ann['bbox']
            left, top = max(0, x), max(0, y)
            right = min(width - 1, left + max(0, w - 1))
            bottom = min(height - 1, top + max(0, h - 1))
            if ann['area'] > 0 and right >= left and bottom >= top:
                rows.append(([left, top, right, bottom], self._coco_cat_id_to_class_ind[ann['category_id']], ann['area'], bool(ann['iscrowd'])))
        n = len(rows)
        boxes = np.array([r[0] for r in rows], dtype=np.float64).reshape(n, 4).astype(np.uint16)          # fractions truncate
        gt_classes = np.array([r[1] for r in rows], dtype=np.int32).reshape(n)
        seg_areas = np.array([r[2] for r in rows], dtype=np.float32).reshape(n)
        overlaps = np.zeros((n, self.num_classes), dtype=np.float32)
        for k, (_, cls, _, crowd) in enumerate(rows):
            if crowd:
                overlaps[k, :] = -1.0                              # no class may take a crowd region as foreground or background
            else:
                overlaps[k, cls] = 1.0
        assert (boxes[:, 2] >= boxes[:, 0]).all() and (boxes[:, 3] >= boxes[:, 1]).all() and (boxes[:, 2] < width).all() and (boxes[:, 3] < height).all()
        return {'width': width, 'height': height, 'boxes': boxes, 'gt_classes': gt_classes,
                'gt_overlaps': scipy.sparse.csr_matrix(overlaps), 'flipped': False, 'seg_areas': seg_areas}

    def _get_widths(self):
        return [r['width'] for r in self.roidb]

    def append_flipped_images(self):
        """coco.py:184-203: unlike the base class the twins keep width / height / seg_areas."""
        num_images = self.num_images
        widths = self._get_widths()
        for i in range(num_images):
            src = self.roidb[i]
            boxes = src['boxes'].copy()
            oldx1, oldx2 = boxes[:, 0].copy(), boxes[:, 2].copy()
            boxes[:, 0] = widths[i] - oldx2 - 1
            boxes[:, 2] = widths[i] - oldx1 - 1
            assert (boxes[:, 2] >= boxes[:, 0]).all()
            self.roidb.append({'width': widths[i], 'height': src['height'], 'boxes': boxes, 'gt_classes': src['gt_classes'],
                               'gt_overlaps': src['gt_overlaps'], 'flipped': True, 'seg_areas': src['seg_areas']})
        self._image_index = self._image_index * 2

    def _print_detection_eval_metrics(self, coco_eval):
        """What coco.py:212-242 prints: the header, then the mean AP over IoU .50:.95 (area = all, 100 detections) of all categories and of
        each category in class order, in percent with one decimal (`nan` for a category without countable ground truth), then the 12
        summary lines."""
        thrs = coco_eval.params.iouThrs
        t_lo, t_hi = (int(np.argmin(np.abs(thrs - v))) for v in (0.5, 0.95))
        assert np.isclose(thrs[t_lo], 0.5) and np.isclose(thrs[t_hi], 0.95)
        cells = coco_eval.eval['precision'][t_lo:t_hi + 1, :, :, 0, 2]       # [T, R, K] at area = all, maxDets = 100

        def percent(p):
            return '{:.1f}'.format(100 * np.mean(p[p > -1]))
        print('~~~~ Mean and per-category AP @ IoU=[{:.2f},{:.2f}] ~~~~'.format(0.5, 0.95))
        print(percent(cells))
        for k in range(self.num_classes - 1):                      # category k is class k + 1
            print(percent(cells[:, :, k]))
        print('~~~~ Summary metrics ~~~~')
        coco_eval.summarize()

    def _do_detection_eval(self, res_file, output_dir):
        coco_dt = self._COCO.loadRes(res_file)
        coco_eval = COCOeval(self._COCO, coco_dt, match=self._match)
        coco_eval.evaluate()
        coco_eval.accumulate()
        with np.errstate(invalid='ignore'), _quiet_empty_mean():
            self._print_detection_eval_metrics(coco_eval)
        eval_file = os.path.join(output_dir, 'detection_results.pkl')
        p = coco_eval.params
        with open(eval_file, 'wb') as fid:                         # a plain dict (the reference pickles the evaluator object itself)
            pickle.dump({'params': {'iouThrs': p.iouThrs, 'recThrs': p.recThrs, 'maxDets': list(p.maxDets), 'areaRng': p.areaRng,
                                    'areaRngLbl': p.areaRngLbl, 'imgIds': [int(i) for i in p.imgIds], 'catIds': [int(c) for c in p.catIds]},
                         'precision': coco_eval.eval['precision'], 'recall': coco_eval.eval['recall'], 'stats': coco_eval.stats,
                         'match': coco_eval.match}, fid, pickle.HIGHEST_PROTOCOL)
        print('Wrote COCO eval results to: {}'.format(eval_file))
        return coco_eval

    def _coco_results_one_category(self, boxes, cat_id):
        return results.coco_results_one_category(boxes, self.image_index, cat_id)

    def evaluate_detections(self, all_boxes, output_dir):
        os.makedirs(output_dir, exist_ok=True)
        res_file = os.path.join(output_dir, 'detections_' + self._image_set + self._year + '_results')
        if self.config['use_salt']:
            res_file += '_{}'.format(str(uuid.uuid4()))
        res_file += '.json'
        print('Writing results json to {}'.format(res_file))
        results.write_coco_results_file(all_boxes, self._classes, self._image_index, self._class_to_coco_cat_id, res_file)
        coco_eval = None
        if self._image_set.find('test') == -1:                     # only sets with annotations are evaluated
            coco_eval = self._do_detection_eval(res_file, output_dir)
        if self.config['cleanup']:
            os.remove(res_file)
        return coco_eval

    def competition_mode(self, on):
        self.config['use_salt'] = not on
        self.config['cleanup'] = not on


class _quiet_empty_mean(object):
    """np.mean of an empty selection (a category without ground truth prints `nan`, as in the reference) warns; keep the output to the
    reference's lines."""

    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter('ignore', RuntimeWarning)

    def __exit__(self, *exc):
        return self._w.__exit__(*exc)
