"""A PASCAL VOC devkit: image index, class list, ground-truth roidb, results files, AP.

Evaluation side: what `imdb.evaluate_detections(all_boxes, output_dir)` needs at the end of model.test.test_net
(reference: lib/datasets/pascal_voc.py:27-50 constructor fields, :92-103 image index, :186-201 results path,
:203-263 writer + python eval, :281-296 evaluate_detections / competition_mode).  Training side: `gt_roidb` from the
annotation XML (:98-120, :141-185), flipping and the `roidb` property through datasets.imdb.  The reference's on-disk
`cache/<name>_gt_roidb.pkl` is left out on purpose: it is keyed by the dataset name only and goes stale when the devkit
under it changes; parsing the XML again costs seconds.  Selective-search / RPN-file proposal methods are not provided.
"""
import os
import uuid
import xml.etree.ElementTree as ET

import numpy as np
import scipy.sparse

from datasets import results
from datasets.imdb import imdb

VOC_CLASSES = ('__background__', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
               'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')


class pascal_voc(imdb):
    def __init__(self, image_set, year, devkit_path=None, use_diff=False, classes=VOC_CLASSES):
        imdb.__init__(self, 'voc_' + year + '_' + image_set + ('_diff' if use_diff else ''), tuple(classes))
        if devkit_path is None:                                    # pascal_voc.py:92-96: <cfg.DATA_DIR>/VOCdevkit<year>
            from model.config import cfg
            devkit_path = os.path.join(cfg.DATA_DIR, 'VOCdevkit' + year)
        self._year, self._image_set, self._devkit_path = year, image_set, devkit_path
        self._data_path = os.path.join(devkit_path, 'VOC' + year)
        self._class_to_ind = dict(zip(self._classes, range(len(self._classes))))
        self._roidb_handler = self.gt_roidb
        self._salt = str(uuid.uuid4())
        self._comp_id = 'comp4'
        self.config = {'cleanup': True, 'use_salt': True, 'use_diff': use_diff}
        if not os.path.exists(self._data_path):
            raise IOError('Path does not exist: {}'.format(self._data_path))
        with open(self._image_set_file()) as f:
            self._image_index = [line.strip() for line in f.readlines()]

    def _image_set_file(self):
        return os.path.join(self._data_path, 'ImageSets', 'Main', self._image_set + '.txt')

    def image_path_at(self, i):
        return os.path.join(self._data_path, 'JPEGImages', self._image_index[i] + '.jpg')

    def gt_roidb(self):
        """pascal_voc.py:98-120 without the pickle cache (see the module docstring): one entry per image of the set."""
        return [self._load_pascal_annotation(index) for index in self.image_index]

    def _load_pascal_annotation(self, index):
        """pascal_voc.py:141-185: boxes uint16 [n,4] (0-based pixels), gt_classes int32 [n], gt_overlaps csr float32 [n,classes],
        seg_areas float32 [n]; objects marked difficult are dropped unless config['use_diff']."""
        objs = ET.parse(os.path.join(self._data_path, 'Annotations', index + '.xml')).findall('object')
        if not self.config['use_diff']:
            objs = [obj for obj in objs if int(obj.find('difficult').text) == 0]
        num_objs = len(objs)
        boxes = np.zeros((num_objs, 4), dtype=np.uint16)
        gt_classes = np.zeros((num_objs), dtype=np.int32)
        overlaps = np.zeros((num_objs, self.num_classes), dtype=np.float32)
        seg_areas = np.zeros((num_objs), dtype=np.float32)
        for ix, obj in enumerate(objs):
            bbox = obj.find('bndbox')
            x1, y1, x2, y2 = (float(bbox.find(k).text) - 1 for k in ('xmin', 'ymin', 'xmax', 'ymax'))
            cls = self._class_to_ind[obj.find('name').text.lower().strip()]
            boxes[ix, :] = [x1, y1, x2, y2]
            gt_classes[ix] = cls
            overlaps[ix, cls] = 1.0
            seg_areas[ix] = (x2 - x1 + 1) * (y2 - y1 + 1)
        return {'boxes': boxes, 'gt_classes': gt_classes, 'gt_overlaps': scipy.sparse.csr_matrix(overlaps), 'flipped': False,
                'seg_areas': seg_areas}

    def _get_comp_id(self):
        return self._comp_id + '_' + self._salt if self.config['use_salt'] else self._comp_id

    def _get_voc_results_file_template(self):
        # VOCdevkit/results/VOC2007/Main/<comp_id>_det_test_aeroplane.txt
        d = os.path.join(self._devkit_path, 'results', 'VOC' + self._year, 'Main')
        os.makedirs(d, exist_ok=True)
        return os.path.join(d, self._get_comp_id() + '_det_' + self._image_set + '_{:s}.txt')

    def evaluate_detections(self, all_boxes, output_dir, verbose=True):
        template = self._get_voc_results_file_template()
        files = results.write_voc_results_file(all_boxes, self._classes, self._image_index, template)
        aps = results.do_python_eval(self._classes, template, os.path.join(self._data_path, 'Annotations', '{:s}.xml'),
                                     self._image_set_file(), os.path.join(self._devkit_path, 'annotations_cache'), self._year,
                                     output_dir, self.config['use_diff'], verbose)
        if self.config['cleanup']:
            for path in files:
                os.remove(path)
        return aps

    def competition_mode(self, on):
        self.config['use_salt'] = not on
        self.config['cleanup'] = not on
