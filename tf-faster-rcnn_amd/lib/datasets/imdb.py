"""datasets.imdb -- the image-database base class of the reference (lib/datasets/imdb.py:20-214, 258-260): name, classes, image index,
the lazily built roidb behind a proposal method, append_flipped_images and evaluate_recall (proposal recall; the matching is
datasets.recall's, on the device or in its C host statement).  Roidbs built from external box lists (create_roidb_from_box_list,
merge_roidbs: selective search, RPN files) are not provided, because the network here has no Fast R-CNN mode that would consume such a
roidb: 'gt' is the only proposal method."""
import os

import numpy as np
import PIL.Image


class imdb(object):
    def __init__(self, name, classes=None):
        self._name = name
        self._classes = classes if classes else []
        self._image_index = []
        self._obj_proposer = 'gt'
        self._roidb = None
        self._roidb_handler = self.default_roidb
        self.config = {}

    name = property(lambda self: self._name)
    classes = property(lambda self: self._classes)
    num_classes = property(lambda self: len(self._classes))
    image_index = property(lambda self: self._image_index)
    num_images = property(lambda self: len(self.image_index))

    @property
    def roidb_handler(self):
        return self._roidb_handler

    @roidb_handler.setter
    def roidb_handler(self, val):
        self._roidb_handler = val

    def set_proposal_method(self, method):
        handler = getattr(self, method + '_roidb', None)
        if handler is None:
            raise NotImplementedError("proposal method '%s': only 'gt' roidbs are provided" % method)
        self.roidb_handler = handler

    @property
    def roidb(self):
        """A list of dicts with the keys boxes, gt_overlaps, gt_classes, flipped (, seg_areas); built on first use."""
        if self._roidb is None:
            self._roidb = self.roidb_handler()
        return self._roidb

    def image_path_at(self, i):
        raise NotImplementedError

    def default_roidb(self):
        raise NotImplementedError

    def evaluate_detections(self, all_boxes, output_dir=None):
        raise NotImplementedError

    def _get_widths(self):
        return [PIL.Image.open(self.image_path_at(i)).size[0] for i in range(self.num_images)]

    def append_flipped_images(self):
        """imdb.py:109-124: one mirrored twin per image, appended in order; the twins share gt_overlaps / gt_classes with their
        originals and carry no seg_areas.  The uint16 arithmetic `width - x - 1` is the reference's."""
        widths = self._get_widths()
        for i in range(len(widths)):
            src = self.roidb[i]
            boxes = src['boxes'].copy()
            boxes[:, 0] = widths[i] - src['boxes'][:, 2] - 1
            boxes[:, 2] = widths[i] - src['boxes'][:, 0] - 1
            assert (boxes[:, 2] >= boxes[:, 0]).all()
            self.roidb.append(dict(boxes=boxes, gt_overlaps=src['gt_overlaps'], gt_classes=src['gt_classes'], flipped=True))
        self._image_index = self._image_index * 2

    def evaluate_recall(self, candidate_boxes=None, thresholds=None, area='all', limit=None):
        """imdb.py:126-214, the reference's signature and result: {'ar', 'recalls', 'thresholds', 'gt_overlaps'}.  candidate_boxes: a list
        over images of float32 [n,4] (None: the roidb's non-gt rows).  The matching runs on the device when CUDA is available, else in
        the C host statement (datasets.recall); too few candidates for an image's ground truth raise AssertionError as the reference does."""
        from datasets import recall
        return recall.evaluate([self.roidb[i] for i in range(self.num_images)], candidate_boxes, thresholds, area, limit)

    def competition_mode(self, on):
        pass
