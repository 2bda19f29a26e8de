"""datasets.coco_api -- a dependency-free index over a COCO `instances_*.json` / `image_info_*.json` file: the handful of
`pycocotools.coco.COCO` methods the reference's lib/datasets/coco.py:23,52-57,89-93,143-148,261 calls.  pycocotools is not a
dependency of this project (and not part of the reference tree either); only boxes are handled, no masks, no keypoints."""
import json
from collections import defaultdict


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple, set)) else [x]


class COCO(object):
    def __init__(self, annotation_file=None):
        self.dataset, self.anns, self.cats, self.imgs = {}, {}, {}, {}
        self.imgToAnns = defaultdict(list)
        if annotation_file is not None:
            with open(annotation_file, 'r') as f:
                self.dataset = json.load(f)
            assert isinstance(self.dataset, dict), 'annotation file format {} not supported'.format(type(self.dataset))
            self.createIndex()

    def createIndex(self):
        self.anns, self.cats, self.imgs, self.imgToAnns = {}, {}, {}, defaultdict(list)
        for ann in self.dataset.get('annotations', []):
            self.imgToAnns[ann['image_id']].append(ann)
            self.anns[ann['id']] = ann
        for img in self.dataset.get('images', []):
            self.imgs[img['id']] = img
        for cat in self.dataset.get('categories', []):
            self.cats[cat['id']] = cat

    def getCatIds(self):
        return sorted(self.cats.keys())

    def loadCats(self, ids=()):
        return [self.cats[i] for i in _as_list(ids)]

    def getImgIds(self):
        return sorted(self.imgs.keys())

    def loadImgs(self, ids=()):
        return [self.imgs[i] for i in _as_list(ids)]

    def getAnnIds(self, imgIds=(), iscrowd=None):
        """Annotation ids of the given images (all images if none is given), in file order; iscrowd = None keeps both kinds."""
        imgIds = _as_list(imgIds)
        anns = [a for i in imgIds for a in self.imgToAnns.get(i, [])] if len(imgIds) else self.dataset.get('annotations', [])
        return [a['id'] for a in anns if iscrowd is None or a['iscrowd'] == iscrowd]

    def loadAnns(self, ids=()):
        return [self.anns[i] for i in _as_list(ids)]

    def loadRes(self, resFile):
        """A COCO object over bbox results: a json file name or the list itself, `[{"image_id", "category_id", "bbox": [x,y,w,h],
        "score"}, ...]`.  Per result: area = w*h, id = position + 1, iscrowd = 0."""
        res = COCO()
        res.dataset['images'] = [img for img in self.dataset.get('images', [])]
        if isinstance(resFile, str):
            with open(resFile) as f:
                anns = json.load(f)
        else:
            anns = resFile
        assert isinstance(anns, list), 'results in not an array of objects'
        assert set(a['image_id'] for a in anns) <= set(self.getImgIds()), 'Results do not correspond to current coco set'
        assert all('bbox' in a for a in anns), 'only bbox results are supported'
        res.dataset['categories'] = list(self.dataset.get('categories', []))
        for k, ann in enumerate(anns):
            bb = ann['bbox']
            ann['area'] = bb[2] * bb[3]
            ann['id'] = k + 1
            ann['iscrowd'] = 0
        res.dataset['annotations'] = anns
        res.createIndex()
        return res
