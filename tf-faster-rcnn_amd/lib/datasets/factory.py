"""datasets.factory -- imdbs by name (lib/datasets/factory.py:18-52): `voc_<year>_<split>` and `voc_<year>_<split>_diff` for the years and
splits the reference registers, `coco_2014_{train,val,minival,valminusminival,trainval}` and `coco_2015_{test,test-dev}`.  A COCO set
whose annotation file is absent under cfg.DATA_DIR is an unknown dataset: get_imdb raises KeyError naming the file it looked for."""
import os

from datasets.coco import ann_file, coco
from datasets.pascal_voc import pascal_voc

__sets = {}
for year in ['2007', '2012']:
    for split in ['train', 'val', 'trainval', 'test']:
        __sets['voc_{}_{}'.format(year, split)] = (lambda split=split, year=year: pascal_voc(split, year))
        __sets['voc_{}_{}_diff'.format(year, split)] = (lambda split=split, year=year: pascal_voc(split, year, use_diff=True))


def _coco(split, year):
    path = ann_file(split, year)
    if not os.path.isfile(path):
        raise KeyError('Unknown dataset: coco_{}_{} (no annotation file {})'.format(year, split, path))
    return coco(split, year)


for year, splits in (('2014', ['train', 'val', 'minival', 'valminusminival', 'trainval']), ('2015', ['test', 'test-dev'])):
    for split in splits:
        __sets['coco_{}_{}'.format(year, split)] = (lambda split=split, year=year: _coco(split, year))


def get_imdb(name):
    """Get an imdb (image database) by name."""
    if name not in __sets:
        raise KeyError('Unknown dataset: {}'.format(name))
    return __sets[name]()


def list_imdbs():
    return list(__sets.keys())
