"""datasets.factory -- imdbs by name (lib/datasets/factory.py:18-52): `voc_<year>_<split>` and `voc_<year>_<split>_diff` for the years and
splits the reference registers.  COCO is not provided."""
from datasets.pascal_voc import pascal_voc

__sets = {}
for year in ['2007', '2012']:
    for split in ['train', 'val', 'trainval', 'test']:
        __sets['voc_{}_{}'.format(year, split)] = (lambda split=split, year=year: pascal_voc(split, year))
        __sets['voc_{}_{}_diff'.format(year, split)] = (lambda split=split, year=year: pascal_voc(split, year, use_diff=True))


def get_imdb(name):
    """Get an imdb (image database) by name."""
    if name not in __sets:
        raise KeyError('Unknown dataset: {}'.format(name))
    return __sets[name]()


def list_imdbs():
    return list(__sets.keys())
