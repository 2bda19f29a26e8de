"""roi_data_layer.roidb -- prepare_roidb of the reference (lib/roi_data_layer/roidb.py:19-49): image path, size, and the per-box maximum
overlap / class derived from gt_overlaps, added to every roidb entry in place.  The size comes from PIL, except for an imdb whose name
starts with `coco` (roidb.py:27-34): its entries already carry width / height from the annotation file, and opening 80 000 images
to read two numbers is not free."""
import numpy as np
import PIL.Image


def prepare_roidb(imdb):
    roidb = imdb.roidb
    from_entries = imdb.name.startswith('coco')
    if not from_entries:
        sizes = [PIL.Image.open(imdb.image_path_at(i)).size for i in range(imdb.num_images)]
    for i in range(len(imdb.image_index)):
        roidb[i]['image'] = imdb.image_path_at(i)
        if not from_entries:
            roidb[i]['width'] = sizes[i][0]
            roidb[i]['height'] = sizes[i][1]
        gt_overlaps = roidb[i]['gt_overlaps'].toarray()            # dense for argmax
        max_overlaps = gt_overlaps.max(axis=1)
        max_classes = gt_overlaps.argmax(axis=1)
        roidb[i]['max_classes'] = max_classes
        roidb[i]['max_overlaps'] = max_overlaps
        assert all(max_classes[np.where(max_overlaps == 0)[0]] == 0)          # no overlap <=> background
        assert all(max_classes[np.where(max_overlaps > 0)[0]] != 0)
