#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for the training roidb / data layer (datasets.pascal_voc.gt_roidb, flipping,
roi_data_layer), produced by running the REFERENCE's own lib/datasets/pascal_voc.py, lib/roi_data_layer/{roidb,layer,minibatch}.py and
lib/model/train_val.py (get_training_roidb, filter_roidb) on a small synthetic devkit; writes tests/golden/roidb.npz.  Generation
needs the reference tree; build_devkit() and the fixture layout are also used by tests/test_roidb_*.py, which need neither.

    python fixtures/gen_golden_roidb.py            # regenerate the fixture
    python fixtures/gen_golden_roidb.py --check    # compare the live reference with the stored fixture, exit 1 on mismatch

The devkit is rebuilt from a seed wherever it is needed: the images are written LOSSLESSLY (PNG bytes under the .jpg name; PIL opens by
content), so the decoded pixels are the same on every machine.  The reference runs with a stub `cv2`: imread = PIL decode -> BGR,
resize = frcnn_oracle.cv2_resize_linear.  The recorded `data` blobs therefore pin BGR order, mirror-before-mean-before-resize and the
padding-free single-image blob -- not OpenCV itself (parity unpinned).

Cases: cfg.TRAIN.USE_FLIPPED on / off  x  cfg.TRAIN.ASPECT_GROUPING off / on, cfg.TRAIN.SCALES = SCALES (two entries, so the per-
minibatch randint matters), np.random.seed(SEED) before the data layer is built.  ASPECT_GROUPING reshapes the index list to (-1, 2):
the FILTERED roidb length must be even.  With USE_FLIPPED it always is (entries come in pairs); without, the devkit is built so that it
is (7 images, one of them dropped by the filter).
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "roidb.npz")
YEAR, SPLIT = "2007", "trainval"
SEED = 3                        # cfg.RNG_SEED of the reference
SCALES, MAX_SIZE = (64, 80), 110
DRAWS_PER_LEN = 2.5             # minibatches recorded per case, in units of the filtered roidb length ("epochs"), rounded up
BLOB_DRAWS = 2                  # USE_FLIPPED on, ASPECT_GROUPING off: the first BLOB_DRAWS unflipped and the first BLOB_DRAWS flipped draws keep their `data` blob
CLASSES = ('__background__', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
           'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')
# (h, w): landscape and portrait, two images sharing a size, one odd width
SIZES = ((60, 90), (60, 90), (90, 60), (64, 88), (75, 51), (56, 84), (80, 64))
ALL_DIFFICULT = 3               # every object of this image is `difficult`: without use_diff it has no box and the filter drops it (and its twin)


def synth_devkit_arrays(seed=11):
    """images: list of uint8 RGB [h,w,3]; objects: list per image of (class name, xmin, ymin, xmax, ymax (1-based), difficult)."""
    rng = np.random.RandomState(seed)
    images, objects = [], []
    for i, (h, w) in enumerate(SIZES):
        images.append(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        objs = []
        for k in range(rng.randint(1, 5)):
            x1, y1 = rng.randint(1, w - 12), rng.randint(1, h - 12)
            x2, y2 = rng.randint(x1 + 4, w + 1), rng.randint(y1 + 4, h + 1)
            difficult = 1 if i == ALL_DIFFICULT else int(k > 0 and rng.rand() < 0.3)
            objs.append((CLASSES[rng.randint(1, len(CLASSES))], x1, y1, x2, y2, difficult))
        objects.append(objs)
    return images, objects


def build_devkit(data_dir, seed=11):
    """Writes <data_dir>/VOCdevkit2007/VOC2007/{JPEGImages,Annotations,ImageSets/Main/trainval.txt}; returns the image index."""
    from PIL import Image
    images, objects = synth_devkit_arrays(seed)
    base = os.path.join(data_dir, "VOCdevkit" + YEAR, "VOC" + YEAR)
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    index = ["%06d" % (i + 1) for i in range(len(images))]
    for name, im, objs in zip(index, images, objects):
        with open(os.path.join(base, "JPEGImages", name + ".jpg"), "wb") as f:
            Image.fromarray(im, "RGB").save(f, format="PNG")
        body = "".join("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
                       "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>" % (o[0], o[5], o[1], o[2], o[3], o[4])
                       for o in objs)
        with open(os.path.join(base, "Annotations", name + ".xml"), "w") as f:
            f.write("<annotation><filename>%s.jpg</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>"
                    % (name, im.shape[1], im.shape[0], body))
    with open(os.path.join(base, "ImageSets", "Main", SPLIT + ".txt"), "w") as f:
        f.write("\n".join(index) + "\n")
    return index


def n_draws(filtered_len):
    return int(np.ceil(DRAWS_PER_LEN * filtered_len))


def case_prefix(flipped, grouping=None):
    return "flip%d_" % int(flipped) + ("" if grouping is None else "group%d_" % int(grouping))


def roidb_arrays(prefix, roidb, out):
    """The per-entry arrays of a prepared roidb under `<prefix>e<i>_<field>` (+ `<prefix>n`)."""
    out[prefix + "n"] = np.int64(len(roidb))
    for i, e in enumerate(roidb):
        p = "%se%d_" % (prefix, i)
        out[p + "boxes"], out[p + "gt_classes"] = np.array(e["boxes"]), np.array(e["gt_classes"])
        out[p + "gt_overlaps"] = np.asarray(e["gt_overlaps"].toarray())
        out[p + "flipped"] = np.bool_(e["flipped"])
        out[p + "has_seg_areas"] = np.bool_("seg_areas" in e)
        if "seg_areas" in e:
            out[p + "seg_areas"] = np.array(e["seg_areas"])
        out[p + "size"] = np.array([e["width"], e["height"]], dtype=np.int64)
        out[p + "image"] = np.array(os.path.basename(e["image"]))
        out[p + "max_classes"], out[p + "max_overlaps"] = np.array(e["max_classes"]), np.array(e["max_overlaps"])


class repo_cfg(object):
    """`with repo_cfg(data_dir, flipped, grouping, scales, max_size):` -- the fixture's settings on the REPO's cfg, restored on exit."""

    def __init__(self, data_dir, flipped=True, grouping=False, scales=SCALES, max_size=MAX_SIZE):
        self.data_dir, self.train = data_dir, dict(USE_FLIPPED=flipped, ASPECT_GROUPING=grouping, SCALES=tuple(scales), MAX_SIZE=max_size)

    def __enter__(self):
        from model.config import cfg
        self.old = (cfg.DATA_DIR, {k: cfg.TRAIN[k] for k in self.train})
        cfg.DATA_DIR = self.data_dir
        for k, v in self.train.items():
            cfg.TRAIN[k] = v
        return cfg

    def __exit__(self, *exc):
        from model.config import cfg
        cfg.DATA_DIR = self.old[0]
        for k, v in self.old[1].items():
            cfg.TRAIN[k] = v
        return False


def repo_roidb(quiet=True):
    """The repo's own path to a training roidb under the current cfg: (imdb, prepared roidb, filtered roidb)."""
    import contextlib
    import io
    from datasets.factory import get_imdb
    from model.train_val import filter_roidb, get_training_roidb
    with contextlib.redirect_stdout(io.StringIO() if quiet else sys.stdout):
        imdb = get_imdb("voc_%s_%s" % (YEAR, SPLIT))
        imdb.set_proposal_method("gt")
        roidb = get_training_roidb(imdb)
        filtered = filter_roidb(roidb)
    return imdb, roidb, filtered


def reference_results():
    """Runs the reference on a fresh devkit; returns the fixture dict."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import frcnn_oracle as ora
    import ref_shim
    ref_shim.load_reference()
    if not hasattr(np, "bool"):
        np.bool = bool
    from PIL import Image
    cv2 = types.ModuleType("cv2")                                  # the two calls the reference's minibatch / blob code makes
    cv2.INTER_LINEAR = 1
    cv2.imread = lambda path: np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])
    cv2.resize = lambda im, dsize, dst, fx, fy, interpolation: ora.cv2_resize_linear(im, fx, fy)
    sys.modules["cv2"] = cv2
    tfp = types.ModuleType("tensorflow.python")                    # model/train_val.py imports it, the two functions used here never call it
    tfp.pywrap_tensorflow = None
    sys.modules["tensorflow.python"] = tfp
    from model.config import cfg
    from datasets.pascal_voc import pascal_voc
    from model.train_val import filter_roidb, get_training_roidb
    from roi_data_layer.layer import RoIDataLayer
    import roi_data_layer.minibatch as ref_minibatch

    class RandintSpy(object):
        """Stands where the reference's minibatch module keeps `numpy.random`: passes every call on, remembers the last randint result."""
        def __getattr__(self, name):
            return getattr(np.random, name)

        def randint(self, *a, **kw):
            self.last = np.random.randint(*a, **kw)
            return self.last
    spy = ref_minibatch.npr = RandintSpy()
    out = {}
    with tempfile.TemporaryDirectory() as data_dir:
        cfg.DATA_DIR = data_dir                                    # devkit and the reference's cache pickle both live (and die) here
        build_devkit(data_dir)
        cfg.TRAIN.SCALES, cfg.TRAIN.MAX_SIZE = SCALES, MAX_SIZE
        for flipped in (True, False):
            cfg.TRAIN.USE_FLIPPED = flipped
            imdb = pascal_voc(SPLIT, YEAR)
            imdb.set_proposal_method("gt")
            roidb = get_training_roidb(imdb)
            fp = case_prefix(flipped)
            roidb_arrays(fp, roidb, out)
            filtered = filter_roidb(roidb)
            out[fp + "filtered"] = np.array([k for k, e in enumerate(roidb) if any(e is f for f in filtered)], dtype=np.int64)
            assert len(filtered) % 2 == 0, "ASPECT_GROUPING needs an even filtered roidb length"
            for grouping in (False, True):
                cfg.TRAIN.ASPECT_GROUPING = grouping
                np.random.seed(SEED)
                layer = RoIDataLayer(filtered, imdb.num_classes)
                gp = case_prefix(flipped, grouping)
                n = n_draws(len(filtered))
                db, sc, info, kept = [], [], [], {False: 0, True: 0}
                for k in range(n):
                    blobs = layer.forward()
                    db.append(int(layer._perm[layer._cur - 1]))
                    sc.append(int(spy.last[0]))
                    info.append(blobs["im_info"])
                    out["%sgt%d" % (gp, k)] = blobs["gt_boxes"]
                    is_flipped = bool(filtered[db[-1]]["flipped"])
                    if flipped and not grouping and kept[is_flipped] < BLOB_DRAWS:
                        kept[is_flipped] += 1
                        out["%sdata%d" % (gp, k)] = blobs["data"]
                out[gp + "db_inds"], out[gp + "scale_inds"] = np.array(db, dtype=np.int64), np.array(sc, dtype=np.int64)
                out[gp + "im_info"] = np.stack(info).astype(np.float32)
                out[gp + "rand_after"] = np.float64(np.random.rand())          # pins how much of the stream was consumed
    return out


def compare(a, b):
    return [k for k in sorted(set(a) | set(b))
            if not (k in a and k in b and np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype
                    and np.array_equal(a[k], b[k]))]


def main():
    ref = reference_results()
    if "--check" in sys.argv:
        bad = compare(ref, dict(np.load(GOLD)))
        print("live reference vs fixture:", "bit-exact" if not bad else "MISMATCH %s" % bad[:8])
        return 1 if bad else 0
    np.savez_compressed(GOLD, **ref)
    print("wrote %s (%.1f KB): %s" % (GOLD, os.path.getsize(GOLD) / 1024,
                                      {k: ref[k].tolist() for k in ref if k.endswith("filtered") or k.endswith("db_inds")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
