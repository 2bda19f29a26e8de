#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for the COCO imdb (datasets.coco gt_roidb, its own append_flipped_images,
roi_data_layer.roidb's coco branch, filter_roidb, the minibatch gt rows, _coco_results_one_category), produced by running the
REFERENCE's own lib/datasets/coco.py, lib/roi_data_layer/* and lib/model/train_val.py (get_training_roidb, filter_roidb) unmodified on a
small synthetic COCO tree; writes tests/golden/coco_roidb.npz.  Generation needs the reference tree; build_coco() and the fixture
layout are also used by tests/test_coco_*.py, which need neither.

    python fixtures/gen_golden_coco.py            # regenerate the fixture
    python fixtures/gen_golden_coco.py --check    # compare the live reference with the stored fixture, exit 1 on mismatch

The reference imports `pycocotools`, which is neither installed nor part of its tree: the stub module installed here is built on the
project's own datasets.coco_api (a plain json index), in the spirit of oracle/ref_shim.py.  What the fixture pins is therefore the
reference's coco.py / roidb.py / minibatch.py logic on that index -- category-id maps over gapped ids, the box sanitising, crowd rows
at -1, uint16 flipping, width / height from the entries, the `!= 0 & ...` precedence that keeps crowd boxes among the gt rows -- not
pycocotools itself.  Images are PNG bytes under the .jpg names (PIL opens by content); cv2 is the stub of gen_golden_roidb.py.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gen_golden_roidb as ggr  # noqa: E402  (repo_cfg, roidb_arrays, compare, n_draws, SCALES / MAX_SIZE / SEED)

GOLD = os.path.join(ROOT, "tests", "golden", "coco_roidb.npz")
YEAR = "2014"
# the 80 category ids of COCO: 1..90 with ten gaps
CAT_IDS = [i for i in range(1, 91) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]
# (image id, h, w); ids are not contiguous and not in file order
TRAIN_IMAGES = ((139, 60, 90), (25, 60, 90), (9, 90, 60), (1000, 64, 88), (285, 75, 51), (632, 56, 84), (724, 80, 64), (776, 72, 72),
                (42, 66, 98), (1296, 58, 70))
MINIVAL_IMAGES = ((397133, 60, 90), (37777, 90, 60), (252219, 64, 88), (87038, 75, 51))
ONLY_CROWD = 285                # its single annotation is a crowd: max_overlaps = -1, the filter drops it (and its twin)
ZERO_AREA = 632                 # carries an annotation with area 0 (dropped) beside a normal one
CLIPPED = 724                   # carries a box reaching past the right and bottom border


def synth_set(images, seed):
    """-> (pixel arrays, the dataset dict of an instances file)"""
    rng = np.random.RandomState(seed)
    pix, anns = [], []
    for img_id, h, w in images:
        pix.append(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        for k in range(rng.randint(1, 6)):
            x, y = round(rng.uniform(0, w - 14), 2), round(rng.uniform(0, h - 14), 2)
            bw, bh = round(rng.uniform(4, w - x), 2), round(rng.uniform(4, h - y), 2)
            crowd = int(k > 0 and rng.rand() < 0.25)
            anns.append(dict(image_id=img_id, category_id=CAT_IDS[rng.randint(0, len(CAT_IDS))], bbox=[x, y, bw, bh],
                             area=round(bw * bh * rng.uniform(0.4, 0.9), 4), iscrowd=crowd))
    for a in [a for a in anns if a["image_id"] == ONLY_CROWD][1:]:
        anns.remove(a)
    for a in anns:
        if a["image_id"] == ONLY_CROWD:
            a["iscrowd"] = 1
    if any(i[0] == ZERO_AREA for i in images):
        anns.append(dict(image_id=ZERO_AREA, category_id=CAT_IDS[17], bbox=[5.0, 6.0, 20.0, 0.0], area=0.0, iscrowd=0))
        anns.append(dict(image_id=ZERO_AREA, category_id=CAT_IDS[79], bbox=[10.5, 8.25, 30.0, 21.5], area=401.5, iscrowd=0))
    if any(i[0] == CLIPPED for i in images):
        anns.append(dict(image_id=CLIPPED, category_id=CAT_IDS[0], bbox=[40.2, 51.7, 60.0, 70.0], area=512.0, iscrowd=0))
    order = rng.permutation(len(anns))                             # annotations of one image are not contiguous in the file
    anns = [dict(anns[i], id=1000 + 7 * n) for n, i in enumerate(order)]
    cats = [dict(id=c, name="class_%02d" % c, supercategory="synthetic") for c in CAT_IDS]
    return pix, dict(images=[dict(id=i, height=h, width=w, file_name="") for i, h, w in images], annotations=anns, categories=cats[::-1])


def build_coco(data_dir, seed=21):
    """Writes <data_dir>/coco/{annotations/instances_{train,minival}2014.json, images/{train2014,val2014}/COCO_*.jpg}; returns the two
    dataset dicts."""
    from PIL import Image
    out = {}
    for k, (split, data_name, images) in enumerate((("train", "train2014", TRAIN_IMAGES), ("minival", "val2014", MINIVAL_IMAGES))):
        pix, ds = synth_set(images, seed + k)
        os.makedirs(os.path.join(data_dir, "coco", "annotations"), exist_ok=True)
        os.makedirs(os.path.join(data_dir, "coco", "images", data_name), exist_ok=True)
        for (img_id, _, _), im, rec in zip(images, pix, ds["images"]):
            rec["file_name"] = "COCO_%s_%012d.jpg" % (data_name, img_id)
            with open(os.path.join(data_dir, "coco", "images", data_name, rec["file_name"]), "wb") as f:
                Image.fromarray(im, "RGB").save(f, format="PNG")
        with open(os.path.join(data_dir, "coco", "annotations", "instances_%s%s.json" % (split, YEAR)), "w") as f:
            json.dump(ds, f)
        out[split] = ds
    return out


def synth_dets(num_classes, num_images, seed=5):
    """all_boxes[cls][image] = float32 [n,5] (n may be 0) for _coco_results_one_category"""
    rng = np.random.RandomState(seed)
    return [[(rng.rand(rng.randint(0, 4), 5) * [50, 40, 30, 20, 1] + [0, 0, 50, 40, 0]).astype(np.float32) for _ in range(num_images)]
            for _ in range(num_classes)]


def results_arrays(res):
    """[{image_id, category_id, bbox, score}] -> float64 [n,7]"""
    return np.array([[r["image_id"], r["category_id"]] + list(r["bbox"]) + [r["score"]] for r in res], dtype=np.float64).reshape(-1, 7)


def repo_roidb(quiet=True):
    """The repo's own path to the COCO training roidb under the current cfg: (imdb, prepared roidb, filtered roidb)."""
    import contextlib
    import io
    from datasets.factory import get_imdb
    from model.train_val import filter_roidb, get_training_roidb
    with contextlib.redirect_stdout(io.StringIO() if quiet else sys.stdout):
        imdb = get_imdb("coco_%s_train" % YEAR)
        imdb.set_proposal_method("gt")
        roidb = get_training_roidb(imdb)
        filtered = filter_roidb(roidb)
    return imdb, roidb, filtered


def reference_results():
    """Runs the reference on a fresh tree; returns the fixture dict."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tf-faster-rcnn_amd", "lib", "datasets"))
    import coco_api                                                # the project's json index, loaded as a top-level module: the
    sys.path.pop(0)                                                # reference's own `datasets` package must stay the only one
    import frcnn_oracle as ora
    import ref_shim
    ref_shim.load_reference()
    if not hasattr(np, "bool"):
        np.bool = bool
    for name in ("pycocotools", "pycocotools.coco", "pycocotools.cocoeval", "pycocotools.mask"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pycocotools.coco"].COCO = coco_api.COCO
    sys.modules["pycocotools.cocoeval"].COCOeval = object         # imported, never called here
    sys.modules["pycocotools"].mask = sys.modules["pycocotools.mask"]
    from PIL import Image
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1
    cv2.imread = lambda path: np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])
    cv2.resize = lambda im, dsize, dst, fx, fy, interpolation: ora.cv2_resize_linear(im, fx, fy)
    sys.modules["cv2"] = cv2
    tfp = types.ModuleType("tensorflow.python")
    tfp.pywrap_tensorflow = None
    sys.modules["tensorflow.python"] = tfp
    from model.config import cfg
    from datasets.coco import coco
    from model.train_val import filter_roidb, get_training_roidb
    from roi_data_layer.layer import RoIDataLayer

    class Dets(np.ndarray):
        """`dets == []` (coco.py:262) was False for a non-empty array under the numpy the reference was written for; numpy 2 raises on
        the broadcast.  Restore the old answer for that one comparison (as oracle/gen_golden_eval.py does)."""
        def __eq__(self, other):
            if isinstance(other, list) and len(other) == 0:
                return False
            return np.ndarray.__eq__(self, other)
        __hash__ = None

    out = {}
    with tempfile.TemporaryDirectory() as data_dir:
        cfg.DATA_DIR = data_dir                                    # tree and the reference's cache pickles both live (and die) here
        build_coco(data_dir)
        cfg.TRAIN.SCALES, cfg.TRAIN.MAX_SIZE, cfg.TRAIN.ASPECT_GROUPING = ggr.SCALES, ggr.MAX_SIZE, False
        for flipped in (True, False):
            cfg.TRAIN.USE_FLIPPED = flipped
            cache = os.path.join(data_dir, "cache", "coco_%s_train_gt_roidb.pkl" % YEAR)
            if os.path.exists(cache):
                os.remove(cache)
            imdb = coco("train", YEAR)
            imdb.set_proposal_method("gt")
            roidb = get_training_roidb(imdb)
            fp = ggr.case_prefix(flipped)
            ggr.roidb_arrays(fp, roidb, out)
            filtered = filter_roidb(roidb)
            out[fp + "filtered"] = np.array([k for k, e in enumerate(roidb) if any(e is f for f in filtered)], dtype=np.int64)
            np.random.seed(ggr.SEED)
            layer = RoIDataLayer(filtered, imdb.num_classes)
            db, info = [], []
            for k in range(ggr.n_draws(len(filtered))):
                blobs = layer.forward()
                db.append(int(layer._perm[layer._cur - 1]))
                info.append(blobs["im_info"])
                out["%sgt%d" % (fp, k)] = blobs["gt_boxes"]
            out[fp + "db_inds"], out[fp + "im_info"] = np.array(db, dtype=np.int64), np.stack(info).astype(np.float32)
        out["classes"] = np.array(imdb.classes)
        out["class_cat_ids"] = np.array([imdb._class_to_coco_cat_id[c] for c in imdb.classes[1:]], dtype=np.int64)
        out["image_index"] = np.array(imdb.image_index[:len(TRAIN_IMAGES)], dtype=np.int64)
        mini = coco("minival", YEAR)
        out["minival_image_index"] = np.array(mini.image_index, dtype=np.int64)
        out["minival_image0"] = np.array(os.path.relpath(mini.image_path_at(0), data_dir))
        dets = synth_dets(3, len(mini.image_index))
        out["results_one_category"] = results_arrays(mini._coco_results_one_category([d.view(Dets) for d in dets[1]], 18))
    return out


def main():
    ref = reference_results()
    if "--check" in sys.argv:
        bad = ggr.compare(ref, dict(np.load(GOLD)))
        print("live reference vs fixture:", "bit-exact" if not bad else "MISMATCH %s" % bad[:8])
        return 1 if bad else 0
    np.savez_compressed(GOLD, **ref)
    print("wrote %s (%.1f KB): %s" % (GOLD, os.path.getsize(GOLD) / 1024,
                                      {k: ref[k].tolist() for k in ref if k.endswith("filtered") or k.endswith("db_inds")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
