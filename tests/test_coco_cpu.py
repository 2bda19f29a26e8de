"""CPU: the COCO imdb (datasets.coco_api / datasets.coco / the factory names / roi_data_layer.roidb's coco branch) against
tests/golden/coco_roidb.npz, which fixtures/gen_golden_coco.py produced by running the REFERENCE's own coco.py / roidb.py / minibatch.py on
the same seeded tree, and the bbox evaluator (datasets.coco_eval, host matcher) against hand-derivable known answers and against the
independent second statement fixtures/coco_eval_ref.py (exact equality: the flags are decisions on identical float64 values, everything
after them is integer counts through the same IEEE operations).  Parity with the published evaluator itself is unpinned."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import coco_eval_cases as cases  # noqa: E402
import coco_eval_ref as ref  # noqa: E402
import gen_golden_coco as ggc  # noqa: E402
import gen_golden_roidb as ggr  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "coco_roidb.npz")))


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("coco_data"))
    ggc.build_coco(d)
    return d


# ---------------------------------------------------------------------------------------------------------------- imdb / roidb
@pytest.mark.parametrize("flipped", [True, False])
def test_roidb_fields_filter_and_minibatches_equal_the_reference(fixture, data_dir, flipped):
    from roi_data_layer.layer import RoIDataLayer
    fp = ggr.case_prefix(flipped)
    with ggr.repo_cfg(data_dir, flipped=flipped):
        imdb, roidb, filtered = ggc.repo_roidb()
        np.random.seed(ggr.SEED)
        layer = RoIDataLayer(filtered, imdb.num_classes)
        draws = []
        for _ in range(ggr.n_draws(len(filtered))):
            blobs = layer.forward()
            draws.append((layer.last_draw[0], blobs["im_info"], blobs["gt_boxes"]))
    want = {}
    ggr.roidb_arrays(fp, roidb, want)
    keys = [k for k in fixture if k.startswith(fp + "e") or k == fp + "n"]
    assert sorted(want) == sorted(keys) and len(roidb) == (20 if flipped else 10) == imdb.num_images
    for k in keys:
        assert want[k].dtype == fixture[k].dtype and want[k].shape == fixture[k].shape and np.array_equal(want[k], fixture[k]), k
    e = roidb[0]
    assert e["boxes"].dtype == np.uint16 and e["gt_classes"].dtype == np.int32 and e["seg_areas"].dtype == np.float32
    assert all("seg_areas" in r and "width" in r and "height" in r for r in roidb)          # the twins keep them, unlike the base class
    kept = [k for k, r in enumerate(roidb) if any(r is f for f in filtered)]
    assert kept == fixture[fp + "filtered"].tolist()
    only_crowd = sorted(i for i, _, _ in ggc.TRAIN_IMAGES).index(ggc.ONLY_CROWD)
    assert only_crowd not in kept and len(kept) == (18 if flipped else 9)
    assert roidb[only_crowd]["gt_overlaps"].toarray().tolist() == [[-1.0] * 81]             # a crowd row: -1 for all classes
    # minibatches: the reference's `!= 0 & ...` precedence keeps crowd boxes among the gt rows
    assert [d[0] for d in draws] == fixture[fp + "db_inds"].tolist()
    assert np.array_equal(np.stack([d[1] for d in draws]), fixture[fp + "im_info"])
    crowd_rows = 0
    for k, (db, _, gtb) in enumerate(draws):
        assert gtb.dtype == np.float32 and gtb.shape == fixture["%sgt%d" % (fp, k)].shape and np.array_equal(gtb, fixture["%sgt%d" % (fp, k)]), k
        assert len(gtb) == len(filtered[db]["gt_classes"])
        crowd_rows += int(np.sum(filtered[db]["max_overlaps"] < 0))
    assert crowd_rows > 0


def test_classes_id_maps_paths_and_views(fixture, data_dir):
    from datasets.factory import get_imdb, list_imdbs
    with ggr.repo_cfg(data_dir):
        train, mini = get_imdb("coco_2014_train"), get_imdb("coco_2014_minival")
        assert train.name == "coco_2014_train" and mini.name == "coco_2014_minival" and train.num_classes == 81
        assert np.array_equal(np.array(train.classes), fixture["classes"]) and train.classes[0] == "__background__"
        assert [train._class_to_coco_cat_id[c] for c in train.classes[1:]] == fixture["class_cat_ids"].tolist() == ggc.CAT_IDS
        assert train._coco_cat_id_to_class_ind[90] == 80 and train._coco_cat_id_to_class_ind[13] == 12          # ids have gaps: 12 is missing
        assert train.image_index == fixture["image_index"].tolist() == sorted(i for i, _, _ in ggc.TRAIN_IMAGES)
        assert mini.image_index == fixture["minival_image_index"].tolist()
        assert os.path.relpath(mini.image_path_at(0), data_dir) == str(fixture["minival_image0"]) == \
            os.path.join("coco", "images", "val2014", "COCO_val2014_000000037777.jpg")                          # a view into val2014
        assert mini._get_ann_file() == os.path.join(data_dir, "coco", "annotations", "instances_minival2014.json")
        assert train.image_path_at(0).endswith(os.path.join("train2014", "COCO_train2014_000000000009.jpg"))
        from datasets.coco import ann_file, coco
        assert ann_file("test-dev", "2015", "D") == os.path.join("D", "coco", "annotations", "image_info_test-dev2015.json")
        assert coco("minival", "2014")._view_map == {"minival2014": "val2014", "valminusminival2014": "val2014", "test-dev2015": "test2015"}
        dets = ggc.synth_dets(3, len(mini.image_index))
        assert np.array_equal(ggc.results_arrays(mini._coco_results_one_category(dets[1], 18)), fixture["results_one_category"])
        # the box that needs clipping and the zero-area annotation
        by_id = dict(zip(train.image_index, train.gt_roidb()))
        w, h = [(w, h) for i, h, w in ggc.TRAIN_IMAGES if i == ggc.CLIPPED][0]
        assert [w - 1, h - 1] in by_id[ggc.CLIPPED]["boxes"][:, 2:].tolist()
        n_zero = sum(1 for a in train._COCO.loadAnns(train._COCO.getAnnIds(imgIds=ggc.ZERO_AREA)) if a["area"] == 0)
        assert n_zero == 1 and len(by_id[ggc.ZERO_AREA]["boxes"]) == len(train._COCO.getAnnIds(imgIds=ggc.ZERO_AREA)) - 1
        with pytest.raises(KeyError) as err:
            get_imdb("coco_2014_val")                              # registered, but its annotation file is not there
        assert os.path.join("coco", "annotations", "instances_val2014.json") in str(err.value)
    for name in ("coco_2014_train", "coco_2014_val", "coco_2014_minival", "coco_2014_valminusminival", "coco_2014_trainval", "coco_2015_test",
                 "coco_2015_test-dev", "voc_2007_trainval"):
        assert name in list_imdbs()


def test_coco_api_methods(data_dir):
    from datasets.coco_api import COCO
    c = COCO(os.path.join(data_dir, "coco", "annotations", "instances_train2014.json"))
    assert c.getCatIds() == ggc.CAT_IDS and c.loadCats(c.getCatIds())[0]["name"] == "class_01"                 # sorted, the file is not
    assert c.getImgIds() == sorted(i for i, _, _ in ggc.TRAIN_IMAGES) and c.loadImgs(9)[0]["width"] == 60 and len(c.loadImgs([9, 25])) == 2
    ids = c.getAnnIds(imgIds=139, iscrowd=None)
    assert ids and all(a["image_id"] == 139 for a in c.loadAnns(ids)) and len(c.getAnnIds()) == len(c.dataset["annotations"])
    assert sorted(c.getAnnIds(imgIds=139, iscrowd=0) + c.getAnnIds(imgIds=139, iscrowd=1)) == sorted(ids)
    res = c.loadRes([dict(image_id=139, category_id=1, bbox=[1.0, 2.0, 3.0, 4.5], score=0.5), dict(image_id=9, category_id=2, bbox=[0, 0, 2, 2], score=0.1)])
    assert [(a["id"], a["area"], a["iscrowd"]) for a in res.loadAnns(res.getAnnIds())] == [(1, 13.5, 0), (2, 4, 0)]
    with pytest.raises(AssertionError):
        c.loadRes([dict(image_id=123456, category_id=1, bbox=[1, 2, 3, 4], score=0.5)])


def test_roidb_sizes_come_from_the_entries_for_coco(data_dir, monkeypatch):
    import PIL.Image
    with ggr.repo_cfg(data_dir, flipped=False):
        def boom(*a, **k):
            raise AssertionError("prepare_roidb opened an image of a coco imdb")
        monkeypatch.setattr(PIL.Image, "open", boom)
        _, roidb, _ = ggc.repo_roidb()
    assert [(r["height"], r["width"]) for r in roidb] == [(h, w) for _, h, w in sorted(ggc.TRAIN_IMAGES)]


def test_combined_roidb_and_missing_data(data_dir, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools"))
    import importlib
    tool = importlib.import_module("trainval_net")
    from datasets.factory import get_imdb
    with ggr.repo_cfg(data_dir):
        imdb, roidb = tool.combined_roidb("coco_2014_train+coco_2014_minival", verbose=False)
        assert imdb.name == "coco_2014_train+coco_2014_minival" and imdb.num_classes == 81 and len(roidb) == 28
    with ggr.repo_cfg(str(tmp_path)):
        with pytest.raises(KeyError) as err:
            get_imdb("coco_2014_train")
        assert os.path.join(str(tmp_path), "coco", "annotations", "instances_train2014.json") in str(err.value)


# ---------------------------------------------------------------------------------------------------------------- evaluator
def run(images, cats, gts, dts, match="host"):
    from datasets.coco_eval import COCOeval
    g = cases.dataset(images, cats, gts)
    e = COCOeval(g, g.loadRes([dict(d) for d in dts]), match=match)
    e.evaluate()
    e.accumulate()
    e.summarize(verbose=False)
    return e


def one(v):
    """`v` is the protocol's 1.0: precision is tp / (fp + tp + spacing(1)), so a cell whose curve ends after ONE true positive holds
    1 / (1 + 2^-52) = 1 - 2^-52 (two or more give exactly 1.0), and a mean of such cells lies between the two."""
    return 1.0 - 2.0 ** -52 <= v <= 1.0


def test_known_perfect_detections():
    """(a) detections equal to the non-crowd gts: every AP / AR is 1.0; no gt is medium, so the medium statistics stay -1."""
    gts = [cases.gt(1, 5, [10, 10, 10, 10]), cases.gt(1, 7, [100, 100, 100, 100]), cases.gt(2, 5, [30, 40, 100, 120]), cases.gt(2, 7, [5, 5, 20, 20]),
           cases.gt(2, 7, [200, 200, 150, 150], crowd=1)]
    dts = [cases.det(a["image_id"], a["category_id"], a["bbox"], 0.9 - 0.1 * n) for n, a in enumerate(gts) if not a["iscrowd"]]
    e = run([1, 2], [5, 7], gts, dts)
    assert all(one(e.stats[i]) for i in (0, 1, 2, 3, 5)) and e.stats[6:10].tolist() == [1.0] * 4 and e.stats[11] == 1.0
    assert e.stats[4] == -1.0 and e.stats[10] == -1.0


def test_known_no_detections_and_half_precision():
    """(b) gts without detections: AP 0, AR 0.  (c) one gt, a disjoint detection at .9 and the exact one at .8: tp = [0,1], fp = [1,1],
    precision envelope 0.5 at all 101 recall points of all 10 thresholds."""
    e = run([1], [3, 4], [cases.gt(1, 3, [0, 0, 50, 50]), cases.gt(1, 4, [0, 0, 50, 50])],
            [cases.det(1, 4, [300, 300, 50, 50], 0.9), cases.det(1, 4, [0, 0, 50, 50], 0.8)])
    assert np.all(e.eval["precision"][:, :, 0, 0, 2] == 0.0) and np.all(e.eval["recall"][:, 0, 0, 2] == 0.0)
    assert np.all(e.eval["precision"][:, :, 1, 0, 2] == 0.5) and np.all(e.eval["recall"][:, 1, 0, 2] == 1.0)
    assert e.stats[0] == 0.25 and e.stats[8] == 0.5
    only_b = run([1], [3], [cases.gt(1, 3, [0, 0, 50, 50])], [])
    assert only_b.stats[:3].tolist() == [0.0, 0.0, 0.0] and only_b.stats[6:9].tolist() == [0.0, 0.0, 0.0]
    assert run([1], [4], [cases.gt(1, 4, [0, 0, 50, 50])], [cases.det(1, 4, [300, 300, 50, 50], 0.9), cases.det(1, 4, [0, 0, 50, 50], 0.8)]).stats[0] == 0.5


def test_known_crowd_handling():
    """(d) a detection inside a crowd gt only is ignored: the category has no countable gt and stays -1; two detections may both match
    the one crowd; with a second, exactly detected normal gt the AP is 1.0 (the crowd matches cost nothing)."""
    crowd = cases.gt(1, 2, [0, 0, 100, 100], crowd=1)
    in_crowd = [cases.det(1, 2, [10, 10, 20, 20], 0.9), cases.det(1, 2, [50, 50, 20, 20], 0.95)]
    e = run([1], [2], [crowd], in_crowd)
    assert np.all(e.det_matched[0] == 1) and np.all(e.det_ignored[0] == 1) and e.det_matched.shape == (4, 10, 2)
    assert np.all(e.eval["precision"] == -1) and e.stats.tolist() == [-1.0] * 12
    e = run([1], [2], [crowd, cases.gt(1, 2, [200, 200, 40, 40])], in_crowd + [cases.det(1, 2, [200, 200, 40, 40], 0.5)])
    assert one(e.stats[0]) and e.stats[8] == 1.0 and np.all(e.det_matched[0] == 1)
    assert e.det_ignored[0, 0].tolist() == [1, 1, 0]                # score order: the two crowd matches, then the real one


def test_known_threshold_and_area_boundaries():
    """(e) IoU exactly 0.5 / 0.75 matches at that threshold and not above; (f) a gt of area exactly 32^2 is small AND medium."""
    e = run([1], [1, 2], [cases.gt(1, 1, [0, 0, 10, 10]), cases.gt(1, 2, [0, 0, 10, 10])],
            [cases.det(1, 1, [0, 0, 10, 5], 0.9), cases.det(1, 2, [0, 0, 10, 7.5], 0.9)])
    thrs = e.params.iouThrs
    assert thrs[0] == 0.5 and thrs[5] == 0.75
    assert e.det_matched[0, :, 0].tolist() == [1] + [0] * 9 and e.det_matched[0, :, 1].tolist() == [1] * 6 + [0] * 4
    assert one(e.stats[1]) and 0.5 - 2.0 ** -53 <= e.stats[2] <= 0.5   # AP50: both categories; AP75: only the second (mean of 0 and "1.0")
    e = run([1], [1], [cases.gt(1, 1, [0, 0, 32, 32])], [cases.det(1, 1, [0, 0, 32, 32], 0.9)])
    assert e.gt_ignored[:, 0].tolist() == [0, 0, 0, 1]
    assert one(e.stats[3]) and one(e.stats[4]) and e.stats[5] == -1.0 and e.stats[9] == 1.0 and e.stats[10] == 1.0 and e.stats[11] == -1.0
    e = run([1], [1], [cases.gt(1, 1, [0, 0, 96, 96])], [cases.det(1, 1, [0, 0, 96, 96], 0.9)])
    assert e.gt_ignored[:, 0].tolist() == [0, 1, 0, 0]


def test_known_detection_cuts():
    """(g) 130 exact detections of 130 disjoint gts in one group: cut to the 100 best scores, so AR@100 = 100/130, AR@10 = 10/130 and
    AR@1 = 1/130 (means of ten equal values each; compared to 1e-15)."""
    gts = [cases.gt(1, 1, [20 * (n % 13), 20 * (n // 13), 10, 10]) for n in range(130)]
    scores = np.random.RandomState(1).permutation(130) / 130.0
    e = run([1], [1], gts, [cases.det(1, 1, g["bbox"], s) for g, s in zip(gts, scores)])
    assert e.csr["det_off"].tolist() == [0, 100] and np.array_equal(e.csr["det_score"], np.sort(scores)[::-1][:100])
    assert np.all(e.det_matched[0] == 1) and np.all(e.det_ignored[0] == 0)
    assert np.allclose(e.stats[6:9], [1 / 130.0, 10 / 130.0, 100 / 130.0], rtol=0, atol=1e-15)
    assert np.all(e.eval["recall"][:, 0, 0, :] == np.array([1, 10, 100]) / 130.0)


@pytest.fixture(scope="module")
def random_case():
    images, cats, gts, dts = cases.random_set(seed=0)
    groups = ref.evaluate(cases.dataset(images, cats, gts).dataset["annotations"], dts, images, cats)
    precision, recall = ref.accumulate(groups, len(images), len(cats))
    return images, cats, gts, dts, groups, precision, recall, ref.summarize(precision, recall)


def test_host_matcher_equals_the_second_statement_on_a_random_set(random_case):
    from datasets import coco_eval
    images, cats, gts, dts, groups, precision, recall, stats = random_case
    e = run(images, cats, gts, dts)
    sizes = np.diff(e.csr["det_off"]), np.diff(e.csr["gt_off"])
    # the set is what it claims: cut groups, groups of one kind only, crowds, ties, boundary areas, every kind of outcome
    assert sizes[0].max() == 100 and sizes[1].max() == 40 and (sizes[0] == 0).any() and (sizes[1] == 0).any() and len(sizes[0]) > 150
    assert 0.05 < e.csr["gt_crowd"].mean() < 0.3 and len(np.unique(e.csr["det_score"])) <= 50
    assert (e.csr["gt_area"] == 1024.0).any() and (e.csr["gt_area"] == 9216.0).any()
    matched, ignored, gt_ignored, iou = coco_eval.match_host(e.csr, e.params.iouThrs, e.params.areaRng, want_iou=True)
    want = cases.ref_flags(groups, e.csr)
    assert iou.shape == want[3].shape and np.array_equal(iou, want[3]) and 0 < (iou == 0).mean() < 1
    assert np.array_equal(gt_ignored, want[2]) and np.array_equal(matched, want[0]) and np.array_equal(ignored, want[1])
    assert np.array_equal(matched, e.det_matched) and np.array_equal(ignored, e.det_ignored)
    for a in range(4):
        assert 0 < matched[a].mean() < 1 and 0 < ignored[a].mean() < 1 and (matched[a, 0] != matched[a, 9]).any()
    assert np.array_equal(e.eval["precision"], precision) and np.array_equal(e.eval["recall"], recall) and np.array_equal(e.stats, stats)
    assert 0.05 < stats[0] < 0.95 and (precision > -1).any() and (precision[precision > -1] < 1).any()


def test_evaluating_from_the_written_json_equals_evaluating_from_memory(random_case, data_dir, tmp_path, capsys):
    """datasets.coco.evaluate_detections on the synthetic minival: results json -> loadRes -> evaluator; the 12 summary lines, the pkl, and
    the same numbers as evaluating the in-memory results; salt / cleanup of competition_mode."""
    from datasets.coco_eval import COCOeval
    from datasets.factory import get_imdb
    rng = np.random.RandomState(4)
    with ggr.repo_cfg(data_dir):
        imdb = get_imdb("coco_2014_minival")
        imdb._match = "host"
    all_boxes = [[[] for _ in range(imdb.num_images)] for _ in range(imdb.num_classes)]
    for i, image_id in enumerate(imdb.image_index):
        for a in imdb._COCO.loadAnns(imdb._COCO.getAnnIds(imgIds=image_id)):
            x, y, w, h = a["bbox"]
            rows = [[x, y, x + w - 1, y + h - 1, rng.rand()], [x + 3, y + 2, x + w + 1, y + h - 3, rng.rand()], [1, 2, 9, 11, rng.rand()]]
            c = imdb._coco_cat_id_to_class_ind[a["category_id"]]
            prev = all_boxes[c][i]
            all_boxes[c][i] = np.array(rows, dtype=np.float32) if isinstance(prev, list) else np.vstack([prev, np.array(rows, dtype=np.float32)])
    out = str(tmp_path / "out")
    ev = imdb.evaluate_detections(all_boxes, out)
    text = capsys.readouterr().out
    lines = text.splitlines()
    assert "~~~~ Mean and per-category AP @ IoU=[0.50,0.95] ~~~~" in lines and "~~~~ Summary metrics ~~~~" in lines
    summary = lines[lines.index("~~~~ Summary metrics ~~~~") + 1:][:12]
    assert summary[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ")
    assert summary[8].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ") and len(summary) == 12
    assert [float(s.split("= ")[-1]) for s in summary] == [float("%.3f" % v) for v in ev.stats]
    assert len(lines[lines.index("~~~~ Mean and per-category AP @ IoU=[0.50,0.95] ~~~~") + 1:lines.index("~~~~ Summary metrics ~~~~")]) == 81
    with open(os.path.join(out, "detection_results.pkl"), "rb") as f:
        saved = pickle.load(f)
    assert type(saved) is dict and np.array_equal(saved["stats"], ev.stats) and saved["precision"].shape == (10, 101, 80, 4, 3)
    assert saved["recall"].shape == (10, 80, 4, 3) and saved["params"]["maxDets"] == [1, 10, 100] and 0.2 < ev.stats[0] < 1.0
    assert [f for f in os.listdir(out) if f.endswith(".json")] == []                                    # salted file cleaned up
    # from memory: the same results without the trip through json text
    from datasets import results
    mem = results.write_coco_results_file(all_boxes, imdb.classes, imdb.image_index, imdb._class_to_coco_cat_id, str(tmp_path / "r.json"))
    e2 = COCOeval(imdb._COCO, imdb._COCO.loadRes(mem), match="host")
    e2.evaluate(), e2.accumulate(), e2.summarize(verbose=False)
    assert np.array_equal(e2.stats, ev.stats) and np.array_equal(e2.eval["precision"], ev.eval["precision"])
    imdb.competition_mode(True)
    imdb.evaluate_detections(all_boxes, out)
    assert os.path.isfile(os.path.join(out, "detections_minival2014_results.json"))
    with open(os.path.join(out, "detections_minival2014_results.json")) as f:
        assert len(json.load(f)) == len(mem)


def test_reval_tool_evaluates_a_coco_run(data_dir, tmp_path):
    out = tmp_path / "run"
    out.mkdir()
    boxes = [[np.zeros((0, 5), dtype=np.float32) for _ in range(len(ggc.MINIVAL_IMAGES))] for _ in range(81)]
    boxes[1][0] = np.array([[1, 2, 30, 40, 0.5]], dtype=np.float32)
    with open(str(out / "detections.pkl"), "wb") as f:
        pickle.dump(boxes, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools", "reval.py"), str(out), "--imdb", "coco_2014_minival", "--set",
                        "DATA_DIR", data_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("Average Precision  (AP)") == 6 and r.stdout.count("Average Recall     (AR)") == 6
    assert os.path.isfile(str(out / "detection_results.pkl"))


@pytest.mark.skipif(not os.path.isdir("/root/reference/lib/roi_data_layer"), reason="needs the reference tree")
def test_fixture_matches_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fixtures", "gen_golden_coco.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "bit-exact" in r.stdout, r.stdout + r.stderr
