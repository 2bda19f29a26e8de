"""GPU: frcnn_coco_match (csrc/coco_eval.hip) through ops.coco_match against BOTH host statements of the protocol -- the numpy matcher of
datasets.coco_eval and the plain loops of fixtures/coco_eval_ref.py -- with the float64 IoU compared bit for bit and all three flag arrays
compared exactly, no group skipped; then the COCO imdb through tools/coco_net.py and tools/trainval_net.py on the synthetic tree of
fixtures/gen_golden_coco.py.  No reference tree is needed: expected values come from tests/golden/coco_roidb.npz and the host statements.

Which groups take which tile path (csrc/coco_eval.hip: LDS when D*G*8 + 68*G <= 16384 bytes): with D = 100 detections that is G <= 18 gts.
The random set (D <= 100, G <= 40) has groups on both sides; the minival-scale set adds G up to 90, i.e. workspace tiles of 72 000 bytes."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import coco_eval_cases as cases  # noqa: E402
import coco_eval_ref as ref  # noqa: E402
import gen_golden_coco as ggc  # noqa: E402
import gen_golden_roidb as ggr  # noqa: E402

pytestmark = pytest.mark.gpu
LDS_BYTES = 16384


def in_lds(csr):
    D, G = np.diff(csr["det_off"]), np.diff(csr["gt_off"])
    return D * G * 8 + 68 * G <= LDS_BYTES


def check_against_both(images, cats, gts, dts, stream=None):
    from datasets import coco_eval
    from datasets.coco_eval import COCOeval
    g = cases.dataset(images, cats, gts)
    ev = {}
    for match in ("host", "device"):
        e = COCOeval(g, g.loadRes([dict(d) for d in dts]), match=match)
        if match == "device" and stream is not None:
            with torch.cuda.stream(stream):
                e.evaluate()
        else:
            e.evaluate()
        e.accumulate()
        e.summarize(verbose=False)
        ev[match] = e
    csr = ev["host"].csr
    p = ev["host"].params
    host = coco_eval.match_host(csr, p.iouThrs, p.areaRng, want_iou=True)
    if stream is not None:
        with torch.cuda.stream(stream):
            dev_out = coco_eval.match_device(csr, p.iouThrs, p.areaRng, want_iou=True)
    else:
        dev_out = coco_eval.match_device(csr, p.iouThrs, p.areaRng, want_iou=True)
    second = cases.ref_flags(ref.evaluate(g.dataset["annotations"], dts, images, cats), csr)
    for name, want in (("numpy matcher", host), ("second statement", second)):
        assert dev_out[3].dtype == np.float64 and dev_out[3].shape == want[3].shape, name
        assert np.array_equal(dev_out[3].view(np.int64), want[3].view(np.int64)), name                 # the IoU, bit for bit
        for k, what in enumerate(("det_matched", "det_ignored", "gt_ignored")):
            assert dev_out[k].dtype == np.uint8 and dev_out[k].shape == want[k].shape and np.array_equal(dev_out[k], want[k]), (name, what)
    assert np.array_equal(ev["device"].det_matched, host[0]) and np.array_equal(ev["device"].det_ignored, host[1])
    assert np.array_equal(ev["device"].eval["precision"], ev["host"].eval["precision"]) and np.array_equal(ev["device"].stats, ev["host"].stats)
    return ev["device"], csr


def test_coco_match_equals_both_host_statements_on_the_random_set(dev):
    e, csr = check_against_both(*cases.random_set(seed=0))
    lds = in_lds(csr)
    pairs = np.diff(csr["det_off"]) * np.diff(csr["gt_off"])
    assert (lds & (pairs > 0)).sum() > 50 and (~lds).sum() >= 3                                        # both tile paths ran
    assert 0.05 < e.stats[0] < 0.95
    check_against_both(*cases.random_set(seed=1, n_images=9, n_cats=5), stream=torch.cuda.Stream())    # once on a non-default stream


def test_coco_match_known_answers(dev):
    big_crowd = cases.gt(1, 2, [0, 0, 100, 100], crowd=1)
    e, _ = check_against_both([1], [2], [big_crowd, cases.gt(1, 2, [200, 200, 40, 40])],
                              [cases.det(1, 2, [10, 10, 20, 20], 0.9), cases.det(1, 2, [50, 50, 20, 20], 0.95), cases.det(1, 2, [200, 200, 40, 40], 0.5)])
    assert e.det_matched[0, 0].tolist() == [1, 1, 1] and e.det_ignored[0, 0].tolist() == [1, 1, 0]     # both match the one crowd
    e, _ = check_against_both([1], [1, 2], [cases.gt(1, 1, [0, 0, 10, 10]), cases.gt(1, 2, [0, 0, 10, 10])],
                              [cases.det(1, 1, [0, 0, 10, 5], 0.9), cases.det(1, 2, [0, 0, 10, 7.5], 0.9)])
    assert e.det_matched[0, :, 0].tolist() == [1] + [0] * 9 and e.det_matched[0, :, 1].tolist() == [1] * 6 + [0] * 4   # IoU exactly .5 / .75
    e, _ = check_against_both([1], [1], [cases.gt(1, 1, [0, 0, 32, 32])], [cases.det(1, 1, [0, 0, 32, 32], 0.9)])
    assert e.gt_ignored[:, 0].tolist() == [0, 0, 0, 1]                                                 # 32^2: small and medium
    gts = [cases.gt(1, 1, [20 * (n % 13), 20 * (n // 13), 10, 10]) for n in range(130)]
    scores = np.random.RandomState(1).permutation(130) / 130.0
    e, csr = check_against_both([1], [1], gts, [cases.det(1, 1, g["bbox"], s) for g, s in zip(gts, scores)])
    assert csr["det_off"].tolist() == [0, 100] and not in_lds(csr)[0] and np.all(e.det_matched == 1)   # 100 x 130: a workspace tile
    # groups of one kind only still write their flags; no detections at all, no gts at all
    e, _ = check_against_both([1, 2], [3], [cases.gt(1, 3, [0, 0, 50, 50])], [cases.det(2, 3, [0, 0, 40, 40], 0.9), cases.det(2, 3, [0, 0, 20, 20], 0.8)])
    assert e.gt_ignored[:, 0].tolist() == [0, 1, 0, 1] and e.det_ignored[:, 0, :].tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]]
    check_against_both([1], [3], [cases.gt(1, 3, [0, 0, 50, 50])], [])
    check_against_both([1], [3], [], [cases.det(1, 3, [0, 0, 40, 40], 0.9)])


def test_coco_match_at_minival_scale(dev):
    images, cats, gts, dts = cases.random_set(seed=2, n_images=200, n_cats=80, max_gt=90, fill=0.1)
    e, csr = check_against_both(images, cats, gts, dts)
    lds = in_lds(csr)
    G = np.diff(csr["gt_off"])
    print("groups %d (LDS tiles %d, workspace tiles %d), detections %d, gts %d, pairs %d"
          % (len(lds), lds.sum(), (~lds).sum(), csr["det_off"][-1], csr["gt_off"][-1], int(np.sum(np.diff(csr["det_off"]) * G))))
    assert len(lds) > 3000 and lds.sum() > 1000 and (~lds).sum() > 50 and G.max() == 90


def test_entry_argument_checks(dev):
    import frcnn_hip
    L = frcnn_hip.lib()
    assert L.frcnn_coco_match_workspace_bytes(10, 100, 50, 700) >= 11 * 8 + 700 * 8 + 50 * 64
    assert L.frcnn_coco_match(None, None, None, None, None, None, 1, None, 10, None, 4, None, None, None, None, None, 0, None) == -1
    off = torch.zeros(2, dtype=torch.int64, device=dev)
    thr = torch.zeros(70, dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr()
    assert L.frcnn_coco_match(None, p(off), None, None, None, p(off), 1, p(thr), 10, p(thr), 7, None, None, None, None, p(thr), 560, None) == -3
    assert L.frcnn_coco_match(None, p(off), None, None, None, p(off), 1, p(thr), 10, p(thr), 4, None, None, None, None, p(thr), 8, None) == -2
    torch.cuda.synchronize()


def _tool(name, args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools", name)] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("coco_data"))
    ggc.build_coco(d)
    return d


def test_coco_net_tool_evaluates_the_synthetic_minival(dev, data_dir, tmp_path):
    """tools/coco_net.py --imdb coco_2014_minival with initialiser weights: detections.pkl, the 12 summary lines, detection_results.pkl
    whose stats (device matcher) equal the host evaluator's on the saved detections."""
    from datasets import results
    from datasets.coco_eval import COCOeval
    from datasets.factory import get_imdb
    out = _tool("coco_net.py", ["--net", "res50", "--imdb", "coco_2014_minival", "--set", "DATA_DIR", data_dir, "ROOT_DIR", str(tmp_path),
                                "TEST.SCALES", "[160]", "TEST.MAX_SIZE", "288"], 900)
    lines = out.splitlines()
    summary = lines[lines.index("~~~~ Summary metrics ~~~~") + 1:][:12]
    assert len(summary) == 12 and sum("Average Precision  (AP)" in s for s in summary) == 6 and sum("Average Recall     (AR)" in s for s in summary) == 6
    run_dir = os.path.join(str(tmp_path), "output", "res50", "coco_2014_minival", "default")
    with open(os.path.join(run_dir, "detection_results.pkl"), "rb") as f:
        saved = pickle.load(f)
    with open(os.path.join(run_dir, "detections.pkl"), "rb") as f:
        all_boxes = pickle.load(f)
    assert saved["match"] == "device" and len(all_boxes) == 81 and len(all_boxes[0]) == len(ggc.MINIVAL_IMAGES)
    assert sum(len(all_boxes[c][i]) for c in range(1, 81) for i in range(len(ggc.MINIVAL_IMAGES))) > 0
    with ggr.repo_cfg(data_dir):
        imdb = get_imdb("coco_2014_minival")
    mem = results.write_coco_results_file(all_boxes, imdb.classes, imdb.image_index, imdb._class_to_coco_cat_id, str(tmp_path / "r.json"))
    e = COCOeval(imdb._COCO, imdb._COCO.loadRes(str(tmp_path / "r.json")), match="host")
    e.evaluate(), e.accumulate(), e.summarize(verbose=False)
    assert len(mem) > 0 and np.array_equal(saved["stats"], e.stats) and np.array_equal(saved["precision"], e.eval["precision"])


def test_trainval_net_tool_trains_from_the_coco_roidb(dev, data_dir, tmp_path):
    """tools/trainval_net.py --imdb coco_2014_train --iters 3: the reference's roidb lines, 81 classes, finite losses, a snapshot whose
    cursor sits on the golden draw; and the gt rows staged on the device for the first steps equal the golden file's (crowd boxes
    included)."""
    fixture = dict(np.load(os.path.join(ROOT, "tests", "golden", "coco_roidb.npz")))
    fp = ggr.case_prefix(True)
    out_dir = str(tmp_path / "snapshots")
    out = _tool("trainval_net.py", ["--iters", "3", "--imdb", "coco_2014_train", "--net", "res50", "--output", out_dir, "--set", "DATA_DIR", data_dir,
                                    "TRAIN.SCALES", "[160,176]", "TRAIN.MAX_SIZE", "288", "TRAIN.LEARNING_RATE", "0.000000001", "TRAIN.DISPLAY", "1",
                                    "TRAIN.BATCH_SIZE", "64"], 900)
    for line in ("Loaded dataset `coco_2014_train` for training", "Appending horizontally-flipped training examples...", "20 roidb entries",
                 "Filtered 2 roidb entries: 20 -> 18"):
        assert line in out, (line, out[-3000:])
    losses = [float(ln.split("total loss:")[1]) for ln in out.splitlines() if "total loss:" in ln]
    assert len(losses) == 3 and all(np.isfinite(losses)), out[-3000:]
    with open(os.path.join(out_dir, "res101_faster_rcnn_iter_3.pkl"), "rb") as f:
        meta = pickle.load(f)
    assert meta["iter"] == 3 and int(meta["data_layer"]["perm"][meta["data_layer"]["cur"] - 1]) == fixture[fp + "db_inds"][2]
    # the same draws staged in-process under the fixture's scales
    from frcnn_hip.runtime import Session
    from nets.resnet_v1 import resnetv1
    from roi_data_layer.layer import RoIDataLayer
    sess = Session(device=dev, seed=9)
    net = resnetv1(num_layers=50)
    net.create_architecture("TRAIN", 81, tag="coco_stage", anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
    with ggr.repo_cfg(data_dir):
        imdb, _, filtered = ggc.repo_roidb()
        np.random.seed(ggr.SEED)
        layer = RoIDataLayer(filtered, imdb.num_classes)
        crowd_rows = 0
        for k in range(6):
            blobs = layer.forward()
            with net._train_scope(sess, blobs):
                net._stage_train_inputs(sess, blobs)
                gt = net._gt_boxes.cpu().numpy()
            assert layer.last_draw[0] == fixture[fp + "db_inds"][k]
            assert gt.dtype == np.float32 and np.array_equal(gt, fixture["%sgt%d" % (fp, k)]), k
            assert net._im_info == tuple(float(v) for v in fixture[fp + "im_info"][k])
            crowd_rows += int(np.sum(filtered[layer.last_draw[0]]["max_overlaps"] < 0))
    assert crowd_rows > 0
