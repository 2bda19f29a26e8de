"""GPU: the device half of training from a roidb -- frcnn_prep_train_image (mirror + mean + cv2-linear resize into the staged stem input,
uint16 boxes * im_scale into the static gt buffer), RoIDataLayer's raw-image blobs through Network._stage_train_inputs, one training step
fed either way, and tools/trainval_net.py --imdb voc_2007_trainval on the seeded devkit of fixtures/gen_golden_roidb.py.  No reference
tree is needed: expected values come from tests/golden/roidb.npz and from the oracle's restatement (oracle/frcnn_oracle.py)."""
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import gen_golden_roidb as ggr  # noqa: E402  (test infrastructure: devkit builder + fixture layout)

pytestmark = pytest.mark.gpu
MEANS = np.array([[[102.9801, 115.9465, 122.7717]]])


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "roidb.npz")))


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("voc_data"))
    ggr.build_devkit(d)
    return d


# the size list of tests/test_dense_gpu.py::test_prep_image_vs_oracle plus one odd width
@pytest.mark.parametrize("h,w,target,max_size", [(375, 500, 600, 1000), (480, 640, 600, 1000), (300, 1000, 600, 1000), (600, 800, 600, 1000),
                                                 (97, 131, 64, 80), (120, 171, 96, 200)])
@pytest.mark.parametrize("flipped", [False, True])
def test_prep_train_image_vs_oracle(dev, h, w, target, max_size, flipped):
    """frcnn_prep_train_image == the oracle's get_image_blob of the image mirrored FIRST (minibatch.py:63-64) -- the same f32 operations in
    the same order, compared bit for bit -- for uint8 and float32 sources and 3 / 4 output channels; the staged 4th channel is zero; the
    unflipped call equals frcnn_prep_image."""
    import frcnn_oracle as ora
    from frcnn_hip import ops
    rng = np.random.RandomState(h + w)
    im = (rng.rand(h, w, 3) * 255).astype(np.uint8)
    want, want_scale = ora.get_image_blob(np.ascontiguousarray(im[:, ::-1]) if flipped else im, MEANS, target, max_size)
    scale, OH, OW = ops.prep_image_shape(h, w, target, max_size)
    assert scale == want_scale and (1, OH, OW, 3) == want.shape
    for src in (im, im.astype(np.float32)):
        src_d = torch.from_numpy(src).to(dev)
        for out_c in (3, 4):
            got = ops.prep_train_image(src_d, flipped, MEANS, scale, (OH, OW), out_c=out_c).cpu().numpy()
            assert got.shape == (1, OH, OW, out_c)
            assert np.array_equal(got[..., :3], want), (src.dtype, out_c)
            assert out_c == 3 or np.all(got[..., 3] == 0)
            if not flipped:
                assert np.array_equal(got, ops.prep_image(src_d, MEANS, scale, (OH, OW), out_c=out_c).cpu().numpy())
    if flipped:                                                    # (a random image is not its own mirror: the flag does something)
        assert not np.array_equal(want, ora.get_image_blob(im, MEANS, target, max_size)[0])


def test_prep_train_image_fills_gt_rows(dev):
    """gt rows = (float)((double)uint16 box * im_scale), class as float: numpy's `uint16 array * Python float` assigned into float32."""
    from frcnn_hip import ops
    rng = np.random.RandomState(5)
    for G in (1, 7, 64, 130):
        boxes = rng.randint(0, 65536, size=(G, 4)).astype(np.uint16)
        boxes[0] = [0, 65535, 1, 499]
        classes = rng.randint(1, 81, size=G).astype(np.int32)
        im = torch.zeros((8, 12, 3), dtype=torch.uint8, device=dev)
        for scale in (1.6, 600.0 / 375.0, 1000.0 / 1333.0):
            want = np.empty((G, 5), dtype=np.float32)
            want[:, 0:4] = boxes * scale
            want[:, 4] = classes
            gt = torch.full((G + 3, 5), -7.0, device=dev)
            ops.prep_train_image(im, False, MEANS, scale, (13, 19), boxes=torch.from_numpy(boxes).to(dev), classes=torch.from_numpy(classes).to(dev),
                                 gt_out=gt)
            got = gt.cpu().numpy()
            assert np.array_equal(got[:G], want) and np.all(got[G:] == -7.0)            # rows [0,G) only


def _net(dev, tag, seed=9, init=True):
    from frcnn_hip.runtime import Session
    from nets.resnet_v1 import resnetv1
    sess = Session(device=dev, seed=seed)
    net = resnetv1(num_layers=50)
    net.create_architecture("TRAIN", 21, tag=tag, anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
    if init:
        sess.init_variables(net.variable_specs())
    return sess, net


def test_data_layer_blobs_stage_to_the_golden_data_and_gt(dev, fixture, data_dir):
    """RoIDataLayer -> Network._stage_train_inputs: the staged image equals the reference's `data` blob (recorded under the stub cv2 =
    the oracle's resize) bit for bit, 4th channel zero, for flipped and unflipped draws; the device gt rows equal its gt_boxes."""
    from roi_data_layer.layer import RoIDataLayer
    gp = ggr.case_prefix(True, False)
    sess, net = _net(dev, "roidb_stage", init=False)
    with ggr.repo_cfg(data_dir):
        imdb, _, filtered = ggr.repo_roidb()
        np.random.seed(ggr.SEED)
        layer = RoIDataLayer(filtered, imdb.num_classes)
        checked = []
        for k in range(12):
            blobs = layer.forward()
            with net._train_scope(sess, blobs):
                net._stage_train_inputs(sess, blobs)
                image, gt = net._image.cpu().numpy(), net._gt_boxes.cpu().numpy()
            assert layer.last_draw[0] == fixture[gp + "db_inds"][k]
            assert gt.dtype == np.float32 and np.array_equal(gt, fixture["%sgt%d" % (gp, k)]) and np.array_equal(gt, blobs["gt_boxes"])
            assert image.shape[3] == 4 and np.all(image[..., 3] == 0) and image.shape[1:3] == (int(blobs["im_info"][0]), int(blobs["im_info"][1]))
            assert net._im_info == tuple(float(v) for v in fixture[gp + "im_info"][k])
            if "%sdata%d" % (gp, k) in fixture:
                assert np.array_equal(image[..., :3], fixture["%sdata%d" % (gp, k)]), k
                checked.append(bool(blobs["flipped"]))
    assert sorted(checked) == [False, False, True, True]


def _digest(ts):
    h = hashlib.sha256()
    for sc in sorted(ts.params):
        p = ts.params[sc]
        for t in (p.w, p.acc_w, p.bias, p.acc_b):
            if t is not None:
                h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_a_step_fed_by_raw_image_blobs_equals_one_fed_by_float_data(dev, data_dir):
    """The same entries (one mirrored) as RoIDataLayer's uint8 blobs and as the reference's float `data` blobs built by the oracle's
    restatement: the same image bits reach the same launches, so losses, weights and momentum agree bit for bit over two steps (the
    second one is the recorded step of its shape).  The learning rate is tiny: 0..255 pixels through randomly initialised weights."""
    import frcnn_oracle as ora
    from frcnn_hip.train import TrainState
    from model.config import cfg
    from roi_data_layer.layer import RoIDataLayer
    old = (cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO)
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO = 64, 0.0
    try:
        with ggr.repo_cfg(data_dir, scales=(160, 176), max_size=288):
            imdb, _, filtered = ggr.repo_roidb()
            np.random.seed(ggr.SEED)
            layer = RoIDataLayer(filtered, imdb.num_classes)
            raw = [layer.forward() for _ in range(5)]
            raw = [raw[0], raw[4]]                                   # draw 4 is a mirrored entry (golden db_inds[4] = 11 of 12)
            assert [b["flipped"] for b in raw] == [False, True]
            as_float = []
            for b in raw:
                im = np.ascontiguousarray(b["image"][:, ::-1]) if b["flipped"] else b["image"]
                data, scale = ora.get_image_blob(im, cfg.PIXEL_MEANS, b["target_size"], cfg.TRAIN.MAX_SIZE)
                assert np.float32(scale) == b["im_info"][2] and data.shape[1:3] == (int(b["im_info"][0]), int(b["im_info"][1]))
                as_float.append(dict(data=data, im_info=b["im_info"], gt_boxes=b["gt_boxes"]))
            results = []
            for tag, feed in (("roidb_raw", raw), ("roidb_float", as_float)):
                sess, net = _net(dev, tag)
                ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4)
                ts.lr = 1e-9
                losses = [net.train_step(sess, feed[i % 2], ts) for i in range(4)]
                torch.cuda.synchronize()
                results.append((losses, _digest(ts), dict(net.replay_stats)))
    finally:
        cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO = old
    (l0, d0, s0), (l1, d1, s1) = results
    print("losses (raw-image blobs):", l0)
    assert all(np.isfinite(v) for step in l0 for v in step), l0
    assert [tuple(np.float32(v).tobytes() for v in s) for s in l0] == [tuple(np.float32(v).tobytes() for v in s) for s in l1], (l0, l1)
    assert d0 == d1
    assert s0 == s1, (s0, s1)                                       # both forms take the same eager / recorded / replayed path


def _tool(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools", "trainval_net.py")] + args, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_trainval_net_trains_from_the_devkit_and_resumes(fixture, dev, data_dir, tmp_path):
    """tools/trainval_net.py --imdb voc_2007_trainval: the reference's roidb lines, finite losses, a snapshot whose .pkl carries the data
    layer's cursor; a second invocation resumes there and draws the next indices of the golden sequence (two TRAIN.SCALES entries, like
    the fixture: the index sequence depends on how many scales there are, not on their values).  Tiny learning rate: see above."""
    gp = ggr.case_prefix(True, False)
    want = fixture[gp + "db_inds"].tolist()
    out_dir = str(tmp_path / "snapshots")
    common = ["--imdb", "voc_2007_trainval", "--imdbval", "voc_2007_test", "--net", "res50", "--output", out_dir, "--set", "DATA_DIR", data_dir,
              "TRAIN.SCALES", "[160,176]", "TRAIN.MAX_SIZE", "288", "TRAIN.LEARNING_RATE", "0.000000001", "TRAIN.DISPLAY", "1",
              "TRAIN.BATCH_SIZE", "64"]

    def last_draw(it):
        with open(os.path.join(out_dir, "res101_faster_rcnn_iter_%d.pkl" % it), "rb") as f:
            meta = pickle.load(f)
        assert meta["iter"] == it and meta["data_layer"]["count"] == it and "np_random_state" in meta
        return int(meta["data_layer"]["perm"][meta["data_layer"]["cur"] - 1])

    def losses(out):
        return [float(ln.split("total loss:")[1]) for ln in out.splitlines() if "total loss:" in ln]

    out = _tool(["--iters", "4"] + common[:], 900)
    for line in ("Loaded dataset `voc_2007_trainval` for training", "Set proposal method: gt", "Appending horizontally-flipped training examples...",
                 "Preparing training data...", "14 roidb entries", "Filtered 2 roidb entries: 14 -> 12", "Output will be saved to `%s`" % out_dir):
        assert line in out, (line, out[-3000:])
    assert len(losses(out)) == 4 and all(np.isfinite(losses(out))), out[-3000:]
    assert last_draw(4) == want[3]
    out2 = _tool(["--iters", "6"] + common[:], 900)
    assert "Restoring model snapshots from" in out2 and [ln for ln in out2.splitlines() if ln.startswith("iter: ")][0].startswith("iter: 5 / 6")
    assert len(losses(out2)) == 2 and all(np.isfinite(losses(out2))), out2[-3000:]
    assert last_draw(6) == want[5]                                  # iterations 5 and 6 drew golden entries 4 and 5: the stream went on
