"""GPU: cfg.HIP.TEST_BATCH_IMAGES -- frcnn_prep_image_batched against frcnn_prep_image slot by slot, model.test.detect_bgr_batch against
detect_bgr, and model.test.test_net_imdb in same-size batches against the one-by-one loop: the same bits everywhere, so a padded slot, a
slot order or a deferred read-back never shows in another image's result."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

CLASSES = ('__background__', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
           'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')
MEANS = np.array([[[102.9801, 115.9465, 122.7717]]])

# (h, w) -> (OH, OW): an upscale narrower than one 256-lane block whose last column is the single-tap tail; a fractional scale with an OW
# that is no multiple of 256; scale 1.0
SHAPES = [((7, 9), (12, 15)), ((33, 50), (120, 182)), ((120, 160), (120, 160))]


def _scale(hw, out_hw):
    """an im_scale for which cv2's output size rule gives out_hw from hw"""
    s = out_hw[0] / float(hw[0])
    assert int(np.round(hw[0] * s)) == out_hw[0] and int(np.round(hw[1] * s)) == out_hw[1]
    return s


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("out_c", [3, 4])
@pytest.mark.parametrize("as_float", [False, True], ids=["uint8", "float32"])
@pytest.mark.parametrize("hw,out_hw", SHAPES, ids=["7x9", "33x50", "120x160"])
def test_prep_image_batched_equals_prep_image_slot_by_slot(dev, hw, out_hw, as_float, out_c, B):
    from frcnn_hip import ops
    rng = np.random.RandomState(hw[0] * 10 + B)
    ims = rng.randint(0, 256, size=(B,) + hw + (3,)).astype(np.uint8)
    src = torch.from_numpy(ims.astype(np.float32) if as_float else ims).to(dev)
    scale = _scale(hw, out_hw)
    got = ops.prep_image_batched(src, MEANS, scale, out_hw, out_c=out_c)
    assert got.shape == (B,) + out_hw + (out_c,) and got.dtype == torch.float32
    for b in range(B):
        want = ops.prep_image(src[b], MEANS, scale, out_hw, out_c=out_c)
        assert torch.equal(got[b], want[0]), b
    assert float(got.abs().sum()) > 0


def test_prep_image_batched_into_an_output_that_is_not_16_byte_aligned(dev):
    """out_c = 4 into a view that starts 4 bytes into its allocation: the launcher must leave the float4 path, for every slot"""
    from frcnn_hip import ops
    (hw, out_hw), B = SHAPES[1], 3
    ims = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(B,) + hw + (3,)).astype(np.uint8)).to(dev)
    n = B * out_hw[0] * out_hw[1] * 4
    flat = torch.full((n + 8,), -7.0, dtype=torch.float32, device=dev)
    out = flat[1:1 + n].view((B,) + out_hw + (4,))
    assert out.data_ptr() % 16 == 4
    scale = _scale(hw, out_hw)
    assert ops.prep_image_batched(ims, MEANS, scale, out_hw, out=out, out_c=4) is out
    want = torch.cat([ops.prep_image(ims[b], MEANS, scale, out_hw, out_c=4) for b in range(B)])
    assert torch.equal(out, want)
    assert float(flat[0]) == -7.0 and bool((flat[1 + n:] == -7.0).all())                 # nothing written outside the view


def test_prep_image_batched_refuses_an_empty_batch(dev):
    import frcnn_hip
    lib = frcnn_hip.lib()
    src = torch.zeros((1, 7, 9, 3), dtype=torch.uint8, device=dev)
    out = torch.full((1, 12, 15, 4), 3.0, dtype=torch.float32, device=dev)
    means = (frcnn_hip.c_double * 3)(1.0, 2.0, 3.0)
    st = torch.cuda.current_stream().cuda_stream
    for B in (0, -1):
        assert lib.frcnn_prep_image_batched(src.data_ptr(), 0, B, 7, 9, means, 12 / 7.0, out.data_ptr(), 12, 15, 4, st) == -1      # FRCNN_E_ARG
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---- the loops: a VOC devkit with real JPEG files (the helpers of tests/test_jpeg_gpu.py, restated) ------------------------------------
def picture(w, h, seed):
    """seeded smooth-plus-noise image"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(3):
        smooth = 128 + 90 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (5.0 - c)) + 30 * np.sin((xx + yy) / 11.0)
        chans.append(smooth + rng.randn(h, w) * 12)
    return Image.fromarray(np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8), "RGB")


def build_devkit(data_dir, split, sizes, seed):
    """<data_dir>/VOCdevkit2007/VOC2007/{JPEGImages,Annotations,ImageSets/Main/<split>.txt} with seeded images and one or two boxes each"""
    rng = np.random.RandomState(seed)
    base = os.path.join(data_dir, "VOCdevkit2007", "VOC2007")
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    index = ["%06d" % (i + 1) for i in range(len(sizes))]
    for i, (name, (h, w)) in enumerate(zip(index, sizes)):
        picture(w, h, seed + i).save(os.path.join(base, "JPEGImages", name + ".jpg"), "JPEG", quality=90, subsampling=i % 3)
        body = ""
        for k in range(1 + i % 2):
            x1, y1 = rng.randint(1, w - 12), rng.randint(1, h - 12)
            x2, y2 = rng.randint(x1 + 4, w + 1), rng.randint(y1 + 4, h + 1)
            body += ("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>0</difficult><bndbox><xmin>%d</xmin>"
                     "<ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>" % (CLASSES[rng.randint(1, 21)], x1, y1, x2, y2))
        with open(os.path.join(base, "Annotations", name + ".xml"), "w") as f:
            f.write("<annotation><filename>%s.jpg</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>"
                    % (name, w, h, body))
    with open(os.path.join(base, "ImageSets", "Main", split + ".txt"), "w") as f:
        f.write("\n".join(index) + "\n")
    return index


def _net(dev, mode, tag):
    from frcnn_hip.runtime import Session
    from nets.resnet_v1 import resnetv1
    sess = Session(device=dev, seed=9)
    net = resnetv1(num_layers=50)
    net.create_architecture(mode, 21, tag=tag, anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
    return sess, net


@pytest.fixture(scope="module")
def toy(dev):
    sess, net = _net(dev, "TEST", "batched_imdb")
    sess.init_variables(net.variable_specs())
    yield sess, net
    sess.close()


SIZES = [(120, 160)] * 3 + [(160, 120)] + [(120, 160)] * 2 + [(160, 120)] * 2 + [(96, 160)] + [(120, 160)] * 1 + [(160, 120)]


@pytest.mark.parametrize("jpeg_device", [False, True], ids=["pil", "jpeg_device"])
def test_batched_imdb_loop_equals_the_one_by_one_loop(dev, toy, tmp_path, jpeg_device):
    """11 JPEGs of three sizes, interleaved; TEST_BATCH_IMAGES = 4: (120,160) one full batch and 2 padded to 4, (160,120) one full batch,
    (96,160) a single.  all_boxes equals the TEST_BATCH_IMAGES = 1 run array for array, and the per-image line is printed once per image."""
    from datasets.factory import get_imdb
    from model.config import cfg
    from model.test import plan_batches, test_net_imdb
    assert plan_batches(SIZES, 4) == [([0, 1, 2, 4], 0), ([5, 9], 2), ([3, 6, 7, 10], 0), ([8], 0)]
    data_dir = str(tmp_path / "data")
    build_devkit(data_dir, "test", SIZES, seed=41)
    sess, net = toy
    old = (cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES)
    cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.JPEG_DEVICE = data_dir, (120,), 160, jpeg_device
    runs, logs = [], []
    try:
        for batch in (1, 4):
            cfg.HIP.TEST_BATCH_IMAGES = batch
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                imdb = get_imdb("voc_2007_test")
                runs.append(test_net_imdb(sess, net, imdb, str(tmp_path / ("out%d" % batch)), thresh=0.0))
            logs.append(log.getvalue())
    finally:
        cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES = old
    one, four = runs
    total = 0
    for j in range(1, 21):
        for i in range(len(SIZES)):
            a, b = np.asarray(one[j][i]), np.asarray(four[j][i])
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (j, i)
            total += a.shape[0]
    print("detections in all_boxes: %d" % total)
    assert total > 0
    for log in logs:
        lines = [l for l in log.splitlines() if l.startswith("im_detect: ")]
        assert [l.split()[1] for l in lines] == ["%d/%d" % (i + 1, len(SIZES)) for i in range(len(SIZES))]
    assert os.path.exists(str(tmp_path / "out4" / "detections.pkl"))


def test_detect_bgr_batch_drops_padded_slots_and_equals_detect_bgr(dev, toy):
    from model.config import cfg
    from model.test import detect_bgr, detect_bgr_batch
    sess, net = toy
    ims = [np.ascontiguousarray(np.asarray(picture(160, 120, 60 + k))[:, :, ::-1]) for k in range(4)]
    old = (cfg.TEST.SCALES, cfg.TEST.MAX_SIZE)
    cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = (120,), 160
    try:
        want = [detect_bgr(sess, net, im) for im in ims]
        got = detect_bgr_batch(sess, net, ims, n_valid=3)                                # a list of numpy images, the 4th is padding
        got_d = detect_bgr_batch(sess, net, torch.from_numpy(np.stack(ims)).to(dev), n_valid=2)
        got_all = detect_bgr_batch(sess, net, np.stack(ims))
    finally:
        cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = old
    assert len(got) == 3 and len(got_d) == 2 and len(got_all) == 4
    total = 0
    for res in (got, got_d, got_all):
        for k, per_class in enumerate(res):
            assert len(per_class) == len(want[k]) == 21
            for a, b in zip(per_class, want[k]):
                assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), k
                total += a.shape[0]
    assert total > 0


# Sizes whose h * w is no multiple of 4: slot k of the batch's uint8 buffer starts k * h * w * 3 bytes in, i.e. NOT 4-byte aligned for
# k = 1, and frcnn_jpeg_pixels refuses such an output address (its colour kernel stores dwords).  90 x 121: h * w = 2 mod 4; 99 x 121: odd.
ODD_SIZES = [(90, 121)] * 3 + [(99, 121)] * 2


def test_read_into_a_slot_that_is_not_4_byte_aligned(dev, tmp_path):
    from frcnn_hip import jpeg
    paths = []
    for k in range(3):
        p = str(tmp_path / ("%d.jpg" % k))
        picture(121, 99, 80 + k).save(p, "JPEG", quality=90, subsampling=k % 3)
        paths.append(p)
    stage = torch.full((3, 99, 121, 3), 7, dtype=torch.uint8, device=dev)
    assert stage[1].data_ptr() % 4 != 0 and stage[2].data_ptr() % 4 != 0
    pre = jpeg.JpegPrefetcher(paths, dev)
    for k in range(3):
        assert pre.read_into(stage[k]).data_ptr() == stage[k].data_ptr()
    pre.close()
    out = torch.full((2, 99, 121, 3), 7, dtype=torch.uint8, device=dev)
    assert jpeg.decode_bgr(paths[1], dev, out=out[1]).data_ptr() == out[1].data_ptr()     # the synchronous form, same rule
    for k in range(3):
        assert torch.equal(stage[k].cpu(), torch.from_numpy(jpeg.pil_bgr(paths[k]))), k
    assert torch.equal(out[1], stage[1])


@pytest.mark.parametrize("jpeg_device", [False, True], ids=["pil", "jpeg_device"])
def test_batched_imdb_loop_with_slots_that_are_not_4_byte_aligned(dev, toy, tmp_path, jpeg_device):
    """TEST_BATCH_IMAGES = 2 over ODD_SIZES: a full batch and a padded one of 90 x 121, a full batch of 99 x 121; every second slot is
    misaligned for the device decoder.  all_boxes equals the one-by-one run."""
    from datasets.factory import get_imdb
    from model.config import cfg
    from model.test import plan_batches, test_net_imdb
    assert plan_batches(ODD_SIZES, 2) == [([0, 1], 0), ([2], 1), ([3, 4], 0)]
    data_dir = str(tmp_path / "data")
    build_devkit(data_dir, "test", ODD_SIZES, seed=71)
    sess, net = toy
    old = (cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES)
    cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.JPEG_DEVICE = data_dir, (120,), 160, jpeg_device
    runs = []
    try:
        for batch in (1, 2):
            cfg.HIP.TEST_BATCH_IMAGES = batch
            with contextlib.redirect_stdout(io.StringIO()):
                imdb = get_imdb("voc_2007_test")
                runs.append(test_net_imdb(sess, net, imdb, str(tmp_path / ("out%d" % batch)), thresh=0.0))
    finally:
        cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES = old
    one, two = runs
    total = 0
    for j in range(1, 21):
        for i in range(len(ODD_SIZES)):
            a, b = np.asarray(one[j][i]), np.asarray(two[j][i])
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (j, i)
            total += a.shape[0]
    assert total > 0


def test_a_run_without_a_limit_per_image_keeps_the_one_by_one_loop(dev, toy, tmp_path):
    """max_per_image = 0 (test.py:176: no cut): test_net_imdb under the switch runs, image by image, and gives what it gives without it"""
    from datasets.factory import get_imdb
    from model.config import cfg
    from model.test import test_net_imdb
    data_dir = str(tmp_path / "data")
    build_devkit(data_dir, "test", [(120, 160)] * 3, seed=91)
    sess, net = toy
    old = (cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES)
    cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = data_dir, (120,), 160
    runs = []
    try:
        for batch in (1, 2):
            cfg.HIP.TEST_BATCH_IMAGES = batch
            with contextlib.redirect_stdout(io.StringIO()):
                imdb = get_imdb("voc_2007_test")
                runs.append(test_net_imdb(sess, net, imdb, str(tmp_path / ("out%d" % batch)), max_per_image=0, thresh=0.0))
    finally:
        cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES = old
    total = 0
    for j in range(1, 21):
        for i in range(3):
            a, b = np.asarray(runs[0][j][i]), np.asarray(runs[1][j][i])
            assert a.shape == b.shape and np.array_equal(a, b), (j, i)
            total += a.shape[0]
    assert total > 100 * 3                                                               # more than a limited run could hold
