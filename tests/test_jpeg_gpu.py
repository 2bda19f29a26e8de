"""GPU: the device half of the JPEG path (csrc/jpeg_decode.hip: k_jpeg_idct, k_jpeg_color) against PIL bit for bit, its workspace check, the
chain into frcnn_prep_image, the ordered prefetcher with its ring of pinned buffers and its PIL fallback, and cfg.HIP.JPEG_DEVICE in the
test loop (model.test.test_net_imdb) and in the training data layer (RoIDataLayer -> Network._stage_train_inputs): the switch changes no
detection and no staged input."""
import contextlib
import io
import itertools
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

CLASSES = ('__background__', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
           'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')


def picture(w, h, seed, mode="RGB"):
    """seeded smooth-plus-noise image"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(3):
        smooth = 128 + 90 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (5.0 - c)) + 30 * np.sin((xx + yy) / 11.0)
        chans.append(smooth + rng.randn(h, w) * 12)
    im = Image.fromarray(np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8), "RGB")
    return im if mode == "RGB" else im.convert(mode)


def encode(im, fmt="JPEG", **kw):
    f = io.BytesIO()
    im.save(f, fmt, **kw)
    return f.getvalue()


def pil_pixels(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


# (height, width).  97 x 523 is the smallest size with more than 64 luma block columns (66 at 4:4:4): a block row spans waves; its cropped
# chroma plane (49 x 262 of 56 x 264 at 4:2:0) ends in one-sample tails.  The others: a single block, partial waves, cropped planes.
SIZES = [(1, 1), (7, 9), (17, 23), (31, 97), (97, 523)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_device_pixels_equal_pil_bit_for_bit(dev, size):
    from frcnn_hip import ops
    h, w = size
    for sampling, quality, restart in itertools.product((0, 1, 2, "L"), (75, 100), (0, 3)):
        im = picture(w, h, seed=w * 100 + h, mode="L" if sampling == "L" else "RGB")
        kw = dict(quality=quality, restart_marker_blocks=restart)
        if sampling != "L":
            kw["subsampling"] = sampling
        data = encode(im, **kw)
        geom = ops.jpeg_info(data)
        got = ops.jpeg_pixels(ops.jpeg_entropy_decode(data, geom=geom).to(dev), geom)
        assert got.shape == (h, w, 3) and got.dtype == torch.uint8
        assert torch.equal(got.cpu(), torch.from_numpy(pil_pixels(data))), (size, sampling, quality, restart)


def test_a_workspace_one_byte_short_is_refused_and_nothing_runs(dev):
    import frcnn_hip
    from frcnn_hip import ops
    lib = frcnn_hip.lib()
    data = encode(picture(33, 50, 2), quality=75, subsampling=2)
    geom = ops.jpeg_info(data)
    w, h, nc, hs, vs = geom[:5]
    coef_d = ops.jpeg_entropy_decode(data, geom=geom).to(dev)
    need = lib.frcnn_jpeg_workspace_bytes(w, h, nc, hs, vs)
    assert need >= 48 * 64 + 2 * 32 * 32                                 # the three MCU-padded sample planes
    ws = torch.full((need,), 7, dtype=torch.uint8, device=dev)
    out = torch.full((h, w, 3), 9, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.frcnn_jpeg_pixels(coef_d.data_ptr(), w, h, nc, hs, vs, out.data_ptr(), ws.data_ptr(), need - 1, st)
    torch.cuda.synchronize()
    assert rc == -1                                                      # FRCNN_E_ARG
    assert bool((ws == 7).all()) and bool((out == 9).all())
    assert lib.frcnn_jpeg_pixels(coef_d.data_ptr(), w, h, nc, hs, vs, out.data_ptr(), ws.data_ptr(), need, st) == 0
    assert torch.equal(out.cpu(), torch.from_numpy(pil_pixels(data)))


def test_decode_feeds_prep_image_the_same_bits(dev, tmp_path):
    from frcnn_hip import jpeg, ops
    from model.config import cfg
    data = encode(picture(160, 120, 3), quality=90)
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    im_d = jpeg.decode_bgr(str(path), dev)
    assert im_d.is_cuda and tuple(im_d.shape) == (120, 160, 3)
    scale, OH, OW = ops.prep_image_shape(120, 160, 600, 1000)
    got = ops.prep_image(im_d, cfg.PIXEL_MEANS, scale, (OH, OW))
    want = ops.prep_image(torch.from_numpy(pil_pixels(data)).to(dev), cfg.PIXEL_MEANS, scale, (OH, OW))
    assert got.shape == (1, 600, 800, 4) and torch.equal(got, want)


def test_prefetcher_keeps_order_wraps_its_ring_and_falls_back(dev, tmp_path):
    from frcnn_hip import jpeg
    sizes = [(40, 30), (97, 31), (64, 48), (33, 50), (160, 120)]
    items = [encode(picture(*sizes[i % 5], seed=i), quality=85, subsampling=i % 3, restart_marker_blocks=(i % 2) * 2) for i in range(10)]
    items.insert(3, encode(picture(40, 30, 77), quality=80, progressive=True))
    items.insert(8, encode(picture(64, 48, 78), "PNG"))
    assert len(items) == 12
    paths = []
    for i, d in enumerate(items):
        p = tmp_path / ("%02d.jpg" % i)
        p.write_bytes(d)
        paths.append(str(p))
    pre = jpeg.JpegPrefetcher(paths, dev, workers=3, depth=4)
    got = [t for t in pre]
    torch.cuda.synchronize()
    assert len(got) == 12 and len(pre._cache._slots) == 4                # 10 decodes through 4 pinned buffers: the ring wrapped
    assert all(s.buf is None or s.buf.is_pinned() for s in pre._cache._slots) and any(s.buf is not None for s in pre._cache._slots)
    for i, (t, d) in enumerate(zip(got, items)):
        assert t.is_cuda and torch.equal(t.cpu(), torch.from_numpy(pil_pixels(d))), i


# ---- cfg.HIP.JPEG_DEVICE in the two loops: a VOC devkit with real JPEG files ------------------------------------------------------------
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


def test_the_switch_changes_no_detection(dev, tmp_path):
    from datasets.factory import get_imdb
    from model.config import cfg
    from model.test import test_net_imdb
    data_dir = str(tmp_path / "data")
    build_devkit(data_dir, "test", [(120, 160)] * 6, seed=21)
    sess, net = _net(dev, "TEST", "jpeg_switch")
    sess.init_variables(net.variable_specs())
    old = (cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE)
    cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = data_dir, (120,), 160
    runs = []
    try:
        for on in (False, True):
            cfg.HIP.JPEG_DEVICE = on
            with contextlib.redirect_stdout(io.StringIO()):
                imdb = get_imdb("voc_2007_test")
                runs.append(test_net_imdb(sess, net, imdb, str(tmp_path / ("out%d" % on)), thresh=0.0))
    finally:
        cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = old
    off, on = runs
    total = 0
    for j in range(1, 21):
        for i in range(6):
            a, b = np.asarray(off[j][i]), np.asarray(on[j][i])
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (j, i)
            total += a.shape[0]
    assert total > 0


def test_the_switch_changes_no_staged_training_input(dev, tmp_path):
    """RoIDataLayer (with its decode-ahead under the switch) -> Network._stage_train_inputs: the staged image buffer and the gt rows of
    every draw, flipped and unflipped entries among them, are the same bits either way."""
    from datasets.factory import get_imdb
    from model.config import cfg
    from model.train_val import filter_roidb, get_training_roidb
    from roi_data_layer.layer import RoIDataLayer
    data_dir = str(tmp_path / "data")
    build_devkit(data_dir, "trainval", [(60, 90), (90, 60), (64, 88), (75, 51), (56, 84)], seed=31)
    sess, net = _net(dev, "TRAIN", "jpeg_train_stage")
    keys = ("USE_FLIPPED", "ASPECT_GROUPING", "SCALES", "MAX_SIZE")
    old = (cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, {k: cfg.TRAIN[k] for k in keys})
    cfg.DATA_DIR = data_dir
    cfg.TRAIN.USE_FLIPPED, cfg.TRAIN.ASPECT_GROUPING, cfg.TRAIN.SCALES, cfg.TRAIN.MAX_SIZE = True, False, (64, 80), 110
    runs = []
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            imdb = get_imdb("voc_2007_trainval")
            imdb.set_proposal_method("gt")
            roidb = filter_roidb(get_training_roidb(imdb))
        assert len(roidb) == 10
        for on in (False, True):
            cfg.HIP.JPEG_DEVICE = on
            np.random.seed(3)
            layer = RoIDataLayer(roidb, imdb.num_classes)
            staged = []
            for _ in range(12):                                          # past a reshuffle of the 10 entries
                blobs = layer.forward()
                assert torch.is_tensor(blobs["image"]) == on and (not on or blobs["image"].is_cuda)
                with net._train_scope(sess, blobs):
                    net._stage_train_inputs(sess, blobs)
                    staged.append((layer.last_draw, bool(blobs["flipped"]), net._image.clone(), net._gt_boxes.clone(), net._im_info))
            torch.cuda.synchronize()
            runs.append(staged)
            if on:
                assert layer._jpeg is not None
                layer._jpeg.close()
    finally:
        cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE = old[0], old[1]
        for k, v in old[2].items():
            cfg.TRAIN[k] = v
    off, on = runs
    assert {f for _, f, _, _, _ in off} == {False, True}
    for a, b in zip(off, on):
        assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and float(a[2].abs().sum()) > 0
