"""GPU: tools/demo.py end to end through its main(argv) -- decode on the device, detect, draw from the device-resident records, encode on the
device, Huffman stage and file write on worker threads -- against the composition of the pieces with the HOST statements of the drawing and
of the encoder: every output file byte for byte."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

from test_jpeg_cpu import picture
from test_jpeg_gpu import _net

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# A seeded, untrained network scores every class of every proposal near 1 / 21 = 0.048: at 0.04 most of them pass, and greedy NMS at 0.3
# still leaves boxes of every class -- the test asserts that some were drawn.
CONF = 0.04


def test_demo_main_equals_the_composition_of_its_pieces(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools"))
    try:
        import demo
    finally:
        sys.path.pop(0)
    from frcnn_hip import jpeg
    from model.config import cfg
    from model.test import _get_image_blob
    from utils import visualization as vis
    src = tmp_path / "in"
    src.mkdir()
    paths = []
    for i in range(3):
        p = src / ("%06d.jpg" % (i + 1))
        picture(160, 120, 40 + i).save(str(p), "JPEG", quality=90, subsampling=i % 3)
        paths.append(str(p))
    before = [open(p, "rb").read() for p in paths]
    sess, net = _net(dev, "TEST", "demo")
    sess.init_variables(net.variable_specs())
    out_dir, json_path = str(tmp_path / "out"), str(tmp_path / "dets.json")
    old = (cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.TEST.NMS)
    cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = (120,), 160
    log = io.StringIO()
    try:
        with contextlib.redirect_stdout(log):
            rc = demo.main(["--net", "res50", "--dir", str(src), "--out", out_dir, "--conf", str(CONF), "--nms", "0.3", "--quality", "85",
                            "--json", json_path], network=(sess, net))
        assert rc == 0 and cfg.TEST.NMS == old[2]
        text = log.getvalue()
        for p in paths:
            assert "Demo for %s" % p in text
        assert text.count("Detection took") == 3 and "object proposals" in text
        report = json.load(open(json_path))
        assert [r["image"] for r in report] == paths
        drawn = 0
        cfg.TEST.NMS = 0.3
        for p, entry in zip(paths, report):
            im_d = jpeg.decode_bgr(p, dev)
            assert tuple(im_d.shape) == (120, 160, 3)
            img, im_scale = _get_image_blob(sess, net, im_d)
            im_info = np.array([img.shape[1], img.shape[2], im_scale], dtype=np.float32)
            dets, cnt = net.detect_device(sess, img, im_info, im_d.shape[:2], max_per_image=demo.MAX_PER_IMAGE, thresh=demo.detect_thresh(CONF))
            n = int(cnt.item())
            rec = dets.cpu().numpy()
            kept = rec[:n][rec[:n, 4] >= np.float32(CONF)]
            assert n == len(kept) == len(entry["detections"]) and n <= dets.shape[0]          # the threshold inside detect_device is the rule's
            assert [d["class"] for d in entry["detections"]] == [demo.CLASSES[int(c)] for c in kept[:, 5]]
            drawn += n
            pic = im_d.cpu().numpy().copy()
            vis.draw_detections(pic, rec, n, demo.CLASSES, conf=CONF)                         # the host statement of the drawing ...
            assert n == 0 or not np.array_equal(pic, im_d.cpu().numpy())
            want = jpeg.encode_bgr(pic, quality=85, subsampling=2)                            # ... and of the encoder
            out_path = os.path.join(out_dir, os.path.basename(p))
            assert entry["output"] == out_path and open(out_path, "rb").read() == want, p
        assert drawn >= 1
    finally:
        cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.TEST.NMS = old
    assert [open(p, "rb").read() for p in paths] == before                                    # the inputs are unchanged
    assert sorted(os.listdir(out_dir)) == [os.path.basename(p) for p in paths]
