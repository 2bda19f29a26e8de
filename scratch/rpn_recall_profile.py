"""Proposal recall, the two measurements of profiles/rpn_recall.txt.  python scratch/rpn_recall_profile.py [out.txt]

1. The matcher alone: frcnn_proposal_recall for a batch of 8 images at 300 and 2000 candidates x 10 and 70 ground truths, HIP events
   around ops.proposal_recall after warm-up; beside it the C host statement (frcnn_proposal_recall_host) on the same data, and whether the
   two agree bit for bit.
2. The whole tool: tools/rpn_recall.py's loop (rpn_recall.rpn_recall: propose_device + matcher, no tail, no per-class stage) beside
   model.test.detect_paths_batched, the loop of tools/test_net.py, over the same 200 JPEG files (the set of tools/jpeg_bench.py --e2e:
   375x500 / 480x640 alternating, three chroma samplings, quality 90) written as a VOC devkit; ResNet-101, random weights, the device JPEG
   decoder, TEST_BATCH_IMAGES 1 and 8, one warm-up run and three alternated repeats of each.
3. The tool's stages alone at batch 8: preprocessing, propose_device and forward_device between HIP events, the loop's enqueue / finish
   on a staged batch without decode, the JPEG prefetcher alone."""
import os
import platform
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tf-faster-rcnn_amd", "tools"), os.path.join(ROOT, "tf-faster-rcnn_amd"), os.path.join(ROOT, "tf-faster-rcnn_amd", "lib")]
import jpeg_bench  # noqa: E402
import rpn_recall  # noqa: E402
from datasets import recall  # noqa: E402
from frcnn_hip import ops  # noqa: E402

dev = torch.device("cuda:0")
lines = ["proposal recall on %s; host: %s, numpy %s" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), np.__version__)]


def say(s):
    print(s, flush=True)
    lines.append(s)


# ---- 1. the matcher alone --------------------------------------------------------------------------------------------------------------
say("1. frcnn_proposal_recall, 8 images per launch; ms per call by HIP events around ops.proposal_recall (zero-fill of the slots + the kernel), "
    "50 repeats after 5 warm-up calls; host = frcnn_proposal_recall_host on the same arrays, best of 3 wall times")
for n in (300, 2000):
    for G in (10, 70):
        rng = np.random.RandomState(n + G)
        cands, gts = [], []
        for _ in range(8):
            w, h = rng.randint(20, 200, size=G), rng.randint(20, 200, size=G)
            x, y = rng.randint(0, 800, size=G), rng.randint(0, 400, size=G)
            g = np.stack([x, y, x + w, y + h], axis=1).astype(np.float64)
            c = g[np.arange(n) % G].astype(np.float32) + rng.uniform(-12, 12, size=(n, 4)).astype(np.float32)
            c[n - n // 10:] += 5000
            cands.append(c[rng.permutation(n)]), gts.append(g)
        p = recall.pack(cands, gts)
        t = {k: torch.from_numpy(p[k]).to(dev) for k in ("boxes", "start", "count", "scale", "gt", "gt_off")}
        call = lambda: ops.proposal_recall(t["boxes"], t["start"], t["count"], t["scale"], t["gt"], t["gt_off"], p["max_boxes"])
        for _ in range(5):
            out = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(50):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        host_s = []
        for _ in range(3):
            t0 = time.perf_counter()
            href = ops.proposal_recall_host(p["boxes"], p["start"], p["count"], p["scale"], p["gt"], p["gt_off"], p["max_boxes"])
            host_s.append(time.perf_counter() - t0)
        same = np.array_equal(out[0].cpu().numpy(), href[0]) and np.array_equal(out[1].cpu().numpy(), href[1])
        ms = np.array(ms)
        say("  %4d candidates x %2d gts: device median %.3f ms (min %.3f, max %.3f) = %.3f ms per image; host %.2f ms per call; bit-equal: %s"
            % (n, G, np.median(ms), ms.min(), ms.max(), np.median(ms) / 8, min(host_s) * 1e3, same))

# ---- 2. the whole tool beside the test_net loop ---------------------------------------------------------------------------------------------
from datasets.factory import get_imdb  # noqa: E402
from frcnn_hip.runtime import Session  # noqa: E402
from model.config import cfg  # noqa: E402
from model.test import detect_bgr, detect_paths_batched  # noqa: E402
from nets.resnet_v1 import resnetv1  # noqa: E402

FILES = 200
tmp = tempfile.mkdtemp(prefix="rpn_recall_profile_")
base = os.path.join(tmp, "VOCdevkit2007", "VOC2007")
for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
    os.makedirs(os.path.join(base, d))
rng = np.random.RandomState(1)
index = ["%06d" % (i + 1) for i in range(FILES)]
for i, name in enumerate(index):
    h, w = jpeg_bench.SIZES[i % 2]
    with open(os.path.join(base, "JPEGImages", name + ".jpg"), "wb") as f:
        f.write(jpeg_bench.encode(jpeg_bench.picture(h, w, i), jpeg_bench.SAMPLINGS[i % 3][0]))
    body = ""
    for k in range(1 + i % 3):
        x1, y1 = rng.randint(1, w - 60), rng.randint(1, h - 60)
        x2, y2 = rng.randint(x1 + 20, w + 1), rng.randint(y1 + 20, h + 1)
        body += ("<object><name>car</name><pose>Unspecified</pose><truncated>0</truncated><difficult>0</difficult><bndbox><xmin>%d</xmin>"
                 "<ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>" % (x1, y1, x2, y2))
    with open(os.path.join(base, "Annotations", name + ".xml"), "w") as f:
        f.write("<annotation><filename>%s.jpg</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>" % (name, w, h, body))
with open(os.path.join(base, "ImageSets", "Main", "test.txt"), "w") as f:
    f.write("\n".join(index) + "\n")

try:
    cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE = tmp, True
    cfg.HIP.GRAPH_CACHE_SHAPES = max(int(cfg.HIP.GRAPH_CACHE_SHAPES), 8)
    imdb = get_imdb("voc_2007_test")
    paths = [imdb.image_path_at(i) for i in range(imdb.num_images)]
    sess = Session(seed=3)
    net = resnetv1(num_layers=101)
    net.create_architecture("TEST", 21, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess.init_variables(net.variable_specs())
    areas = ["all", "small", "medium", "large"]

    def detector(batch):
        cfg.HIP.TEST_BATCH_IMAGES = batch
        t0 = time.perf_counter()
        if batch > 1:
            detect_paths_batched(sess, net, paths, batch)
        else:
            from frcnn_hip.jpeg import JpegPrefetcher
            for im in JpegPrefetcher(paths, sess.device):
                detect_bgr(sess, net, im)
        torch.cuda.synchronize()
        return FILES / (time.perf_counter() - t0)

    def tool(batch, limits):
        cfg.HIP.TEST_BATCH_IMAGES = batch
        t0 = time.perf_counter()
        res, _, _ = rpn_recall.rpn_recall(sess, net, imdb, limits, areas)
        torch.cuda.synchronize()
        return FILES / (time.perf_counter() - t0), res
    runs = [("test_net loop (whole detector, 300 proposals)", lambda b: detector(b)),
            ("rpn_recall, limits 100 300 (300 proposals)", lambda b: tool(b, [100, 300])[0]),
            ("rpn_recall, limits 100 300 1000 (1000 proposals)", lambda b: tool(b, [100, 300, 1000])[0])]
    say("2. %d JPEG files (375x500 / 480x640 alternating -> 600x800 blobs, 1-3 ground-truth boxes each), ResNet-101, random weights, JPEG_DEVICE on; "
        "images per second, wall time of the loop incl. the pass over the file headers, one warm-up run, then three alternated repeats" % FILES)
    for batch in (1, 8):
        for _, fn in runs:
            fn(batch)
        res = {name: [] for name, _ in runs}
        for _ in range(3):
            for name, fn in runs:
                res[name].append(fn(batch))
        for name, _ in runs:
            say("  TEST_BATCH_IMAGES %d  %-50s: %s  (min %.1f, max %.1f)" % (batch, name, "  ".join("%.1f" % v for v in res[name]), min(res[name]), max(res[name])))
    # 3. stages alone at batch 8, 1000 proposals: which one bounds the tool
    say("3. stages alone, TEST_BATCH_IMAGES 8, limits 100 300 1000, one staged 8 x 480 x 640 device batch, 3 warm-up + 30 repeats")
    from model.test import _PinnedRing
    gt = [[np.asarray(e["boxes"])[recall.select_gt(e, a)].astype(np.float64).reshape(-1, 4) for e in imdb.roidb] for a in areas]
    loop = rpn_recall.RecallLoop(sess, net, gt, [100, 300, 1000], False)
    stage = torch.randint(0, 256, (8, 480, 640, 3), dtype=torch.uint8, device=sess.device)
    idx = list(range(1, 16, 2))
    saved_post, cfg.TEST.RPN_POST_NMS_TOP_N = cfg.TEST.RPN_POST_NMS_TOP_N, 1000
    try:
        im_scale, OH, OW = ops.prep_image_shape(480, 640, cfg.TEST.SCALES[0], cfg.TEST.MAX_SIZE)
        info = np.array([OH, OW, im_scale], dtype=np.float32)
        with net.shape_scope(sess, (8, OH, OW, 4), (OH, OW)):
            img = sess.buf(net._tag + "/image", (8, OH, OW, 4))

        def events(fn, reps=30):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return np.median(ms), min(ms), max(ms)
        say("  preprocessing (frcnn_prep_image_batched)             : median %.3f ms per batch (min %.3f, max %.3f)"
            % events(lambda: ops.prep_image_batched(stage, cfg.PIXEL_MEANS, im_scale, (OH, OW), out=img, out_c=4)))
        say("  propose_device (graph replay: head + RPN + proposals) : median %.3f ms per batch (min %.3f, max %.3f)" % events(lambda: net.propose_device(sess, img, info)))
        say("  forward_device (graph replay: the whole detector, 1000 proposals) : median %.3f ms per batch (min %.3f, max %.3f)"
            % events(lambda: net.forward_device(sess, img, info)))
        ring = _PinnedRing(2)
        for _ in range(3):
            loop.finish(loop.enqueue(stage, idx, 8, ring))
        torch.cuda.synchronize()
        t0, prev = time.perf_counter(), None
        for _ in range(30):
            cur = loop.enqueue(stage, idx, 8, ring)
            if prev is not None:
                loop.finish(prev)
            prev = cur
        loop.finish(prev)
        dt = time.perf_counter() - t0
        say("  enqueue + deferred finish of the tool's loop, no decode : %.3f ms per batch = %.1f images/s" % (dt / 30 * 1e3, 240 / dt))
        t0 = time.perf_counter()
        for _ in range(30):
            loop.finish(loop.enqueue(stage, idx, 8, ring))
        dt = time.perf_counter() - t0
        say("  the same with every batch waited for before the next      : %.3f ms per batch = %.1f images/s" % (dt / 30 * 1e3, 240 / dt))
        from frcnn_hip.jpeg import JpegPrefetcher
        t0 = time.perf_counter()
        buf = [torch.empty((h, w, 3), dtype=torch.uint8, device=sess.device) for h, w in jpeg_bench.SIZES]
        src = JpegPrefetcher(paths, sess.device, depth=16)
        for i in range(FILES):
            src.read_into(buf[i % 2])
        torch.cuda.synchronize()
        src.close()
        say("  JpegPrefetcher alone over the %d files                   : %.1f images/s" % (FILES, FILES / (time.perf_counter() - t0)))
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N = saved_post
    _, res = tool(8, [100, 300, 1000])
    for r in res:
        say("  (untrained RPN) limit %4d area %-6s AR %.4f num_pos %d" % (r["limit"], r["area"], r["ar"], r["num_pos"]))
finally:
    shutil.rmtree(tmp, ignore_errors=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
