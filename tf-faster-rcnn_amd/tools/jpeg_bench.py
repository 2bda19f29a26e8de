#!/usr/bin/env python
"""Measurements behind cfg.HIP.JPEG_DEVICE (profiles/jpeg_decode.txt); separate from bench.py.

Seeded 375 x 500 and 480 x 640 images at quality 90 in 4:2:0 / 4:2:2 / 4:4:4.  Old and new paths alternate inside one call, after a
warm-up, with a few hundred decodes per timing window.

  --host      ms per image on the host: PIL decode + [:, :, ::-1] copy (the path before) against frcnn_jpeg_entropy_decode alone,
              one thread and 4 threads.  Needs no GPU.
  --kernels   N runs of frcnn_jpeg_pixels per case on the device, nothing else: the process to put under
              `rocprofv3 --kernel-trace --stats -- python tools/jpeg_bench.py --kernels`; prints the algorithmic bytes per image.
  --e2e       images per second of model.test.detect_bgr over 200 JPEG files with cfg.HIP.JPEG_DEVICE off and on, alternated in one
              process, three repeats each.  --batch N [N ...]: the same files through model.test.detect_paths_batched (the loop of
              test_net_imdb under cfg.HIP.TEST_BATCH_IMAGES = N; 1 = the detect_bgr loop above), every (N, switch) pair alternated in
              the same process (profiles/test_net_batched.txt).
  --encode    the other direction (profiles/demo_annotate.txt): 375 x 500 and 600 x 1000 images with 30 seeded boxes, quality 90, 4:2:0.
              The draw launch and the two encode launches between HIP events, the host Huffman stage per image, and files per second of
              draw + JpegWriter (4 workers) against the host path -- D2H copy, PIL draw, PIL save -- on 1 and 4 threads, alternated
              (--files per run; --files 0: the launches alone, the process to put under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import io
import os
import sys
import tempfile
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _init_paths  # noqa: F401

SIZES = ((375, 500), (480, 640))
SAMPLINGS = ((2, "4:2:0"), (1, "4:2:2"), (0, "4:4:4"))


def picture(h, w, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [128 + 90 * np.sin(xx / (30.0 + 9 * c) + c) * np.cos(yy / (50.0 - 7 * c)) + 30 * np.sin((xx + yy) / 110.0) + rng.randn(h, w) * 12
             for c in range(3)]
    return Image.fromarray(np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8), "RGB")


def encode(im, sampling):
    f = io.BytesIO()
    im.save(f, "JPEG", quality=90, subsampling=sampling)
    return f.getvalue()


def pil_bgr(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def window(fn, n, threads):
    """seconds per call of fn over n calls on `threads` threads"""
    t0 = time.perf_counter()
    if threads == 1:
        for _ in range(n):
            fn()
    else:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            list(ex.map(lambda _: fn(), range(n)))
    return (time.perf_counter() - t0) / n


def host(args):
    import torch
    from frcnn_hip import ops
    print("host ms per image, %d decodes per window, %d alternated windows each (min / median)" % (args.n, args.windows))
    print("%-9s %-6s %9s | %-15s | %-15s | %-15s" % ("size", "chroma", "bytes", "PIL+BGR 1 thr", "entropy 1 thr", "entropy 4 thr"))
    for (h, w) in SIZES:
        for sampling, label in SAMPLINGS:
            data = encode(picture(h, w, h + sampling), sampling)
            geom = ops.jpeg_info(data)
            nbytes = ops.jpeg_coef_bytes(geom)
            local = threading.local()                            # one coefficient buffer per thread

            def entropy():
                if not hasattr(local, "buf"):
                    local.buf = torch.empty(nbytes, dtype=torch.uint8)
                ops.jpeg_entropy_decode(data, out=local.buf, geom=geom)

            def pil():
                pil_bgr(data)
            for fn in (pil, entropy):
                window(fn, 20, 1)
            res = {"pil": [], "e1": [], "e4": []}
            for _ in range(args.windows):
                res["pil"].append(window(pil, args.n, 1))
                res["e1"].append(window(entropy, args.n, 1))
                res["e4"].append(window(entropy, args.n, 4))
            cell = lambda v: "%6.3f / %6.3f" % (min(v) * 1e3, float(np.median(v)) * 1e3)
            print("%-9s %-6s %9d | %-15s | %-15s | %-15s" % ("%dx%d" % (h, w), label, len(data), cell(res["pil"]), cell(res["e1"]), cell(res["e4"])))


def kernels(args):
    import torch
    from frcnn_hip import ops
    dev = torch.device("cuda", 0)
    for (h, w) in SIZES:
        for sampling, label in SAMPLINGS:
            data = encode(picture(h, w, h + sampling), sampling)
            geom = ops.jpeg_info(data)
            coef_d = ops.jpeg_entropy_decode(data, geom=geom).to(dev)
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            planes = int(ops.lib().frcnn_jpeg_workspace_bytes(*geom[:5]))
            for _ in range(args.n):
                ops.jpeg_pixels(coef_d, geom, out=out)
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.n):
                ops.jpeg_pixels(coef_d, geom, out=out)
            ev1.record()
            torch.cuda.synchronize()
            print("%dx%d %s: coefficients in %d B, planes out and in 2 x %d B, BGR out %d B = %d algorithmic bytes per image; "
                  "%.2f us per image between events (two launches, back to back, %d images)"
                  % (h, w, label, coef_d.numel(), planes, h * w * 3, coef_d.numel() + 2 * planes + h * w * 3,
                     ev0.elapsed_time(ev1) * 1e3 / args.n, args.n))


def e2e(args):
    import torch
    from frcnn_hip.runtime import Session
    from model.config import cfg
    from nets.resnet_v1 import resnetv1
    torch.cuda.set_device(0)
    sess = Session(seed=3)
    net = resnetv1(num_layers=args.layers)
    net.create_architecture("TEST", 21, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess.init_variables(net.variable_specs())
    tmp = tempfile.mkdtemp(prefix="jpeg_bench_")
    paths = []
    for i in range(args.files):
        h, w = SIZES[i % 2]
        p = os.path.join(tmp, "%04d.jpg" % i)
        with open(p, "wb") as f:
            f.write(encode(picture(h, w, i), SAMPLINGS[i % 3][0]))
        paths.append(p)

    saved = (cfg.HIP.JPEG_DEVICE, cfg.HIP.GRAPH_CACHE_SHAPES)           # the runs set both: main(argv) leaves the caller's cfg as it found it
    try:
        _e2e_runs(args, sess, net, paths)
    finally:
        cfg.HIP.JPEG_DEVICE, cfg.HIP.GRAPH_CACHE_SHAPES = saved
        for p in paths:
            os.remove(p)
        os.rmdir(tmp)


def _e2e_runs(args, sess, net, paths):
    import torch
    from frcnn_hip.jpeg import JpegPrefetcher
    from model.config import cfg
    from model.test import detect_bgr, detect_paths_batched
    # every (batch, shape) pair keeps its graph while the settings alternate: no timed window re-captures one (a test_net run has one batch
    # size, i.e. at most two graphs per shape, used in one contiguous stretch)
    cfg.HIP.GRAPH_CACHE_SHAPES = max(int(cfg.HIP.GRAPH_CACHE_SHAPES), len(SIZES) * 2 * len(args.batch))

    def run(on, batch):
        t0 = time.perf_counter()
        if batch > 1:
            cfg.HIP.JPEG_DEVICE = on
            detect_paths_batched(sess, net, paths, batch)
        elif on:
            for im in JpegPrefetcher(paths, sess.device):
                detect_bgr(sess, net, im)
        else:
            for p in paths:
                with open(p, "rb") as f:
                    detect_bgr(sess, net, pil_bgr(f.read()))
        torch.cuda.synchronize()
        return len(paths) / (time.perf_counter() - t0)
    cases = [(on, b) for b in args.batch for on in (False, True)]
    for on, b in cases:                                         # warm-up: graphs of every (batch, shape), pinned buffers, file cache
        run(on, b)
    res = {c: [] for c in cases}
    for _ in range(3):
        for c in cases:
            res[c].append(run(*c))
    print("detect_bgr over %d JPEG files (375x500 / 480x640 alternating, 4:2:0 / 4:2:2 / 4:4:4, quality 90), ResNet-%d, images per second, "
          "three alternated repeats" % (len(paths), args.layers))
    for on, b in cases:
        v = res[(on, b)]
        print("  batch %d  JPEG_DEVICE %-5s: %s  (min %.1f, max %.1f)" % (b, on, "  ".join("%.1f" % x for x in v), min(v), max(v)))
    if max(args.batch) > 1:
        # what each stage of the batched loop sustains ALONE, same files, same process: the slowest one bounds the loop
        from model import test as mt

        def alone(fn):
            fn()
            v = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                v.append(len(paths) / (time.perf_counter() - t0))
            return "  ".join("%.1f" % x for x in v)

        def pil_only():
            for p in paths:
                pil_bgr(open(p, "rb").read())

        def prefetch_only():
            for _ in JpegPrefetcher(paths, sess.device):
                pass
        print("stages alone, images per second, three repeats:")
        print("  PIL decode + BGR copy, one thread (JPEG_DEVICE False)      : %s" % alone(pil_only))
        print("  JpegPrefetcher, 4 workers + copy + 2 launches (True)       : %s" % alone(prefetch_only))
        for b in args.batch:
            stages = [torch.randint(0, 256, (b, h, w, 3), dtype=torch.uint8, device=sess.device) for (h, w) in SIZES]

            def chain_only():
                ring, prev = mt._PinnedRing(2), None
                for k in range(len(paths) // b):
                    cur = mt._enqueue_batch(sess, net, stages[(k * b // (len(paths) // 2)) % 2], b, 100, 0., ring)
                    if prev is not None:
                        mt._finish_batch(prev)
                    prev = cur
                mt._finish_batch(prev)
            print("  prep + chain + post + deferred read-back, batch %d, no decode : %s" % (b, alone(chain_only)))


ENCODE_SIZES = ((375, 500), (600, 1000))
ENCODE_CLASSES = ("__background__", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
                  "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")


def _boxes(h, w, n, seed):
    """n seeded detection records [n,6] inside an h x w image, scores 0.8 .. 1"""
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(0, w * 0.7, n), rng.uniform(0, h * 0.7, n)
    return np.stack([x1, y1, x1 + rng.uniform(20, w * 0.3, n), y1 + rng.uniform(20, h * 0.3, n), rng.uniform(0.8, 1.0, n),
                     rng.randint(1, 21, n)], axis=1).astype(np.float32)


def _pil_annotate(bgr, dets, path, quality):
    """the host path of today: PIL draws the boxes and labels on the image read back from the device, PIL encodes"""
    from PIL import Image, ImageDraw, ImageFont
    from utils.visualization import COLORS
    pic = Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]))
    draw, font = ImageDraw.Draw(pic), ImageFont.load_default()
    for x1, y1, x2, y2, s, c in dets:
        colour = COLORS[int(c) % len(COLORS)]
        draw.rectangle([x1, y1, x2, y2], outline=colour, width=2)
        label = "%s %.3f" % (ENCODE_CLASSES[int(c)], s)
        l, t, r, b = draw.textbbox((0, 0), label, font=font)
        ty = y1 - (b - t) - 4 if y1 - (b - t) - 4 >= 0 else y1
        draw.rectangle([x1, ty, x1 + r - l + 4, ty + b - t + 4], fill=colour)
        draw.text((x1 + 2, ty + 2 - t), label, fill=(0, 0, 0), font=font)
    pic.save(path, "JPEG", quality=quality)


def encode_bench(args):
    """--encode: the annotate-and-write half of tools/demo.py (profiles/demo_annotate.txt)"""
    import torch
    from frcnn_hip import jpeg, ops
    from utils.visualization import draw_detections
    dev = torch.device("cuda", 0)
    quality, ndet = 90, 30
    tmp = tempfile.mkdtemp(prefix="jpeg_bench_enc_")
    try:
        for (h, w) in ENCODE_SIZES:
            base = torch.from_numpy(np.ascontiguousarray(np.asarray(picture(h, w, h))[:, :, ::-1])).to(dev)
            dets = _boxes(h, w, ndet, h)
            dets_d, cnt_d = torch.from_numpy(dets).to(dev), torch.tensor([ndet], dtype=torch.int32, device=dev)
            im_d = base.clone()
            geom = ops.jpeg_encode_geom(h, w, 2)

            def events(fn):
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(args.n):
                    fn()
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) * 1e3 / args.n
            t_draw = events(lambda: draw_detections(im_d, dets_d, cnt_d, ENCODE_CLASSES, conf=0.8))
            t_coef = events(lambda: ops.jpeg_coefs(im_d, quality, 2))
            coef = ops.jpeg_coefs(im_d, quality, 2).cpu()
            scratch = np.empty(ops.jpeg_stream_bound(geom), dtype=np.uint8)
            nbytes = len(ops.jpeg_entropy_encode(coef, geom, out=scratch))
            window(lambda: ops.jpeg_entropy_encode(coef, geom, out=scratch), 20, 1)
            t_huff = [window(lambda: ops.jpeg_entropy_encode(coef, geom, out=scratch), args.n, 1) for _ in range(args.windows)]
            print("%dx%d 4:2:0 quality %d, %d boxes: draw %.2f us, ycc + fdct %.2f us per image between events (%d launches each, back to "
                  "back); coefficients %d B over PCIe against %d B of BGR; host Huffman stage %.3f / %.3f ms per image (min / median of %d "
                  "windows of %d, one thread); file %d B" % (h, w, quality, ndet, t_draw, t_coef, args.n, coef.numel(), h * w * 3,
                                                              min(t_huff) * 1e3, float(np.median(t_huff)) * 1e3, args.windows, args.n, nbytes))
            files = args.files
            if files <= 0:                                       # --files 0: the launches alone (the process to put under a kernel trace)
                continue

            def device_path():
                wr = jpeg.JpegWriter(dev, workers=4, depth=8)
                for i in range(files):
                    im_d.copy_(base)
                    draw_detections(im_d, dets_d, cnt_d, ENCODE_CLASSES, conf=0.8)
                    wr.submit(os.path.join(tmp, "d%04d.jpg" % i), im_d, quality=quality)
                wr.close()

            def host_path(threads):
                def one(i):
                    _pil_annotate(base.cpu().numpy(), dets, os.path.join(tmp, "h%04d.jpg" % i), quality)
                if threads == 1:
                    for i in range(files):
                        one(i)
                else:
                    with ThreadPoolExecutor(max_workers=threads) as ex:
                        list(ex.map(one, range(files)))
            cases = (("device draw + JpegWriter, 4 workers", device_path), ("D2H + PIL draw + PIL save, 1 thread", lambda: host_path(1)),
                     ("D2H + PIL draw + PIL save, 4 threads", lambda: host_path(4)))
            res = {name: [] for name, _ in cases}
            for _, fn in cases:
                fn()
            for _ in range(3):
                for name, fn in cases:
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    res[name].append(files / (time.perf_counter() - t0))
            print("  %d files per run, files per second, three alternated repeats:" % files)
            for name, _ in cases:
                print("    %-38s: %s" % (name, "  ".join("%.1f" % v for v in res[name])))
    finally:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--n", type=int, default=300, help="decodes per timing window / launches per case")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--layers", type=int, default=101)
    ap.add_argument("--batch", type=int, nargs="+", default=[1], help="--e2e: same-size images per launch (1 = the detect_bgr loop)")
    args = ap.parse_args(argv)
    if not (args.host or args.kernels or args.e2e or args.encode):
        ap.error("one of --host / --kernels / --e2e / --encode")
    if args.encode:
        encode_bench(args)
    if args.host:
        host(args)
    if args.kernels:
        kernels(args)
    if args.e2e:
        e2e(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
