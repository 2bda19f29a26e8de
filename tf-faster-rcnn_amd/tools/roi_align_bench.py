#!/usr/bin/env python
"""What POOLING_MODE 'align' costs next to 'crop', measured on the device (MI355X); prints a text report and writes it to --out
(section 1 of profiles/roi_align.txt is the report of one such run).

    python tf-faster-rcnn_amd/tools/roi_align_bench.py --out report.txt [--no-e2e]

Every time is the median of `--repeats` HIP-event intervals after `--warmup` untimed launches; crop and align alternate inside ONE
loop of one process, so clock and tenancy changes hit both.  Each interval holds `--inner` launches (a single launch of ~50 us is
shorter than the event resolution is trustworthy for).  min / max of the repeats are printed next to the median.

  forward   8 images x 300 RoIs (R = 2400) on a 38 x 63 map, C = 1024 (pool5), 512 and 2048 (the two maps of the fused tail entry),
            crop 7x7 against align 7x7 at S = 1 and S = 2; bytes = map read once + output written; GB/s = bytes / time
  backward  R = 256, C = 1024, one image, the same map
  end to end  ResNet-101, 600 x 1000, 8 images per forward pass (captured graph), fused tail entry on, seeded weights with bench.py's
            RPN calibration: images/s with 'crop' and with 'align' (S = 2), alternating"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
for p in (ROOT, PKG, os.path.join(PKG, "lib")):
    if p not in sys.path:
        sys.path.insert(0, p)

from frcnn_hip import ops  # noqa: E402
from model.config import cfg  # noqa: E402

H, W, STRIDE, P = 38, 63, 16.0, 7


def rois_for(rng, images, per_image):
    """proposal-like boxes in a 600 x 1000 image: sides 32..500 pixels, a tenth of them over an edge"""
    n = images * per_image
    w, h = rng.uniform(32, 500, n), rng.uniform(32, 400, n)
    x1, y1 = rng.uniform(-20, 1000 - 0.8 * w), rng.uniform(-20, 600 - 0.8 * h)
    img = np.repeat(np.arange(images), per_image)
    return np.stack([img, x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)


def timed(fns, warmup, repeats, inner):
    """fns: name -> callable; alternating; -> name -> (median, min, max) seconds per call"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e-3 / inner)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def forward_rows(dev, args, lines):
    rng = np.random.RandomState(1)
    rois = torch.from_numpy(rois_for(rng, 8, 300)).to(dev)
    lines.append("forward: R = 2400 (8 images x 300), map 38 x 63, P = 7; bytes = 8 maps read once + output written")
    lines.append("%6s %-12s %10s %10s %10s %10s %9s %8s" % ("C", "kernel", "median us", "min us", "max us", "MB", "GB/s", "x crop"))
    for C in (1024, 512, 2048):
        feat = torch.from_numpy(rng.randn(8, H, W, C).astype(np.float32)).to(dev)
        out = torch.empty((2400, P, P, C), device=dev)
        fns = {"crop": lambda: ops.crop_and_resize(feat, rois, STRIDE, P, out=out),
               "align S=1": lambda: ops.roi_align(feat, rois, STRIDE, P, 1, out=out),
               "align S=2": lambda: ops.roi_align(feat, rois, STRIDE, P, 2, out=out)}
        t = timed(fns, args.warmup, args.repeats, args.inner)
        nbytes = 4 * (feat.numel() + out.numel())
        for k, (med, lo, hi) in t.items():
            lines.append("%6d %-12s %10.1f %10.1f %10.1f %10.1f %9.0f %8.2f" % (C, k, med * 1e6, lo * 1e6, hi * 1e6, nbytes / 1e6, nbytes / med / 1e9,
                                                                           med / t["crop"][0]))
        del feat, out
    lines.append("")


def backward_rows(dev, args, lines):
    rng = np.random.RandomState(2)
    C, R = 1024, 256
    rois = torch.from_numpy(rois_for(rng, 1, R)).to(dev)
    dout = torch.from_numpy(rng.randn(R, P, P, C).astype(np.float32)).to(dev)
    dfeat = torch.zeros((1, H, W, C), device=dev)
    fns = {"crop": lambda: ops.crop_and_resize_bwd(dout, rois, STRIDE, dfeat),
           "align S=1": lambda: ops.roi_align_bwd(dout, rois, STRIDE, 1, dfeat),
           "align S=2": lambda: ops.roi_align_bwd(dout, rois, STRIDE, 2, dfeat)}
    t = timed(fns, args.warmup, args.repeats, max(1, args.inner // 4))
    nbytes = 4 * (dout.numel() + 2 * dfeat.numel())
    lines.append("backward: R = 256, C = 1024, one 38 x 63 map; bytes = dout read once + dfeat read and written")
    lines.append("%-12s %10s %10s %10s %10s %9s %8s" % ("kernel", "median us", "min us", "max us", "MB", "GB/s", "x crop"))
    for k, (med, lo, hi) in t.items():
        lines.append("%-12s %10.1f %10.1f %10.1f %10.1f %9.0f %8.2f" % (k, med * 1e6, lo * 1e6, hi * 1e6, nbytes / 1e6, nbytes / med / 1e9, med / t["crop"][0]))
    lines.append("")


def end_to_end(dev, args, lines):
    import bench
    from frcnn_hip.runtime import Session
    from nets.resnet_v1 import resnetv1
    c = bench.CONFIGS["c2"]
    old = (cfg.POOLING_MODE, cfg.HIP.ROI_ALIGN_SAMPLES, cfg.TEST.RPN_POST_NMS_TOP_N)
    cfg.TEST.RPN_POST_NMS_TOP_N = c["post"]
    try:
        sess = Session(device=dev, seed=3)
        net = resnetv1(num_layers=101)
        net.create_architecture("TEST", c["classes"], tag="align_bench", anchor_scales=c["scales"], anchor_ratios=bench.ANCHOR_RATIOS)
        sess.init_variables(net.variable_specs())
        net._fuse_tail_entry = True
        im_info = np.array([c["H"], c["W"], bench.IM_SCALE], dtype=np.float32)
        bench.calibrate_rpn(sess, net, net._stage_image(sess, bench.synth_image(c, 0)), im_info)
        batch = net._stage_image(sess, np.concatenate([bench.synth_image(c, s) for s in range(8)], axis=0))

        def run(mode):
            def f():
                cfg.POOLING_MODE = mode
                net.forward_device(sess, batch, im_info)
            return f
        with torch.cuda.stream(sess.stream):
            t = timed({"crop": run("crop"), "align S=2": run("align")}, 3, args.e2e_repeats, 1)
            valid = {}
            for mode in ("crop", "align"):
                cfg.POOLING_MODE = mode
                net.forward_device(sess, batch, im_info)
                sess.stream.synchronize()
                valid[mode] = int(net._num_rois.sum().item())
        lines.append("end to end: ResNet-101, 600 x 1000, 8 images per forward pass (captured graph), fused tail entry on, 300 proposals per image")
        lines.append("(the pooling launches of a pass: 2 x [2400,7,7,C] with C = 2048 and 512 written = %.1f MB)" % (2400 * 49 * 2560 * 4 / 1e6))
        lines.append("%-12s %12s %10s %10s %10s %12s" % ("mode", "median ms", "min ms", "max ms", "images/s", "valid RoIs"))
        for k, (med, lo, hi) in t.items():
            lines.append("%-12s %12.2f %10.2f %10.2f %10.1f %12d" % (k, med * 1e3, lo * 1e3, hi * 1e3, 8 / med, valid["crop" if k == "crop" else "align"]))
        lines.append("")
    finally:
        cfg.POOLING_MODE, cfg.HIP.ROI_ALIGN_SAMPLES, cfg.TEST.RPN_POST_NMS_TOP_N = old


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the report here as well as to stdout")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed interval")
    ap.add_argument("--e2e-repeats", dest="e2e_repeats", type=int, default=15)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("roi_align_bench needs the GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    lines = ["%s; HIP events, %d warm-up, median of %d intervals of %d launches, crop and align alternating in one process"
             % (torch.cuda.get_device_name(0), args.warmup, args.repeats, args.inner), ""]
    forward_rows(dev, args, lines)
    backward_rows(dev, args, lines)
    if not args.no_e2e:
        end_to_end(dev, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
