#!/usr/bin/env python
"""What cfg.HIP.OHEM costs a training step, measured on the device (MI355X); prints a text report and writes it to --out (the table of
profiles/ohem.txt is the report of one such run).

    python tf-faster-rcnn_amd/tools/ohem_bench.py --out report.txt

ResNet-101, one 600 x 1000 image a step, 21 classes, BATCH_SIZE 256, seeded initialisers, the recorded step (cfg.HIP.TRAIN_REPLAY), with
TRAIN.RPN_POST_NMS_TOP_N = 2000 (the training default) and 300, the switch off and on: four sessions, one after the other in one process.
Every time is the median of `--repeats` intervals of `--steps` steps between two device synchronisations, after `--warmup` untimed steps
(the eager step, the recorded one and the first replays); min / max of the intervals are printed next to the median.  The read-only pass
runs over all RPN_POST_NMS_TOP_N rows of the padded proposal buffer whatever number of them is valid, so the seeded weights' proposal
count does not enter the cost."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
for p in (ROOT, PKG, os.path.join(PKG, "lib")):
    if p not in sys.path:
        sys.path.insert(0, p)

from model.config import cfg  # noqa: E402

H, W, CLASSES = 600, 1000, 21
GT = np.array([[60, 80, 420, 500, 3], [500, 120, 930, 560, 7], [300, 300, 640, 590, 12], [20, 400, 180, 580, 15], [700, 30, 990, 200, 9]], dtype=np.float32)


def one(dev, post, ohem, args):
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.resnet_v1 import resnetv1
    cfg.TRAIN.RPN_POST_NMS_TOP_N, cfg.HIP.OHEM = post, ohem
    sess = Session(device=dev, seed=cfg.RNG_SEED)
    net = resnetv1(num_layers=101)
    net.create_architecture("TRAIN", CLASSES, tag="ohem_bench_%d_%d" % (post, int(ohem)))
    sess.init_variables(net.variable_specs())
    rng = np.random.RandomState(1)
    image = ((rng.rand(1, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)) * np.float32(1 / 256.0)
    blobs = dict(data=torch.from_numpy(image).to(dev), im_info=np.array([H, W, 1.6], dtype=np.float32), gt_boxes=torch.from_numpy(GT).to(dev))
    ts = TrainState(sess, net, momentum=cfg.TRAIN.MOMENTUM, weight_decay=cfg.TRAIN.WEIGHT_DECAY)
    ts.lr = 1e-4
    for _ in range(args.warmup):
        net.train_step_async(sess, blobs, ts)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = net.train_step_async(sess, blobs, ts)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / args.steps)
    counts = net._proposal_targets["counts"].cpu().numpy().tolist()
    finite = bool(torch.isfinite(out).all().item())
    stats = dict(net.replay_stats)
    sess.close()
    del sess, net, ts
    torch.cuda.empty_cache()
    return float(np.median(times)), float(np.min(times)), float(np.max(times)), counts, finite, stats


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the report here as well as to stdout")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="steps per timed interval")
    ap.add_argument("--posts", type=int, nargs="+", default=[2000, 300])
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ohem_bench needs the GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    old = (cfg.TRAIN.RPN_POST_NMS_TOP_N, cfg.HIP.OHEM, cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_PICK_STREAMS)
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_PICK_STREAMS = 256, 0.0, 0
    lines = ["%s; ResNet-101 training step, 600 x 1000, 21 classes, BATCH_SIZE 256, recorded step; %d warm-up steps, median of %d intervals of %d steps"
             % (torch.cuda.get_device_name(0), args.warmup, args.repeats, args.steps),
             "%-8s %-6s %10s %10s %10s %10s   %s" % ("post_nms", "OHEM", "median ms", "min ms", "max ms", "x off", "counts {fg sel, bg sel, fg cand, bg cand}; replay")]
    try:
        for post in args.posts:
            base = None
            for ohem in (False, True):
                med, lo, hi, counts, finite, stats = one(dev, post, ohem, args)
                base = med if base is None else base
                lines.append("%-8d %-6s %10.2f %10.2f %10.2f %10.2f   %s; %s%s" % (post, "on" if ohem else "off", med * 1e3, lo * 1e3, hi * 1e3, med / base, counts,
                                                                               stats, "" if finite else "; NON-FINITE LOSS"))
    finally:
        cfg.TRAIN.RPN_POST_NMS_TOP_N, cfg.HIP.OHEM, cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_PICK_STREAMS = old
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
