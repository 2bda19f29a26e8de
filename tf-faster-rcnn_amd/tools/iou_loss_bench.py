#!/usr/bin/env python
"""What the IoU-family box regression losses (cfg.HIP.BBOX_LOSS / RPN_BBOX_LOSS) cost, measured on the device (MI355X); prints a text
report and writes it to --out (profiles/iou_loss.txt is the report of one such run).

    python tf-faster-rcnn_amd/tools/iou_loss_bench.py --out report.txt

1. The loss launches alone, between two HIP events around `--calls` back-to-back calls after `--calls` untimed ones, the median of
   `--repeats` such intervals: ops.smooth_l1_loss (k_smooth_l1 + k_sum_finish) and ops.iou_loss of each kind (k_iou_loss + k_iou_finish) at
   the head shapes 256 rows x 21 / 81 classes (64 foreground rows with one active slice each) and the RPN shapes 38 x 63 x 9 and
   50 x 84 x 15 anchors (128 active).
2. The training step of bench.py's configs[4] -- ResNet-152, one 600 x 1000 image, 81 classes, anchor scales 4 8 16 32, BATCH_SIZE 256,
   the recorded step -- with the default keys and with BBOX_LOSS = RPN_BBOX_LOSS = 'giou': two sessions in one process, timed in
   ALTERNATING intervals of `--steps` steps between two device synchronisations (default, giou, default, giou, ...), so that clock and
   neighbours on the machine touch both alike; median, min and max of each side's `--repeats` intervals.  The default side's min .. max is
   the run-to-run spread a difference has to be read against.  Once at learning rate 1e-4 -- the two sides' weights part ways, so proposals,
   RoIs and every data-dependent launch differ with them -- and once at learning rate 0, where both sides keep the seeded weights and do
   the same work except for the loss launches and the gradients they seed."""
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

H, W, CLASSES, SCALES = 600, 1000, 81, (4, 8, 16, 32)
GT = np.array([[60, 80, 420, 500, 3], [500, 120, 930, 560, 7], [300, 300, 640, 590, 12], [20, 400, 180, 580, 15], [700, 30, 990, 200, 9]], dtype=np.float32)
SHAPES = (("head 256 x 21", 256, 21, 64), ("head 256 x 81", 256, 81, 64), ("rpn 38 x 63 x 9", 38 * 63 * 9, 1, 128), ("rpn 50 x 84 x 15", 50 * 84 * 15, 1, 128))
KEYS = ("BBOX_LOSS", "RPN_BBOX_LOSS")


def loss_inputs(dev, N, K, active, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 800, N)
    y = rng.uniform(0, 500, N)
    box = np.stack([x, y, x + rng.uniform(16, 300, N), y + rng.uniform(16, 300, N)], axis=1).astype(np.float32)
    refs = box if K == 1 else np.concatenate([np.zeros((N, 1), np.float32), box], axis=1)
    pred = (rng.randn(N, 4 * K) * 0.3).astype(np.float32)
    tg, iw, ow = (np.zeros((N, 4 * K), np.float32) for _ in range(3))
    for r in rng.choice(N, active, replace=False):
        k = 0 if K == 1 else rng.randint(1, K)
        tg[r, 4 * k:4 * k + 4] = rng.randn(4) * 0.3
        iw[r, 4 * k:4 * k + 4], ow[r, 4 * k:4 * k + 4] = 1.0, 1.0 / active
    return [torch.from_numpy(a).to(dev) for a in (pred, tg, iw, ow, refs)]


def time_calls(fn, args):
    for _ in range(args.calls):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / args.calls)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def launches(dev, args):
    from frcnn_hip import ops
    lines = ["%-18s %-10s %10s %8s %8s   (us a call = two launches; median, min, max of %d intervals of %d calls)"
             % ("shape", "loss", "median us", "min", "max", args.repeats, args.calls)]
    for name, N, K, active in SHAPES:
        pred, tg, iw, ow, refs = loss_inputs(dev, N, K, active)
        stds = (1.0, 1.0, 1.0, 1.0) if K == 1 else (0.1, 0.1, 0.2, 0.2)
        div = 1.0 if K == 1 else float(N)
        runs = [("smooth_l1", lambda: ops.smooth_l1_loss(pred, tg, iw, ow, 3.0 if K == 1 else 1.0, div))]
        for kind in ("iou", "giou", "diou", "ciou"):
            runs.append((kind, lambda kind=kind: ops.iou_loss(pred, tg, iw, ow, refs, (0.0, 0.0, 0.0, 0.0), stds, kind, 1.0, div, K)))
        for label, fn in runs:
            lines.append("%-18s %-10s %10.2f %8.2f %8.2f" % ((name, label) + time_calls(fn, args)))
    return lines


def make_step(dev, tag, lr):
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.resnet_v1 import resnetv1
    sess = Session(device=dev, seed=cfg.RNG_SEED)
    net = resnetv1(num_layers=152)
    net.create_architecture("TRAIN", CLASSES, tag=tag, anchor_scales=SCALES)
    sess.init_variables(net.variable_specs())
    rng = np.random.RandomState(1)
    image = ((rng.rand(1, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)) * np.float32(1 / 256.0)
    blobs = dict(data=torch.from_numpy(image).to(dev), im_info=np.array([H, W, 1.6], dtype=np.float32), gt_boxes=torch.from_numpy(GT).to(dev))
    ts = TrainState(sess, net, momentum=cfg.TRAIN.MOMENTUM, weight_decay=cfg.TRAIN.WEIGHT_DECAY)
    ts.lr = lr
    return sess, net, ts, blobs


def steps(dev, args, lr):
    sides = [("default", "smooth_l1"), ("giou", "giou")]
    made = {}

    def run(label, loss, n):
        for k in KEYS:
            cfg.HIP[k] = loss                                # read by every step: it is part of the recorded-step key
        sess, net, ts, blobs = made[label]
        out = None
        for _ in range(n):
            out = net.train_step_async(sess, blobs, ts)
        torch.cuda.synchronize()
        return out
    for label, loss in sides:
        for k in KEYS:
            cfg.HIP[k] = loss
        made[label] = make_step(dev, "iou_loss_bench_%s_%g" % (label, lr), lr)
        run(label, loss, args.warmup)
    times = {label: [] for label, _ in sides}
    last = {}
    for _ in range(args.repeats):
        for label, loss in sides:
            t0 = time.perf_counter()
            last[label] = run(label, loss, args.steps)
            times[label].append((time.perf_counter() - t0) / args.steps)
    lines = ["ResNet-152 training step, 600 x 1000, 81 classes, A = 12, BATCH_SIZE 256, recorded step, learning rate %g; %d warm-up steps a side, "
             "then %d alternating intervals of %d steps a side" % (lr, args.warmup, args.repeats, args.steps),
             "%-10s %10s %10s %10s %10s   %s" % ("losses", "median ms", "min ms", "max ms", "x default", "last step's five losses; replay")]
    base = float(np.median(times["default"]))
    for label, _ in sides:
        t = times[label]
        lines.append("%-10s %10.2f %10.2f %10.2f %10.3f   %s; %s" % (label, np.median(t) * 1e3, np.min(t) * 1e3, np.max(t) * 1e3, np.median(t) / base,
                                                                  ["%.4f" % v for v in last[label].cpu().tolist()], dict(made[label][1].replay_stats)))
    for label, _ in sides:
        made[label][0].close()
    made.clear()
    torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the report here as well as to stdout")
    ap.add_argument("--calls", type=int, default=200, help="loss calls per timed interval")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed interval")
    ap.add_argument("--lrs", type=float, nargs="+", default=[1e-4, 0.0], help="learning rates of the step comparison, one table each")
    ap.add_argument("--no-step", action="store_true", help="only the loss launches")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("iou_loss_bench needs the GPU: a time taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    old = (cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_PICK_STREAMS, cfg.HIP.BBOX_LOSS, cfg.HIP.RPN_BBOX_LOSS)
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_PICK_STREAMS = 256, 0.0, 0
    lines = [torch.cuda.get_device_name(0)]
    try:
        lines += launches(dev, args)
        if not args.no_step:
            for lr in args.lrs:
                lines += [""] + steps(dev, args, lr)
    finally:
        cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_PICK_STREAMS, cfg.HIP.BBOX_LOSS, cfg.HIP.RPN_BBOX_LOSS = old
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
