#!/usr/bin/env python
"""Measurements behind the TensorBoard summaries (profiles/tb_summary.txt); separate from bench.py.  Needs the MI355X.

ResNet-101 TRAIN graph on seeded synthetic 600 x 1000 minibatches (model.train_val.synthetic_data_layer), cfg defaults.  After a warm-up long
enough for the recording and the stream search of the replayed step, in ONE process:

  plain step        ms per replayed Network.train_step_async, a window of --steps steps between two device synchronisations
  summary step      ms per Network.train_step_with_summary (the same replayed step + statistics kernel + read-back + host encoding + PNG)
  validation step   ms per Network.get_summary (eager TRAIN-mode forward + losses + PNG)
  kernel            frcnn_summary_stats alone by HIP events: over the trainable variables, and over the whole list of a summary step;
                    bytes = 4 * elements read, once
The three step figures are host clocks around work that ends in a synchronise; windows alternate --repeats times."""
import argparse
import time

import numpy as np
import torch

import _init_paths  # noqa: F401
from frcnn_hip import ops
from frcnn_hip.runtime import Session
from model.config import cfg
from model.train_val import SolverWrapper, synthetic_data_layer
from test_net import NETS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="res101")
    ap.add_argument("--warmup", type=int, default=150)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    sess = Session(seed=cfg.RNG_SEED)
    net = NETS[args.net]()
    net.create_architecture("TRAIN", 21, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess.init_variables(net.variable_specs())
    data = synthetic_data_layer(21, seed=cfg.RNG_SEED, image_gain=1.0 / 256.0)
    val = synthetic_data_layer(21, seed=cfg.RNG_SEED + 77, image_gain=1.0 / 256.0)
    sw = SolverWrapper(sess, net, data)
    sw.state.lr = cfg.TRAIN.LEARNING_RATE
    blobs = [next(data) for _ in range(4)]
    vblobs = [next(val) for _ in range(2)]
    for i in range(args.warmup):
        net.train_step_async(sess, blobs[i % 4], sw.state)
    net.train_step_with_summary(sess, blobs[0], sw.state)
    net.get_summary(sess, vblobs[0], sw.state)
    torch.cuda.synchronize()
    print("%s, image %s, replay_stats after warm-up %s, stream search done: %s" % (args.net, tuple(net._image.shape), net.replay_stats,
                                                                                  sess.picked_streams is not None or not sess.picking))

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    rows = {"plain": [], "summary": [], "validation": []}
    for _ in range(args.repeats):
        rows["plain"].append(window(lambda i: net.train_step_async(sess, blobs[i % 4], sw.state), args.steps))
        rows["summary"].append(window(lambda i: net.train_step_with_summary(sess, blobs[i % 4], sw.state), 4))
        rows["validation"].append(window(lambda i: net.get_summary(sess, vblobs[i % 2], sw.state), 4))
    for k, v in rows.items():
        print("%-16s ms per step: %s   (median %.2f)" % (k, "  ".join("%.2f" % x for x in v), float(np.median(v))))
    print("replay_stats at the end %s" % (net.replay_stats,))

    net.train_step_async(sess, blobs[0], sw.state)
    items = net._summary_tensors(sw.state)
    groups = (("trainable variables", [t for _, kind, t in items if kind == "train"]),
              ("whole summary list", [t if t.is_contiguous() else t.contiguous() for _, _, t in items]))
    for name, ts in groups:
        plan = ops.SummaryPlan(ts)
        for _ in range(3):
            plan.launch()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
        ev[0].record()
        for i in range(20):
            plan.launch()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(20))
        nbytes = 4 * sum(t.numel() for t in ts)
        print("frcnn_summary_stats, %-20s %4d tensors, %7.1f MB read, record read-back %5.2f MB: median %.3f ms (min %.3f, max %.3f) = %.0f GB/s"
              % (name + ":", len(ts), nbytes / 1e6, plan.out.numel() * 8 / 1e6, ms[10], ms[0], ms[-1], nbytes / (ms[10] * 1e-3) / 1e9))


if __name__ == "__main__":
    main()
