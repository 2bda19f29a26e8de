#!/usr/bin/env python
"""Measurements behind Soft-NMS (profiles/soft_nms.txt); separate from bench.py.  Needs the MI355X.

  one class         frcnn_soft_nms alone by HIP events on n clustered boxes with min_score = 0 (n dependent steps of ONE wave): median per
                    launch and per step, the step also in cycles of a 2.4 GHz clock -- the figure the kernel's comment estimated
  detect_post       ops.detect_post by HIP events, hard / linear / Gaussian, at (B, R, C) = (8, 300, 21) and (4, 1000, 81) on clustered
                    synthetic inputs with score_thresh = 0: every box of every class is a candidate, the worst case test_net produces
  test_net          model.test.test_net over the 8 seeded 600 x 1000 images of `test_net.py --imdb synthetic_8` (res50, reference
                    initialisers), images/s with cfg.HIP.SOFT_NMS at 0, 1 and 2

Every figure: a warm-up first, then --repeats rounds in which the variants alternate (a drift of the clock hits all of them alike), the
median over the rounds; the detect_post / one-class figures are medians of --launches event-timed launches inside a round."""
import argparse
import contextlib
import io
import time

import numpy as np
import torch

import _init_paths  # noqa: F401
from frcnn_hip import ops
from frcnn_hip.runtime import Session
from model.config import cfg
from model.test import test_net
from test_net import NETS, synthetic_images

NAMES = {0: "hard", 1: "linear", 2: "gaussian"}
CLOCK_GHZ = 2.4


def clustered(rng, n, width=1000.0, height=600.0):
    """n boxes around a few centres with jittered position and size, scores in (0, 1): float32 [n,5]"""
    centres = max(1, min(8, n // 12 + 1))
    cx, cy = rng.uniform(100, width - 100, centres), rng.uniform(100, height - 100, centres)
    bw, bh = rng.uniform(60, 220, centres), rng.uniform(60, 220, centres)
    c = rng.randint(0, centres, n)
    x, y = cx[c] + rng.uniform(-0.25, 0.25, n) * bw[c], cy[c] + rng.uniform(-0.25, 0.25, n) * bh[c]
    w, h = bw[c] * rng.uniform(0.7, 1.3, n), bh[c] * rng.uniform(0.7, 1.3, n)
    d = np.stack([np.maximum(x - w / 2, 0), np.maximum(y - h / 2, 0), np.minimum(x + w / 2, width - 1), np.minimum(y + h / 2, height - 1),
                  rng.uniform(0.002, 0.999, n)], axis=1)
    return np.ascontiguousarray(d, dtype=np.float32)


def event_median(fn, launches):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    ev[0].record()
    for i in range(launches):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(launches)]))


def alternate(variants, repeats, launches, warmup=5):
    """variants: {name: fn} -> {name: (median of the rounds' medians, min, max)} in ms"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    rows = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            rows[k].append(event_median(fn, launches))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in rows.items()}


def one_class(dev, args):
    print("one class (frcnn_soft_nms, min_score 0: n steps of one wave)")
    for n in (64, 128, 300, 512, 1024):
        d = torch.from_numpy(clustered(np.random.RandomState(n), n)).to(dev)
        res = alternate({NAMES[m]: (lambda m=m: ops.soft_nms(d, 0.3, 0, m, 0.5, 0.0)) for m in (1, 2)}, args.repeats, args.launches)
        for k, (ms, lo, hi) in res.items():
            print("  n %4d %-8s median %7.3f ms (rounds %.3f ... %.3f) = %6.0f ns = %5.0f cycles a step"
                  % (n, k, ms, lo, hi, ms * 1e6 / n, ms * 1e6 / n * CLOCK_GHZ))


def detect_post(dev, args):
    for B, R, C in ((8, 300, 21), (4, 1000, 81)):
        rng = np.random.RandomState(R + C)
        rois = np.zeros((B * R, 5), dtype=np.float32)
        for b in range(B):
            rois[b * R:(b + 1) * R, 1:] = clustered(rng, R)[:, :4]
        t = [torch.from_numpy(a).to(dev) for a in (rng.uniform(0, 1, (B * R, C)).astype(np.float32),
                                                   (rng.randn(B * R, 4 * C) * 0.1).astype(np.float32), rois)]
        num = torch.full((B,), R, dtype=torch.int32, device=dev)
        out = torch.empty((B, 128, 6), dtype=torch.float32, device=dev)
        cnt = torch.zeros((B,), dtype=torch.int32, device=dev)

        def run(soft):
            return ops.detect_post(t[0], t[1], t[2], num, 1.0, 600, 1000, 0.3, 0.0, 100, out=out, count=cnt, batch=B, soft=soft)
        res = alternate({NAMES[s]: (lambda s=s: run(s)) for s in (0, 1, 2)}, args.repeats, args.launches)
        print("detect_post (B, R, C) = (%d, %d, %d), score_thresh 0, max_per_image 100" % (B, R, C))
        for k, (ms, lo, hi) in res.items():
            print("  %-8s median %7.3f ms (rounds %.3f ... %.3f)  %+7.3f ms against hard" % (k, ms, lo, hi, ms - res["hard"][0]))


def test_net_rate(dev, args):
    net = NETS["res50"]()
    net.create_architecture("TEST", 21, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess = Session(seed=cfg.RNG_SEED)
    sess.init_variables(net.variable_specs())
    images = list(synthetic_images(8))
    old = cfg.HIP.SOFT_NMS
    rows = {s: [] for s in (0, 1, 2)}
    try:
        for rnd in range(args.repeats + 1):                       # round 0 warms up (graph capture, workspaces)
            for s in (0, 1, 2):
                cfg.HIP.SOFT_NMS = s
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):           # (test_net prints the reference's line per image)
                    all_boxes = test_net(sess, net, iter(images), max_per_image=100)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rnd:
                    rows[s].append(len(images) / dt)
                n_det = sum(len(all_boxes[j][i]) for j in range(1, 21) for i in range(len(images)))
    finally:
        cfg.HIP.SOFT_NMS = old
    print("test_net, res50, 8 synthetic 600 x 1000 images (reference initialisers), max_per_image 100; %d detections in the last pass" % n_det)
    for s, v in rows.items():
        print("  HIP.SOFT_NMS = %d (%-8s) median %6.1f images/s (rounds %.1f ... %.1f)" % (s, NAMES[s], float(np.median(v)), min(v), max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--skip-test-net", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    one_class(dev, args)
    detect_post(dev, args)
    if not args.skip_test_net:
        test_net_rate(dev, args)


if __name__ == "__main__":
    main()
