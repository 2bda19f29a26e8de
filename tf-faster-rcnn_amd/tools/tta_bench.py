#!/usr/bin/env python
"""Measurements behind the test-time flip ensemble and box voting (profiles/tta.txt); separate from bench.py.  Needs the MI355X.

  one class         frcnn_box_vote alone by HIP events: n clustered candidates, kept = the rows hard NMS keeps (a few) and kept = all n
                    (what Soft-NMS at min_score 0 hands over: every thread of the kernel busy)
  detect_post       ops.detect_post by HIP events with vote off / on (0.8) for hard / linear / Gaussian, at (B, R, C) = (8, 300, 21) and
                    (4, 1000, 81) on clustered synthetic inputs with score_thresh = 0: every box of every class is a candidate
  end to end        Network.detect_device on staged 600 x 1000 images (ResNet-101, reference initialisers, 300 proposals), images/s with
                    cfg.HIP.TEST_FLIP and cfg.HIP.BBOX_VOTE each off and on, for 1 and for --batch images a call

Every figure: a warm-up first, then --repeats rounds in which the settings alternate (a drift of the clock hits all of them alike), the
median over the rounds with the rounds' min ... max; the event-timed figures are medians of --launches launches inside a round.  The
base of every comparison is the same build with the switches off, which makes exactly the calls it made before they existed."""
import argparse
import time

import numpy as np
import torch

import _init_paths  # noqa: F401
from frcnn_hip import ops
from frcnn_hip.runtime import Session
from model.config import cfg
from soft_nms_bench import NAMES, alternate, clustered
from test_net import NETS

VOTE = 0.8


def hard_keep(d, thresh=0.3):
    """rows greedy NMS keeps (numpy, float32 IoU with +1 widths), for the one-class timing's short kept list"""
    order = np.argsort(-d[:, 4], kind="stable")
    area = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)
    alive, keep = np.ones(len(d), dtype=bool), []
    for i in order:
        if not alive[i]:
            continue
        keep.append(i)
        w = np.maximum(0, np.minimum(d[i, 2], d[:, 2]) - np.maximum(d[i, 0], d[:, 0]) + 1)
        h = np.maximum(0, np.minimum(d[i, 3], d[:, 3]) - np.maximum(d[i, 1], d[:, 1]) + 1)
        alive &= ~(w * h / (area[i] + area - w * h) >= thresh)
    return np.array(keep)


def one_class(dev, args):
    print("one class (frcnn_box_vote at %.1f; kept = the rows hard NMS keeps | kept = all n)" % VOTE)
    for n in (64, 300, 1024):
        d = clustered(np.random.RandomState(n), n)
        cands, few = torch.from_numpy(d).to(dev), torch.from_numpy(np.ascontiguousarray(d[hard_keep(d)])).to(dev)
        res = alternate({"few": lambda: ops.box_vote(few, cands, VOTE), "all": lambda: ops.box_vote(cands, cands, VOTE)}, args.repeats,
                        args.launches)
        print("  n %4d  m %3d: median %6.3f ms (rounds %.3f ... %.3f)   m %4d: median %6.3f ms (rounds %.3f ... %.3f)"
              % ((n, few.shape[0]) + res["few"] + (n,) + res["all"]))


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

        def run(soft, vote):
            return ops.detect_post(t[0], t[1], t[2], num, 1.0, 600, 1000, 0.3, 0.0, 100, out=out, count=cnt, batch=B, soft=soft, vote=vote)
        res = alternate({(s, v): (lambda s=s, v=v: run(s, v)) for s in (0, 1, 2) for v in (0.0, VOTE)}, args.repeats, args.launches)
        print("detect_post (B, R, C) = (%d, %d, %d), score_thresh 0, max_per_image 100, vote_thresh %.1f" % (B, R, C, VOTE))
        for s in (0, 1, 2):
            off, on = res[(s, 0.0)], res[(s, VOTE)]
            print("  %-8s vote off median %6.3f ms (rounds %.3f ... %.3f)   on median %6.3f ms (rounds %.3f ... %.3f)   %+6.3f ms"
                  % ((NAMES[s],) + off + on + (on[0] - off[0],)))


def end_to_end(dev, args):
    net = NETS["res101"]()
    net.create_architecture("TEST", 21, tag="default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess = Session(seed=cfg.RNG_SEED)
    sess.init_variables(net.variable_specs())
    H, W, scale = 600, 1000, 1.6
    im_info, orig = np.array([H, W, scale], dtype=np.float32), (int(H / scale), int(W / scale))
    settings = [(False, False), (False, True), (True, False), (True, True)]
    old = (cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH)
    cfg.HIP.BBOX_VOTE_THRESH = VOTE
    try:
        for B in (1, args.batch):
            rng = np.random.RandomState(cfg.RNG_SEED)
            image = (rng.rand(B, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)
            img = net._stage_image(sess, image, im_info)
            rows, dets = {s: [] for s in settings}, {}
            for rnd in range(args.repeats + 1):                   # round 0 warms up (graph capture, workspaces)
                for s in settings:
                    cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE = s
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        _, cnt = net.detect_device(sess, img, im_info, orig)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if rnd:
                        rows[s].append(B * args.steps / dt)
                    dets[s] = int(cnt.sum().item())
            base = float(np.median(rows[settings[0]]))
            print("end to end: res101, %d x 600 x 1000 a call (reference initialisers, 300 proposals, max_per_image 100), %d calls a round" % (B, args.steps))
            for s in settings:
                m = float(np.median(rows[s]))
                print("  TEST_FLIP %-5s BBOX_VOTE %-5s median %6.1f images/s (rounds %.1f ... %.1f)  %6.3f ms an image, x %.3f of the base; "
                      "%d detections" % (s[0], s[1], m, min(rows[s]), max(rows[s]), 1e3 / m, base / m, dets[s]))
    finally:
        cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH = old
        sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20, help="detect_device calls per timed round of the end-to-end figure")
    ap.add_argument("--batch", type=int, default=8, help="images per call of the batched end-to-end figure")
    ap.add_argument("--skip-end-to-end", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    one_class(dev, args)
    detect_post(dev, args)
    if not args.skip_end_to_end:
        end_to_end(dev, args)


if __name__ == "__main__":
    main()
