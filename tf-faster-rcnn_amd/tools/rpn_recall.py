#!/usr/bin/env python
"""Proposal recall of the RPN over an imdb, on the MI355X path: at 100, 300, 1000 ... proposals per image, what fraction of the ground
truth does the proposal stage cover, per IoU threshold and per object size (the reference's imdb.evaluate_recall, lib/datasets/imdb.py:
126-214, fed by its own RPN).

    python tools/rpn_recall.py --imdb voc_2007_test --net res101 --model <ckpt> --limits 100 300 1000 --areas all small medium large \
        --out <dir> [--save-proposals] [--cfg file] [--set KEY VALUE ...]

The loop is model.test's batched one (same-size images cfg.HIP.TEST_BATCH_IMAGES at a time, the JPEG prefetcher under
cfg.HIP.JPEG_DEVICE, batched preprocessing), with Network.propose_device in place of the whole detector -- no crop, no tail, no per-class
stage -- and frcnn_proposal_recall straight on the batch's `rois` and `num_rois` (stride 5, the batch's im_scale): one launch per limit,
every (area, image) pair a group of it.  TEST.RPN_POST_NMS_TOP_N is set to the largest limit; every limit is matched from the same
rois.  Per batch only the per-gt IoUs, the flags and num_rois go back to the host (one non-blocking copy into pinned memory), and the
proposals too under --save-proposals, which writes proposals.pkl in the reference's candidate_boxes form (a list over images of [n,4]
float32 in image coordinates: imdb.evaluate_recall(candidate_boxes=..., limit=L) reproduces every line printed here).  One line per
(limit, area): AR, recall at IoU 0.5 and 0.7, num_pos; --out also gets recall.json.  WITHOUT --model the seeded reference initialisers
are used and the tool says so (the numbers then mean nothing, the path is the same)."""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

import _init_paths  # noqa: F401  (adds tf-faster-rcnn_amd/ and tf-faster-rcnn_amd/lib to sys.path)
from datasets import recall
from frcnn_hip import ops
from frcnn_hip.runtime import Session
from model.config import cfg, cfg_from_file, cfg_from_list, pooling_description
from test_net import NETS


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Proposal recall of the RPN over an imdb (MI355X path)")
    ap.add_argument("--net", dest="net", default="res50", choices=sorted(NETS), help="vgg16, res50, res101, res152, mobile")
    ap.add_argument("--imdb", dest="imdb_name", default="voc_2007_test", help="a datasets.factory name: voc_<year>_<split>, coco_<year>_<split>")
    ap.add_argument("--model", default=None, help="TF V2 checkpoint prefix or .npz of variables; default: the seeded initialisers")
    ap.add_argument("--cfg", dest="cfg_file", default=None, help="optional config file")
    ap.add_argument("--limits", type=int, nargs="+", default=[100, 300, 1000], help="proposals per image that count")
    ap.add_argument("--areas", nargs="+", default=["all", "small", "medium", "large"], choices=sorted(recall.AREAS, key=recall.AREAS.get))
    ap.add_argument("--out", default=None, help="directory for recall.json (and proposals.pkl)")
    ap.add_argument("--save-proposals", dest="save_proposals", action="store_true", help="write proposals.pkl (needs --out)")
    ap.add_argument("--tag", default="", help="tag of the model")
    ap.add_argument("--set", dest="set_cfgs", nargs=argparse.REMAINDER, default=None, help="set config keys")
    args = ap.parse_args(argv)
    if min(args.limits) <= 0:
        ap.error("--limits must be positive")
    if args.save_proposals and not args.out:
        ap.error("--save-proposals needs --out")
    return args


def load_network(args, num_classes):
    net = NETS[args.net]()
    net.create_architecture("TEST", num_classes, tag=args.tag or "default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess = Session(seed=cfg.RNG_SEED)
    sess.init_variables(net.variable_specs())
    if args.model and args.model.endswith(".npz"):
        sess.load_variables(dict(np.load(args.model)))
        print("Loaded network {:s}".format(args.model))
    elif args.model:
        sess.restore(args.model)
        print("Loaded network {:s}".format(args.model))
    else:
        print("No --model: seeded reference initialisers (seed %d) -- the recall is that of an untrained RPN" % cfg.RNG_SEED)
    return sess, net


class _Pending(object):
    """one enqueued batch: its pinned record, the event behind the copy that fills it, and where everything sits in it"""
    __slots__ = ("host", "ev", "B", "n_valid", "post", "n_gt", "gt_off", "scale", "save")


class RecallLoop(object):
    """The per-batch halves run_paths_batched calls.  gt[a][i]: float64 [g,4], the ground truth of image i that counts for area a."""

    def __init__(self, sess, net, gt, limits, save):
        self.sess, self.net, self.gt, self.limits, self.save = sess, net, gt, list(limits), bool(save)
        self._const = {}

    def _constants(self, B, post, scale):
        """start row and scale of every (area, slot) group of a launch: the same for every batch of one shape"""
        key = (B, post, float(scale))
        if key not in self._const:
            A, dev = len(self.gt), self.sess.device
            self._const[key] = ((torch.arange(B, dtype=torch.int64, device=dev) * post).repeat(A).contiguous(),
                                torch.full((A * B,), float(scale), dtype=torch.float32, device=dev))
        return self._const[key]

    def enqueue(self, stage, idx, n_valid, ring):
        sess, net = self.sess, self.net
        B, h, w = int(stage.shape[0]), int(stage.shape[1]), int(stage.shape[2])
        im_scale, OH, OW = ops.prep_image_shape(h, w, cfg.TEST.SCALES[0], cfg.TEST.MAX_SIZE)
        with net.shape_scope(sess, (B, OH, OW, 4), (OH, OW)):
            img = sess.buf(net._tag + "/image", (B, OH, OW, 4))
        ops.prep_image_batched(stage, cfg.PIXEL_MEANS, im_scale, (OH, OW), out=img, out_c=4)
        rois, _, num = net.propose_device(sess, img, np.array([OH, OW, im_scale], dtype=np.float32))
        post, A, L = rois.shape[0] // B, len(self.gt), len(self.limits)
        # groups: area-major, the batch's slots inside an area; padded slots have no ground truth, so nothing is matched for them
        empty = np.zeros((0, 4))
        groups = [self.gt[a][idx[b]] if b < n_valid else empty for a in range(A) for b in range(B)]
        gt_off = np.concatenate([[0], np.cumsum([g.shape[0] for g in groups])]).astype(np.int64)
        n_gt = int(gt_off[-1])
        gt_d = torch.from_numpy(np.concatenate(groups)).to(sess.device, non_blocking=True)
        gt_off_d = torch.from_numpy(gt_off).to(sess.device, non_blocking=True)
        start_d, scale_d = self._constants(B, post, im_scale)
        count_d = num.repeat(A)
        # the record of THIS batch: L x n_gt IoUs (float64), then L x A*B flags and B counts (int32), then the proposals (float32)
        nbytes = 8 * L * n_gt + 4 * (L * A * B + B) + (4 * rois.numel() if self.save else 0)
        rec = torch.zeros((nbytes,), dtype=torch.uint8, device=sess.device)
        iou = rec[:8 * L * n_gt].view(torch.float64).view(L, n_gt)
        ints = rec[8 * L * n_gt:8 * L * n_gt + 4 * (L * A * B + B)].view(torch.int32)
        for k, limit in enumerate(self.limits):
            ops.proposal_recall(rois, start_d, count_d, scale_d, gt_d, gt_off_d, post, limit, out=iou[k], ran_out=ints[k * A * B:(k + 1) * A * B])
        ints[L * A * B:].copy_(num)
        if self.save:
            rec[8 * L * n_gt + 4 * (L * A * B + B):].view(torch.float32).copy_(rois.view(-1))
        p = _Pending()
        p.host, k = ring.take(nbytes)
        p.host.copy_(rec, non_blocking=True)
        p.ev = ring.mark(k)
        p.B, p.n_valid, p.post, p.n_gt, p.gt_off, p.scale, p.save = B, int(n_valid), post, n_gt, gt_off, np.float32(im_scale), self.save
        return p

    def finish(self, p):
        """-> per valid image: (picks[limit][area] float64 (empty when the image has no proposals), ran_out[limit][area], proposals | None)"""
        p.ev.synchronize()
        A, L, B = len(self.gt), len(self.limits), p.B
        a = p.host.numpy()
        iou = a[:8 * L * p.n_gt].view(np.float64).reshape(L, p.n_gt)
        ints = a[8 * L * p.n_gt:8 * L * p.n_gt + 4 * (L * A * B + B)].view(np.int32)
        flags, num = ints[:L * A * B].reshape(L, A, B), ints[L * A * B:]
        rois = a[8 * L * p.n_gt + 4 * (L * A * B + B):].view(np.float32).reshape(B * p.post, 5) if p.save else None
        out = []
        for b in range(p.n_valid):
            n = min(int(num[b]), p.post)
            picks = [[iou[k, p.gt_off[g * B + b]:p.gt_off[g * B + b + 1]].copy() if n > 0 else np.zeros(0) for g in range(A)] for k in range(L)]
            boxes = (rois[b * p.post:b * p.post + n, 1:5] / p.scale).astype(np.float32) if p.save else None
            out.append((picks, flags[:, :, b].copy(), boxes))
        return out


def rpn_recall(sess, net, imdb, limits, areas, save=False):
    """-> (results: list of dict(limit, area, ar, recalls, thresholds, num_pos), proposals: list over images of [n,4] float32 or None,
    seconds of the loop)"""
    from model.test import run_paths_batched
    roidb = [imdb.roidb[i] for i in range(imdb.num_images)]
    gt = [[np.asarray(e["boxes"])[recall.select_gt(e, area)].astype(np.float64).reshape(-1, 4) for e in roidb] for area in areas]
    loop = RecallLoop(sess, net, gt, limits, save)
    saved = cfg.TEST.RPN_POST_NMS_TOP_N
    cfg.TEST.RPN_POST_NMS_TOP_N = int(max(limits))
    try:
        t0 = [time.time()]
        per_image = run_paths_batched(sess, [imdb.image_path_at(i) for i in range(imdb.num_images)], int(cfg.HIP.TEST_BATCH_IMAGES),
                                      loop.enqueue, loop.finish, on_start=lambda: t0.__setitem__(0, time.time()))
        seconds = time.time() - t0[0]
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N = saved
    results = []
    for k, limit in enumerate(limits):
        for g, area in enumerate(areas):
            short = [i for i, (_, flags, _) in enumerate(per_image) if flags[k][g]]
            assert not short, "gt_ovr >= 0: image(s) %s have fewer than their ground-truth boxes' number of proposals at limit %d" % (short, limit)
            res = recall.summarise(np.concatenate([picks[k][g] for picks, _, _ in per_image] + [np.zeros(0)]), sum(x.shape[0] for x in gt[g]))
            results.append(dict(limit=int(limit), area=area, ar=float(res["ar"]), recalls=res["recalls"].tolist(),
                                thresholds=res["thresholds"].tolist(), num_pos=int(sum(x.shape[0] for x in gt[g]))))
    return results, ([b for _, _, b in per_image] if save else None), seconds


def main(argv=None, network=None):
    """network: a (sess, net) pair of the caller's instead of the one --net / --model describe"""
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if args.cfg_file:
        cfg_from_file(args.cfg_file)
    if args.set_cfgs:
        cfg_from_list(args.set_cfgs)
    print(pooling_description() + " (the RPN-only pass does not pool; the key only has to be a supported one)")
    from datasets.factory import get_imdb
    imdb = get_imdb(args.imdb_name)
    sess, net = load_network(args, imdb.num_classes) if network is None else network
    results, proposals, seconds = rpn_recall(sess, net, imdb, args.limits, args.areas, args.save_proposals)
    for r in results:
        t = np.asarray(r["thresholds"])
        print("limit {:d} area {:s}: AR {:.4f} recall@0.5 {:.4f} recall@0.7 {:.4f} num_pos {:d}".format(
            r["limit"], r["area"], r["ar"], r["recalls"][int(np.argmin(np.abs(t - 0.5)))], r["recalls"][int(np.argmin(np.abs(t - 0.7)))], r["num_pos"]))
    print("{:d} images in {:.3f}s ({:.1f} images/s), batches of {:d}".format(imdb.num_images, seconds, imdb.num_images / max(seconds, 1e-9),
                                                                           int(cfg.HIP.TEST_BATCH_IMAGES)))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "recall.json"), "w") as f:
            json.dump(dict(imdb=imdb.name, images=imdb.num_images, results=results), f, indent=1)
        if proposals is not None:
            with open(os.path.join(args.out, "proposals.pkl"), "wb") as f:
                pickle.dump(proposals, f, pickle.HIGHEST_PROTOCOL)
    return 0


if __name__ == "__main__":
    sys.exit(main())
