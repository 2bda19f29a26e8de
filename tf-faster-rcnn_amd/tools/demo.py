#!/usr/bin/env python
"""Demo: detections drawn on sample images, on the MI355X path from the file to the file.

Keeps the reference's flags `--net` and `--dataset` and their defaults (the reference's tools/demo.py:102-111) and prints its two lines per
image ("Demo for ...", "Detection took ...s for N object proposals").  What differs: no TensorFlow session and no matplotlib window --
`--model` takes a TensorFlow V2 checkpoint prefix (read without TensorFlow) or an .npz of variables; WITHOUT it the seeded reference
initialisers are used and the tool says so (the boxes then mean nothing, the path is the same) -- and the result is one annotated JPEG
per input under `--out`, all classes on it.

Per image nothing but file bytes crosses to the host and back: frcnn_hip.jpeg.JpegPrefetcher (host Huffman stage, IDCT + colour on the
device) -> Network.detect_device (records [n,6] and their count stay in HBM) -> utils.visualization.draw_detections (one launch, reads the
device-resident count) -> frcnn_hip.jpeg.JpegWriter (colour + DCT on the device, host Huffman stage on worker threads).

Matching the reference's demo (tools/demo.py:89-100, CONF_THRESH 0.8, NMS_THRESH 0.3):
  * it has no cap per image: detect_device runs with max_per_image = 0, its "no limit" form -- the record then has room for all
    R * (num_classes - 1) = 300 * 20 = 6000 candidates, the largest number it can hold;
  * it runs NMS per class and THEN keeps score >= CONF_THRESH; here the threshold comes first (detect_device's `thresh`, the float32 just
    below --conf, so that `score > thresh` is `score >= conf`).  The kept set is the same: greedy NMS visits boxes by descending score and a
    box is only ever suppressed by a higher-scored one, so the boxes below the threshold never decide the fate of one above it.

`--soft-nms linear|gaussian` (with `--sigma`) sets cfg.HIP.SOFT_NMS for the run: a neighbour keeps a decayed score instead of being deleted
(csrc/softnms_math.h).  A box is likewise only ever decayed by a higher-scored one; rows whose DECAYED score falls below --conf stay in the
record and are skipped by the drawing kernel and the JSON, which both test score >= conf.

`--flip` sets cfg.HIP.TEST_FLIP (every image runs together with its mirror, the two views' proposals are merged before the per-class stage;
about twice the forward pass) and `--vote [THRESH]` sets cfg.HIP.BBOX_VOTE / BBOX_VOTE_THRESH (default 0.8): every kept box becomes the
score-weighted mean of the class's candidates whose IoU with it is >= THRESH (csrc/boxvote_math.h).  The candidates are the boxes with
score >= --conf, since the threshold comes first here: a box below it does not vote.
"""
import argparse
import json
import os
import sys

import numpy as np

import _init_paths  # noqa: F401
from model.config import cfg, cfg_from_file, cfg_from_list, pooling_description
from utils.timer import Timer

CLASSES = ('__background__', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
           'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')
NETS = ("vgg16", "res101", "res50", "res152", "mobile")
DATASETS = {'pascal_voc': ('voc_2007_trainval',), 'pascal_voc_0712': ('voc_2007_trainval+voc_2012_trainval',)}
IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp")
MAX_PER_IMAGE = 0                    # detect_device's "no limit": a record of R * (num_classes - 1) rows
SOFT_NMS = {"linear": 1, "gaussian": 2}


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Faster R-CNN demo (MI355X path)")
    ap.add_argument('--net', dest='demo_net', help='Network to use [vgg16 res101]', choices=NETS, default='res101')
    ap.add_argument('--dataset', dest='dataset', help='Trained dataset [pascal_voc pascal_voc_0712]', choices=sorted(DATASETS),
                    default='pascal_voc_0712')
    ap.add_argument('--model', default=None, help='TF V2 checkpoint prefix or .npz of variables; default: the seeded initialisers')
    src = ap.add_mutually_exclusive_group()
    src.add_argument('--images', nargs='+', default=None, help='image files')
    src.add_argument('--dir', dest='image_dir', default=None, help='a directory of images (default: <cfg.DATA_DIR>/demo)')
    ap.add_argument('--out', default='demo_out', help='directory of the annotated JPEGs')
    ap.add_argument('--conf', type=float, default=0.8, help='keep detections with score >= this')
    ap.add_argument('--nms', type=float, default=0.3, help='NMS overlap threshold (cfg.TEST.NMS)')
    ap.add_argument('--soft-nms', dest='soft_nms', choices=sorted(SOFT_NMS), default=None,
                    help='Soft-NMS instead of hard per-class NMS (cfg.HIP.SOFT_NMS): neighbours keep a decayed score')
    ap.add_argument('--sigma', type=float, default=None, help='the Gaussian Soft-NMS width (cfg.HIP.SOFT_NMS_SIGMA)')
    ap.add_argument('--flip', action='store_true', help='horizontal-flip ensemble (cfg.HIP.TEST_FLIP): the image and its mirror in one pass')
    ap.add_argument('--vote', type=float, nargs='?', const=0.8, default=None, metavar='THRESH',
                    help='bounding-box voting (cfg.HIP.BBOX_VOTE) with this IoU threshold in (0, 1] (cfg.HIP.BBOX_VOTE_THRESH, 0.8 if omitted)')
    ap.add_argument('--pooling', choices=('crop', 'align'), default=None,
                    help="RoI pooling (cfg.POOLING_MODE): 'crop' = tf.image.crop_and_resize, 'align' = RoIAlign; must be what the model was trained with")
    ap.add_argument('--quality', type=int, default=90, help='JPEG quality of the output')
    ap.add_argument('--json', dest='json_path', default=None, help='also write the kept detections of every image to this file')
    ap.add_argument('--cfg', dest='cfg_file', default=None, help='optional config file')
    ap.add_argument('--set', dest='set_cfgs', nargs=argparse.REMAINDER, default=None, help='set config keys')
    return ap.parse_args(argv)


def load_network(args):
    from frcnn_hip.runtime import Session
    from nets.mobilenet_v1 import mobilenetv1
    from nets.resnet_v1 import resnetv1
    from nets.vgg16 import vgg16
    make = {"vgg16": vgg16, "mobile": mobilenetv1, "res50": lambda: resnetv1(num_layers=50), "res101": lambda: resnetv1(num_layers=101),
            "res152": lambda: resnetv1(num_layers=152)}
    net = make[args.demo_net]()
    net.create_architecture("TEST", len(CLASSES), tag='default', anchor_scales=[8, 16, 32])
    sess = Session(seed=cfg.RNG_SEED)
    sess.init_variables(net.variable_specs())
    if args.model and args.model.endswith(".npz"):
        sess.load_variables(dict(np.load(args.model)))
        print('Loaded network {:s}'.format(args.model))
    elif args.model:
        sess.restore(args.model)
        print('Loaded network {:s}'.format(args.model))
    else:
        print('No --model: seeded reference initialisers (seed %d) -- the boxes are those of an untrained network, trained on %s would be '
              'the default' % (cfg.RNG_SEED, DATASETS[args.dataset][0]))
    return sess, net


def image_paths(args):
    if args.images:
        return list(args.images)
    d = args.image_dir or os.path.join(cfg.DATA_DIR, 'demo')
    if not os.path.isdir(d):
        raise IOError('{:s} not found: give --images or --dir'.format(d))
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(IMAGE_SUFFIXES)]


def detect_thresh(conf):
    """detect_device keeps score > thresh: the float32 just below conf makes that score >= float32(conf), the rule of the drawing"""
    return float(np.nextafter(np.float32(conf), np.float32(-np.inf)))


def demo(sess, net, paths, out_dir, conf=0.8, quality=90, keep_records=False):
    """Annotated copies of `paths` under out_dir -> [(output path, records or None)]; records (device tensors dets [n,6], count [1], cloned)
    only when keep_records, for --json."""
    import torch
    from frcnn_hip.jpeg import JpegPrefetcher, JpegWriter
    from model.test import _get_image_blob
    from utils.visualization import draw_detections
    os.makedirs(out_dir, exist_ok=True)
    results = []
    writer = JpegWriter(sess.device, workers=4, depth=8)
    try:
        for path, im_d in zip(paths, JpegPrefetcher(paths, sess.device)):
            print('~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~')
            print('Demo for {}'.format(path))
            timer = Timer()
            timer.tic()
            img, im_scale = _get_image_blob(sess, net, im_d)
            im_info = np.array([img.shape[1], img.shape[2], im_scale], dtype=np.float32)
            dets, cnt = net.detect_device(sess, img, im_info, im_d.shape[:2], max_per_image=MAX_PER_IMAGE, thresh=detect_thresh(conf))
            proposals = net._rois_per_image if net._num_rois is None else int(net._num_rois.reshape(-1)[0].item())
            torch.cuda.synchronize()
            timer.toc()
            print('Detection took {:.3f}s for {:d} object proposals'.format(timer.total_time, int(proposals)))
            draw_detections(im_d, dets, cnt, CLASSES, conf=conf)
            out_path = os.path.join(out_dir, os.path.splitext(os.path.basename(path))[0] + '.jpg')
            writer.submit(out_path, im_d, quality=quality)
            results.append((out_path, (dets.clone(), cnt.clone()) if keep_records else None))
    finally:
        writer.close()
    return results


def records_json(paths, results, conf):
    out = []
    for path, (out_path, (dets, cnt)) in zip(paths, results):
        n = min(int(cnt.reshape(-1)[0].item()), dets.shape[0])
        rec = dets[:n].cpu().numpy()
        rec = rec[rec[:, 4] >= np.float32(conf)]
        out.append({"image": path, "output": out_path,
                    "detections": [{"class": CLASSES[int(r[5])], "score": float(r[4]), "bbox": [float(v) for v in r[:4]]} for r in rec]})
    return out


def main(argv=None, network=None):
    """network: a (sess, net) pair of the caller's instead of the one --net / --model describe"""
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if args.cfg_file:
        cfg_from_file(args.cfg_file)
    if args.set_cfgs:
        cfg_from_list(args.set_cfgs)
    saved = (cfg.TEST.HAS_RPN, cfg.TEST.NMS)
    saved_soft = (cfg.HIP.SOFT_NMS, cfg.HIP.SOFT_NMS_SIGMA)
    saved_tta = (cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH)
    saved_pooling = cfg.POOLING_MODE
    if args.pooling is not None:
        cfg.POOLING_MODE = args.pooling
    print(pooling_description())
    cfg.TEST.HAS_RPN, cfg.TEST.NMS = True, float(args.nms)                 # demo.py:114; NMS_THRESH
    if args.soft_nms is not None:
        cfg.HIP.SOFT_NMS = SOFT_NMS[args.soft_nms]
    if args.sigma is not None:
        if not args.sigma > 0:
            raise SystemExit("--sigma must be > 0")
        cfg.HIP.SOFT_NMS_SIGMA = float(args.sigma)
    if args.flip:
        cfg.HIP.TEST_FLIP = True
    if args.vote is not None:
        if not 0.0 < args.vote <= 1.0:
            raise SystemExit("--vote must be in (0, 1]")
        cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH = True, float(args.vote)
    try:
        sess, net = load_network(args) if network is None else network
        paths = image_paths(args)
        results = demo(sess, net, paths, args.out, conf=args.conf, quality=args.quality, keep_records=args.json_path is not None)
        if args.json_path:
            with open(args.json_path, "w") as f:
                json.dump(records_json(paths, results, args.conf), f, indent=1)
        print('%d annotated images in %s' % (len(results), args.out))
    finally:
        cfg.TEST.HAS_RPN, cfg.TEST.NMS = saved
        cfg.HIP.SOFT_NMS, cfg.HIP.SOFT_NMS_SIGMA = saved_soft
        cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH = saved_tta
        cfg.POOLING_MODE = saved_pooling
    return 0


if __name__ == '__main__':
    sys.exit(main())
