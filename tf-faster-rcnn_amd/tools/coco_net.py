#!/usr/bin/env python
"""Test a Faster R-CNN network on a COCO set: `coco_net.py --net res101 --imdb coco_2014_minival --model <ckpt>`.

The command line is tools/test_net.py's (its parser and network table are imported, so --cfg --model --imdb --comp --num_dets --tag --net
--set mean the same); what differs is the dataset: `--imdb coco_<year>_<set>` builds datasets.coco from `<cfg.DATA_DIR>/coco`, the network
gets that imdb's 81 classes, every image goes through the raw-image device path (model.test.test_net_imdb), `detections.pkl` and the COCO
results json are written under output/<net>/<imdb>/<tag>, and -- for sets with annotations -- the bbox evaluation runs (datasets.coco_eval:
IoU and matching on the device), printing the per-category AP and the 12 summary lines and writing `detection_results.pkl`.  --comp keeps
the unsalted results json (what an evaluation server takes for the test sets).  tools/test_net.py itself stays as it is: its dataset switch
and its class count of 21 are fixed, and it is kept byte for byte."""
import os
import pprint
import sys

import numpy as np

import _init_paths  # noqa: F401
import test_net as base
from frcnn_hip.runtime import Session
from model.config import cfg, cfg_from_file, cfg_from_list, pooling_description
from model.test import test_net_imdb


def main(argv):
    ap = base.build_parser()
    ap.description = "Test a Faster R-CNN network on a COCO set (MI355X path)"
    ap.set_defaults(imdb_name="coco_2014_minival")
    if not argv:
        ap.print_help()
        return 1
    args = ap.parse_args(argv)
    if args.cfg_file:
        cfg_from_file(args.cfg_file)
    if args.set_cfgs:
        cfg_from_list(args.set_cfgs)
    print("Called with args:\n%s\nUsing config:" % (args,))
    pprint.pprint(cfg)
    print(pooling_description())
    if not args.imdb_name.startswith("coco_"):
        raise SystemExit("--imdb coco_<year>_<set> (tools/test_net.py takes synthetic_N and voc_<year>_<split>)")
    if args.net not in base.NETS:
        raise NotImplementedError(args.net)
    from datasets.factory import get_imdb
    imdb = get_imdb(args.imdb_name)
    imdb.competition_mode(args.comp_mode)
    net = base.NETS[args.net]()
    net.create_architecture("TEST", imdb.num_classes, tag=args.tag or "default", anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess = Session(seed=cfg.RNG_SEED)
    sess.init_variables(net.variable_specs())
    if args.model and args.model.endswith(".npz"):
        print("Loading variables from %s" % args.model)
        sess.load_variables(dict(np.load(args.model)))
    elif args.model:
        print("Loading model check point from {:s}".format(args.model))
        sess.restore(args.model)
        print("Loaded.")
    else:
        print("No --model: reference initialisers, seed %d" % cfg.RNG_SEED)
    out_dir = os.path.join(cfg.ROOT_DIR, "output", args.net, imdb.name, args.tag or "default")
    test_net_imdb(sess, net, imdb, out_dir, max_per_image=args.max_per_image)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
