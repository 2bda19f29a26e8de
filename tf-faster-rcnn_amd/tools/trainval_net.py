#!/usr/bin/env python
"""Train a Faster R-CNN network on the MI355X path -- entry point of the reference's tools/trainval_net.py:29-139
with the same flags (--cfg --weight --imdb --imdbval --iters --tag --net --set).  `--imdb voc_2007_trainval` (or `a+b`) trains
on the roidb of `<cfg.DATA_DIR>/VOCdevkit<year>`, `--imdb coco_2014_train` on that of `<cfg.DATA_DIR>/coco` (81 classes; crowd boxes are no
foreground), through roi_data_layer.layer.RoIDataLayer: flipped twins iff cfg.TRAIN.USE_FLIPPED,
snapshots under get_output_dir(imdb, tag) unless --output names another directory; `--imdb synthetic` (default) feeds seeded synthetic
images + gt boxes and writes snapshots only with --output.  TensorBoard event files (frcnn_hip/summary.py, no TensorFlow) go to
get_output_tb_dir(imdb, tag) for a dataset -- iteration 1, then one summary every cfg.TRAIN.SUMMARY_INTERVAL seconds -- and --imdbval names
the dataset whose minibatches (never flipped, trainval_net.py:113-119) feed the `_val` writer; for `--imdb synthetic`, --tbdir names the
directory and without it no summaries are written.  --net: vgg16, mobile, res50, res101, res152.  Multi-GPU: `python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 tools/trainval_net.py ...` (one
image per rank per step -- rank r of W takes minibatches r, r+W, ... of the one seeded stream -- bucketed RCCL all-reduce of the
gradients)."""
import argparse
import os
import pprint
import sys

import numpy as np
import torch

import _init_paths  # noqa: F401
from frcnn_hip import parallel
from frcnn_hip.runtime import Session
from model.config import box_loss_description, cfg, cfg_from_file, cfg_from_list, get_output_dir, get_output_tb_dir, ohem_description, pooling_description
from model.train_val import filter_roidb, get_training_roidb, synthetic_data_layer, train_net
from test_net import NETS


def parse_args():
    parser = argparse.ArgumentParser(description='Train a Faster R-CNN network')
    parser.add_argument('--cfg', dest='cfg_file', help='optional config file', default=None, type=str)
    parser.add_argument('--weight', dest='weight', help='initialize with pretrained model weights (TF V2 checkpoint prefix, or .npz)', type=str)
    parser.add_argument('--output', dest='output_dir', help='directory for snapshots (default: output/<EXP_DIR>/<imdb>/<tag> for a dataset, none for synthetic)', default=None, type=str)
    parser.add_argument('--imdb', dest='imdb_name', help='dataset to train on: synthetic | voc_<year>_<split> | coco_<year>_<set> [+...]', default='synthetic', type=str)
    parser.add_argument('--imdbval', dest='imdbval_name', help='dataset to validate on', default='synthetic', type=str)
    parser.add_argument('--iters', dest='max_iters', help='number of iterations to train', default=70000, type=int)
    parser.add_argument('--tag', dest='tag', help='tag of the model', default=None, type=str)
    parser.add_argument('--net', dest='net', help='vgg16, mobile, res50, res101, res152', default='res50', type=str)
    parser.add_argument('--tbdir', dest='tb_dir', help='directory for TensorBoard event files (default: tensorboard/<EXP_DIR>/<imdb>/<tag> for a dataset, none for synthetic)', default=None, type=str)
    parser.add_argument('--set', dest='set_cfgs', help='set config keys', default=None, nargs=argparse.REMAINDER)
    if len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    return parser.parse_args()


def combined_roidb(imdb_names, verbose=True):
    """trainval_net.py:63-85 of the reference: the training roidbs of `a+b+...` concatenated; the imdb of a combination carries the
    joined name and the classes of its second member."""
    import datasets.imdb
    from datasets.factory import get_imdb
    say = print if verbose else (lambda *a: None)

    def get_roidb(imdb_name):
        imdb = get_imdb(imdb_name)
        say('Loaded dataset `{:s}` for training'.format(imdb.name))
        imdb.set_proposal_method(cfg.TRAIN.PROPOSAL_METHOD)
        say('Set proposal method: {:s}'.format(cfg.TRAIN.PROPOSAL_METHOD))
        return get_training_roidb(imdb)

    names = imdb_names.split('+')
    roidbs = [get_roidb(s) for s in names]
    roidb = roidbs[0]
    for r in roidbs[1:]:
        roidb.extend(r)
    imdb = datasets.imdb.imdb(imdb_names, get_imdb(names[1]).classes) if len(names) > 1 else get_imdb(imdb_names)
    return imdb, roidb


if __name__ == '__main__':
    args = parse_args()
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    if args.set_cfgs is not None:
        cfg_from_list(args.set_cfgs)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    torch.cuda.set_device(local)
    all_reduce = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        all_reduce = parallel.make_grad_all_reduce()
    if rank == 0:
        print('Called with args:')
        print(args)
        print('Using config:')
        pprint.pprint(cfg)
        print(pooling_description())
        if ohem_description() is not None:
            print(ohem_description())
        if box_loss_description() is not None:
            print(box_loss_description())
    np.random.seed(cfg.RNG_SEED)
    if args.net not in NETS:
        raise NotImplementedError(args.net)
    out_dir = getattr(args, 'output_dir', None)
    tb_dir = getattr(args, 'tb_dir', None)
    imdb, valroidb = None, None
    if args.imdb_name != 'synthetic':
        imdb, roidb = combined_roidb(args.imdb_name)
        print('{:d} roidb entries'.format(len(roidb)))
        if out_dir is None:
            out_dir = get_output_dir(imdb, args.tag)
        print('Output will be saved to `{:s}`'.format(out_dir))
        if tb_dir is None:
            tb_dir = get_output_tb_dir(imdb, args.tag)
        print('TensorFlow summaries will be saved to `{:s}`'.format(tb_dir))
        if args.imdbval_name != 'synthetic' and rank == 0:
            orgflip, cfg.TRAIN.USE_FLIPPED = cfg.TRAIN.USE_FLIPPED, False      # the validation set is never flipped (:113-119)
            try:
                _, valroidb = combined_roidb(args.imdbval_name)
                print('{:d} validation roidb entries'.format(len(valroidb)))
                valroidb = filter_roidb(valroidb)
            except (IOError, OSError, KeyError, AssertionError) as e:
                # a split that is not under cfg.DATA_DIR (launch scripts name voc_2007_test whether or not it was unpacked): the run
                # trains and writes its train summaries; only the `_val` writer is left out, and says so
                print('Validation set `{:s}` is not available ({}): no validation summaries'.format(args.imdbval_name, e))
                valroidb = None
            finally:
                cfg.TRAIN.USE_FLIPPED = orgflip
        roidb = filter_roidb(roidb)
    num_classes = 21 if imdb is None else imdb.num_classes
    sess = Session(seed=cfg.RNG_SEED)                                  # same weights on every rank
    net = NETS[args.net]()
    net.create_architecture("TRAIN", num_classes, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    sess.init_variables(net.variable_specs())
    pretrained = None
    if args.weight and args.weight.endswith('.npz'):
        sess.load_variables(dict(np.load(args.weight)))
    elif args.weight:
        pretrained = args.weight                                        # ImageNet checkpoint: restore + fix_variables
    if imdb is None:
        data = synthetic_data_layer(num_classes, seed=cfg.RNG_SEED + 1000 * rank, image_gain=1.0 / 256.0)
        data_val = None
    else:
        from roi_data_layer.layer import RoIDataLayer
        data = RoIDataLayer(roidb, num_classes, rank=rank, world_size=world)       # the same seeded stream on every rank
        data_val = RoIDataLayer(valroidb, num_classes, random=True) if valroidb else None      # (its own seeded stream: numpy's global one is not drawn from)
    # every rank resumes from the snapshots in out_dir (same weights, Momentum slots, iteration and sampling seed on all replicas);
    # only rank 0 writes new ones
    train_net(net, sess, data, max_iters=args.max_iters, all_reduce=all_reduce, world_size=world, pretrained_model=pretrained,
              output_dir=out_dir, write_snapshots=(rank == 0), tb_dir=tb_dir, data_layer_val=data_val)
