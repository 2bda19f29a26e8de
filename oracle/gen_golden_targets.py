#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/targets_edges.npz: the REFERENCE's own anchor_target_layer / proposal_target_layer
(imported through oracle/ref_shim.py, like oracle/gen_golden.py) run on the cases of oracle/target_cases.py that it can run, with its cfg
set to each case's thresholds, batch sizes and modes and its `npr.choice` draws recorded.  Data only: the draws and the outputs; the inputs
are regenerated from oracle/target_cases.py.  Pins oracle/frcnn_oracle.py (the same numpy stream) and oracle/target_ref.py (the recorded
draws injected) against the reference on every case, bit for bit.  Runs only where the reference tree is present.

    python oracle/gen_golden_targets.py            # regenerate the fixture + pin report
    python oracle/gen_golden_targets.py --check    # pin only (no file written); exit 1 on mismatch
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402
from gen_golden import FAIL, GOLD, pin  # noqa: E402

f32 = np.float32
SEED = 7
AT_KEYS = ("labels", "targets", "inside", "outside")
PT_KEYS = ("rois", "scores", "labels", "targets", "inside", "outside")


def main(write=True):
    ref = ref_shim.load_reference()
    import frcnn_oracle as ora  # after the reference: module names do not collide
    import target_cases as tc
    import target_ref as tr
    t = ref.cfg.TRAIN
    out = {}
    draws = []
    real_choice = np.random.choice

    def recording_choice(a, size=None, replace=True, p=None):
        r = real_choice(a, size=size, replace=replace, p=p)
        draws.append(np.array(r))
        return r
    np.random.choice = recording_choice
    try:
        for c in tc.anchor_cases():
            if not c.golden:
                continue
            A = c.base.shape[0]
            anc = tr.anchor_f32(c.base, c.H, c.W, c.stride)
            score = np.zeros((1, c.H, c.W, 2 * A), dtype=f32)
            info = np.array([c.im_h, c.im_w, 1.0], dtype=f32)
            (t.RPN_BATCHSIZE, t.RPN_FG_FRACTION, t.RPN_POSITIVE_OVERLAP, t.RPN_NEGATIVE_OVERLAP, t.RPN_CLOBBER_POSITIVES, t.RPN_POSITIVE_WEIGHT,
             t.RPN_BBOX_INSIDE_WEIGHTS) = c.batch, c.fg_fraction, c.pos_ov, c.neg_ov, c.clobber, c.pos_weight, c.inside_w
            del draws[:]
            np.random.seed(SEED)
            at = ref.anchor_target_layer(score, c.gt, info, [c.stride], anc, A)
            inside = np.where((anc[:, 0] >= 0) & (anc[:, 1] >= 0) & (anc[:, 2] < info[1]) & (anc[:, 3] < info[0]))[0]
            disable = inside[np.concatenate(draws)].astype(np.int32) if draws else np.zeros((0,), dtype=np.int32)
            kw = dict(batchsize=c.batch, fg_fraction=c.fg_fraction, pos_ov=c.pos_ov, neg_ov=c.neg_ov, clobber_positives=c.clobber,
                      positive_weight=c.pos_weight, inside_weights=c.inside_w)
            pin("oracle anchor_target_layer " + c.name, at, ora.anchor_target_layer(score, c.gt, info, [c.stride], anc, A,
                                                                                    rng=np.random.RandomState(SEED), **kw))
            pin("restatement anchor_target_layer " + c.name, at,
                tr.anchor_target_layer(c.base, c.stride, c.H, c.W, c.im_h, c.im_w, c.gt, c.batch, c.fg_fraction, c.pos_ov, c.neg_ov,
                                       clobber=c.clobber, pos_weight=c.pos_weight, inside_w=c.inside_w, disable=disable))
            out["at." + c.name + ".disable"] = disable
            for k, v in zip(AT_KEYS, at):
                out["at." + c.name + "." + k] = v
        for c in tc.roi_cases():
            if not c.golden:
                continue
            n = c.rois.shape[0] if c.num is None else c.num
            rois, sc = c.rois[:n], c.scores[:n].reshape(-1, 1)
            (t.BATCH_SIZE, t.FG_FRACTION, t.FG_THRESH, t.BG_THRESH_HI, t.BG_THRESH_LO, t.USE_GT, t.BBOX_INSIDE_WEIGHTS) = (
                c.batch, c.fg_fraction, c.fg_thresh, c.bg_hi, c.bg_lo, c.use_gt, c.inside_w)
            del draws[:]
            np.random.seed(SEED)
            with np.errstate(invalid="ignore"):
                pt = ref.proposal_target_layer(rois, sc, c.gt, tc.NUM_CLASSES)
            keep = np.concatenate(draws).astype(np.int32)
            n_fg = np.int32(draws[0].size if len(draws) == 2 else (draws[0].size if (pt[2] > 0).all() else 0))
            kw = dict(batch_size=c.batch, fg_fraction=c.fg_fraction, fg_thresh=c.fg_thresh, bg_hi=c.bg_hi, bg_lo=c.bg_lo, use_gt=c.use_gt,
                      inside_weights=c.inside_w)
            with np.errstate(invalid="ignore"):
                pin("oracle proposal_target_layer " + c.name, pt,
                    ora.proposal_target_layer(rois, sc, c.gt, tc.NUM_CLASSES, rng=np.random.RandomState(SEED), **kw))
                got = tr.proposal_target_layer(rois, sc, c.gt, tc.NUM_CLASSES, use_gt=c.use_gt, inside_w=c.inside_w, keep_inds=keep, n_fg=n_fg)
            pin("restatement proposal_target_layer " + c.name, pt, got[:6])
            out["pt." + c.name + ".keep_inds"], out["pt." + c.name + ".n_fg"] = keep, n_fg
            for k, v in zip(PT_KEYS, pt):
                out["pt." + c.name + "." + k] = v
    finally:
        np.random.choice = real_choice
    if write:
        path = os.path.join(GOLD, "targets_edges.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
    if FAIL:
        print("ORACLE NOT PINNED:", FAIL)
        return 1
    print("oracle and restatement pinned against the reference on all cases")
    return 0


if __name__ == "__main__":
    sys.exit(main(write="--check" not in sys.argv))
