"""TEST INFRASTRUCTURE ONLY -- the smallest inputs at which the anchor target layer and the proposal target layer of
csrc/train_kernels.hip can go wrong.  The inputs the suite had (38x63x9 anchors, synth.gt_boxes(7, 21, seed=15), one recorded reference
run) put no anchor on the image border, no IoU on a threshold, no gt box without an overlapping anchor, fewer foreground candidates than
either layer keeps, and one N for the rank launch.  The C entries take the base anchors, the stride, the image size, the thresholds and
the batch size as arguments, so every case here brings its own tiny anchor set.  Shared by tests/test_targets_cpu.py (the numpy
restatement oracle/target_ref.py and its planted mistakes), tests/test_targets_gpu.py (the kernels) and oracle/gen_golden_targets.py
(the reference's own runs, tests/golden/targets_edges.npz); stated once, here.

Every gt class lies in [1, NUM_CLASSES).  Every foreground pair keeps its width and height ratios inside [1/32, 32], the range the
regression-target bounds of the GPU tests were set for."""
import collections

import numpy as np

import target_ref as ref

f32 = np.float32
NUM_CLASSES = 21
SEEDS = (0, 1, 2 ** 31, 2 ** 63 - 1, -1)

AnchorCase = collections.namedtuple("AnchorCase", "name base stride H W im_h im_w gt batch fg_fraction pos_ov neg_ov clobber pos_weight "
                                                  "inside_w golden")
RoiCase = collections.namedtuple("RoiCase", "name rois scores gt batch fg_fraction fg_thresh bg_hi bg_lo use_gt inside_w num golden")

BASE3 = np.array([[0, 0, 15, 15], [-8, 0, 23, 15], [0, -8, 15, 23]], dtype=np.float64)
_SIZES = ((16, 16), (32, 32), (64, 64), (16, 32), (32, 16), (32, 64), (64, 32), (48, 48), (24, 24))


def square_bases(A):
    """A base anchors of side 16 / 32 / 64 (and their 1:2 rectangles) centred on the 16-pixel cell"""
    return np.array([[7.5 - 0.5 * (w - 1), 7.5 - 0.5 * (h - 1), 7.5 + 0.5 * (w - 1), 7.5 + 0.5 * (h - 1)] for w, h in _SIZES[:A]],
                    dtype=np.float64)


def _acase(name, base, H, W, im_h, im_w, gt, batch=256, fg_fraction=0.5, pos_ov=0.7, neg_ov=0.3, clobber=False, pos_weight=-1.0,
           inside_w=(1.0, 1.0, 1.0, 1.0), golden=True):
    return AnchorCase(name, np.asarray(base, dtype=np.float64), 16, H, W, float(im_h), float(im_w), np.asarray(gt, dtype=f32), batch,
                      fg_fraction, float(pos_ov), float(neg_ov), bool(clobber), float(pos_weight), tuple(inside_w), golden)


def random_gt(n, im_h, im_w, seed, lo=10.0, hi=90.0, fractional=True):
    """n gt boxes inside the image, sides in [lo, hi], classes in [1, NUM_CLASSES)"""
    rng = np.random.RandomState(seed)
    w, h = lo + rng.rand(n) * (hi - lo), lo + rng.rand(n) * (hi - lo)
    w, h = np.minimum(w, im_w - 2), np.minimum(h, im_h - 2)
    x1, y1 = rng.rand(n) * (im_w - 1 - w), rng.rand(n) * (im_h - 1 - h)
    g = np.stack([x1, y1, x1 + w, y1 + h, 1 + rng.randint(0, NUM_CLASSES - 1, size=n)], axis=1)
    if not fractional:
        g = np.round(g)
    return g.astype(f32)


# gt of `border`: an exact anchor, an exact wide anchor, and boxes hanging over the right / bottom rows of cells, so that the anchors
# whose x2 == im_w or y2 == im_h would be labelled if they were taken for inside
BORDER_GT = np.array([[16, 16, 31, 31, 3], [40, 0, 71, 15, 7], [88, 20, 110, 52, 12], [30, 58, 70, 78, 5], [96, 64, 110.5, 78.5, 9]],
                     dtype=f32)
# gt of `tie_zero`: two boxes mirrored about the anchor (32,32,47,47), different classes -- their IoUs with it tie exactly --; a third
# box that overlaps no inside anchor, so its maximum is 0 and `overlaps == gt_max_overlaps` holds for EVERY inside anchor
TIE_ZERO_GT = np.array([[28, 32, 43, 47, 3], [36, 32, 51, 47, 7], [300, 300, 330, 330, 11]], dtype=f32)
FRACTIONAL_GT = random_gt(6, 80, 112, seed=21, lo=12.0, hi=60.0)


def threshold_value():
    """(anchor index, v): the first inside anchor of the `fractional` case that is no gt-argmax, whose float64 maximum IoU v lies in
    (0.05, 0.65) and whose IoU in float32 arithmetic is a different number"""
    info = {}
    ref.anchor_target_layer(BASE3, 16, 5, 7, 80, 112, FRACTIONAL_GT, seed=-1, info=info)
    ov32 = ref.iou(info["anchors"], FRACTIONAL_GT, f32).max(axis=1)
    hit = (info["ov"] == info["gtmax"][None, :]).any(axis=1)
    for n in np.where(info["inside"] & ~hit)[0]:
        v = float(info["maxov"][n])
        if 0.05 < v < 0.65 and ov32[n] != v:
            return int(n), v
    raise AssertionError("no anchor fits")


def _chunk_gt(im_h, im_w, seed, n=8):
    return random_gt(n, im_h, im_w, seed, lo=14.0, hi=70.0)


def anchor_cases():
    cs = [_acase("border", BASE3, 5, 7, 79, 111, BORDER_GT),
          _acase("tie_zero", BASE3, 5, 7, 80, 112, TIE_ZERO_GT),
          _acase("tie_zero_b32", BASE3, 5, 7, 80, 112, TIE_ZERO_GT, batch=32),
          _acase("fractional", BASE3, 5, 7, 80, 112, FRACTIONAL_GT, batch=16)]
    _, v = threshold_value()
    for tag, t in (("below", np.nextafter(v, 0.0)), ("at", v), ("above", np.nextafter(v, 1.0))):
        cs.append(_acase("threshold_neg_" + tag, BASE3, 5, 7, 80, 112, FRACTIONAL_GT, neg_ov=t))
        cs.append(_acase("threshold_pos_" + tag, BASE3, 5, 7, 80, 112, FRACTIONAL_GT, pos_ov=t, neg_ov=0.02))
    # N at the seams of launch_key_rank; the image is smaller than the map, so whole 256-thread blocks hold no candidate.  (The 4320-anchor
    # cases have no recorded reference run: the injected entry launches no rank kernel, and the fixture stays small.)
    cs += [_acase("chunks_2049", square_bases(3), 1, 683, 16, 16 * 400, random_gt(24, 16, 16 * 400, 31, lo=11.0, hi=15.5), batch=16, pos_ov=0.5, neg_ov=0.2),
           _acase("chunks_2048", square_bases(8), 16, 16, 160, 256, _chunk_gt(160, 256, 32), batch=16, pos_ov=0.5, neg_ov=0.2),
           _acase("chunks_4320", square_bases(9), 20, 24, 192, 384, _chunk_gt(192, 384, 33), batch=16, pos_ov=0.5, neg_ov=0.2, golden=False)]
    modes = dict(clobber=True, pos_weight=0.3, inside_w=(1.0, 0.5, 2.0, 1.0), batch=8)
    cs += [_acase("modes_border", BASE3, 5, 7, 79, 111, BORDER_GT, neg_ov=0.35, **modes),
           _acase("modes_tie_zero", BASE3, 5, 7, 80, 112, TIE_ZERO_GT, **modes)]
    cs += [_acase("many_gt_1", square_bases(9), 20, 24, 320, 384, random_gt(1, 320, 384, 41, lo=40.0, hi=80.0), batch=64, golden=False),
           _acase("many_gt_100", square_bases(9), 20, 24, 320, 384, random_gt(100, 320, 384, 42, lo=12.0, hi=120.0), batch=64, golden=False)]
    return cs


# ----------------------------------------------------------------------------- proposal target layer
IM_H, IM_W = 320.0, 400.0


def _rois(n_fg, n_bg, gt, seed, im_h=IM_H, im_w=IM_W):
    """n_fg rows that are a gt box moved by up to 10 % of its side (IoU well above 0.5), n_bg random boxes, shuffled"""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n_fg):
        g = gt[rng.randint(0, gt.shape[0]), :4].astype(np.float64)
        w, h = g[2] - g[0] + 1, g[3] - g[1] + 1
        d = (rng.rand(4) - 0.5) * 0.2 * np.array([w, h, w, h])
        rows.append(np.clip(g + d, 0, [im_w - 1, im_h - 1, im_w - 1, im_h - 1]))
    for i in range(n_bg):
        w, h = 8 + rng.rand() * 120, 8 + rng.rand() * 120
        x1, y1 = rng.rand() * (im_w - 1 - w), rng.rand() * (im_h - 1 - h)
        rows.append(np.array([x1, y1, x1 + w, y1 + h]))
    boxes = np.array(rows, dtype=np.float64).reshape(-1, 4)[rng.permutation(n_fg + n_bg)]
    rois = np.concatenate([np.zeros((boxes.shape[0], 1)), boxes], axis=1).astype(f32)
    scores = (1.0 - np.arange(rois.shape[0]) / (rois.shape[0] + 1.0)).astype(f32)         # unique, so that a wrong row shows in roi_scores
    return rois, scores


def _rcase(name, rois, scores, gt, batch, fg_fraction=0.25, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.0, use_gt=False,
           inside_w=(1.0, 1.0, 1.0, 1.0), num=None, golden=True):
    return RoiCase(name, np.ascontiguousarray(rois, dtype=f32), np.ascontiguousarray(scores, dtype=f32), np.asarray(gt, dtype=f32), int(batch),
                   fg_fraction, float(fg_thresh), float(bg_hi), float(bg_lo), bool(use_gt), tuple(inside_w), num, golden)


def roi_cases():
    cs = []
    gt1, gt3, gt40 = random_gt(1, IM_H, IM_W, 51, 40, 120), random_gt(3, IM_H, IM_W, 52, 40, 120), random_gt(40, IM_H, IM_W, 53, 20, 120)
    # sizes; nfg above and below fg_per_image; every branch of the sampling plan
    cs.append(_rcase("n1_fg_repl", *_rois(1, 0, gt1, 1), gt1, 16, bg_lo=0.1))
    cs.append(_rcase("n1_bg_repl", *_rois(0, 1, gt1, 2), gt1, 16))
    cs.append(_rcase("n63_g3_b16", *_rois(20, 43, gt3, 3), gt3, 16))                              # nfg 20 > 4: fg subsampled
    cs.append(_rcase("n63_g3_b256_bg_repl", *_rois(9, 54, gt3, 4), gt3, 256))                     # nfg 9 < 64; bg drawn with replacement
    cs.append(_rcase("n1025_g40_b256", *_rois(200, 825, gt40, 5), gt40, 256))                     # past the 1024-thread stride
    cs.append(_rcase("n3072_g3_b1030", *_rois(400, 2672, gt3, 6), gt3, 1030, golden=False))       # fg_per_image = round(257.5) = 258
    r, s = _rois(5, 30, gt3, 7)
    cs.append(_rcase("fg_only_repl", r, s, gt3, 16, bg_hi=0.0, bg_lo=0.0))                        # [0, 0) is empty: no background
    cs.append(_rcase("bg_only_repl", *_rois(0, 7, gt3, 8), gt3, 16, fg_thresh=0.99))
    # IoU exactly on a threshold: a 10x10 gt box against its 10x5 half (0.5) and its 10x1 strip (0.1)
    gte = np.array([[10, 10, 19, 19, 4], [200, 100, 259, 159, 9]], dtype=f32)
    re = np.array([[0, 10, 10, 19, 14], [0, 10, 10, 19, 10], [0, 200, 100, 259, 159], [0, 100, 200, 140, 240], [0, 150, 20, 190, 70],
                   [0, 10, 10, 19, 15], [0, 10, 11, 19, 11]], dtype=f32)
    cs.append(_rcase("exact_thresholds", re, np.linspace(0.9, 0.3, 7), gte, 16, bg_lo=0.1))
    # duplicate and mirrored gt boxes with different classes: the first arg-max decides the class and the target
    gtt = np.array([[50, 50, 99, 99, 2], [50, 50, 99, 99, 5], [146, 150, 175, 179, 8], [154, 150, 183, 179, 3]], dtype=f32)
    rt = np.array([[0, 50, 50, 99, 99], [0, 150, 150, 179, 179], [0, 52, 50, 97, 99], [0, 250, 20, 300, 60], [0, 10, 200, 60, 260]], dtype=f32)
    cs.append(_rcase("tied_gt", rt, np.linspace(0.9, 0.5, 5), gtt, 16))
    # USE_GT: the gt boxes are candidates; N + G = 3072 exactly is the largest supported set
    cs.append(_rcase("use_gt_n63", *_rois(9, 54, gt3, 9), gt3, 64, use_gt=True, inside_w=(1.0, 1.0, 0.5, 0.0)))
    cs.append(_rcase("use_gt_3072", *_rois(300, 2769, gt3, 10), gt3, 256, use_gt=True, golden=False))
    # the device-resident row count: rows past *num are copies of a gt box, so any use of them shows as foreground rows
    r, s = _rois(9, 54, gt3, 11)
    for num in (0, 1, 62, 63):
        rr = r.copy()
        rr[num:, 1:5] = gt3[1, :4]
        cs.append(_rcase("dn_num_%d" % num, rr, s, gt3, 16, num=num, golden=num > 0))
    cs.append(_rcase("dn_num_40_use_gt", np.concatenate([r[:40], np.tile(np.concatenate([[0], gt3[1, :4]]).astype(f32), (23, 1))]), s, gt3, 16,
                     num=40, use_gt=True))
    # a NaN row and an Inf row are neither foreground nor background
    rn, sn = _rois(6, 20, gt3, 12)
    rn[3, 1:5] = np.nan
    rn[7, 1:5] = [np.inf, np.inf, np.inf, np.inf]
    cs.append(_rcase("nonfinite_bg_lo_0.1", rn, sn, gt3, 32, bg_lo=0.1))
    rn2 = rn.copy()
    rn2[7, 1:5] = rn[8, 1:5]
    cs.append(_rcase("nan_rows_bg_lo_0", rn2, sn, gt3, 32))
    # neither foreground nor background: every output zero, counts {0, 0, 0, 0} (the reference stops in pdb there: no golden)
    far = np.array([[0, 300, 250, 340, 290], [0, 320, 10, 390, 60]], dtype=f32)
    cs.append(_rcase("neither", far, [0.5, 0.25], np.array([[10, 10, 60, 60, 4]], dtype=f32), 16, bg_lo=0.1, golden=False))
    return cs


def unsupported_roi_case():
    """N + G = 3073 with USE_GT: FRCNN_E_UNSUPPORTED before any launch"""
    gt3 = random_gt(3, IM_H, IM_W, 52, 40, 120)
    return _rcase("use_gt_3073", *_rois(10, 3060, gt3, 13), gt3, 16, use_gt=True, golden=False)


def old_anchor_inputs():
    """The anchor-layer inputs the suite had: (name, base, H, W, im_h, im_w, gt, kwargs) -- tests/golden/targets.npz, targets_modes.npz and
    tests/test_edges_gpu.py::test_target_layers_degenerate_samples"""
    import frcnn_oracle as ora
    import synth
    base = ora.generate_anchors()
    gt = synth.gt_boxes(7, 21, seed=15)
    return [("targets", base, 38, 63, 600.0, 1000.0, gt, {}),
            ("targets_modes", base, 38, 63, 600.0, 1000.0, gt, dict(neg_ov=0.35, clobber=True, pos_weight=0.3, inside_w=(1.0, 0.5, 2.0, 1.0))),
            ("degenerate", base, 38, 63, 600.0, 1000.0, np.array([[300, 200, 330, 240, 5]], dtype=f32), {})]


def old_roi_inputs(golden_targets):
    """The proposal-layer inputs the suite had: (name, rois, scores, gt, kwargs); golden_targets = tests/golden/targets.npz"""
    import synth
    g = golden_targets
    rois50 = np.hstack([np.zeros((50, 1), dtype=f32), synth.random_dets(50, seed=3)[:, :4]]).astype(f32)
    one = np.array([[0, 10, 10, 60, 60]], dtype=f32)
    return [("targets", g["pt_in_rois"], g["pt_in_scores"].ravel(), g["gt"], dict(batch=256)),
            ("targets_modes", g["pt_in_rois"], g["pt_in_scores"].ravel(), g["gt"], dict(batch=256, use_gt=True, inside_w=(1.0, 1.0, 0.5, 0.0))),
            ("degenerate_bg", rois50, np.ones(50, dtype=f32), np.array([[900, 500, 999, 599, 2]], dtype=f32), dict(batch=64, fg_thresh=0.99)),
            ("degenerate_fg", np.tile(one, (5, 1)), np.ones(5, dtype=f32), np.array([[10, 10, 60, 60, 4]], dtype=f32), dict(batch=16, bg_lo=0.1))]
