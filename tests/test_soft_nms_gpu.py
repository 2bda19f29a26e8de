"""GPU: Soft-NMS in the device post-processing.  The kernels (one wave per class, the class in registers) against the host entry
frcnn_soft_nms_host -- the same header csrc/softnms_math.h on both sides, every weight written out in IEEE arithmetic, so the comparison
is bit for bit -- and ops.detect_post(soft=...) against: per-class boxes from ops.im_detect_boxes, the host entry per class, the
reference's max_per_image cut (lib/model/test.py:172-180) in numpy."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import soft_nms_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NMS, SIGMA, MIN_SCORE, SCORE_THRESH = 0.3, 0.5, 0.001, 0.05
IM_H, IM_W = 600, 800


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 300, 1024])
def test_soft_nms_equals_the_host_entry_bit_for_bit(dev, n):
    from frcnn_hip import ops
    dets = ref.clustered(np.random.RandomState(100 + n), n)
    if n >= 64:
        dets[5, 4] = dets[40, 4] = dets[63, 4]                      # equal scores across lanes and slots: the lower row first
    d = T(dets, dev)
    for method in (1, 2):
        for rule in (0, 1):
            for min_score in (MIN_SCORE, 0.0):
                out, index, count = ops.soft_nms(d, NMS, rule, method, SIGMA, min_score)
                want, widx = ops.soft_nms_host(dets, NMS, rule, method, SIGMA, min_score)
                m = int(count.item())
                what = (n, method, rule, min_score)
                assert m == len(widx) and (min_score > 0 or m == n), what
                assert np.array_equal(index[:m].cpu().numpy(), widx), what
                assert out[:m].cpu().numpy().tobytes() == want.tobytes(), what
                assert not out[m:].any().item() and bool((index[m:] == -1).all().item()), what


def make_inputs(B, R, C, seed):
    """clustered rois (image coordinates at scale 1.5), small deltas, scores in (0, 1): about 5 % fall under SCORE_THRESH"""
    rng = np.random.RandomState(seed)
    rois = np.zeros((B * R, 5), dtype=np.float32)
    for b in range(B):
        rois[b * R:(b + 1) * R, 1:] = ref.clustered(rng, R, width=IM_W, height=IM_H)[:, :4] * np.float32(1.5)
    bbox_pred = (rng.randn(B * R, 4 * C) * 0.1).astype(np.float32)
    cls_prob = rng.uniform(0.0, 1.0, (B * R, C)).astype(np.float32)
    return cls_prob, bbox_pred, rois


def expected_records(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image, min_score=MIN_SCORE, scale=1.5):
    """per image: [(n,6) records, class-major, emission order inside a class] by the host entry + the reference's cut"""
    from frcnn_hip import ops
    out = []
    for b in range(B):
        sl = slice(b * R, (b + 1) * R)
        bp = None if bbox_pred is None else T(bbox_pred[sl], dev)
        boxes = ops.im_detect_boxes(T(rois[sl], dev), bp, scale, IM_H, IM_W, num_classes=C).cpu().numpy()
        per_class = []
        for j in range(1, C):
            s = cls_prob[sl, j]
            inds = np.flatnonzero((np.arange(R) < num_rois[b]) & (s > np.float32(SCORE_THRESH)))
            dets = np.hstack([boxes[inds, 4 * j:4 * j + 4], s[inds, None]]).astype(np.float32)
            per_class.append(ops.soft_nms_host(dets, NMS, rule, soft, SIGMA, min_score)[0])
        scores = np.concatenate([d[:, 4] for d in per_class]) if per_class else np.zeros(0, np.float32)
        if max_per_image > 0 and len(scores) > max_per_image:                    # test.py:172-180
            srt = np.sort(scores)
            th = srt[-max_per_image]
            assert srt[-max_per_image - 1] < th, "the inputs must not tie at the cut"
            per_class = [d[d[:, 4] >= th] for d in per_class]
        out.append(np.concatenate([np.hstack([d, np.full((len(d), 1), j + 1, np.float32)]) for j, d in enumerate(per_class)]))
    return out


def run_detect(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image, min_score=MIN_SCORE, scale=1.5):
    from frcnn_hip import ops
    dets, count = ops.detect_post(T(cls_prob, dev), None if bbox_pred is None else T(bbox_pred, dev), T(rois, dev),
                                  T(np.array(num_rois, dtype=np.int32), dev), scale, IM_H, IM_W, NMS, SCORE_THRESH, max_per_image,
                                  max_out=R * (C - 1), batch=B, rule=rule, soft=soft, sigma=SIGMA, min_score=min_score)
    dets, count = dets.cpu().numpy().reshape(B, -1, 6), count.cpu().numpy()
    return [dets[b, :count[b]] for b in range(B)]


@pytest.mark.parametrize("B,R,C,num_rois_sets", [(1, 70, 3, ([70], [1], [0])), (2, 130, 3, ([130, 0], [1, 123])),
                                                 (2, 300, 21, ([300, 1], [0, 293]))])
def test_detect_post_soft_equals_host_entry_plus_cut(dev, B, R, C, num_rois_sets):
    cls_prob, bbox_pred, rois = make_inputs(B, R, C, seed=R + C)
    for num_rois in num_rois_sets:
        for soft in (1, 2):
            for rule in (0, 1):
                for max_per_image in (5, 100):
                    got = run_detect(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image)
                    want = expected_records(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image)
                    for b in range(B):
                        what = (num_rois, soft, rule, max_per_image, b)
                        assert got[b].shape == want[b].shape, what
                        assert got[b].tobytes() == want[b].tobytes(), what
                        if num_rois[b] == 0:
                            assert len(got[b]) == 0
                        elif num_rois[b] >= 70:
                            assert len(got[b]) == max_per_image or max_per_image == 100, what      # 5: the cut bites


def test_detect_post_soft_without_bbox_regression(dev):
    B, R, C = 2, 130, 3
    cls_prob, _, rois = make_inputs(B, R, C, seed=11)
    got = run_detect(dev, cls_prob, None, rois, [130, 64], B, R, C, 0, 2, 100)
    want = expected_records(dev, cls_prob, None, rois, [130, 64], B, R, C, 0, 2, 100)
    for b in range(B):
        assert len(want[b]) > 0 and got[b].tobytes() == want[b].tobytes()


def test_detect_post_soft_is_batch_invariant(dev):
    R, C = 130, 5
    cls_prob, bbox_pred, rois = make_inputs(1, R, C, seed=12)
    two = [np.concatenate([a, a]) for a in (cls_prob, bbox_pred, rois)]
    for soft in (1, 2):
        one = run_detect(dev, cls_prob, bbox_pred, rois, [R], 1, R, C, 0, soft, 100)[0]
        both = run_detect(dev, two[0], two[1], two[2], [R, R], 2, R, C, 0, soft, 100)
        assert len(one) > 0 and both[0].tobytes() == one.tobytes() and both[1].tobytes() == one.tobytes()


def test_linear_equals_hard_nms_where_nothing_overlaps_enough(dev):
    """boxes of 51 x 51 on a grid of pitch 40: neighbours overlap with IoU 0.12 and 0.03, all below TEST.NMS = 0.3, so linear Soft-NMS
    decays nothing and hard NMS deletes nothing: the same records, bit for bit"""
    B, R, C = 2, 130, 4
    rng = np.random.RandomState(13)
    rois = np.zeros((B * R, 5), dtype=np.float32)
    g = np.arange(B * R) % R
    rois[:, 1], rois[:, 2] = (g % 13) * 40, (g // 13) * 40
    rois[:, 3], rois[:, 4] = rois[:, 1] + 50, rois[:, 2] + 50
    cls_prob = rng.uniform(0.0, 1.0, (B * R, C)).astype(np.float32)
    for bbox_pred in (None, np.zeros((B * R, 4 * C), dtype=np.float32)):
        for rule in (0, 1):
            for max_per_image in (5, 100):
                hard = run_detect(dev, cls_prob, bbox_pred, rois, [R, 77], B, R, C, rule, 0, max_per_image, scale=1.0)
                soft = run_detect(dev, cls_prob, bbox_pred, rois, [R, 77], B, R, C, rule, 1, max_per_image, min_score=0.0, scale=1.0)
                for b in range(B):
                    assert len(hard[b]) > 0 and soft[b].tobytes() == hard[b].tobytes(), (rule, max_per_image, b)


def test_network_detect_device_reads_the_switch_per_call(dev):
    """HIP.SOFT_NMS = 2 through Network.detect_device equals ops.detect_post(soft=2) on the net's own outputs; back at 0 the same net and
    shape reproduce the first hard result"""
    from frcnn_hip import ops
    from frcnn_hip.runtime import Session
    from model.config import cfg
    from nets.resnet_v1 import resnetv1
    old = (cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.SOFT_NMS, cfg.HIP.SOFT_NMS_SIGMA, cfg.HIP.SOFT_NMS_MIN_SCORE)
    cfg.TEST.RPN_POST_NMS_TOP_N = 48
    try:
        sess = Session(device=dev, seed=3)
        net = resnetv1(num_layers=50)
        net.create_architecture("TEST", 21, tag="default", anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
        sess.init_variables(net.variable_specs())
        rng = np.random.RandomState(5)
        H, W = 150, 200
        image = (rng.rand(1, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)
        im_info = np.array([H, W, 1.0], dtype=np.float32)
        img_d = net._stage_image(sess, image)

        def detect():
            dets, cnt = net.detect_device(sess, img_d, im_info, (H, W))
            return dets[:int(cnt.item())].cpu().numpy().copy()
        hard = detect()
        cfg.HIP.SOFT_NMS, cfg.HIP.SOFT_NMS_SIGMA, cfg.HIP.SOFT_NMS_MIN_SCORE = 2, 0.4, 0.002
        soft = detect()
        p = net._predictions
        want, cnt = ops.detect_post(p["cls_prob"], p["bbox_pred"], p["rois"], net._num_rois, 1.0, H, W, float(cfg.TEST.NMS), 0.0, 100,
                                    rule=net._nms_rule(), soft=2, sigma=0.4, min_score=0.002)
        want = want[:int(cnt.item())].cpu().numpy()
        assert len(hard) > 0 and soft.tobytes() == want.tobytes()
        assert soft.shape != hard.shape or soft.tobytes() != hard.tobytes()           # the switch did something
        cfg.HIP.SOFT_NMS = 0
        assert detect().tobytes() == hard.tobytes()
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.SOFT_NMS, cfg.HIP.SOFT_NMS_SIGMA, cfg.HIP.SOFT_NMS_MIN_SCORE = old
