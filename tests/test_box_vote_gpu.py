"""GPU: bounding-box voting and the horizontal-flip ensemble in the device post-processing.  The kernels against the host entries --
the same header csrc/boxvote_math.h on both sides, IEEE double sums in the same order, so every comparison is bit for bit -- and
ops.detect_post(vote=...) against the host composition: per-class boxes from ops.im_detect_boxes, per-class hard NMS (the numpy statement)
or ops.soft_nms_host, ops.box_vote_host on the class's candidates, the reference's max_per_image cut (lib/model/test.py:172-180) in numpy.
Every equality test runs both thresholds, 0.8 and 0.5, and asserts that at 0.5 the vectors are not trivial."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import box_vote_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NMS, SIGMA, MIN_SCORE, SCORE_THRESH = 0.3, 0.5, 0.001, 0.05
IM_H, IM_W = 600, 800
VOTES = (0.8, 0.5)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 300, 1024])
def test_box_vote_equals_the_host_entry_bit_for_bit(dev, n):
    """kept lists from hard NMS (a few rows) and from Soft-NMS at min_score 0 (m = n: every thread of the kernel up to 1024)"""
    from frcnn_hip import ops
    cands = ref.clustered(np.random.RandomState(100 + n), n)
    soft = ops.soft_nms_host(cands, NMS, 0, 1, SIGMA, 0.0)[0]
    assert len(soft) == n
    for kept in (cands[ref.hard_nms(cands, NMS)], soft):
        for t in VOTES + (1.0,):
            got = ops.box_vote(T(kept, dev), T(cands, dev), t).cpu().numpy()
            want = ops.box_vote_host(kept, cands, t)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (n, len(kept), t)
            assert got[:, 4].tobytes() == kept[:, 4].tobytes()
            if t == 1.0:
                assert got.tobytes() == kept.tobytes()                                      # distinct boxes: the input bits
            if t == 0.5 and n >= 63:
                voters = ref.count_voters(kept, cands, t)
                assert 2 * int((voters >= 2).sum()) > len(voters) and got[:, :4].tobytes() != kept[:, :4].tobytes(), (n, len(kept))


def make_inputs(B, R, C, seed):
    """clustered rois (image coordinates at scale 1.5), small deltas, scores in (0, 1): about 5 % fall under SCORE_THRESH"""
    rng = np.random.RandomState(seed)
    rois = np.zeros((B * R, 5), dtype=np.float32)
    for b in range(B):
        rois[b * R:(b + 1) * R, 1:] = ref.clustered(rng, R, width=IM_W, height=IM_H)[:, :4] * np.float32(1.5)
    bbox_pred = (rng.randn(B * R, 4 * C) * 0.1).astype(np.float32)
    cls_prob = rng.uniform(0.0, 1.0, (B * R, C)).astype(np.float32)
    return cls_prob, bbox_pred, rois


def expected_records(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image, vote, scale=1.5, stats=None):
    """per image: [(n,6) records, class-major, emission order inside a class] by the host composition"""
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
            cands = np.ascontiguousarray(np.hstack([boxes[inds, 4 * j:4 * j + 4], s[inds, None]]), dtype=np.float32)
            kept = cands[ref.hard_nms(cands, NMS, rule)] if soft == 0 else ops.soft_nms_host(cands, NMS, rule, soft, SIGMA, MIN_SCORE)[0]
            voted = ops.box_vote_host(kept, cands, vote) if vote else kept
            if stats is not None and len(kept):
                stats.append((int((ref.count_voters(kept, cands, vote) >= 2).sum()), len(kept), voted[:, :4].tobytes() != kept[:, :4].tobytes()))
            per_class.append(voted)
        scores = np.concatenate([d[:, 4] for d in per_class]) if per_class else np.zeros(0, np.float32)
        if max_per_image > 0 and len(scores) > max_per_image:                    # test.py:172-180
            srt = np.sort(scores)
            th = srt[-max_per_image]
            assert srt[-max_per_image - 1] < th, "the inputs must not tie at the cut"
            per_class = [d[d[:, 4] >= th] for d in per_class]
        out.append(np.concatenate([np.hstack([d, np.full((len(d), 1), j + 1, np.float32)]) for j, d in enumerate(per_class)]))
    return out


def run_detect(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image, vote, min_score=MIN_SCORE, scale=1.5):
    from frcnn_hip import ops
    dets, count = ops.detect_post(T(cls_prob, dev), None if bbox_pred is None else T(bbox_pred, dev), T(rois, dev),
                                  T(np.array(num_rois, dtype=np.int32), dev), scale, IM_H, IM_W, NMS, SCORE_THRESH, max_per_image,
                                  max_out=R * (C - 1), batch=B, rule=rule, soft=soft, sigma=SIGMA, min_score=min_score, vote=vote)
    dets, count = dets.cpu().numpy().reshape(B, -1, 6), count.cpu().numpy()
    return [dets[b, :count[b]] for b in range(B)]


def assert_votes_happened(stats, what):
    """at 0.5 more than half of the kept detections (over the classes that kept any) have a second voter, and a box changed bits"""
    assert stats and 2 * sum(s[0] for s in stats) > sum(s[1] for s in stats) and any(s[2] for s in stats), what


@pytest.mark.parametrize("B,R,C,num_rois_sets", [(1, 70, 3, ([70], [1], [0])), (2, 130, 3, ([130, 0], [1, 123])),
                                                 (2, 300, 21, ([300, 1], [0, 293]))])
def test_detect_post_vote_equals_the_host_composition(dev, B, R, C, num_rois_sets):
    cls_prob, bbox_pred, rois = make_inputs(B, R, C, seed=R + C)
    for num_rois in num_rois_sets:
        for soft in (0, 1, 2):
            for rule in (0, 1):
                for vote in VOTES:
                    for max_per_image in (5, 100):
                        stats = [] if vote == 0.5 else None
                        got = run_detect(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image, vote)
                        want = expected_records(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, max_per_image, vote, stats=stats)
                        for b in range(B):
                            what = (num_rois, soft, rule, vote, max_per_image, b)
                            assert got[b].shape == want[b].shape, what
                            assert got[b].tobytes() == want[b].tobytes(), what
                            if num_rois[b] == 0:
                                assert len(got[b]) == 0
                            elif num_rois[b] >= 70:
                                assert len(got[b]) == max_per_image or max_per_image == 100, what  # 5: the cut bites
                        if vote == 0.5 and max(num_rois) >= 70:
                            assert_votes_happened(stats, (num_rois, soft, rule))
                    # the vote changes boxes only: scores, classes and order are those of the run without it
                    plain = run_detect(dev, cls_prob, bbox_pred, rois, num_rois, B, R, C, rule, soft, 100, 0.0)
                    for b in range(B):
                        assert got[b][:, 4:].tobytes() == plain[b][:, 4:].tobytes(), (num_rois, soft, rule, b)


def test_detect_post_vote_without_bbox_regression(dev):
    B, R, C = 2, 130, 3
    cls_prob, _, rois = make_inputs(B, R, C, seed=11)
    for soft in (0, 2):
        for vote in VOTES:
            stats = [] if vote == 0.5 else None
            got = run_detect(dev, cls_prob, None, rois, [130, 64], B, R, C, 0, soft, 100, vote)
            want = expected_records(dev, cls_prob, None, rois, [130, 64], B, R, C, 0, soft, 100, vote, stats=stats)
            for b in range(B):
                assert len(want[b]) > 0 and got[b].tobytes() == want[b].tobytes(), (soft, vote, b)
            if vote == 0.5:
                assert_votes_happened(stats, soft)


def test_detect_post_vote_is_batch_invariant(dev):
    R, C = 130, 5
    cls_prob, bbox_pred, rois = make_inputs(1, R, C, seed=12)
    two = [np.concatenate([a, a]) for a in (cls_prob, bbox_pred, rois)]
    for soft in (0, 1, 2):
        for vote in VOTES:
            one = run_detect(dev, cls_prob, bbox_pred, rois, [R], 1, R, C, 0, soft, 100, vote)[0]
            both = run_detect(dev, two[0], two[1], two[2], [R, R], 2, R, C, 0, soft, 100, vote)
            plain = run_detect(dev, cls_prob, bbox_pred, rois, [R], 1, R, C, 0, soft, 100, 0.0)[0]
            assert len(one) > 0 and both[0].tobytes() == one.tobytes() and both[1].tobytes() == one.tobytes(), (soft, vote)
            assert vote != 0.5 or one.tobytes() != plain.tobytes()


def test_vote_at_one_equals_vote_off_where_no_two_candidates_share_a_box(dev):
    """boxes of 51 x 51 on a grid of pitch 40 (the grid of test_soft_nms_gpu.py): neighbours overlap but no two rows of an image share a
    box, so at vote_thresh 1.0 a detection's only voter is itself and (s * x) / s is exact: the records of the run without voting"""
    B, R, C = 2, 130, 4
    rng = np.random.RandomState(13)
    rois = np.zeros((B * R, 5), dtype=np.float32)
    g = np.arange(B * R) % R
    rois[:, 1], rois[:, 2] = (g % 13) * 40, (g // 13) * 40
    rois[:, 3], rois[:, 4] = rois[:, 1] + 50, rois[:, 2] + 50
    cls_prob = rng.uniform(0.0, 1.0, (B * R, C)).astype(np.float32)
    for bbox_pred in (None, np.zeros((B * R, 4 * C), dtype=np.float32)):
        for soft, min_score in ((0, MIN_SCORE), (1, 0.0), (2, 0.0)):
            for rule in (0, 1):
                for max_per_image in (5, 100):
                    off = run_detect(dev, cls_prob, bbox_pred, rois, [R, 77], B, R, C, rule, soft, max_per_image, 0.0, min_score=min_score, scale=1.0)
                    one = run_detect(dev, cls_prob, bbox_pred, rois, [R, 77], B, R, C, rule, soft, max_per_image, 1.0, min_score=min_score, scale=1.0)
                    for b in range(B):
                        assert len(off[b]) > 0 and one[b].tobytes() == off[b].tobytes(), (soft, rule, max_per_image, b)


def _views(rng, B, R, C, width):
    rows = 2 * B * R
    rois = np.zeros((rows, 5), dtype=np.float32)
    rois[:, 0] = np.arange(rows) // R
    rois[:, 1:] = np.concatenate([ref.clustered(rng, R, width=width, height=IM_H * 1.5)[:, :4] for _ in range(2 * B)])
    return rng.uniform(0, 1, (rows, C)).astype(np.float32), (rng.randn(rows, 4 * C) * 0.1).astype(np.float32), rois


@pytest.mark.parametrize("B,R,C,nums", [(1, 1, 2, ([1, 1], [0, 1], [0, 0])), (2, 48, 21, ([48, 48, 48, 48], [0, 31, 17, 0], None)),
                                        (3, 300, 21, ([300, 300, 0, 300, 291, 7],)), (1, 512, 3, ([512, 512], [500, 7]))])
def test_merge_flip_views_equals_numpy(dev, B, R, C, nums):
    from frcnn_hip import ops
    prob, pred, rois = _views(np.random.RandomState(B * 1000 + R), B, R, C, 1200.0)
    for num in nums:
        for bp in (pred, None):
            got = ops.merge_flip_views(T(prob, dev), None if bp is None else T(bp, dev), T(rois, dev),
                                       None if num is None else T(np.array(num, dtype=np.int32), dev), 1200.0, batch=B)
            want = ref.merge_flip_views(prob, bp, rois, num, 1200.0, B)
            host = ops.merge_flip_views_host(prob, bp, rois, num, 1200.0, batch=B)
            for g, w, h, name in zip(got, want, host, ("cls_prob", "bbox_pred", "rois", "num_rois")):
                if bp is None and name == "bbox_pred":
                    assert g is None and w is None and h is None
                    continue
                g = g.cpu().numpy()
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() == h.tobytes(), (num, name)


def test_detect_post_on_1024_merged_rows(dev):
    """two views of 512 rows merged into one image of 1024, the largest the post-processing holds, then voted: the host composition"""
    from frcnn_hip import ops
    B, R, C = 1, 512, 3
    cls_prob, bbox_pred, rois = make_inputs(2, R, C, seed=21)
    rois[:, 0] = np.arange(2 * R) // R
    for num in ([512, 512], [512, 300]):
        m = ops.merge_flip_views(T(cls_prob, dev), T(bbox_pred, dev), T(rois, dev), T(np.array(num, dtype=np.int32), dev), IM_W * 1.5, batch=B)
        m_prob, m_pred, m_rois, m_num = [a.cpu().numpy() for a in m]
        assert m_prob.shape == (1024, C) and int(m_num[0]) == sum(num)
        for soft in (0, 2):
            for vote in VOTES:
                stats = [] if vote == 0.5 else None
                got = run_detect(dev, m_prob, m_pred, m_rois, [int(m_num[0])], 1, 2 * R, C, 0, soft, 100, vote)
                want = expected_records(dev, m_prob, m_pred, m_rois, [int(m_num[0])], 1, 2 * R, C, 0, soft, 100, vote, stats=stats)
                assert len(want[0]) > 0 and got[0].tobytes() == want[0].tobytes(), (num, soft, vote)
                if vote == 0.5:
                    assert_votes_happened(stats, (num, soft))


@pytest.mark.parametrize("B,OH,OW,c", [(1, 3, 1, 4), (2, 5, 7, 3), (3, 37, 300, 4)])
def test_mirror_views_equals_numpy(dev, B, OH, OW, c):
    from frcnn_hip import ops
    a = np.random.RandomState(OW).randn(B, OH, OW, c).astype(np.float32)
    flat = torch.full((2 * B * OH * OW * c + 16,), -7.0, dtype=torch.float32, device=dev)
    out = flat[8:-8].view(2 * B, OH, OW, c)
    assert ops.mirror_views(T(a, dev), out=out) is out
    got = ops.mirror_views(T(a, dev)).cpu().numpy()
    want = np.empty((2 * B, OH, OW, c), dtype=np.float32)
    want[0::2], want[1::2] = a, a[:, :, ::-1]
    assert got.tobytes() == want.tobytes() and out.cpu().numpy().tobytes() == want.tobytes()
    assert bool((flat[:8] == -7.0).all()) and bool((flat[-8:] == -7.0).all())                # nothing written outside the views
    with pytest.raises(ValueError):
        ops.mirror_views(T(a, dev), out=torch.empty((B, OH, OW, c), dtype=torch.float32, device=dev))


def test_network_detect_device_reads_the_switches_per_call(dev):
    """HIP.TEST_FLIP / HIP.BBOX_VOTE through Network.detect_device equal the explicit composition -- mirror_views, forward_device on the
    2-view batch, merge_flip_views, ops.detect_post(vote=...) -- on the net's own outputs; back off, the same net and shape reproduce the
    first plain result"""
    from frcnn_hip import ops
    from frcnn_hip.runtime import Session
    from model.config import cfg
    from nets.resnet_v1 import resnetv1
    old = (cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH, cfg.HIP.SOFT_NMS)
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

        def composed(flip, vote, soft=0):
            if flip:
                p = net.forward_device(sess, ops.mirror_views(img_d), im_info)
                assert p["cls_prob"].shape[0] == 2 * 48 and net._num_rois.shape[0] == 2
                prob, pred, rois, num = ops.merge_flip_views(p["cls_prob"], p["bbox_pred"], p["rois"], net._num_rois, float(W), batch=1)
            else:
                p = net.forward_device(sess, img_d, im_info)
                prob, pred, rois, num = p["cls_prob"], p["bbox_pred"], p["rois"], net._num_rois
            want, cnt = ops.detect_post(prob, pred, rois, num, 1.0, H, W, float(cfg.TEST.NMS), 0.0, 100, rule=net._nms_rule(), soft=soft,
                                        sigma=float(cfg.HIP.SOFT_NMS_SIGMA), min_score=float(cfg.HIP.SOFT_NMS_MIN_SCORE), vote=vote)
            return want[:int(cnt.item())].cpu().numpy().copy()
        plain = detect()
        assert len(plain) > 0
        results = {}
        for flip, vote, soft in ((False, 0.5, 0), (True, 0.0, 0), (True, 0.5, 0), (True, 0.8, 2)):
            cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH, cfg.HIP.SOFT_NMS = flip, vote > 0, vote if vote else 0.8, soft
            got = detect()
            assert got.tobytes() == composed(flip, vote, soft).tobytes(), (flip, vote, soft)
            assert got.shape != plain.shape or got.tobytes() != plain.tobytes(), (flip, vote, soft)     # the switches did something
            results[(flip, vote, soft)] = got
        assert results[(False, 0.5, 0)][:, 4:].tobytes() == plain[:, 4:].tobytes()          # voting alone: boxes only
        cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.SOFT_NMS = False, False, 0
        assert detect().tobytes() == plain.tobytes()
        cfg.HIP.TEST_FLIP, cfg.TEST.RPN_POST_NMS_TOP_N = True, 1000                         # read per call: refused, not truncated
        with pytest.raises(NotImplementedError, match="1024"):
            detect()
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH, cfg.HIP.SOFT_NMS = old


SIZES = [(120, 160)] * 3 + [(160, 120)] + [(120, 160)] * 2
CLASSES = ('__background__', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
           'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')


def build_devkit(data_dir, split, sizes, seed):
    """<data_dir>/VOCdevkit2007/VOC2007/{JPEGImages,Annotations,ImageSets/Main/<split>.txt} with seeded smooth-plus-noise images and one box
    each (the helper of tests/test_batched_imdb_gpu.py, restated)"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    base = os.path.join(data_dir, "VOCdevkit2007", "VOC2007")
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    index = ["%06d" % (i + 1) for i in range(len(sizes))]
    for i, (name, (h, w)) in enumerate(zip(index, sizes)):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        chans = [128 + 90 * np.sin(xx / (3.0 + c) + c + i) * np.cos(yy / (5.0 - c)) + 30 * np.sin((xx + yy) / 11.0) + rng.randn(h, w) * 12
                 for c in range(3)]
        Image.fromarray(np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8), "RGB").save(
            os.path.join(base, "JPEGImages", name + ".jpg"), "JPEG", quality=90, subsampling=i % 3)
        x1, y1 = rng.randint(1, w - 12), rng.randint(1, h - 12)
        x2, y2 = rng.randint(x1 + 4, w + 1), rng.randint(y1 + 4, h + 1)
        body = ("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>0</difficult><bndbox><xmin>%d</xmin>"
                "<ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>" % (CLASSES[rng.randint(1, 21)], x1, y1, x2, y2))
        with open(os.path.join(base, "Annotations", name + ".xml"), "w") as f:
            f.write("<annotation><filename>%s.jpg</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>"
                    % (name, w, h, body))
    with open(os.path.join(base, "ImageSets", "Main", split + ".txt"), "w") as f:
        f.write("\n".join(index) + "\n")


def test_batched_imdb_loop_with_the_flip_ensemble_equals_the_one_by_one_loop(dev, tmp_path):
    """6 JPEGs of two sizes, TEST_FLIP and BBOX_VOTE on: TEST_BATCH_IMAGES = 4 (a batch of 4 images = 8 views, then singles of 2 views)
    gives the all_boxes of TEST_BATCH_IMAGES = 1, array for array, and not those of the run without the flip"""
    from datasets.factory import get_imdb
    from frcnn_hip.runtime import Session
    from model.config import cfg
    from model.test import plan_batches, test_net_imdb
    from nets.resnet_v1 import resnetv1
    assert plan_batches(SIZES, 4) == [([0, 1, 2, 4], 0), ([5], 0), ([3], 0)]
    data_dir = str(tmp_path / "data")
    build_devkit(data_dir, "test", SIZES, seed=43)
    old = (cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.TEST_FLIP,
           cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH)
    cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.TEST.RPN_POST_NMS_TOP_N = data_dir, (120,), 160, 64
    runs = []
    sess = Session(device=dev, seed=9)
    try:
        net = resnetv1(num_layers=50)
        net.create_architecture("TEST", 21, tag="flip_imdb", anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
        sess.init_variables(net.variable_specs())
        for flip, batch in ((True, 1), (True, 4), (False, 4)):
            cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH, cfg.HIP.TEST_BATCH_IMAGES = flip, flip, 0.5, batch
            with contextlib.redirect_stdout(io.StringIO()):
                imdb = get_imdb("voc_2007_test")
                runs.append(test_net_imdb(sess, net, imdb, str(tmp_path / ("out%d%d" % (flip, batch))), thresh=0.0))
    finally:
        (cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.TEST_FLIP,
         cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH) = old
        sess.close()
    one, four, plain = runs
    total, differs = 0, False
    for j in range(1, 21):
        for i in range(len(SIZES)):
            a, b, c = np.asarray(one[j][i]), np.asarray(four[j][i]), np.asarray(plain[j][i])
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (j, i)
            total += a.shape[0]
            differs = differs or a.shape != c.shape or not np.array_equal(a, c)
    assert total > 0 and differs
