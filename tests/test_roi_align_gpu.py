"""RoIAlign (cfg.POOLING_MODE = 'align') on the device: the kernels of csrc/roi_align.hip against the host statements of the same
header (bytes), under every launch shape; the mode through the network in TEST mode (three backbones, fused tail entry, batches, flip
ensemble) and through one TRAIN step against float64 autograd (the recipe and the bounds of
tests/test_train_gpu.py::test_full_train_step_matches_torch_autograd)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import roi_align_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
SCALES, RATIOS = (4, 8, 16), (0.5, 1, 2)
STRIDE = 16.0


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rel_err(got, want):
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def make_rois(rng, n, H, W, images):
    """the six edge RoIs, a row without an image at either end of the index range, then boxes inside, across and beyond an H x W map"""
    x1 = rng.uniform(-48, W * STRIDE, n)
    y1 = rng.uniform(-48, H * STRIDE, n)
    w = rng.uniform(0, 1, n) ** 2 * (W * STRIDE + 40)
    h = rng.uniform(0, 1, n) ** 2 * (H * STRIDE + 40)
    r = np.stack([rng.randint(0, images, n).astype(np.float64), x1, y1, x1 + w, y1 + h], axis=1).astype(f32)
    head = np.concatenate([ref.EDGE_ROIS, np.array([[7, 16, 16, 48, 48], [-1, 16, 16, 48, 48]], dtype=f32)])
    head[:, 0] = np.where(head[:, 0] == 1, images - 1, head[:, 0])
    return np.concatenate([head, r])[:n].astype(f32)


@pytest.fixture(scope="module")
def forward_cases():
    """per (map, C): two images, 300 RoIs and the host statement's output for them, computed once"""
    from frcnn_hip import ops
    cases = {}
    for H, W in ((5, 6), (38, 63)):
        for C in (4, 64, 512, 1024):
            rng = np.random.RandomState(H * 1000 + C)
            feat = rng.randn(2, H, W, C).astype(f32)
            rois = make_rois(rng, 300, H, W, 2)
            cases[(H, W, C)] = (feat, rois, ops.roi_align_host(feat, rois, STRIDE, 7, 2))
    return cases


@pytest.mark.parametrize("C", [4, 64, 512, 1024])
@pytest.mark.parametrize("H,W", [(5, 6), (38, 63)])
def test_forward_equals_the_host_statement(dev, forward_cases, H, W, C):
    import frcnn_hip
    from frcnn_hip import ops
    feat, rois, want = forward_cases[(H, W, C)]
    fd, rd = T(feat, dev), T(rois, dev)
    for R in (0, 1, 6, 65, 300):                        # rows are independent: the first R rows of the host result
        out = torch.full((R, 7, 7, C), float("nan"), device=dev)                                # garbage: every element must be overwritten
        got = ops.roi_align(fd, rd[:R].contiguous(), STRIDE, 7, 2, out=out).cpu().numpy()
        assert got.shape == (R, 7, 7, C) and np.array_equal(bits(got), bits(want[:R])), R
    assert not want[6:8].any() and want[:6].any()
    # one image: the rows of image 0 alone, and the same map as slot 1 of a batch of two
    first = rois[rois[:, 0] == 0]
    alone = ops.roi_align(T(feat[:1], dev), T(first, dev), STRIDE, 7, 2).cpu().numpy()
    assert np.array_equal(bits(alone), bits(want[rois[:, 0] == 0]))
    second = first.copy()
    second[:, 0] = 1
    slot1 = ops.roi_align(T(np.stack([feat[1], feat[0]]), dev), T(second, dev), STRIDE, 7, 2).cpu().numpy()
    assert np.array_equal(bits(slot1), bits(alone))
    # every channel-slab count gives the same bytes (frcnn_detect_set_tuning key 4)
    try:
        for slabs in (1, 2, 4, 8):
            if (C // 4) % slabs:
                continue
            frcnn_hip.lib().frcnn_detect_set_tuning(4, slabs)
            got = ops.roi_align(fd, rd, STRIDE, 7, 2).cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), slabs
    finally:
        frcnn_hip.lib().frcnn_detect_set_tuning(4, -1)


@pytest.mark.parametrize("P,S", [(7, 1), (7, 3), (2, 1), (14, 4)])
def test_forward_other_grids_and_the_bias_relu_epilogue(dev, P, S):
    from frcnn_hip import ops
    H, W, C = 5, 6, 64
    rng = np.random.RandomState(10 * P + S)
    feat, rois, bias = rng.randn(2, H, W, C).astype(f32), make_rois(rng, 40, H, W, 2), rng.randn(C).astype(f32)
    want = ops.roi_align_host(feat, rois, STRIDE, P, S)
    got = ops.roi_align(T(feat, dev), T(rois, dev), STRIDE, P, S).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    fused = want + bias
    fused = np.where(fused < 0, f32(0), fused)
    fused[6:8] = 0                                       # a row without an image is zero, bias or not
    out = torch.full((40, P, P, C), float("nan"), device=dev)
    got = ops.roi_align_bias_act(T(feat, dev), T(rois, dev), STRIDE, P, S, T(bias, dev), 1, out=out).cpu().numpy()
    assert np.array_equal(bits(got), bits(fused))
    assert np.array_equal(bits(got), bits(ops.roi_align_host(feat, rois, STRIDE, P, S, bias=bias, act=1)))


def test_forward_refuses_what_it_cannot_run(dev):
    import frcnn_hip
    from frcnn_hip import ops
    rois = T(ref.EDGE_ROIS, dev)
    with pytest.raises(frcnn_hip.FrcnnHipError, match="not supported"):
        ops.roi_align(torch.zeros((1, 5, 6, 6), device=dev), rois, STRIDE, 7, 2)                 # C % 4 != 0
    for P, S in ((7, 0), (7, 5), (0, 2)):
        with pytest.raises(frcnn_hip.FrcnnHipError):
            ops.roi_align(torch.zeros((1, 5, 6, 8), device=dev), rois, STRIDE, P, S)


@pytest.mark.parametrize("C", [64, 300])
@pytest.mark.parametrize("W", [6, 70])
def test_backward_equals_the_host_statement_under_every_launch_plan(dev, W, C):
    """The LDS budget argument forces NT = 256, 128 and 64 with a windowed hit list (4 x NT entries for 130 x 7 x 2 = 1820 sample rows) on
    small inputs, as tests/test_edges_gpu.py does for the crop; every plan must give the bytes of the host statement."""
    from frcnn_hip import ops
    H, R, P, S = 5, 130, 7, 2
    rng = np.random.RandomState(W * 1000 + C)
    rois = make_rois(rng, R, H, W, 1)
    dout, base = rng.randn(R, P, P, C).astype(f32), rng.randn(H, W, C).astype(f32)
    want = ops.roi_align_bwd_host(dout, rois, STRIDE, S, base.copy())
    assert not np.array_equal(want, base)
    budgets = [0, W * 256 * 4 + 4 * 256 * 4, W * 128 * 4 + 4 * 128 * 4, W * 64 * 4 + 4 * 64 * 4]
    for b in budgets:
        dfeat = T(base, dev).clone()
        ops.roi_align_bwd(T(dout, dev), T(rois, dev), STRIDE, S, dfeat, max_lds=b)
        assert np.array_equal(bits(dfeat.cpu().numpy()), bits(want)), b
    dfeat = T(base, dev).clone()                          # R = 0: nothing is added
    ops.roi_align_bwd(torch.zeros((0, P, P, C), device=dev), torch.zeros((0, 5), device=dev), STRIDE, S, dfeat)
    assert np.array_equal(bits(dfeat.cpu().numpy()), bits(base))


def test_backward_refuses_a_map_too_wide_for_the_row_buffer(dev):
    import frcnn_hip
    from frcnn_hip import ops
    dfeat = torch.zeros((4, 700, 64), device=dev)
    with pytest.raises(frcnn_hip.FrcnnHipError, match="not supported"):
        ops.roi_align_bwd(torch.ones((1, 7, 7, 64), device=dev), torch.zeros((1, 5), device=dev), STRIDE, 2, dfeat)
    assert not dfeat.any().item()                         # nothing was launched


@pytest.fixture
def align_cfg():
    from model.config import cfg
    old = (cfg.POOLING_MODE, cfg.HIP.ROI_ALIGN_SAMPLES, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.TEST_FLIP)
    cfg.POOLING_MODE, cfg.TEST.RPN_POST_NMS_TOP_N = "align", 48
    yield cfg
    cfg.POOLING_MODE, cfg.HIP.ROI_ALIGN_SAMPLES, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.TEST_FLIP = old


def _image(rng, H, W, scale=1.0):
    from model.config import cfg
    return ((rng.rand(1, H, W, 3) * 255.0).astype(f32) - cfg.PIXEL_MEANS.astype(f32)) * f32(scale)


def test_resnet_in_align_mode(dev, align_cfg):
    from frcnn_hip import ops
    from frcnn_hip.runtime import Session
    from nets.resnet_v1 import resnetv1
    cfg = align_cfg
    sess = Session(device=dev, seed=3)
    net = resnetv1(num_layers=50)
    net.create_architecture("TEST", 21, tag="align", anchor_scales=SCALES, anchor_ratios=RATIOS)
    sess.init_variables(net.variable_specs())
    rng = np.random.RandomState(5)
    H, W = 128, 160
    image, img2 = _image(rng, H, W), _image(rng, H, W)
    im_info = np.array([H, W, 1.0], dtype=f32)
    base = net.test_image(sess, image, im_info)
    rois = base[3]
    n = rois.shape[0]
    assert 0 < n <= 48
    head = net._layers["head"].cpu().numpy()
    want = ops.roi_align_host(head, rois, STRIDE, 7, 2)
    assert np.array_equal(bits(net._layers["pool5"][:n].cpu().numpy()), bits(want)) and want.any()
    # the other sample count is another graph with other values
    cfg.HIP.ROI_ALIGN_SAMPLES = 1
    net.test_image(sess, image, im_info)
    assert np.array_equal(bits(net._layers["pool5"][:n].cpu().numpy()), bits(ops.roi_align_host(head, rois, STRIDE, 7, 1)))
    cfg.HIP.ROI_ALIGN_SAMPLES = 2
    # fused tail entry: the pooling commuted past block4/unit_1's 1x1 convolutions, the bound of the crop's fused entry (test_network_gpu.py)
    net._fuse_tail_entry = True
    try:
        fused = net.test_image(sess, image, im_info)
    finally:
        net._fuse_tail_entry = False
    assert np.array_equal(base[3], fused[3])
    for a, b in zip(base[:3], fused[:3]):
        assert rel_err(b, a) <= 2e-5
    # the same image alone and in a batch of two: identical bits
    keys = ("rois", "cls_prob", "bbox_pred")
    p = net.forward_device(sess, net._stage_image(sess, image), im_info)
    torch.cuda.synchronize()
    single = {k: p[k].cpu().numpy().copy() for k in keys}
    p = net.forward_device(sess, net._stage_image(sess, np.concatenate([img2, image], axis=0)), im_info)
    torch.cuda.synchronize()
    per = net._rois_per_image
    sl = slice(per, 2 * per)
    assert np.array_equal(p["rois"][sl].cpu().numpy()[:, 1:], single["rois"][:, 1:])
    for k in ("cls_prob", "bbox_pred"):
        assert np.array_equal(bits(p[k][sl].cpu().numpy()), bits(single[k])), k
    # the flip ensemble builds and runs in this mode
    cfg.HIP.TEST_FLIP = True
    dets, cnt = net.detect_device(sess, net._stage_image(sess, image), im_info, (H, W))
    assert int(cnt.cpu().numpy().ravel()[0]) > 0 and torch.isfinite(dets).all().item()


@pytest.mark.parametrize("arch", ["vgg16", "mobile"])
def test_vgg16_and_mobilenet_pool_seven_by_seven_directly(dev, align_cfg, arch):
    from frcnn_hip import ops
    from frcnn_hip.runtime import Session
    from nets.mobilenet_v1 import mobilenetv1
    from nets.vgg16 import vgg16
    align_cfg.TEST.RPN_POST_NMS_TOP_N = 24
    sess = Session(device=dev, seed=7)
    net = vgg16() if arch == "vgg16" else mobilenetv1()
    net.create_architecture("TEST", 21, tag="align_" + arch, anchor_scales=SCALES, anchor_ratios=RATIOS)
    sess.init_variables(net.variable_specs())
    H, W = 121, 170
    image = _image(np.random.RandomState(11), H, W, 1 / 64.0 if arch == "vgg16" else 1.0)
    _, cls_prob, _, rois = net.test_image(sess, image, np.array([H, W, 1.0], dtype=f32))
    n = rois.shape[0]
    pool5 = net._layers["pool5"][:n].cpu().numpy()
    assert n > 0 and pool5.shape == (n, 7, 7, 512) and np.isfinite(cls_prob).all()
    assert np.array_equal(bits(pool5), bits(ops.roi_align_host(net._layers["head"].cpu().numpy(), rois, STRIDE, 7, 2)))


def _train_step(dev, tag):
    """tests/test_train_gpu.py::test_full_train_step_matches_torch_autograd's step (shipped switches) -> losses, rois / targets, state"""
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.resnet_v1 import resnetv1
    sess = Session(device=dev, seed=5)
    net = resnetv1(num_layers=50)
    net.create_architecture("TRAIN", 21, tag=tag, anchor_scales=SCALES, anchor_ratios=RATIOS)
    sess.init_variables(net.variable_specs())
    H, W = 128, 160
    image = _image(np.random.RandomState(2), H, W, 1 / 256.0)
    gt = np.array([[16, 16, 79, 79, 3], [60, 30, 150, 110, 7], [5, 70, 60, 120, 12]], dtype=f32)
    losses = net.train_forward(sess, dict(data=image, im_info=np.array([H, W, 1.0], dtype=f32), gt_boxes=gt))
    ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4).build()
    ts.backward(net._loss_seeds)
    torch.cuda.synchronize()
    return sess, net, ts, image, {k: f32(v.item()) for k, v in losses.items()}


def test_train_step_matches_float64_autograd_and_repeats_bit_for_bit(dev, align_cfg):
    cfg = align_cfg
    old = (cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO)
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO = 64, 0.0
    try:
        sess, net, ts, image, losses = _train_step(dev, "align_train_a")
        assert [r["kind"] for r in net._tape].count("roi_align") == 1 and not any(r["kind"] == "crop" for r in net._tape)
        pt, at = net._proposal_targets, net._anchor_targets
        counts = pt["counts"].cpu().numpy()
        assert counts[0] > 0 and counts[0] + counts[1] == 64
        Ref = ref.align_train_ref()
        r64 = Ref(sess.variables, 50, 21, SCALES, RATIOS, net.trainable_scope)
        to_np = lambda d_: {k: v.cpu().numpy() for k, v in d_.items()}
        rl = r64.losses(image, pt["rois"].cpu().numpy(), to_np(at), to_np(pt))
        for k in ("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box"):
            assert abs(float(losses[k]) - rl[k].item()) <= 1e-4 * max(1.0, abs(rl[k].item())), k
        sum(rl.values()).backward()
        checked = 0
        for sc in ("/cls_score", "/bbox_pred", "/rpn_cls_score", "/rpn_conv/3x3", "/block4/unit_3/bottleneck_v1/conv2",
                   "/block4/unit_1/bottleneck_v1/shortcut", "/block3/unit_6/bottleneck_v1/conv3", "/block3/unit_1/bottleneck_v1/conv1",
                   "/block2/unit_4/bottleneck_v1/conv2", "/block2/unit_1/bottleneck_v1/conv1", "/block2/unit_1/bottleneck_v1/shortcut"):
            scope = net._scope + sc
            p = ts.params[scope]
            g = r64._cache[scope + "/weights"].grad.numpy()
            if g.ndim == 2:
                g = g[None, None]
            want = np.transpose(g, (3, 0, 1, 2))
            got = p.grad_w.cpu().numpy()
            if p.scale is not None:
                got = got * p.scale.cpu().numpy()[:, None, None, None]
            err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-12)
            assert err <= 2e-3, (sc, err)
            checked += 1
        assert checked == 11
        # the same step again, from scratch: the atomic-free backward leaves no run-to-run bits upstream of the pooling
        up = net._scope + "/block3/unit_1/bottleneck_v1/conv1"
        g_a = ts.params[up].grad_w.cpu().numpy().copy()
        _, _, ts_b, _, losses_b = _train_step(dev, "align_train_b")
        assert all(losses[k].tobytes() == losses_b[k].tobytes() for k in losses)
        assert np.abs(g_a).max() > 0 and np.array_equal(bits(g_a), bits(ts_b.params[up].grad_w.cpu().numpy()))
    finally:
        cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO = old


def test_replayed_training_steps_equal_eager_steps(dev, align_cfg):
    """cfg.HIP.TRAIN_REPLAY with the roi_align record on the tape: four steps eager and replayed, the same loss bits"""
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.resnet_v1 import resnetv1
    cfg = align_cfg
    old = (cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_REPLAY)
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO = 64, 0.0
    H, W = 128, 160
    blob = dict(data=_image(np.random.RandomState(4), H, W, 1 / 256.0), im_info=np.array([H, W, 1.0], dtype=f32),
                gt_boxes=np.array([[16, 16, 79, 79, 3], [60, 30, 150, 110, 7]], dtype=f32))
    runs = []
    try:
        for replay in (False, True):
            cfg.HIP.TRAIN_REPLAY = replay
            sess = Session(device=dev, seed=9)
            net = resnetv1(num_layers=50)
            net.create_architecture("TRAIN", 21, tag="align_rp%d" % replay, anchor_scales=SCALES, anchor_ratios=RATIOS)
            sess.init_variables(net.variable_specs())
            ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4)
            ts.lr = 1e-3
            runs.append([tuple(net.train_step(sess, blob, ts)) for _ in range(4)])
            torch.cuda.synchronize()
            if replay:
                assert net.replay_stats["replayed"] >= 1, net.replay_stats
    finally:
        cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.HIP.TRAIN_REPLAY = old
    assert all(np.isfinite(v) for step in runs[0] for v in step) and runs[0] == runs[1], runs
