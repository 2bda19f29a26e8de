"""GPU: online hard example mining (cfg.HIP.OHEM; csrc/ohem_math.h, csrc/ohem.hip).  The device entry against the host entry byte for
byte -- tests/test_ohem_cpu.py holds the host entry to the float64 statement --, then the training step with the switch on: the
selection is the host entry's on the read-only pass's own outputs, losses and filter gradients are those of torch float64 autograd fed the
selected RoIs (a read-only pass that leaked onto the tape would double them), a replayed run equals an eager one bit for bit, the
read-only pass reads derived filters that followed the solver, and VGG16 (no dropout in the read-only pass) and MobileNet run."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import gen_golden_ohem as gen  # noqa: E402

SC, RT = (4, 8, 16), (0.5, 1, 2)
GT = np.array([[16, 16, 79, 79, 3], [60, 30, 150, 110, 7], [5, 70, 60, 120, 12]], dtype=np.float32)
H, W = 128, 160
ELEVEN = ("/cls_score", "/bbox_pred", "/rpn_cls_score", "/rpn_conv/3x3", "/block4/unit_3/bottleneck_v1/conv2",
          "/block4/unit_1/bottleneck_v1/shortcut", "/block3/unit_6/bottleneck_v1/conv3", "/block3/unit_1/bottleneck_v1/conv1",
          "/block2/unit_4/bottleneck_v1/conv2", "/block2/unit_1/bottleneck_v1/conv1", "/block2/unit_1/bottleneck_v1/shortcut")


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


# ---- the device entry against the host entry ---------------------------------------------------------------------------------------------
#        N     n    C    B   G
SHAPES = ((1, 1, 21, 4, 1), (64, 37, 21, 16, 3), (300, 300, 81, 128, 20), (3072, 2000, 21, 128, 5), (64, 0, 21, 16, 3), (64, 9, 21, 16, 3))


def _both(dev, N, n, C, B, G, rule=0, thr=0.7, nan_row=None):
    from frcnn_hip import ops
    rois, scores, gt, cls, pred = gen.draw(np.random.RandomState(N + 7 * n + C), N, n, C, G, "plain")
    if nan_row is not None:
        cls[nan_row, 1] = np.nan
    kw = dict(batch_size=B, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.1, means=(0.0, 0.0, 0.0, 0.0), stds=(0.1, 0.1, 0.2, 0.2),
              opts=ops.roi_target_opts(False, (1.0, 1.0, 0.5, 2.0)), nms_thresh=thr, rule=rule)
    host = ops.ohem_select_host(rois, scores, n, gt, C, cls, pred, **kw)
    got = ops.ohem_select(T(rois, dev), T(scores, dev), T(np.array([n], np.int32), dev), T(gt, dev), C, T(cls, dev), T(pred, dev), **kw)
    torch.cuda.synchronize()
    return host, [t.cpu().numpy() for t in got]


@pytest.mark.parametrize("N,n,C,B,G", SHAPES)
def test_device_entry_equals_host_entry_byte_for_byte(dev, N, n, C, B, G):
    host, got = _both(dev, N, n, C, B, G)
    names = ("rois", "scores", "labels", "targets", "inside", "outside", "counts", "keep_inds", "roi_loss")
    for name, h, g in zip(names, host, got):
        assert h.dtype == g.dtype and h.shape == g.shape and h.tobytes() == g.tobytes(), name
    counts, keep = got[6], got[7]
    m = int(counts[2] + counts[3])
    if n == 0:
        assert m == 0 and np.all(keep == -1) and not got[0].any()
    else:
        assert 0 < m <= n and counts[0] + counts[1] == B and np.all((keep >= 0) & (keep < n))
        assert (len(set(keep.tolist())) == min(m, B)) or m >= B                                # fewer candidates than B: every one, repeated
    if (N, n) == (64, 9):
        assert m < B


@pytest.mark.parametrize("rule,thr,nan_row", [(1, 0.7, None), (0, 0.0, None), (0, 0.7, 11), (1, 1.0, None)])
def test_device_entry_equals_host_entry_rules_no_nms_and_nan(dev, rule, thr, nan_row):
    host, got = _both(dev, 64, 37, 21, 16, 3, rule=rule, thr=thr, nan_row=nan_row)
    for h, g in zip(host, got):
        assert h.tobytes() == g.tobytes()
    if nan_row is not None and got[8][nan_row] != 0:                                           # (a candidate: it ranks first, so it is selected)
        assert np.isnan(got[8][nan_row]) and nan_row in got[7].tolist()


def test_same_bits_on_every_run_and_labels_of_the_target_layer(dev):
    """two runs give the same bytes; labels and the dx / dy targets equal frcnn_proposal_target_layer_inject on the selected rows, the dw /
    dh targets agree with it to the few ulps between the device's logf and the header's logarithm"""
    from frcnn_hip import ops
    N, n, C, B, G = 300, 300, 21, 64, 5
    rois, scores, gt, cls, pred = gen.draw(np.random.RandomState(3), N, n, C, G, "plain")
    args = (T(rois, dev), T(scores, dev), T(np.array([n], np.int32), dev), T(gt, dev), C, T(cls, dev), T(pred, dev))
    a = [t.clone() for t in ops.ohem_select(*args, batch_size=B, bg_lo=0.1)]
    b = ops.ohem_select(*args, batch_size=B, bg_lo=0.1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    keep, n_fg = a[7], int(a[6][0].item())
    inj = ops.proposal_target_layer_inject(args[0], args[1], args[3], C, keep, n_fg)
    assert torch.equal(inj[0], a[0]) and torch.equal(inj[2], a[2]) and torch.equal(inj[4], a[4]) and torch.equal(inj[5], a[5])
    col = torch.arange(4 * C, device=dev) % 4
    assert torch.equal(inj[3][:, col < 2], a[3][:, col < 2])
    assert torch.allclose(inj[3], a[3], rtol=1e-6, atol=1e-6)


# ---- the training step -------------------------------------------------------------------------------------------------------------------
class _Cfg(object):
    """cfg keys for the duration of a test"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from model.config import cfg
        self.old = []
        for k, v in self.kw.items():
            holder = cfg.HIP if k in cfg.HIP else cfg.TRAIN
            self.old.append((holder, k, holder[k]))
            holder[k] = v

    def __exit__(self, *exc):
        for holder, k, v in self.old:
            holder[k] = v
        return False


def _blobs():
    from model.config import cfg
    rng = np.random.RandomState(2)
    image = ((rng.rand(1, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)) * np.float32(1 / 256.0)
    return image, dict(data=image, im_info=np.array([H, W, 1.0], dtype=np.float32), gt_boxes=GT)


def _host_selection(net):
    """the host entry on the read-only pass's own outputs, as the network called the device entry"""
    from frcnn_hip import ops
    from model.config import cfg
    t, o = cfg.TRAIN, net._ohem
    np_ = lambda x: x.detach().cpu().numpy()
    return ops.ohem_select_host(np_(o["proposals"]), np_(o["proposal_scores"]).ravel(), int(o["num_rois"].item()), np_(net._gt_boxes), net._num_classes,
                                np_(o["cls_score"]), np_(o["bbox_pred"]), t.BATCH_SIZE, t.FG_THRESH, t.BG_THRESH_HI, t.BG_THRESH_LO,
                                t.BBOX_NORMALIZE_MEANS, t.BBOX_NORMALIZE_STDS, ops.roi_target_opts(False, t.BBOX_INSIDE_WEIGHTS),
                                float(cfg.HIP.OHEM_NMS_THRESH), net._nms_rule())


def _check_selection(net):
    host = _host_selection(net)
    pt, o = net._proposal_targets, net._ohem
    assert np.array_equal(o["keep_inds"].cpu().numpy(), host[7]) and o["roi_loss"].cpu().numpy().tobytes() == host[8].tobytes()
    assert np.array_equal(pt["counts"].cpu().numpy(), host[6]) and pt["rois"].cpu().numpy().tobytes() == host[0].tobytes()
    assert pt["labels"].cpu().numpy().tobytes() == host[2].tobytes() and pt["bbox_targets"].cpu().numpy().tobytes() == host[3].tobytes()
    assert set(net._proposal_targets) == {"rois", "labels", "bbox_targets", "bbox_inside_weights", "bbox_outside_weights", "counts"}
    return host


@pytest.mark.parametrize("N,B", [(96, 32), (64, 64)], ids=["n96_b32", "n_equals_b"])
def test_resnet50_ohem_step_matches_torch_autograd(dev, N, B):
    """the set-up of test_full_train_step_matches_torch_autograd with the switch on; N == B: the read-only pass and the training pass have
    buffers of the same names and shapes and must not share them"""
    from dense_ref import TrainRef
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.resnet_v1 import resnetv1
    with _Cfg(OHEM=True, RPN_POST_NMS_TOP_N=N, BATCH_SIZE=B, BG_THRESH_LO=0.0):
        sess = Session(device=dev, seed=5)
        net = resnetv1(num_layers=50)
        net.create_architecture("TRAIN", 21, tag="ohem_%d_%d" % (N, B), anchor_scales=SC, anchor_ratios=RT)
        sess.init_variables(net.variable_specs())
        image, blobs = _blobs()
        losses = net.train_forward(sess, blobs)
        torch.cuda.synchronize()
        host = _check_selection(net)
        pt, at, o = net._proposal_targets, net._anchor_targets, net._ohem
        assert tuple(o["cls_score"].shape) == (N, 21) and tuple(net._predictions["cls_score"].shape) == (B, 21)
        assert o["cls_score"].data_ptr() != net._predictions["cls_score"].data_ptr()
        keep = host[7]
        assert host[6][0] + host[6][1] == B and np.all(keep >= 0)
        # the training pass on the selected rows computes what the read-only pass computed for them (frozen batch norm, no dropout)
        assert torch.allclose(net._predictions["cls_score"], o["cls_score"][torch.from_numpy(keep).long().to(dev)], rtol=1e-4, atol=1e-5)
        ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4).build()
        ts.winograd = (4, 64, True)
        ts.backward(net._loss_seeds)
        torch.cuda.synchronize()
        ref = TrainRef(sess.variables, 50, 21, SC, RT, net.trainable_scope)
        to_np = lambda d_: {k: v.cpu().numpy() for k, v in d_.items()}
        rl = ref.losses(image, pt["rois"].cpu().numpy(), to_np(at), to_np(pt))
        for k in ("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box"):
            print(k, losses[k].item(), rl[k].item())
            assert abs(losses[k].item() - rl[k].item()) <= 1e-4 * max(1.0, abs(rl[k].item())), k
        # the mean of the selected rows' losses is the step's loss: the per-RoI loss is the per-row term of _add_losses
        L = o["roi_loss"].cpu().numpy().astype(np.float64)[keep]
        total = rl["cross_entropy"].item() + rl["loss_box"].item()
        assert abs(L.mean() - total) <= 1e-4 * max(1.0, abs(total))
        sum(rl.values()).backward()
        for sc in ELEVEN:
            scope = net._scope + sc
            p = ts.params[scope]
            g = ref._cache[scope + "/weights"].grad.numpy()
            if g.ndim == 2:
                g = g[None, None]
            want = np.transpose(g, (3, 0, 1, 2))
            got = p.grad_w.cpu().numpy()
            if p.scale is not None:
                got = got * p.scale.cpu().numpy()[:, None, None, None]
            err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-12)
            print(sc, err)
            assert err <= 2e-3, (sc, err)


def _four_steps(dev, replay, tag):
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.resnet_v1 import resnetv1
    with _Cfg(OHEM=True, RPN_POST_NMS_TOP_N=96, BATCH_SIZE=32, BG_THRESH_LO=0.0, TRAIN_REPLAY=replay, TRAIN_PICK_STREAMS=0):
        sess = Session(device=dev, seed=5)
        net = resnetv1(num_layers=50)
        net.create_architecture("TRAIN", 21, tag=tag, anchor_scales=SC, anchor_ratios=RT)
        sess.init_variables(net.variable_specs())
        _, blobs = _blobs()
        ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4)
        ts.lr = 1e-3
        out = [net.train_step_async(sess, blobs, ts).clone() for _ in range(4)]
        torch.cuda.synchronize()
        _check_selection(net)                                            # the fourth step's selection, replayed or not
        filters = [ts.params[net._scope + s].w.clone() for s in ("/cls_score", "/block4/unit_2/bottleneck_v1/conv2")]
        return out, filters, dict(net.replay_stats), net._ohem["keep_inds"].clone()


def test_replayed_ohem_steps_equal_eager_ones(dev):
    a, fa, sa, ka = _four_steps(dev, True, "ohem_replay")
    b, fb, sb, kb = _four_steps(dev, False, "ohem_eager")
    assert sa["recorded"] == 1 and sa["replayed"] == 2 and sb["replayed"] == 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert all(torch.equal(x, y) for x, y in zip(fa, fb)) and torch.equal(ka, kb)
    assert not torch.equal(a[0], a[3])                                   # (the steps did change the weights)


def test_read_only_pass_reads_filters_that_followed_the_solver(dev):
    """h2 forced onto the small network: the read-only pass's launches read operand planes of the tail's filters.  After one step at a
    learning rate that moves cls_score far beyond the bound, the next read-only pass must give the float64 forward of the UPDATED weights."""
    from dense_ref import TrainRef
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.resnet_v1 import resnetv1
    with _Cfg(OHEM=True, RPN_POST_NMS_TOP_N=96, BATCH_SIZE=32, BG_THRESH_LO=0.0, H2_TRAIN=True, H2_MIN_TILES=1, H2_TRAIN_MIN_TILES=None,
              TRAIN_REPLAY=False):
        sess = Session(device=dev, seed=5)
        net = resnetv1(num_layers=50)
        net.create_architecture("TRAIN", 21, tag="ohem_stale", anchor_scales=SC, anchor_ratios=RT)
        sess.init_variables(net.variable_specs())
        image, blobs = _blobs()
        ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4)
        ts.lr = 0.01
        before = {k: np.array(v, copy=True) for k, v in sess.variables.items()}
        net.train_step(sess, blobs, ts)
        assert len(sess.h2) >= 20, "the forward pass did not take the h2 path"
        net.train_forward(sess, blobs)                                   # the next step's forward: its read-only pass sees the updated weights
        torch.cuda.synchronize()
        host = _check_selection(net)
        keep = np.unique(host[7])
        got = net._ohem["cls_score"].cpu().numpy()[keep].astype(np.float64)
        rois = net._ohem["proposals"].cpu().numpy()[keep]
        after = dict(before)
        after.update(ts.export_variables(slots=False))

        def forward(variables):
            ref = TrainRef(variables, 50, 21, SC, RT, net.trainable_scope)
            with torch.no_grad():
                fc7 = ref.train_tail(ref.head(image), rois)
                return (fc7 @ ref.w(ref.scope + "/cls_score/weights") + ref.w(ref.scope + "/cls_score/biases")).numpy()
        want, stale = forward(after), forward(before)
        bound = 1e-4 * max(1.0, np.abs(want).max())
        print("distance to the updated weights %.3g, to the pre-step weights %.3g, bound %.3g" % (np.abs(got - want).max(), np.abs(got - stale).max(), bound))
        assert np.abs(stale - want).max() >= 10 * bound                  # the step moved the scores: stale filters would be seen
        assert np.abs(got - want).max() <= bound


def test_vgg16_and_mobilenet_ohem_steps(dev):
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from nets.mobilenet_v1 import mobilenetv1
    from nets.vgg16 import vgg16
    with _Cfg(OHEM=True, RPN_POST_NMS_TOP_N=96, BATCH_SIZE=32, BG_THRESH_LO=0.0, TRAIN_REPLAY=False):
        for make, tag in ((vgg16, "ohem_vgg"), (mobilenetv1, "ohem_mob")):
            sess = Session(device=dev, seed=5)
            net = make()
            net.create_architecture("TRAIN", 21, tag=tag, anchor_scales=SC, anchor_ratios=RT)
            sess.init_variables(net.variable_specs())
            _, blobs = _blobs()
            ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4)
            ts.lr = 1e-3
            out = net.train_step(sess, blobs, ts)
            torch.cuda.synchronize()
            assert len(out) == 5 and all(np.isfinite(out)) and out[4] > sum(out[:4])
            host = _check_selection(net)
            assert host[6][0] + host[6][1] == 32
            if make is vgg16:                                            # no dropout in the read-only pass: the seed does not reach its scores
                scores = []
                for seed in (10, 20):
                    net._sample_seed = seed
                    net.train_forward(sess, blobs)
                    scores.append(net._ohem["cls_score"].clone())
                    assert len([r for r in net._tape if r["kind"] == "dropout"]) == 2          # (the training pass has its two)
                assert torch.equal(scores[0], scores[1])
