"""GPU: the IoU-family box regression losses (cfg.HIP.BBOX_LOSS / RPN_BBOX_LOSS; csrc/iouloss_math.h, csrc/iou_loss.hip).  The device entry
on every golden case and kind against the float64 statement at 2 float32 ulps (the bound tests/test_iou_loss_cpu.py holds the host entry
to, for the reason fixtures/gen_golden_iou_loss.py gives) and against the host entry byte for byte; then toy training steps with the keys
set: a replayed run equals an eager one bit for bit, the step's two regression losses are the host entry's on the step's own tensors, and
with the default keys they are ops.smooth_l1_loss's."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import gen_golden_iou_loss as gen  # noqa: E402
import iou_loss_ref as ref  # noqa: E402

CASES = tuple(c[0] for c in gen.DRAWN) + gen.HAND
KINDS = ref.KINDS
SC, RT = (4, 8, 16), (0.5, 1, 2)
GT = np.array([[16, 16, 79, 79, 3], [60, 30, 150, 110, 7], [5, 70, 60, 120, 12]], dtype=np.float32)
H, W = 128, 160


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(gen.GOLD))


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device(g, case, kind, dev):
    from frcnn_hip import ops
    a = [g[case + "/" + k] for k in ("pred", "targets", "inside", "outside", "refs")]
    rest = (g[case + "/means"], g[case + "/stds"], kind, g[case + "/weight"], g[case + "/divisor"], int(g[case + "/K"]))
    loss, grad = ops.iou_loss(*[T(x, dev) for x in a], *rest)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), grad.cpu().numpy()), ops.iou_loss_host(*a, *rest)


@pytest.mark.parametrize("case", CASES)
def test_device_entry_against_the_statement_and_the_host_entry(dev, gold, case):
    for kind in KINDS:
        (loss, grad), (hloss, hgrad) = _device(gold, case, kind, dev)
        p = case + "/" + kind + "/"
        dg, dl = ref.ulps(grad, gold[p + "grad"]), ref.ulps(loss, gold[p + "loss"])
        print("%s %s: largest distance gradient %d ulp, loss %d ulp" % (case, kind, int(dg.max()), int(dl.max())))
        assert dg.max() <= 2 and dl.max() <= 2
        assert grad.dtype == hgrad.dtype and grad.shape == hgrad.shape and grad.tobytes() == hgrad.tobytes(), kind
        assert loss.tobytes() == hloss.tobytes(), kind


def test_two_runs_give_identical_bits_and_every_element_is_written(dev, gold):
    from frcnn_hip import ops
    case = "head_70x21"
    a = [T(gold[case + "/" + k], dev) for k in ("pred", "targets", "inside", "outside", "refs")]
    rest = (gold[case + "/means"], gold[case + "/stds"], "ciou", 2.0, 70.0, 21)
    first = [t.clone() for t in ops.iou_loss(*a, *rest)]
    torch.empty_like(first[1]).fill_(float("nan"))                       # (whatever the allocator hands out next: the op must write all of it)
    second = ops.iou_loss(*a, *rest)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert bool(torch.isfinite(second[1]).all()) and int((second[1].view(-1, 4) != 0).any(dim=1).sum()) == int((a[2].view(-1, 4) != 0).any(dim=1).sum())


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


def _nets():
    from nets.resnet_v1 import resnetv1
    from nets.vgg16 import vgg16
    return {"res50": lambda: resnetv1(num_layers=50), "vgg16": vgg16}


def _steps(dev, arch, tag, n, **keys):
    """n training steps of the toy network; -> the [5] losses of each, the network, and two filters after the last step"""
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from model.config import cfg
    with _Cfg(BATCH_SIZE=64, BG_THRESH_LO=0.0, TRAIN_PICK_STREAMS=0, **keys):
        sess = Session(device=dev, seed=5)
        net = _nets()[arch]()
        net.create_architecture("TRAIN", 21, tag=tag, anchor_scales=SC, anchor_ratios=RT)
        sess.init_variables(net.variable_specs())
        rng = np.random.RandomState(2)
        image = ((rng.rand(1, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)) * np.float32(1 / 256.0)
        blobs = dict(data=image, im_info=np.array([H, W, 1.0], dtype=np.float32), gt_boxes=GT)
        ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4)
        ts.lr = 1e-3
        out = [net.train_step_async(sess, blobs, ts).clone() for _ in range(n)]
        torch.cuda.synchronize()
        filters = [ts.params[net._scope + s].w.clone() for s in ("/cls_score", "/bbox_pred", "/rpn_bbox_pred")]
        return out, net, filters


def _host_losses(net, head_kind, rpn_kind, head_w=1.0, rpn_w=1.0):
    """ops.iou_loss_host on the step's own read-back tensors, as Network._add_losses called the device entry"""
    from frcnn_hip import ops
    from model.config import cfg
    np_ = lambda x: x.detach().cpu().numpy()
    p, at, pt = net._predictions, net._anchor_targets, net._proposal_targets
    rpn = ops.iou_loss_host(np_(p["rpn_bbox_pred"]), np_(at["rpn_bbox_targets"]), np_(at["rpn_bbox_inside_weights"]),
                            np_(at["rpn_bbox_outside_weights"]), np_(net._rpn_anchors), (0, 0, 0, 0), (1, 1, 1, 1), rpn_kind, rpn_w, 1.0, 1)
    rows = p["bbox_pred"].shape[0]
    head = ops.iou_loss_host(np_(p["bbox_pred"]), np_(pt["bbox_targets"]), np_(pt["bbox_inside_weights"]), np_(pt["bbox_outside_weights"]),
                             np_(pt["rois"]), cfg.TRAIN.BBOX_NORMALIZE_MEANS, cfg.TRAIN.BBOX_NORMALIZE_STDS, head_kind, head_w, float(rows),
                             net._num_classes)
    return rpn, head


@pytest.mark.parametrize("arch", ["res50", "vgg16"])
def test_toy_step_with_giou_and_diou(dev, arch):
    keys = dict(BBOX_LOSS="giou", RPN_BBOX_LOSS="diou", BBOX_LOSS_WEIGHT=2.0, RPN_BBOX_LOSS_WEIGHT=0.5)
    a, net, fa = _steps(dev, arch, "iou_replay_" + arch, 4, TRAIN_REPLAY=True, **keys)
    b, net_b, fb = _steps(dev, arch, "iou_eager_" + arch, 4, TRAIN_REPLAY=False, **keys)
    assert net.replay_stats["recorded"] == 1 and net.replay_stats["replayed"] == 2 and net_b.replay_stats["replayed"] == 0
    for x, y in zip(a, b):                                               # the replayed step equals the eager step bit for bit
        assert torch.equal(x, y)
    assert all(torch.equal(x, y) for x, y in zip(fa, fb)) and not torch.equal(a[0], a[3])
    # the fourth step's regression losses (replayed in `net`, eager in `net_b`) are the host entry's on the step's own tensors
    for n_, out in ((net, a[3]), (net_b, b[3])):
        rpn, head = _host_losses(n_, "giou", "diou", 2.0, 0.5)
        got = out.cpu().numpy()
        print(arch, "rpn_loss_box", got[1], rpn[0][0], "loss_box", got[3], head[0][0])
        assert got[1:2].tobytes() == rpn[0].tobytes() and got[3:4].tobytes() == head[0].tobytes()
        assert n_._losses["loss_box"].cpu().numpy().tobytes() == head[0].tobytes()
        assert rpn[0][0] > 0 and head[0][0] > 0 and np.isfinite(got).all()
        active = (n_._proposal_targets["bbox_inside_weights"].view(-1, 4) != 0).any(dim=1)
        assert 0 < int(active.sum()) <= 64 and tuple(n_._rpn_anchors.shape) == (n_._predictions["rpn_bbox_pred"].numel() // 4, 4)
    # the total is the sum of its parts: the regularisation term of the first step depends on the initial weights alone, so it is the
    # default run's; four float32 additions on each side, each off by at most 2^-24 of the total
    c, net_c, _ = _steps(dev, arch, "iou_default_" + arch, 1, TRAIN_REPLAY=False)
    x, y = a[0].cpu().numpy().astype(np.float64), c[0].cpu().numpy().astype(np.float64)
    reg_x, reg_y = x[4] - x[:4].sum(), y[4] - y[:4].sum()
    print(arch, "regularisation", reg_x, reg_y)
    assert reg_x > 0 and abs(reg_x - reg_y) <= 8 * 2.0 ** -24 * max(x[4], y[4])
    assert x[0] == y[0] and x[2] == y[2] and x[1] != y[1] and x[3] != y[3]       # the classification losses of the first step do not move


def test_default_keys_are_smooth_l1_bit_for_bit(dev):
    from frcnn_hip import ops
    out, net, _ = _steps(dev, "res50", "iou_off", 2, TRAIN_REPLAY=False)
    assert net._rpn_anchors is None
    p, at, pt = net._predictions, net._anchor_targets, net._proposal_targets
    rpn, _ = ops.smooth_l1_loss(p["rpn_bbox_pred"], at["rpn_bbox_targets"], at["rpn_bbox_inside_weights"], at["rpn_bbox_outside_weights"], 3.0, 1.0)
    head, _ = ops.smooth_l1_loss(p["bbox_pred"], pt["bbox_targets"], pt["bbox_inside_weights"], pt["bbox_outside_weights"], 1.0,
                                 float(p["bbox_pred"].shape[0]))
    torch.cuda.synchronize()
    assert torch.equal(out[1][1:2], rpn) and torch.equal(out[1][3:4], head) and float(rpn) > 0 and float(head) > 0
