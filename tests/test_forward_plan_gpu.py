"""The stand-ins of tests/test_forward_plan_cpu.py against the real session: a TEST-mode ResNet-50 forward on one 320 x 320 image (the
smallest shape at which block1's launches still cross the 150-tile threshold through PLAN_IMAGES) makes, mark for mark, the launches
the CPU harness plans for the same shape and switches; and a switch the plan reads (cfg.HIP.WINOGRAD_FUSED_F2) toggled on a live
session gets a captured graph of its own."""
import numpy as np
import pytest
import torch

import test_forward_plan_cpu as harness

pytestmark = pytest.mark.gpu
H = W = 320
POST = 48


def _session(dev, tag):
    from frcnn_hip.runtime import Session
    from model.config import cfg
    from nets.resnet_v1 import resnetv1
    sess = Session(device=dev, seed=7)
    net = resnetv1(num_layers=50)
    net.create_architecture("TEST", 21, tag=tag)
    sess.init_variables(net.variable_specs())
    image = (np.random.RandomState(8).rand(1, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)
    return sess, net, image, np.array([H, W, 1.0], dtype=np.float32)


@pytest.mark.parametrize("h2", [True, False])
def test_the_real_session_makes_the_marks_the_cpu_harness_plans(dev, h2):
    from model.config import cfg
    switches = {"HIP.MFMA_H2": h2, "TEST.RPN_POST_NMS_TOP_N": POST}
    want = harness.tags(harness.plan_trace("res50", hw=(H, W), switches=switches))
    keep = (cfg.HIP.MFMA_H2, cfg.TEST.RPN_POST_NMS_TOP_N)
    cfg.HIP.MFMA_H2, cfg.TEST.RPN_POST_NMS_TOP_N = h2, POST
    try:
        sess, net, image, im_info = _session(dev, "plan_h2" if h2 else "plan_x3")
        sess.profile = []
        net.forward_device(sess, net._stage_image(sess, image), im_info, use_graph=False)
        torch.cuda.synchronize()
        got = [t[0] for t in sess.profile]
        sess.profile = None
        sess.close()
    finally:
        cfg.HIP.MFMA_H2, cfg.TEST.RPN_POST_NMS_TOP_N = keep
    assert len(want) > 80 and any(t.startswith("conv:h2:") for t in want) == h2
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, got[max(0, i - 2):i + 2], want[max(0, i - 2):i + 2])
    assert len(got) == len(want)


def test_a_plan_switch_toggled_on_a_live_session_gets_its_own_graph(dev):
    from model.config import cfg
    keep = (cfg.HIP.WINOGRAD_FUSED_F2, cfg.TEST.RPN_POST_NMS_TOP_N)
    cfg.TEST.RPN_POST_NMS_TOP_N = POST
    try:
        sess, net, image, im_info = _session(dev, "toggle")
        img = net._stage_image(sess, image)
        keys, outs = [], []
        for fused in (True, False):
            cfg.HIP.WINOGRAD_FUSED_F2 = fused
            p = net.forward_device(sess, img, im_info)
            torch.cuda.synchronize()
            keys.append(net.graph_key(img.shape, net._im_info))
            assert keys[-1] in sess.graphs and sum(1 for k in sess.graphs if k in keys) == len(keys)
            assert net._plan.winograd_fused_f2 == fused          # the build the graph was captured from read this setting
            outs.append({k: p[k].cpu().numpy().copy() for k in ("rois", "cls_prob", "bbox_pred")})
        assert keys[0] != keys[1] and sess.graphs[keys[0]].graph is not sess.graphs[keys[1]].graph
        for k in outs[0]:                                        # (the fused launch gives the bits of the three launches it replaces)
            assert np.array_equal(outs[0][k].view(np.int32), outs[1][k].view(np.int32)), k
        sess.close()
    finally:
        cfg.HIP.WINOGRAD_FUSED_F2, cfg.TEST.RPN_POST_NMS_TOP_N = keep
