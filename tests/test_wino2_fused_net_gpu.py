"""cfg.HIP.WINOGRAD_FUSED_F2 in the network: a TEST-mode ResNet-101 forward on one 320 x 320 image (block1 is 80 x 80: 1 600 tiles,
so its stride-1 conv2 layers are x3-eligible) with the switch on and off gives the same bits, and with the switch on the two layers
run as one launch each -- no input or output transform beside their `conv:x3:` mark."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SCALES, RATIOS = (4, 8, 16), (0.5, 1, 2)
FUSED_SCOPES = ("block1/unit_1/bottleneck_v1/conv2", "block1/unit_2/bottleneck_v1/conv2")


def _forward(dev, fused):
    from frcnn_hip.runtime import Session
    from model.config import cfg
    from nets.resnet_v1 import resnetv1
    keep = (cfg.HIP.WINOGRAD_FUSED_F2, cfg.TEST.RPN_POST_NMS_TOP_N)
    cfg.HIP.WINOGRAD_FUSED_F2, cfg.TEST.RPN_POST_NMS_TOP_N = fused, 48
    try:
        sess = Session(device=dev, seed=7)
        net = resnetv1(num_layers=101)
        net.create_architecture("TEST", 21, tag="fused" if fused else "unfused", anchor_scales=SCALES, anchor_ratios=RATIOS)
        sess.init_variables(net.variable_specs())
        rng = np.random.RandomState(8)
        H = W = 320
        image = (rng.rand(1, H, W, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)
        im_info = np.array([H, W, 1.0], dtype=np.float32)
        _, cls_prob, bbox_pred, rois = net.test_image(sess, image, im_info)
        out = {"rois": np.array(rois), "cls_prob": np.array(cls_prob), "bbox_pred": np.array(bbox_pred)}
        sess.profile = []
        net.forward_device(sess, net._stage_image(sess, image), im_info)
        torch.cuda.synchronize()
        tags = [t[0] for t in sess.profile]
        sess.profile = None
        sess.close()
        return out, tags
    finally:
        cfg.HIP.WINOGRAD_FUSED_F2, cfg.TEST.RPN_POST_NMS_TOP_N = keep


def test_switch_on_and_off_give_the_same_bits_and_the_fused_layers_run_alone(dev):
    on, tags_on = _forward(dev, True)
    off, tags_off = _forward(dev, False)
    for name in ("rois", "cls_prob", "bbox_pred"):
        assert on[name].shape == off[name].shape and on[name].dtype == np.float32
        assert np.array_equal(on[name].view(np.int32), off[name].view(np.int32)), name
    assert on["rois"].shape[0] > 0
    for tags, fused in ((tags_on, True), (tags_off, False)):
        for scope in FUSED_SCOPES:
            at = [i for i, t in enumerate(tags) if t.startswith("conv:x3:") and t.endswith(scope)]
            assert len(at) == 1, (scope, fused)                 # the layer is x3-eligible at this size, under either setting
            i = at[0]
            assert (tags[i - 1] == "op:wino_in") == (not fused), (scope, fused)
            assert (tags[i + 1] == "op:wino_out") == (not fused), (scope, fused)
    # nothing else moved: the other Winograd layers keep their transforms
    assert tags_off.count("op:wino_in") - tags_on.count("op:wino_in") == 2
    assert tags_off.count("op:wino_out") - tags_on.count("op:wino_out") == 2
    assert [t for t in tags_on if not t.startswith("op:wino_")] == [t for t in tags_off if not t.startswith("op:wino_")]
