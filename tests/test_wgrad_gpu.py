"""GPU: frcnn_conv2d_wgrad (csrc/wgrad_tn.hip, f32 matrix pipe) and frcnn_conv2d_wgrad_h2 (csrc/wgrad_h2.hip, two-piece fp16 operands
split in registers) -- the filter gradient of slim.conv2d read straight from dY and X in NHWC -- against
torch's float64 autograd of the same convolution, over the layer kinds of the three backbones' reverse sweeps (pointwise, strided
shortcut, 3x3 SAME, 3x3 stride 2 with conv2d_same's explicit padding, the RoI tail's 7x7 maps, a fully connected layer as a 1x1
convolution), both tile sizes, one slice and many, and a pixel count that is not a multiple of the 32-pixel slab."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [
    # N, H, W, Cin, Cout, k, stride, pad (top, bottom, left, right)
    ("pointwise", 1, 38, 63, 256, 128, 1, 1, (0, 0, 0, 0)),
    ("shortcut_s2", 1, 38, 63, 128, 256, 1, 2, (0, 0, 0, 0)),
    ("same3x3", 1, 20, 30, 64, 64, 3, 1, (1, 1, 1, 1)),
    ("same3x3_s2", 1, 21, 31, 128, 128, 3, 2, (0, 1, 0, 1)),
    ("roi_tail", 40, 7, 7, 128, 256, 3, 1, (1, 1, 1, 1)),
    ("fc_as_1x1", 96, 1, 1, 1024, 192, 1, 1, (0, 0, 0, 0)),
    ("rpn3x3", 1, 38, 63, 256, 512, 3, 1, (1, 1, 1, 1)),
]


def _reference(x, gy, Cout, k, stride, pad):
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    w = torch.zeros((Cout, x.shape[-1], k, k), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, (pad[2], pad[3], pad[0], pad[1])), w, stride=stride)
    y.backward(torch.from_numpy(gy).double().permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).contiguous().numpy()                 # [Cout, KH, KW, Cin]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("plan", [(0, 0), (64, 1), (128, 4096)], ids=["auto", "t64_one_slice", "t128_many_slices"])
@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
def test_conv2d_wgrad_vs_float64_autograd(dev, case, plan, h2):
    from frcnn_hip import lib, ops
    _, N, H, W, Cin, Cout, k, stride, pad = case
    OH = (H + pad[0] + pad[1] - k) // stride + 1
    OW = (W + pad[2] + pad[3] - k) // stride + 1
    rng = np.random.RandomState(Cin + Cout + k)
    x = np.maximum(rng.randn(N, H, W, Cin), 0).astype(np.float32)                       # post-ReLU activations
    gy = (rng.randn(N, OH, OW, Cout) * (rng.rand(N, OH, OW, Cout) < 0.4)).astype(np.float32)  # gated gradients
    ref = _reference(x, gy, Cout, k, stride, pad)
    assert ops.conv2d_wgrad_supported(Cin, Cout) and not ops.conv2d_wgrad_supported(Cin, 21) and not ops.conv2d_wgrad_supported(3, Cout)
    out = torch.full((Cout, k, k, Cin), float("nan"), dtype=torch.float32, device=dev)
    setter = lib().frcnn_conv2d_wgrad_h2_set_plan if h2 else lib().frcnn_conv2d_wgrad_set_plan
    setter(*plan)
    try:
        ops.conv2d_wgrad(torch.from_numpy(gy).to(dev), torch.from_numpy(x).to(dev), k, k, stride, pad, out, h2=h2)
        torch.cuda.synchronize()
    finally:
        setter(0, 0)
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("wgrad %s %s plan %s: max err / max |dW| = %.2e" % ("h2 " if h2 else "f32", case[0], plan, err))
    assert np.isfinite(got).all() and err <= 2e-6, err


def test_conv2d_wgrad_refuses_what_it_does_not_cover(dev):
    from frcnn_hip import FrcnnHipError, ops
    gy = torch.zeros((1, 8, 8, 21), dtype=torch.float32, device=dev)
    x = torch.zeros((1, 8, 8, 64), dtype=torch.float32, device=dev)
    out = torch.zeros((21, 1, 1, 64), dtype=torch.float32, device=dev)
    with pytest.raises(FrcnnHipError):
        ops.conv2d_wgrad(gy, x, 1, 1, 1, (0, 0, 0, 0), out)


def _block4_operands(R_, Cin, Cout, seed):
    """the shipped block4 conv3's operands: dY = spatial_mean_bwd of a per-RoI gradient (constant over each RoI's 49 pixels), RoIs of
    magnitudes 2^-8 .. 2^8 (fg vs bg), gated by the ReLU mask of conv3's output; X post-ReLU with a few outlier channels"""
    rng = np.random.RandomState(seed)
    g = rng.randn(R_, 1, 1, Cout) * 2.0 ** rng.randint(-8, 9, size=(R_, 1, 1, 1)) / 49.0
    gy = (np.broadcast_to(g, (R_, 7, 7, Cout)) * (rng.rand(R_, 7, 7, Cout) < 0.5)).astype(np.float32)
    x = np.maximum(rng.randn(R_, 7, 7, Cin), 0)
    x[..., rng.choice(Cin, size=8, replace=False)] *= 64.0
    return gy, x.astype(np.float32)


@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
def test_conv2d_wgrad_block4_conv3_structured_operands(dev, h2):
    """block4/unit_3 conv3 as shipped (M = 256 RoIs x 49, Cin 512, Cout 2048, 1x1) on block4-tail operands: the 2e-6 bound of the
    cases above; elementwise |got - want| <= 16 2^-23 B (B = the float64 product of |dY| and |X|); and for h2 the f32 class against
    the f32 TN kernel on the same data (error / 2^-23 B at most 3x, plus a floor of 1e-7 of the scale).  k_wgrad_h2 scales each
    (channel, 64-pixel slab) block of dY, and a slab spans two RoIs whose magnitudes differ by up to 2^16."""
    import dgrad_ref as R
    from frcnn_hip import ops
    R_, Cin, Cout = 256, 512, 2048
    gy, x = _block4_operands(R_, Cin, Cout, 11)
    pad = (0, 0, 0, 0)
    want = R.wgrad64(gy, x, 1, 1, 1, pad)
    B = R.wgrad64(np.abs(gy), x, 1, 1, 1, pad)
    got = {}
    for hh in ((False, True) if h2 else (False,)):
        out = torch.full((Cout, 1, 1, Cin), float("nan"), dtype=torch.float32, device=dev)
        ops.conv2d_wgrad(torch.from_numpy(gy).to(dev), torch.from_numpy(x).to(dev), 1, 1, 1, pad, out, h2=hh)
        torch.cuda.synchronize()
        got[hh] = out.cpu().numpy().astype(np.float64)
    g = got[h2]
    err = np.abs(g - want).max() / np.abs(want).max()
    r = R.ratio(g, want, B)
    line = "wgrad %s block4 conv3 structured: max err / max |dW| = %.2e, max |err| / (2^-23 B) = %.3f" % ("h2 " if h2 else "f32", err, r)
    if h2:
        r32 = R.ratio(got[False], want, B)
        e32 = np.abs(got[False] - want).max() / np.abs(want).max()
        line += "; f32 TN %.3f (max-rel %.2e), h2 / f32 = %.2f" % (r32, e32, r / max(r32, 1e-30))
    print(line)
    assert np.isfinite(g).all() and err <= 2e-6, err
    assert r <= 16.0, r
    if h2:
        assert r <= 3.0 * r32 + 1e-7 / R.EPS, (r, r32)
