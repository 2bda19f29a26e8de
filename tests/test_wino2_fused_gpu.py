"""frcnn_winograd2_conv_x3 (csrc/winograd2_fused.hip): F(2x2,3x3), 64 -> 64 channels, input transform + 16 products + output transform
in one launch, against the three launches it replaces -- ops.winograd_input_transform -> ops.gemm_x3 (G = 16) ->
ops.winograd_output_transform on the same operands.  Every assertion is bit equality (compared as int32).

Outputs are filled with a sentinel first and allocated PAD pixel rows longer than the tensor: what lies behind the tensor must still
be the sentinel, and a pixel the launch did not write shows as a sentinel inside it.  A workgroup owns a run of 64 consecutive tiles
in (img, ty, tx) order; the shapes are the smallest that reach each way that can go wrong."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 64                         # pixels of sentinel behind every output tensor
SENT32 = 0x7FC0BEEF              # a NaN no kernel produces
C = 64

SHAPES = [
    (1, 4, 4),                   # 4 tiles: one partial workgroup, every tile touches the padding
    (1, 5, 7),                   # odd H and W: the last tile row and column are half outside the image
    (3, 9, 11),                  # 90 tiles: an image boundary inside a workgroup's run, and a partial last workgroup
    (2, 16, 16),                 # 128 tiles: exactly two full runs
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _operands(N, H, W):
    """device operands of a shape, made once and shared by its cases (never modified): x, the packed filter planes, a bias"""
    from frcnn_hip import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(N * 1000003 + H * 1009 + W)
    x = torch.randn(N, H, W, C, device=dev, generator=g).clamp_(min=0) * torch.exp(torch.rand(N, H, W, 1, device=dev, generator=g) * 4 - 2)
    w = (torch.randn(3, 3, C, C, device=dev, generator=g) / 24).cpu().numpy()
    u = torch.from_numpy(ops.winograd_filter_transform(w, m=2)).to(dev)
    b = torch.randn(C, device=dev, generator=g)
    return x.contiguous(), ops.gemm_x3_pack(u), b


def _out(N, H, W, dev):
    buf = torch.full(((N * H * W + PAD) * C,), SENT32, dtype=torch.int32, device=dev)
    return buf, buf.view(torch.float32)[:N * H * W * C].view(N, H, W, C)


def _intact_and_full(buf, N, H, W):
    n = N * H * W * C
    return bool((buf[n:] == SENT32).all()) and not bool((buf[:n] == SENT32).any())


def _fused(x, planes, bias, act):
    from frcnn_hip import ops
    N, H, W, _ = x.shape
    buf, y = _out(N, H, W, x.device)
    ops.winograd2_conv_x3(x, planes, bias, act, y)
    torch.cuda.synchronize()
    return buf


@functools.lru_cache(maxsize=None)
def _three_launches(shape, act, with_bias):
    """the reference of a case, computed once"""
    from frcnn_hip import ops
    N, H, W = shape
    x, planes, b = _operands(*shape)
    T = ops.winograd_tiles(N, H, W, 2)
    v = torch.empty(16, T, C, device=x.device)
    ops.winograd_input_transform(x, v, 2)
    mm = ops.gemm_x3(v, planes, 16, T, C, C)
    buf, y = _out(N, H, W, x.device)
    ops.winograd_output_transform(mm, b if with_bias else None, act, y, 2)
    torch.cuda.synchronize()
    assert _intact_and_full(buf, N, H, W)
    return buf


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_launch_equals_the_three_launches_bit_for_bit(dev, shape, act, with_bias):
    N, H, W = shape
    x, planes, b = _operands(*shape)
    want = _three_launches(shape, act, with_bias)
    got = _fused(x, planes, b if with_bias else None, act)
    assert _intact_and_full(got, N, H, W), "wrote behind the tensor or left a pixel unwritten"
    assert torch.equal(got, want)
    if act == 1:
        assert bool((got.view(torch.float32)[:N * H * W * C] >= 0).all())
    assert float(got.view(torch.float32)[:N * H * W * C].abs().max()) > 0


def test_an_image_inside_a_batch_equals_the_image_alone(dev):
    """image 1 of the N = 3 case starts and ends inside workgroups' runs"""
    N, H, W = 3, 9, 11
    x, planes, b = _operands(N, H, W)
    batch = _fused(x, planes, b, 1)[:N * H * W * C].view(N, H * W * C)
    alone = _fused(x[1:2].contiguous(), planes, b, 1)
    assert _intact_and_full(alone, 1, H, W)
    assert torch.equal(alone[:H * W * C], batch[1])


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=[IDS[2], IDS[3]])
def test_two_runs_give_equal_bits(dev, shape):
    x, planes, b = _operands(*shape)
    assert torch.equal(_fused(x, planes, b, 1), _fused(x, planes, b, 1))
