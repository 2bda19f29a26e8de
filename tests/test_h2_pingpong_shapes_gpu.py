"""The 256 x 128 ping-pong tiles of frcnn_gemm_h2 (csrc/gemm_h2.hip, cfg 21 / 34) on row counts whose last row tile is half empty or
less -- the waves whose 64 rows all lie past M skip that tile's fragment reads, MFMAs, fold and stores -- and the by-shape rule that
sends shape classes to them (run_h2: cfg -1) against the rule before those classes (cfg -9).

Every assertion is bit equality against cfg 9 on the same operands, over everything a launch writes: the float32 result, both operand
planes and the block scales.  Every output buffer is filled with a sentinel first and allocated PAD rows longer than the tensor:
what lies behind the tensor must still be the sentinel, and a row the launch did not write shows as a sentinel inside it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 64                         # rows of sentinel behind every output tensor
SENT32 = 0x7FC0BEEF              # a NaN no kernel produces (float32 result, block scales)
SENT8 = 0xA5                     # plane bytes

# (G, M, N, K): the smallest shapes that reach the half-empty tile
SHAPES = [
    (3, 300, 128, 512),          # last tile of an entry: 44 valid rows -- group 1 empty, and the second wave row of group 0
    (2, 384, 256, 512),          # exactly half full: group 1 empty, group 0 full; two column tiles
    (1, 257, 128, 128),          # one row into the second tile; one 128-k block (no fold inside the K loop)
]


@functools.lru_cache(maxsize=None)
def _operands(G, M, N, K):
    """device operands of a shape, made once and shared by its cases (never modified): x planes, packed filters, bias, residual
    as float32 and as planes"""
    from frcnn_hip import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(G * 1000003 + M * 1009 + N * 7 + K)
    x = torch.randn(G * M, K, device=dev, generator=g).clamp_(min=0) * torch.exp(torch.rand(G * M, 1, device=dev, generator=g) * 4 - 2)
    w = torch.randn(G, N, K, device=dev, generator=g) / K ** 0.5
    b = torch.randn(N, device=dev, generator=g)
    r = torch.randn(G * M, N, device=dev, generator=g).clamp_(min=0)
    return ops.h2_split(x), ops.h2_pack_w(w), b, r, ops.h2_split(r)


class _Out(object):
    """sentinel-filled output buffers of one launch, PAD rows longer than the tensors; `all` = every byte of them as int tensors"""

    def __init__(self, rows, N, dev, f32, planes):
        from frcnn_hip import ops
        self.y = self.yp = None
        self.all = []
        if f32:
            buf = torch.full(((rows + PAD) * N,), SENT32, dtype=torch.int32, device=dev)
            self.y = buf.view(torch.float32)[:rows * N].view(rows, N)
            self.all.append(buf)
            self.tails = [buf[rows * N:]]
        else:
            self.tails = []
        if planes:
            nb = 2 * rows * N * 2
            pbuf = torch.full((nb + PAD * N * 2,), SENT8, dtype=torch.uint8, device=dev)
            ibuf = torch.full(((N // 128) * rows + PAD,), SENT32, dtype=torch.int32, device=dev)
            self.yp = ops.H2(pbuf[:nb], ibuf.view(torch.float32)[:(N // 128) * rows].view(N // 128, rows), rows, N)
            self.all += [pbuf, ibuf]
            self.tails += [pbuf[nb:], ibuf[(N // 128) * rows:]]

    def tails_intact(self):
        return all(bool((t == (SENT8 if t.dtype == torch.uint8 else SENT32)).all()) for t in self.tails)

    def fully_written(self, rows, N):
        """no sentinel left inside the tensors (a plane byte may equal SENT8 by value: count whole rows of it)"""
        ok = True
        if self.y is not None:
            ok = ok and not bool((self.all[0][:rows * N] == SENT32).any())
        if self.yp is not None:
            ok = ok and not bool((self.yp.planes.view(2 * rows, N * 2) == SENT8).all(dim=1).any())
            ok = ok and not bool((self.yp.inv.view(torch.int32) == SENT32).any())
        return ok


FORMS = {
    # name: (residual, float32 out, planes out)
    "f32out": (None, True, False),
    "f32res_planes": ("f32", True, True),
    "f32res_planes_only": ("f32", False, True),
    "planesres_planes_only": ("planes", False, True),
}


def _launch(shape, form, cfg):
    from frcnn_hip import ops
    G, M, N, K = shape
    xp, wp, b, r, rp = _operands(*shape)
    res_kind, f32, planes = FORMS[form]
    res = {None: None, "f32": r, "planes": rp}[res_kind]
    out = _Out(G * M, N, xp.planes.device, f32, planes)
    # (a bias is per column of ONE filter bank: batched launches with G filter banks carry none, like the Winograd products)
    ops.gemm_h2(xp, wp, G, M, N, K, b if G == 1 else None, res, 1, out=out.y, out_planes=out.yp, want_f32=False, cfg=cfg)
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a.all) == len(b.all) and all(torch.equal(u, v) for u, v in zip(a.all, b.all))


@pytest.mark.parametrize("form", ["f32out", "f32res_planes"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_pingpong_tiles_with_a_half_empty_last_tile_equal_cfg9_bit_for_bit(dev, shape, form):
    G, M, N, K = shape
    want = _launch(shape, form, 9)
    assert want.tails_intact() and want.fully_written(G * M, N)
    for cfg in (21, 34):
        got = _launch(shape, form, cfg)
        assert got.tails_intact(), "cfg %d wrote past row G * M" % cfg
        assert _same(got, want), "cfg %d differs from cfg 9" % cfg


# the shape classes of run_h2 at reduced M, the tile-count thresholds reached through G (and N): name -> (shape, form)
CLASSES = {
    # batched float32-out products, K = 512, 258 tiles of 256 x 128, M wastes 1.3 % in 64-row wave blocks (5.1 % in 256-row tiles)
    "products_k512": ((43, 632, 256, 512), "f32out"),
    # conv3 with a float32 residual and planes out, K = 512
    "conv3_f32res_k512": ((43, 632, 256, 512), "f32res_planes_only"),
    "conv3_f32res_k512_f32too": ((43, 632, 256, 512), "f32res_planes"),
    # long K on an under-filled chip, 128 tiles of 256 x 128, K = 1024 (measured as a class, not kept: the same tile under both rules)
    "underfilled_k1024": ((32, 250, 512, 1024), "f32out"),
    # planes residual, planes only out: K = 512 leaves the deferred epilogue, K = 256 keeps it (192 tiles of 128 x 128 each)
    "conv3_planesres_k512": ((64, 300, 128, 512), "planesres_planes_only"),
    "conv3_planesres_k256": ((64, 300, 128, 256), "planesres_planes_only"),
    # ... and launches no class names: one tile short of the products' threshold, and a short-K product
    "products_252_tiles": ((42, 632, 256, 512), "f32out"),
    "products_k256": ((43, 632, 256, 256), "f32out"),
}


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_by_shape_rule_equals_the_rule_before_the_classes_bit_for_bit(dev, name):
    shape, form = CLASSES[name]
    G, M, N, K = shape
    before = _launch(shape, form, -9)
    assert before.tails_intact() and before.fully_written(G * M, N)
    got = _launch(shape, form, -1)
    assert got.tails_intact(), "cfg -1 wrote past row G * M"
    assert _same(got, before), "cfg -1 differs from cfg -9"
    assert _same(_launch(shape, form, 9), before), "cfg -9 differs from cfg 9"
