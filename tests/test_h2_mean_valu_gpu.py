"""frcnn_gemm_h2_mean (csrc/gemm_h2.hip: the tail's last conv3 + reduce_mean) held to its stated reduction order BIT FOR BIT:
the result equals mean_emulate (tests/test_h2_mean_tree_cpu.py: the 32-row block partials by the pairwise tree in row order, the
blocks of a group added in ascending order from 0.0f, times 1.0f / rows) applied to the float32 result of frcnn_gemm_h2 under cfg 9
on the same operands, one batch entry per image -- for every residual form, with and without ReLU, under every tile configuration
that carries the reduction (standalone epilogue, light boundary, 64-row tiles, deferred-epilogue ids, ping-pong, by shape).
No tolerance anywhere: every assertion is bit equality."""
import functools

import numpy as np
import pytest
import torch

from test_h2_mean_tree_cpu import mean_emulate

pytestmark = pytest.mark.gpu

CFGS = (9, 31, 33, 40, 21, -1)
# (G, R, rows, N, K): G images of R groups of `rows` rows -- the smallest shapes at which the form can go wrong
SHAPES = [
    (2, 92, 49, 2048, 512),    # 1152 tiles of 128 x 128: two to three per workgroup, a drain happens under a next tile; M tail of 28 rows
    (4, 30, 49, 256, 128),     # a tile is exactly the four slabs a drain needs; tails inside batch entries
    (1, 37, 49, 256, 128),     # one tile per workgroup: nothing to defer
    (2, 40, 32, 128, 256),     # blocks never straddle two groups: the no-second-group path only
    (1, 24, 64, 128, 128),     # a block lies inside one group of two blocks
]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _operands(shape):
    """host operands of a shape, made once and shared by its cases (never modified)"""
    G, R, rows, N, K = shape
    rng = np.random.RandomState(G * 1000 + R)
    M = R * rows
    x = np.maximum(rng.randn(G * M, K), 0).astype(np.float32)
    w = (rng.randn(N, K) / np.sqrt(K)).astype(np.float32)
    b = rng.randn(N).astype(np.float32)
    r = (rng.randn(G * M, N) * np.exp(rng.uniform(-2, 2, size=(G * M, 1)))).astype(np.float32)
    return x, w, b, r


def _mean_into_nan(ops, lib, dev, xp, wp, G, M, N, K, bias, res, act, rows, cfg):
    """one launch into a NaN-filled output, over a NaN-filled partial-sum workspace (a partial row read but not written shows)"""
    ws = ops.workspace(lib.frcnn_gemm_h2_mean_workspace_bytes(G, M, N), dev, "h2_mean")
    ws.fill_(0xFF)
    out = torch.full((G * (M // rows), N), float("nan"), dtype=torch.float32, device=dev)
    got = ops.gemm_h2_mean(xp, wp, G, M, N, K, bias, res, act, rows, out=out, cfg=cfg)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy()


@pytest.mark.parametrize("act", [1, 0], ids=["relu", "noact"])
@pytest.mark.parametrize("residual", ["planes", "f32", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_gemm_h2_mean_is_the_stated_tree_of_the_f32_result_bit_for_bit(dev, shape, residual, act):
    import frcnn_hip
    from frcnn_hip import ops
    lib = frcnn_hip.lib()
    G, R, rows, N, K = shape
    M = R * rows
    x, w, b, r = _operands(shape)
    xp, bd = ops.h2_split(T(x, dev)), T(b, dev)
    wp = ops.h2_pack_w(T(w[None], dev))                                  # the mean form shares one filter bank between the batch entries
    wpg = ops.h2_pack_w(T(np.repeat(w[None], G, axis=0), dev))           # ... frcnn_gemm_h2 takes one per entry: the same one G times
    res = {"planes": lambda: ops.h2_split(T(r, dev)), "f32": lambda: T(r, dev), "none": lambda: None}[residual]()
    y, _ = ops.gemm_h2(xp, wpg, G, M, N, K, bd, res, act, cfg=9)
    want = mean_emulate(y.cpu().numpy(), G, M, rows)
    assert want.shape == (G * R, N) and not np.isnan(want).any()
    for cfg in CFGS:
        got = _mean_into_nan(ops, lib, dev, xp, wp, G, M, N, K, bd, res, act, rows, cfg)
        assert got.shape == want.shape
        bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
        assert bad.size == 0, "cfg %d: %d of %d group rows differ, first %s" % (cfg, bad.size, G * R, bad[:8])


@pytest.mark.parametrize("cfg", [-1, 9, 33])
def test_gemm_h2_mean_with_a_planes_residual_is_slot_invariant(dev, cfg):
    """one batch entry per image: the same image (operand planes and residual planes) gives the same bits alone, in slot 0 and in
    slot 2 of a batch of three, and another image in slot 1 does not"""
    import frcnn_hip
    from frcnn_hip import ops
    lib = frcnn_hip.lib()
    R, rows, N, K = 37, 49, 256, 128
    M = R * rows
    rng = np.random.RandomState(11)
    imgs = [np.maximum(rng.randn(M, K), 0).astype(np.float32) for _ in range(2)]
    ress = [np.maximum(rng.randn(M, N), 0).astype(np.float32) for _ in range(2)]
    w = (rng.randn(N, K) / np.sqrt(K)).astype(np.float32)
    wp, bd = ops.h2_pack_w(T(w[None], dev)), T(rng.randn(N).astype(np.float32), dev)

    def run(order):
        xp = ops.h2_split(T(np.concatenate([imgs[i] for i in order], axis=0), dev))
        rp = ops.h2_split(T(np.concatenate([ress[i] for i in order], axis=0), dev))
        return _mean_into_nan(ops, lib, dev, xp, wp, len(order), M, N, K, bd, rp, 1, rows, cfg)
    one, three = run([0]), run([0, 1, 0])
    assert not np.isnan(three).any()
    assert np.array_equal(_bits(three[:R]), _bits(one)) and np.array_equal(_bits(three[2 * R:]), _bits(one))
    assert not np.array_equal(_bits(three[R:2 * R]), _bits(one))
