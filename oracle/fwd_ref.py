"""TEST INFRASTRUCTURE ONLY -- float64 statements of the forward convolutions (csrc/conv_igemm.hip, gemm_h2.hip, gemm_x3.hip, winograd*.hip,
k_dwconv3x3 of dense_misc.hip) and the elementwise error bound the op-level tests hold them to, in the manner of oracle/dgrad_ref.py:

    |got - want| <= c * 2^-23 * B,    B = the same float64 operation on |x|, |W|, |bias| (+ |residual|), no activation

so one missing border tap, or a wrong value in an output of small magnitude, fails it -- the max-norm checks of tests/test_dense_gpu.py
and tests/test_h2_gpu.py (2e-5 or 1e-4 of max |y|) do not see either.  The Winograd routes' rounding lives in their transforms and is
shared by the m x m outputs of a tile: their B is the tile's maximum (dgrad_ref.tile_max).  B is floored at the smallest normal float32
wherever anything was summed (wgrad_ref._normal): x holds 1.18e-38, whose products are subnormal.

CASES lists every route's shapes; each runs on two operand kinds (operands()).  tests/test_fwd_gpu.py runs them on the device,
tests/test_fwd_bounds_cpu.py proves for each of them that the route's c passes a float32 statement of the same convolution with half the
room to spare and rejects every reference of perturbed().

Left out, because an existing test pins them bit for bit to a form that is covered here:
  * the streaming-GEMM configurations (k_gemm_stream, ids 100 ..): test_streaming_gemm_configurations_bit_identical_to_igemm pins each to
    the k_conv_igemm configuration of the route 'direct_cfg';
  * the fused F(2,3) launch (frcnn_winograd2_conv_x3): tests/test_wino2_fused_gpu.py pins it to the chain of the route 'wino_x3';
  * gemm_h2's cfgs 30-34 and 40 / 41, the ping-pong and deferred forms: tests/test_h2_gpu.py and tests/test_h2_pingpong_shapes_gpu.py pin them
    to cfg 9 / 12 / 21 of the route 'h2'."""
import collections
import functools

import numpy as np
import torch

import dgrad_ref
from dgrad_ref import EPS, SAME3, ZERO, conv_out, ratio, tile_max  # noqa: F401  (re-exported to the tests)
from wgrad_ref import _normal

# One case: the geometry of dgrad_ref.CASES (H, W: the input), then what the launch fuses -- bias (bool), act (0 none, 1 ReLU, 2 ReLU6),
# res (0: none, else the residual's res_stride) -- and m, the Winograd scheme of the routes that do not carry it in their name.
Case = collections.namedtuple("Case", "id N H W Cin Cout k stride pad bias act res m")


def _c(id_, N, H, W, Cin, Cout, k=3, stride=1, pad=SAME3, bias=True, act=1, res=0, m=None):
    return Case(id_, N, H, W, Cin, Cout, k, stride, pad, bias, act, res, m)


def _from_dgrad(route, prefix="", **kw):
    return [_c(prefix + c[0], *c[1:], **kw) for c in dgrad_ref.CASES[route]]


# route -> cases.  The routes and the call each one makes are in tests/test_fwd_gpu.py (launch_*).
CASES = {
    # ops.conv2d under the automatic plan
    "direct": _from_dgrad("flipped") + [
        _c("valid_9x11", 2, 9, 11, 96, 160, 3, 1, ZERO),                       # VALID, batch 2, Cin = 3 slabs
        _c("same_s2_37x63", 1, 37, 63, 64, 32, 3, 2, SAME3, bias=False, act=0),  # conv2d_same at stride 2, odd size: -> 19x32
        _c("same_s2_34x51", 1, 34, 51, 64, 64, 3, 2, SAME3),                   # ... even x odd: the bottom pad row is never read
        _c("tfsame_s2_34x51", 1, 34, 51, 32, 64, 3, 2, (0, 1, 0, 1), act=2),   # TF SAME at an even size: asymmetric pad
        _c("shortcut_s2_34x51", 1, 34, 51, 64, 128, 1, 2, ZERO, act=0),        # strided shortcut: row 33 and column 50 are never read
        _c("res1_17x26", 1, 17, 26, 256, 64, 1, 1, ZERO, res=1),               # residual + ReLU in the tile epilogue
        _c("res2_20x24", 1, 20, 24, 32, 128, 3, 2, SAME3, res=2),              # residual subsampled at stride 2
    ] + _from_dgrad("padded", act=0) + [                                       # heads whose Cout is no tile multiple
        _c("relu6_c20", 1, 13, 17, 32, 20, 3, 1, SAME3, act=2),                # Cout <= 32 tiles
    ],
    # the same call with frcnn_set_tuning(0, id) for id in DIRECT_CFGS
    "direct_cfg": [
        _c("tail27_37x63", 1, 37, 63, 64, 128, 3, 1, SAME3),                   # M = 2331 leaves a 27-row tail in 128-row tiles
        _c("roi37_res", 37, 7, 7, 128, 256, 1, 1, ZERO, res=1),
    ],
    # ops.conv2d where the plan splits K: bias + residual + ReLU run in k_splitk_finish
    "splitk": [
        _c("splitk_1x1_k512", 1, 9, 13, 512, 64, 1, 1, ZERO, res=1),           # 16 slabs in 2 chunks
        _c("splitk_3x3_c128", 1, 9, 13, 128, 64, 3, 1, SAME3, res=1),          # 36 slabs in chunks of 9: a split starts inside a tap
    ],
    # ops.conv2d(fold_w=True): 7x7 / 2 on an image padded to 4 channels
    "stem": [
        _c("stem_21x29", 1, 21, 29, 4, 64, 7, 2, (3, 3, 3, 3)),
        _c("stem_22x30", 1, 22, 30, 4, 64, 7, 2, (3, 3, 3, 3)),
    ],
    # ops.conv3x3_winograd, f32 products
    "wino2": [
        _c("37x63_m2", 1, 37, 63, 64, 64),
        _c("1x9_m2", 1, 1, 9, 64, 64),
        _c("8x10_c20_m2", 2, 8, 10, 32, 20, bias=False, act=0),
        _c("pixel_m2", 3, 1, 1, 64, 36),                                       # every tap but the centre is padding
    ],
    "wino4": [c for c in _from_dgrad("winograd") if c.id.endswith("_m4")] + [_c("pixel_m4", 3, 1, 1, 64, 36)],
    "wino7": [c for c in _from_dgrad("winograd") if c.id.endswith("_m7")],     # (7x7 maps only: no single-pixel form)
    # ops.conv3x3_winograd(u_planes=h2_pack_w(u)): winograd_input_transform_h2 -> gemm_h2 -> output transform
    "wino_h2": [
        _c("h2p_37x63_m4", 1, 37, 63, 128, 128, m=4),
        _c("h2p_34x51_m4", 1, 34, 51, 256, 128, m=4),
        _c("h2p_roi37_m7", 37, 7, 7, 256, 256, m=7),
        _c("h2p_roi1_m7", 1, 7, 7, 128, 128, m=7),
    ],
    # winograd_input_transform -> gemm_x3(G = points) -> winograd_output_transform
    "wino_x3": [
        _c("x3p_37x63_m2", 1, 37, 63, 64, 64, m=2),                            # the block1 form
        _c("x3p_8x10_m2", 2, 8, 10, 64, 64, m=2),
        _c("x3p_37x63_m4", 1, 37, 63, 64, 128, m=4),
    ],
    # h2_split -> ops.gemm_h2 under H2_CFGS; the residual (H2_RES) is given once as float32 and once as operand planes
    "h2": _from_dgrad("h2", prefix="h2_", res=1) + [
        _c("h2_long_k_17x26", 1, 17, 26, 1024, 128, 1, 1, ZERO, res=1),               # 8 scale blocks
    ],
    # gemm_x3_pack -> ops.gemm_x3, cfg -1
    "x3": [
        _c("x3_37x63_k96", 1, 37, 63, 96, 256, 1, 1, ZERO, act=2, res=1),      # 3 slabs; bias + residual + ReLU6
        _c("x3_3x43_k2048", 1, 3, 43, 2048, 128, 1, 1, ZERO),                  # M = 129: one row past a tile, long K
        _c("x3_17x26_n192", 1, 17, 26, 64, 192, 1, 1, ZERO, act=0),            # N % 128 != 0
    ],
    # ops.dwconv3x3 ([3,3,C] filters; Cin = Cout = C)
    "dw": [
        _c("dw_21x33_s1", 1, 21, 33, 64, 64, 3, 1, SAME3, act=2),
        _c("dw_21x33_s2_tf", 1, 21, 33, 64, 64, 3, 2, (0, 1, 0, 1), act=2),
        _c("dw_21x33_s2", 1, 21, 33, 64, 64, 3, 2, SAME3, act=2),
        _c("dw_7x9_s1", 2, 7, 9, 128, 128, 3, 1, SAME3, bias=False, act=0),
        _c("dw_7x9_s2_tf", 2, 7, 9, 128, 128, 3, 2, (0, 1, 0, 1), act=2),
        _c("dw_7x9_s2", 2, 7, 9, 128, 128, 3, 2, SAME3, act=2),
    ],
}
DIRECT_CFGS = (4, 15, 20, 21)           # k_conv_igemm tile configurations (csrc/conv_igemm.hip launch_cfg)
H2_CFGS = (-1, 9, 12, 21)
H2_RES = ("f32", "planes")
KINDS = ("random", "trunk")

# c per route and operand kind, in units of 2^-23 B.  None comes from the device's own numbers.
#   'random': the project's constants for the same kernels on the same operand statistics (dgrad_ref.ROUTE_C: frcnn_conv2d_nhwc is its
#   route 'flipped', 8; h2 8; Winograd 64); x3 is 3 x direct, the factor test_gemm_x3_exact_bf16_split_is_f32_class asserts.
#   'dw' (both kinds) is proven: nine fmaf and a bias give |err| <= gamma_10 B = 5 2^-23 B -- any excess there is a defect, not rounding.
#   'trunk': 4 x the random constant.  A plain float32 statement of the same convolution (torch on the CPU) over the dgrad_ref.CASES
#   shapes, bias and ReLU on and off, needs at most 2.68 on 'random' operands and 11.40 on 'trunk' ones (3x3: 10.9-11.4, 1x1: 6.3-6.7):
#   a sound float32 sum needs about 4x more room when a few channels dominate B.  tests/test_fwd_bounds_cpu.py holds the float32
#   statement of every case here to c / 2 (over CASES it needs at most 2.48 / 11.57).
# Every constant stays under the max-norm gate of the existing test of the same kernel: CAP.
# Beside each: the largest max |got - want| / (2^-23 B) the MI355X shows over the route's cases, random / trunk.
_RANDOM_C = {
    "direct": 8.0,          # measured 1.89 / 3.98
    "direct_cfg": 8.0,      # measured 2.16 / 8.00
    "splitk": 8.0,          # measured 0.52 / 2.06
    "stem": 8.0,            # measured 1.81 / 1.62
    "wino2": 64.0,          # measured 0.71 / 4.43
    "wino4": 64.0,          # measured 14.4 / 93.7
    "wino7": 64.0,          # measured 11.2 / 121
    "wino_h2": 64.0,        # measured 11.2 / 65.8
    "wino_x3": 64.0,        # measured 6.5 / 37.3
    "h2": 8.0,              # measured 2.37 / 5.19
    "x3": 24.0,             # measured 1.17 / 2.73
    "dw": 8.0,              # measured 1.51 / 1.75
}
ROUTE_C = {"random": dict(_RANDOM_C), "trunk": {r: (c if r == "dw" else 4.0 * c) for r, c in _RANDOM_C.items()}}
WINO_ROUTES = ("wino2", "wino4", "wino7", "wino_h2", "wino_x3")
CAP = {r: (1e-4 / EPS if r in WINO_ROUTES else 2e-5 / EPS) for r in _RANDOM_C}      # 839 (test_conv3x3_winograd_f4) and 168
# f32 class: a route's ratio against that of its yardstick route on the same data (and the same B), plus FLOOR.  h2 and x3 hold the 3x of
# test_gemm_h2_is_f32_class / test_gemm_x3_exact_bf16_split_is_f32_class against the direct kernel; the Winograd chains with h2 / x3
# products hold 3x against the chain with f32 products of the same m; the Winograd chains themselves hold dgrad_ref.CLASS_FACTOR's 48x
# against the direct kernel (they are not f32 class: DESIGN.md section 7).  Largest ratio to the yardstick measured on the MI355X:
# h2 1.83, x3 2.29, wino_h2 1.45, wino_x3 1.00, wino2 3.91, wino4 33.8, wino7 29.6.
CLASS_FACTOR = {"h2": 3.0, "x3": 3.0, "wino_h2": 3.0, "wino_x3": 3.0,
                "wino2": dgrad_ref.CLASS_FACTOR["winograd"], "wino4": dgrad_ref.CLASS_FACTOR["winograd"], "wino7": dgrad_ref.CLASS_FACTOR["winograd"]}
YARDSTICK = {"h2": "direct", "x3": "direct", "wino_h2": "wino", "wino_x3": "wino", "wino2": "direct", "wino4": "direct", "wino7": "direct"}
FLOOR = 1e-7 / EPS                      # 1e-7 of the scale, in units of 2^-23 B


def wino_m(route, case):
    """the Winograd scheme of a launch (2, 4, 7), None for the other routes"""
    if route not in WINO_ROUTES:
        return None
    return case.m if case.m is not None else int(route[-1])


def out_hw(case):
    return conv_out(case.H, case.k, case.stride, case.pad[0], case.pad[1]), conv_out(case.W, case.k, case.stride, case.pad[2], case.pad[3])


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _padded(x, pad):
    """x [N,H,W,C] float64 tensor with pad = (top, bottom, left, right) rows / columns of zeros added -- or, where negative, cut off"""
    N, H, W, C = x.shape
    t, b, l, r = pad
    out = torch.zeros((N, H + t + b, W + l + r, C), dtype=torch.float64)
    h0, h1, w0, w1 = max(0, -t), H - max(0, -b), max(0, -l), W - max(0, -r)
    if h1 > h0 and w1 > w0:
        out[:, max(t, 0):max(t, 0) + h1 - h0, max(l, 0):max(l, 0) + w1 - w0] = x[:, h0:h1, w0:w1]
    return out


def _strided_res(res, res_stride, OH, OW):
    return np.asarray(res, np.float64)[:, ::res_stride, ::res_stride][:, :OH, :OW]


def _act(y, act):
    return y if act == 0 else np.maximum(y, 0) if act == 1 else np.clip(y, 0, 6)


def conv64(x, wf, bias, stride, pad, res=None, res_stride=1, act=0, depthwise=False):
    """x [N,H,W,Cin] float32, wf packed [Cout,KH,KW,Cin] (depthwise: [3,3,C]) -> float64 [N,OH,OW,Cout] of
    act(conv2d(pad(x), W, stride) + bias + res[:, ::res_stride, ::res_stride]), tap by tap; pad = (top, bottom, left, right), any sign."""
    xx = _t(x).double()
    w = _t(wf).double()
    N, H, W, Cin = xx.shape
    KH, KW = (w.shape[0], w.shape[1]) if depthwise else (w.shape[1], w.shape[2])
    Cout = Cin if depthwise else w.shape[0]
    OH, OW = conv_out(H, KH, stride, pad[0], pad[1]), conv_out(W, KW, stride, pad[2], pad[3])
    xp = _padded(xx, pad)
    y = torch.zeros((N, OH, OW, Cout), dtype=torch.float64)
    for kh in range(KH):
        for kw in range(KW):
            xs = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            if depthwise:
                y += xs * w[kh, kw]
            else:
                y += (xs.reshape(-1, Cin) @ w[:, kh, kw, :].t()).reshape(N, OH, OW, Cout)
    y = y.numpy()
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if res is not None:
        y = y + _strided_res(res, res_stride, OH, OW)
    return _act(y, act)


def conv32(x, wf, bias, stride, pad, res=None, res_stride=1, act=0, depthwise=False):
    """The same operation stated in float32 (torch on the CPU): what a sound float32 kernel may differ from conv64 by."""
    F = torch.nn.functional
    xx = F.pad(_t(x).float().permute(0, 3, 1, 2), (pad[2], pad[3], pad[0], pad[1]))
    w = _t(wf).float()
    b = None if bias is None else _t(bias).float()
    if depthwise:
        y = F.conv2d(xx, w.permute(2, 0, 1)[:, None].contiguous(), b, stride=stride, groups=w.shape[2])
    else:
        y = F.conv2d(xx, w.permute(0, 3, 1, 2).contiguous(), b, stride=stride)
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + _t(res).float()[:, ::res_stride, ::res_stride][:, :y.shape[1], :y.shape[2]]
    y = y if act == 0 else y.clamp(min=0) if act == 1 else y.clamp(min=0, max=6)
    return y.contiguous().numpy()


def bound(x, wf, bias, stride, pad, res=None, res_stride=1, wino_m=None, depthwise=False):
    """B: the same operation on |x|, |W|, |bias| (for a Winograd route the maximum of that over each output tile) + |res|, no activation"""
    b = conv64(np.abs(x), np.abs(wf), None if bias is None else np.abs(bias), stride, pad, depthwise=depthwise)
    if wino_m is not None:
        b = tile_max(b, wino_m)
    if res is not None:
        b = b + np.abs(_strided_res(res, res_stride, b.shape[1], b.shape[2]))
    return _normal(b)


def last_read(n, k, stride, lo, hi):
    """index of the last input row (column) any tap reads; < n - 1 where the stride leaves the end of the map unread"""
    return min(n - 1, (conv_out(n, k, stride, lo, hi) - 1) * stride - lo + k - 1)


def taps_read(n, k, stride, lo, hi):
    """the taps of one axis that fall inside the map for at least one output"""
    return [t for t in range(k) if any(0 <= o * stride - lo + t < n for o in range(conv_out(n, k, stride, lo, hi)))]


def perturbed(x, wf, bias, stride, pad, res=None, res_stride=1, act=0, depthwise=False):
    """references a kernel could wrongly compute, each with everything else right: the last input row / column the geometry reads taken as
    zero, the pad shifted by one in h / in w, kh and kw transposed, the bias left out, the residual read one pixel late.  Only those that
    apply are yielded."""
    wf = np.asarray(wf)
    KH, KW = (wf.shape[0], wf.shape[1]) if depthwise else (wf.shape[1], wf.shape[2])

    def ref(x_=x, wf_=wf, bias_=bias, pad_=pad, res_=res):
        return conv64(x_, wf_, bias_, stride, pad_, res_, res_stride, act, depthwise)

    r = last_read(x.shape[1], KH, stride, pad[0], pad[1])
    if r >= 0:
        z = np.array(x, copy=True)
        z[:, r] = 0
        yield "zero_last_row_read", ref(x_=z)
    r = last_read(x.shape[2], KW, stride, pad[2], pad[3])
    if r >= 0:
        z = np.array(x, copy=True)
        z[:, :, r] = 0
        yield "zero_last_col_read", ref(x_=z)
    yield "pad_shift_h", ref(pad_=(pad[0] + 1, pad[1] - 1, pad[2], pad[3]))
    yield "pad_shift_w", ref(pad_=(pad[0], pad[1], pad[2] + 1, pad[3] - 1))
    rows, cols = taps_read(x.shape[1], KH, stride, pad[0], pad[1]), taps_read(x.shape[2], KW, stride, pad[2], pad[3])
    if KH == KW and any(a != b for a in rows for b in cols):           # (a single pixel reads the centre tap alone)
        yield "taps_transposed", ref(wf_=np.ascontiguousarray(wf.transpose(1, 0, 2) if depthwise else wf.transpose(0, 2, 1, 3)))
    if bias is not None:
        yield "bias_omitted", ref(bias_=None)
    if res is not None:
        yield "residual_one_pixel_late", ref(res_=np.roll(res, -1, axis=2))


def _blocks7(f, n0, n1):
    """f [N, ceil(n0/7), ceil(n1/7), 1] -> one factor per pixel of an n0 x n1 map, constant over 7x7 blocks"""
    return np.repeat(np.repeat(f, 7, axis=1), 7, axis=2)[:, :n0, :n1]


def operands(kind, case, seed=None):
    """(x, wf, bias or None, res or None) float32 of one case.
    'random': x is post-ReLU randn holding exact zeros, -0.0 and tiny positive values (dgrad_ref._edge_values), W is He-scaled, bias and
    residual are randn.
    'trunk': the same, but Cin // 64 (at least 1) channels of x are 64 times larger -- the outlier channels of the full-size test -- and
    x as a whole is scaled by 2^[-8, 8] per 7x7 block, the magnitude spread of the RoIs; the residual of an output pixel carries the
    factor of the block its centre tap reads.
    The stem (Cin = 4: three real channels) takes an image in [-110, 145] under either kind.
    res has res_stride * (OH, OW) pixels, as the shortcut of a strided unit has."""
    c = case
    seed = c.N + c.H + c.W + c.Cin + c.Cout if seed is None else seed
    rng = np.random.RandomState(seed + 7919 * (kind == "trunk"))
    OH, OW = out_hw(c)
    dw = c in CASES["dw"]
    if dw:
        wf = (rng.randn(c.k, c.k, c.Cin) * np.sqrt(2.0 / (c.k * c.k))).astype(np.float32)
    else:
        real = 3 if c.Cin == 4 else c.Cin
        wf = (rng.randn(c.Cout, c.k, c.k, c.Cin) * np.sqrt(2.0 / (c.k * c.k * real))).astype(np.float32)
        wf[..., real:] = 0
    bias = rng.randn(c.Cout).astype(np.float32) if c.bias else None
    rs = max(c.res, 1)
    res = rng.randn(c.N, OH * rs, OW * rs, c.Cout) if c.res else None
    if c.Cin == 4:
        x = np.zeros((c.N, c.H, c.W, 4), dtype=np.float32)
        x[..., :3] = rng.rand(c.N, c.H, c.W, 3) * 255 - 110
        return x, wf, bias, res
    x = np.maximum(rng.randn(c.N, c.H, c.W, c.Cin), 0)
    if kind == "trunk":
        x[..., rng.choice(c.Cin, size=max(1, c.Cin // 64), replace=False)] *= 64.0
        f = _blocks7(2.0 ** rng.randint(-8, 9, size=(c.N, -(-c.H // 7), -(-c.W // 7), 1)), c.H, c.W)
        x *= f
        if res is not None:
            ih = np.clip(np.arange(OH * rs) // rs * c.stride - c.pad[0] + c.k // 2, 0, c.H - 1)
            iw = np.clip(np.arange(OW * rs) // rs * c.stride - c.pad[2] + c.k // 2, 0, c.W - 1)
            res *= f[:, ih][:, :, iw]
    else:
        assert kind == "random", kind
    x = x.astype(np.float32)
    dgrad_ref._edge_values(x, rng)
    return x, wf, bias, (None if res is None else res.astype(np.float32))


def find(route, case_id):
    return next(c for c in CASES[route] if c.id == case_id)


Ref = collections.namedtuple("Ref", "x wf bias res want B res_raw")


@functools.lru_cache(maxsize=4)
def reference(route, case_id, kind, res_planes=False):
    """One case and operand kind, computed once and shared read-only by the tests that follow each other on it: the operands, want =
    conv64 of them and B = bound of them.  res_planes: res is the residual as gemm_h2 reads it from operand planes, (h + l) 2^-e of
    h2_ref.split -- a float32 tensor again; res_raw is the tensor the planes are split from (else res itself)."""
    c = find(route, case_id)
    x, wf, bias, res_raw = operands(kind, c)
    res = res_raw
    if res_planes:
        import h2_ref
        h, l, inv = h2_ref.split(res_raw.reshape(-1, c.Cout))
        res = ((h.astype(np.float32) + l.astype(np.float32)) * np.repeat(inv.T, h2_ref.KB, axis=1)).reshape(res_raw.shape)
    dw = route == "dw"
    rs = max(c.res, 1)
    out = Ref(x, wf, bias, res, conv64(x, wf, bias, c.stride, c.pad, res, rs, c.act, dw),
              bound(x, wf, bias, c.stride, c.pad, res, rs, wino_m(route, c), dw), res_raw)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out
