"""TEST INFRASTRUCTURE ONLY -- float64 statements of the data gradients of the reverse sweep (frcnn_hip/sweep.py: dgrad_route names
them, DGRAD issues them) and the elementwise error bound the op-level tests hold them to.

dX of y = conv2d(pad(x), W, stride) is a scatter of dY through the filter taps; dgrad64 states it tap by tap in float64 (any pad,
negative ones included, so a shifted pad can be stated too).  The bound of a float32 result is elementwise and scaled to the magnitude
of what was summed:

    |got - want| <= c * 2^-23 * B,    B = the same float64 operation on |dY| and |W|  (+ |residual|)

so one missing border tap fails it (a max-relative bound would not see it), while cancellation inside a sum does not.  The Winograd
route's rounding lives in its transforms and is shared by the m x m outputs of a tile: its B is the tile's maximum of the above.

CASES lists every route's shapes; tests/test_dgrad_gpu.py runs them on the device, tests/test_dgrad_bounds_cpu.py proves for each of
them (both operand sets) that the route's c rejects a reference with the last output row or column dropped or the pad shifted by one."""
import numpy as np
import torch

EPS = 2.0 ** -23

# c per route: the largest max |got - want| / (2^-23 B) measured on the MI355X over the cases below (random and block4-tail operands,
# fresh and accumulating), with about 4x headroom.  c 2^-23 stays under the max-relative bound of the forward test of the same kernel
# (test_conv3x3_winograd_f4 1e-4 = 839 2^-23; the direct kernel and test_gemm_h2_is_f32_class 2e-5 = 168 2^-23).
ROUTE_C = {
    "winograd": 64.0,       # measured 14.7 -- F(4x4,3x3) / mixed 7x7 scheme: the transforms amplify rounding (|B^T| rows sum to 10)
    "flipped": 8.0,         # measured 1.88 -- frcnn_conv2d_nhwc[_masked][_ws] with the flipped / transposed filter
    "h2": 8.0,              # measured 2.05 -- frcnn_gemm_h2[_masked]: two-piece fp16 operands
    "padded": 8.0,          # measured 1.92 -- zero-padded dY and filter on frcnn_conv2d_nhwc
    "upsampled": 8.0,       # measured 1.66 -- frcnn_add_strided + frcnn_conv2d_nhwc with asymmetric pads
    "gather": 8.0,          # measured 2.44 -- frcnn_conv2d_dgrad_strided
}
# f32 class: a route's max |got - want| / (2^-23 B) against that of the flipped-direct float32 route on the same data.  h2 holds the 3x
# of test_gemm_h2_is_f32_class (measured <= 2.2x).  The Winograd data gradient is not f32 class (measured 7x .. 35x: its transforms
# amplify rounding); keeping it is the recorded decision of DESIGN.md section 7 (rerouting costs 1.5 ms of a 16.8 ms C5 step and moves
# no sampled full-size gradient), and 48x is the limit that decision sets.
CLASS_FACTOR = {"h2": 3.0, "winograd": 48.0}

SAME3 = (1, 1, 1, 1)
ZERO = (0, 0, 0, 0)
# route -> [(id, N, H, W, Cin, Cout, k, stride, pad)]  (H, W: the input x of the forward convolution)
CASES = {
    "winograd": [
        ("37x63_m4", 1, 37, 63, 128, 128, 3, 1, SAME3),        # odd both ways: ragged last tile row and column
        ("34x51_m4", 1, 34, 51, 128, 64, 3, 1, SAME3),         # even x odd
        ("1x9_m4", 1, 1, 9, 64, 64, 3, 1, SAME3),              # a single pixel row
        ("roi1_m7", 1, 7, 7, 128, 128, 3, 1, SAME3),           # the RoI tail's 7x7 maps: mixed F(4,3)+F(3,3) scheme
        ("roi37_m7", 37, 7, 7, 256, 256, 3, 1, SAME3),
        ("roi256_m7", 256, 7, 7, 128, 128, 3, 1, SAME3),
    ],
    "flipped": [
        ("3x3_37x63", 1, 37, 63, 64, 128, 3, 1, SAME3),
        ("3x3_17x26", 2, 17, 26, 96, 64, 3, 1, SAME3),
        ("3x3_1x40", 1, 1, 40, 32, 64, 3, 1, SAME3),
        ("3x3_roi37", 37, 7, 7, 128, 128, 3, 1, SAME3),
        ("1x1_75x125", 1, 75, 125, 64, 256, 1, 1, ZERO),
        ("1x1_roi256", 256, 7, 7, 128, 256, 1, 1, ZERO),
    ],
    "h2": [
        ("37x63", 1, 37, 63, 128, 256, 1, 1, ZERO),            # M = 2331: no multiple of the tile
        ("17x26", 1, 17, 26, 256, 128, 1, 1, ZERO),
        ("1x77", 1, 1, 77, 128, 128, 1, 1, ZERO),
        ("roi1", 1, 7, 7, 128, 256, 1, 1, ZERO),
        ("roi37", 37, 7, 7, 256, 512, 1, 1, ZERO),
        ("roi256", 256, 7, 7, 128, 256, 1, 1, ZERO),
    ],
    "padded": [
        ("cls_score21", 256, 1, 1, 2048, 21, 1, 1, ZERO),
        ("bbox_pred84", 256, 1, 1, 2048, 84, 1, 1, ZERO),
        ("cls_score81", 37, 1, 1, 2048, 81, 1, 1, ZERO),
        ("rpn_cls18", 1, 37, 63, 512, 18, 1, 1, ZERO),
        ("rpn_bbox36", 1, 17, 26, 512, 36, 1, 1, ZERO),
    ],
    "upsampled": [
        ("34x51", 1, 34, 51, 64, 64, 3, 2, SAME3),             # -> 17x26: up_pad bottom 2, right 1
        ("75x125", 1, 75, 125, 32, 32, 3, 2, SAME3),           # -> 38x63
        ("37x63", 1, 37, 63, 64, 32, 3, 2, SAME3),             # -> 19x32
        ("2x3", 2, 2, 3, 32, 64, 3, 2, SAME3),                 # -> 1x2
    ],
    "gather": [
        ("1x1s2_34x51", 1, 34, 51, 64, 128, 1, 2, ZERO),       # strided shortcut -> 17x26
        ("1x1s2_17x26", 1, 17, 26, 128, 256, 1, 2, ZERO),      # -> 9x13
        ("3x3s2_37x63_c36", 1, 37, 63, 20, 36, 3, 2, SAME3),   # channel counts no multiple of 32
        ("3x3s1_19x23_c20", 1, 19, 23, 12, 20, 3, 1, SAME3),
        ("3x3s2_9x13", 2, 9, 13, 64, 64, 3, 2, SAME3),         # pipe_dgrads = False
    ],
}


def conv_out(n, k, stride, lo, hi):
    return (n + lo + hi - k) // stride + 1


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def dgrad64(gy, wf, stride, pad, H, W, depthwise=False):
    """gy [N,OH,OW,Cout], wf packed [Cout,KH,KW,Cin] (depthwise: [KH,KW,C]) -> float64 dX [N,H,W,Cin] of y = conv2d(pad(x), W, stride);
    pad = (top, bottom, left, right), any sign (only top / left place the taps)."""
    g = _t(gy).double()
    w = _t(wf).double()
    N, OH, OW, _ = g.shape
    KH, KW = (w.shape[0], w.shape[1]) if depthwise else (w.shape[1], w.shape[2])
    Cin = w.shape[-1]
    dx = torch.zeros((N, H, W, Cin), dtype=torch.float64)

    def span(O, k, lo, n):
        # output indices o with 0 <= o * stride + k - lo < n, as a slice of o and of the input
        o0 = max(0, -(-(lo - k) // stride))
        o1 = min(O, (n - 1 + lo - k) // stride + 1)
        if o1 <= o0:
            return None
        i0 = o0 * stride + k - lo
        return slice(o0, o1), slice(i0, i0 + (o1 - o0 - 1) * stride + 1, stride)

    for kh in range(KH):
        sh = span(OH, kh, pad[0], H)
        if sh is None:
            continue
        for kw in range(KW):
            sw = span(OW, kw, pad[2], W)
            if sw is None:
                continue
            part = g[:, sh[0], sw[0], :]
            if depthwise:
                dx[:, sh[1], sw[1], :] += part * w[kh, kw]
            else:
                dx[:, sh[1], sw[1], :] += (part.reshape(-1, part.shape[-1]) @ w[:, kh, kw, :]).reshape(part.shape[:3] + (Cin,))
    return dx.numpy()


def tile_max(b, m):
    """elementwise bound of the Winograd route: max of b [N,H,W,C] over each m x m output tile (m = 7: the whole 7x7 map)."""
    N, H, W, C = b.shape
    if m == 7:
        return np.broadcast_to(b.max(axis=(1, 2), keepdims=True), b.shape).copy()
    TH, TW = -(-H // m), -(-W // m)
    p = np.zeros((N, TH * m, TW * m, C))
    p[:, :H, :W] = b
    t = p.reshape(N, TH, m, TW, m, C).max(axis=(2, 4), keepdims=True)
    return np.broadcast_to(t, (N, TH, m, TW, m, C)).reshape(N, TH * m, TW * m, C)[:, :H, :W].copy()


def finish(dx, res, mask):
    """what the route writes: (dX + residual) gated by mask > 0, float64"""
    out = dx if res is None else dx + np.asarray(res, np.float64)
    return out if mask is None else np.where(np.asarray(mask) > 0, out, 0.0)


def bound(gy, wf, stride, pad, H, W, res=None, wino_m=None, depthwise=False):
    b = dgrad64(np.abs(gy), np.abs(wf), stride, pad, H, W, depthwise)
    if wino_m is not None:
        b = tile_max(b, wino_m)
    return b if res is None else b + np.abs(np.asarray(res, np.float64))


def ratio(got, want, B):
    """max over elements of |got - want| / (2^-23 B)  (0 / 0 = 0, x / 0 = inf; NaN = inf)"""
    d = np.abs(np.asarray(got, np.float64) - want)
    d = np.where(np.isnan(d), np.inf, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / (EPS * B))
    return float(r.max()) if r.size else 0.0


def perturbed(gy, wf, stride, pad, H, W, depthwise=False):
    """references a kernel could wrongly compute: the last output row / column of dY dropped, the pad shifted by one pixel"""
    g = np.array(gy, copy=True)
    g[:, -1] = 0
    yield "drop_last_row", dgrad64(g, wf, stride, pad, H, W, depthwise)
    g = np.array(gy, copy=True)
    g[:, :, -1] = 0
    yield "drop_last_col", dgrad64(g, wf, stride, pad, H, W, depthwise)
    yield "pad_shift_h", dgrad64(gy, wf, stride, (pad[0] + 1, pad[1] - 1, pad[2], pad[3]), H, W, depthwise)
    yield "pad_shift_w", dgrad64(gy, wf, stride, (pad[0], pad[1], pad[2] + 1, pad[3] - 1), H, W, depthwise)


def _edge_values(a, rng):
    """exact zeros, -0.0 and tiny positive values in a post-ReLU tensor: the mask must take y > 0 exactly"""
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, size=min(flat.size, 4 * max(1, flat.size // 50)), replace=False)
    q = len(idx) // 4
    flat[idx[:q]] = 0.0
    flat[idx[q:2 * q]] = -0.0
    flat[idx[2 * q:3 * q]] = 1e-30
    flat[idx[3 * q:]] = np.float32(1.1754944e-38)            # the smallest normal float32


def operands(kind, N, H, W, Cin, Cout, k, stride, pad, seed=0, with_res=False):
    """(gy, wf, x, res) float32 for one layer.  kind 'random'; or 'block4', shaped like the real block4 tail: dY comes from
    spatial_mean_bwd (constant over each RoI's 49 pixels -- on maps larger than 7x7 over 7x7 blocks), its RoIs differ in magnitude by up
    to 2^+-8 (fg vs bg) and it is gated by a ReLU mask; X is post-ReLU with a few outlier channels.  x (the mask source) always holds
    exact zeros, -0.0 and tiny positive values."""
    rng = np.random.RandomState(seed + 7919 * (kind == "block4"))
    OH, OW = conv_out(H, k, stride, pad[0], pad[1]), conv_out(W, k, stride, pad[2], pad[3])
    wf = (rng.randn(Cout, k, k, Cin) * np.sqrt(2.0 / (k * k * Cin))).astype(np.float32)
    x = np.maximum(rng.randn(N, H, W, Cin), 0)
    if kind == "random":
        gy = rng.randn(N, OH, OW, Cout) * (rng.rand(N, OH, OW, Cout) < 0.6)
        res = rng.randn(N, H, W, Cin)
    else:
        bh, bw = -(-OH // 7), -(-OW // 7)
        mag = 2.0 ** rng.randint(-8, 9, size=(N, bh, bw, 1))
        g = rng.randn(N, bh, bw, Cout) * mag / 49.0
        gy = np.repeat(np.repeat(g, 7, axis=1), 7, axis=2)[:, :OH, :OW] * (rng.rand(N, OH, OW, Cout) < 0.5)
        x[..., rng.choice(Cin, size=max(1, Cin // 64), replace=False)] *= 64.0
        rm = np.repeat(np.repeat(2.0 ** rng.randint(-8, 9, size=(N, -(-H // 7), -(-W // 7), 1)), 7, axis=1), 7, axis=2)[:, :H, :W]
        res = rng.randn(N, H, W, Cin) * rm / 49.0
    x = x.astype(np.float32)
    _edge_values(x, rng)
    return gy.astype(np.float32), wf, x, (res.astype(np.float32) if with_res else None)


def wgrad64(gy, x, KH, KW, stride, pad):
    """float64 dW [Cout,KH,KW,Cin] of y = conv2d(pad(x), W, stride) from dY [N,OH,OW,Cout] and X [N,H,W,Cin]"""
    g = _t(gy).double()
    xx = _t(x).double()
    N, OH, OW, Cout = g.shape
    _, H, W, Cin = xx.shape
    xp = torch.zeros((N, H + max(pad[0], 0) + KH, W + max(pad[2], 0) + KW, Cin), dtype=torch.float64)
    xp[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W] = xx
    out = torch.empty((Cout, KH, KW, Cin), dtype=torch.float64)
    gm = g.reshape(-1, Cout)
    for kh in range(KH):
        for kw in range(KW):
            xs = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            out[:, kh, kw, :] = gm.t() @ xs.reshape(-1, Cin)
    return out.numpy()
