"""GPU: every data-gradient route of the reverse sweep, through the route function the sweep itself calls (frcnn_hip/sweep.py DGRAD: its
filter preparation, pads, accumulate / residual handling, ReLU mask and operand planes) -- against the float64 statement of the
same operation (oracle/dgrad_ref.py), plus the other kernels of the sweep: stride-2 depthwise dgrad at MobileNet's asymmetric SAME
pads, relu_bwd / relu6_bwd at their edges, add_strided, spatial_mean_bwd and the heads' filter-gradient fallback.

Two bounds, both must hold (oracle/dgrad_ref.py): elementwise |got - want| <= c 2^-23 B with B the float64 operation on |dY|, |W|
(+ |residual|) and c per route (dgrad_ref.ROUTE_C); and for the Winograd and h2 routes the f32 class of test_gemm_h2_is_f32_class:
their max |got - want| / (2^-23 B) is at most dgrad_ref.CLASS_FACTOR (h2: 3x; Winograd: 48x, it is not f32 class -- DESIGN.md section 7) times that of the
flipped-direct float32 route on the same data, plus a floor of 1e-7 of the scale.  Both operand sets: random, and shaped like the real block4 tail (dgrad_ref.operands).  Every output buffer sits in front of a
sentinel tail that must survive.  tests/test_dgrad_bounds_cpu.py proves, per case, that the bounds reject a dropped border row /
column and a shifted pad."""
import numpy as np
import pytest
import torch

import dgrad_ref as R

pytestmark = pytest.mark.gpu

SENT = 12345.5
FLOOR = 1e-7 / R.EPS            # the f32-class rule's floor, in units of 2^-23 B
KINDS = ["random", "block4"]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(shape, dev, init=None):
    n = int(np.prod(shape))
    g = torch.full((n + 4096,), SENT, dtype=torch.float32, device=dev)
    v = g[:n].view(shape)
    if init is not None:
        v.copy_(init)
    return g, v


def _tail_ok(g, shape):
    return bool((g[int(np.prod(shape)):] == SENT).all())


def _planes_np(h2):
    raw = h2.planes.cpu().numpy().view(np.uint16).reshape(2, h2.rows, h2.K)
    return raw[0], raw[1], h2.inv.cpu().numpy()


def _same_planes(got, want):
    for g_, w_, name in zip(_planes_np(got), want, ("h", "l", "inv")):
        w_ = w_.view(np.uint16) if w_.dtype == np.float16 else w_
        assert np.array_equal(g_, w_), name


class Scratch(object):
    """What the route functions are given in the session's place (frcnn_hip/sweep.py: buf / h2_buf / buf_pair): fresh device tensors, zeroed
    where the route asks for zeros and filled with the sentinel where it does not, operand planes pre-filled 0x5a / -1.0, so that an
    element a kernel should have written and did not is seen; `handed` keeps every buffer by the name it was asked for under."""

    def __init__(self, dev):
        self.dev, self.handed = dev, {}

    def buf(self, name, shape, zero=False):
        t = torch.zeros(tuple(shape), dtype=torch.float32, device=self.dev) if zero else torch.full(tuple(shape), SENT, dtype=torch.float32, device=self.dev)
        self.handed[name] = t
        return t

    def h2_buf(self, name, rows, K):
        from frcnn_hip import ops
        p = self.handed[name] = ops.H2.empty(rows, K, self.dev)
        p.planes.fill_(0x5a), p.inv.fill_(-1.0)
        return p

    def buf_pair(self, name, N, K):
        from frcnn_hip import ops
        return (torch.empty(int(ops.lib().frcnn_h2_planes_bytes(int(N), int(K))), dtype=torch.uint8, device=self.dev),
                torch.empty((1, int(N)), dtype=torch.float32, device=self.dev))


def prepared(key, fn):
    return fn()


def run_route(route, case, gy, wf, x, res, dev, mask=True):
    """One data gradient through the route function the sweep calls (frcnn_hip/sweep.py DGRAD[route]), asked to emit operand planes wherever
    the route can.  had = res is not None (accumulate into a buffer that holds res).
    Returns (dX float32 [N,H,W,Cin] on the host, operand planes or None, what the mask was (None when the route took none))."""
    from frcnn_hip import ops, sweep
    _, N, H, W, Cin, Cout, k, stride, pad = case
    OH, OW = gy.shape[1], gy.shape[2]
    shape = (N, H, W, Cin)
    guard, gx = _guarded(shape, dev, None if res is None else T(res, dev))
    m = (7 if (OH == 7 and OW == 7) else 4) if route == "winograd" else None
    masked, planes, _, _ = sweep.DGRAD[route](ops, Scratch(dev), prepared, case[0], T(gy, dev), T(wf, dev), k, stride, pad, gx, None if res is None else gx,
                                              T(x, dev) if mask else None, emit=True, m=m)
    torch.cuda.synchronize()
    assert _tail_ok(guard, shape), "%s wrote past the end of dX" % route
    return gx.cpu().numpy(), planes, (x if masked else None)


def _wino_out_groups(m, N, H, W):
    """row -> plane-scale group of the Winograd output transform: the pixels of one output row of one tile share a scale"""
    if m == 7:
        return np.arange(N * 49) // 7
    TW = (W + m - 1) // m
    img, rem = np.divmod(np.arange(N * H * W), H * W)
    oh, ow = np.divmod(rem, W)
    return (img * H + oh) * TW + ow // m


def _route_ids():
    return [(r, c) for r in R.CASES for c in R.CASES[r]]


ROUTE_CASES = _route_ids()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("had", [False, True], ids=["fresh", "had"])
@pytest.mark.parametrize("rc", ROUTE_CASES, ids=["%s-%s" % (r, c[0]) for r, c in ROUTE_CASES])
def test_dgrad_route_vs_float64(dev, rc, had, kind):
    route, case = rc
    _, N, H, W, Cin, Cout, k, stride, pad = case
    gy, wf, x, res = R.operands(kind, N, H, W, Cin, Cout, k, stride, pad, seed=N + H + W + Cin + Cout, with_res=had)
    # the heads behind the mean of the RoI tail (cls_score / bbox_pred read fc7) get no mask; every other input here is a ReLU output
    use_mask = not (route == "padded" and H == 1)
    got, planes, mk = run_route(route, case, gy, wf, x, res, dev, mask=use_mask)
    dx = R.dgrad64(gy, wf, stride, pad, H, W)
    want = R.finish(dx, res, mk)
    m = (7 if H == 7 and W == 7 else 4) if route == "winograd" else None
    B = R.bound(gy, wf, stride, pad, H, W, res, wino_m=m)
    c = R.ROUTE_C[route]
    r = R.ratio(got, want, B)
    if mk is not None:
        assert np.all(got[~(mk > 0)] == 0), "the mask let a gradient through where x <= 0"
    msg = "dgrad %-9s %-18s %-5s %-6s: max |err| / (2^-23 B) = %7.3f (c = %g)" % (route, case[0], "had" if had else "fresh", kind, r, c)
    if route in ("winograd", "h2"):
        f32, _, _ = run_route("flipped", case, gy, wf, x, res, dev, mask=(mk is not None))
        r32 = R.ratio(f32, want, B)
        msg += "; flipped-direct f32 %7.3f, ratio %.2f" % (r32, r / max(r32, 1e-30))
        print(msg)
        assert r <= R.CLASS_FACTOR[route] * r32 + FLOOR, (route, r, r32)
    else:
        print(msg)
    assert np.isfinite(got).all() and r <= c, (route, case[0], r)
    if planes is not None:
        if route == "h2":
            from frcnn_hip import ops
            ref = ops.h2_split(T(got.reshape(-1, Cin), dev))
            _same_planes(planes, _planes_np(ref))
        else:
            import h2_ref
            _same_planes(planes, h2_ref.split_grouped(got.reshape(-1, Cin), _wino_out_groups(m, N, H, W)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [
    # id, N, H, W, conv2 Cin, conv2 Cout, conv1 Cin
    ("37x63_m4", 1, 37, 63, 128, 256, 256),
    ("34x51_m4", 1, 34, 51, 256, 128, 128),
    ("roi37_m7", 37, 7, 7, 256, 256, 512),
], ids=lambda c: c[0])
def test_h2_dgrad_on_winograd_emitted_planes_vs_float64(dev, case, kind):
    """The bottleneck in reverse as the sweep runs it: conv2's Winograd data gradient (masked, fresh) emits its result as operand planes with
    row-group scales (emitted[key]), and conv1's h2 data gradient reads them as its dY instead of an h2_split.  Against float64 of conv1's
    data gradient of conv2's float32 result: the route's elementwise bound and the f32 class of the flipped-direct kernel on the same dY."""
    from frcnn_hip import ops, sweep
    _, N, H, W, C2in, C2out, C1in = case
    M = N * H * W
    case2 = (case[0], N, H, W, C2in, C2out, 3, 1, R.SAME3)
    gy2, wf2, x2, _ = R.operands(kind, N, H, W, C2in, C2out, 3, 1, R.SAME3, seed=M + C2in)
    dy1, planes, _ = run_route("winograd", case2, gy2, wf2, x2, None, dev)
    assert planes is not None
    case1 = (case[0], N, H, W, C1in, C2in, 1, 1, R.ZERO)
    _, wf1, x1, _ = R.operands(kind, N, H, W, C1in, C2in, 1, 1, R.ZERO, seed=M + C1in + 1)
    guard, gx = _guarded((N, H, W, C1in), dev)
    sweep.dgrad_h2(ops, Scratch(dev), prepared, case[0], T(dy1, dev), T(wf1, dev), 1, 1, R.ZERO, gx, None, T(x1, dev), gy_planes=planes)
    torch.cuda.synchronize()
    assert _tail_ok(guard, (N, H, W, C1in))
    got = gx.cpu().numpy()
    want = R.finish(R.dgrad64(dy1, wf1, 1, R.ZERO, H, W), None, x1)
    B = R.bound(dy1, wf1, 1, R.ZERO, H, W)
    r = R.ratio(got, want, B)
    f32, _, _ = run_route("flipped", case1, dy1, wf1, x1, None, dev)
    r32 = R.ratio(f32, want, B)
    print("dgrad h2 on Winograd planes %-9s %-6s: max |err| / (2^-23 B) = %.3f; flipped-direct f32 %.3f, ratio %.2f"
          % (case[0], kind, r, r32, r / max(r32, 1e-30)))
    assert np.isfinite(got).all() and r <= R.ROUTE_C["h2"], r
    assert r <= R.CLASS_FACTOR["h2"] * r32 + FLOOR, (r, r32)


@pytest.mark.parametrize("N,H,W,C,pad", [
    (2, 17, 21, 32, (1, 1, 1, 1)),            # what lib/nets/mobilenet_v1.py builds for stride 2: explicit pad 1 + VALID, odd sizes
    (1, 38, 63, 64, (1, 1, 1, 1)),            # ... even x odd
    (2, 18, 22, 32, (0, 1, 0, 1)),            # TF 'SAME' at stride 2 on even sizes: pad (0, 1) -- asymmetric
    (1, 38, 64, 64, (0, 1, 0, 1)),
    (1, 2, 4, 8, (0, 1, 0, 1)),               # one output row
])
def test_dwconv3x3_dgrad_stride2_accumulates(dev, N, H, W, C, pad):
    """stride-2 depthwise data gradient at the network's symmetric pad and at TF SAME's asymmetric (0, 1, 0, 1) (even sizes), accumulating
    into a buffer that already holds a gradient as the sweep does"""
    from frcnn_hip import ops
    rng = np.random.RandomState(H * W + C)
    OH, OW = R.conv_out(H, 3, 2, pad[0], pad[1]), R.conv_out(W, 3, 2, pad[2], pad[3])
    g = rng.randn(N, OH, OW, C).astype(np.float32)
    w = rng.randn(3, 3, C).astype(np.float32)
    res = rng.randn(N, H, W, C).astype(np.float32)
    guard, dx = _guarded((N, H, W, C), dev, T(res, dev))
    ops.dwconv3x3_dgrad(T(g, dev), T(w, dev), 2, pad, dx, accumulate=True)
    torch.cuda.synchronize()
    assert _tail_ok(guard, (N, H, W, C))
    want = R.dgrad64(g, w, 2, pad, H, W, depthwise=True) + res
    B = R.bound(g, w, 2, pad, H, W, res, depthwise=True)
    r = R.ratio(dx.cpu().numpy(), want, B)
    print("dwconv3x3_dgrad s2 %s %s: max |err| / (2^-23 B) = %.3f" % (pad, (N, H, W, C), r))
    assert r <= 4.0
    for name, p in R.perturbed(g, w, 2, pad, H, W, depthwise=True):
        assert R.ratio(p + res, want, B) > 4.0, name


@pytest.mark.parametrize("reps", [6, 25, 2731])
def test_relu_and_relu6_bwd_edges(dev, reps):
    """frcnn_relu_bwd: gradient where y > 0; frcnn_relu6_bwd: where 0 < y < 6 (TF's Relu6Grad) -- at exactly 0, -0.0, 6, NaN, +-inf.
    n = 72, 300 and 32 772: inside one 256-thread block, a partly filled block, a last block of one float4 (the ABI takes n % 4 == 0 only:
    the sweep's tensors have channel counts that are multiples of 4, and any other n is refused, not rounded)"""
    from frcnn_hip import FrcnnHipError, ops
    y = np.array([0.0, -0.0, 6.0, np.nan, 1e-30, 1.1754944e-38, 5.9999995, 6.0000005, -1.0, 3.0, np.inf, -np.inf], dtype=np.float32)
    y = np.tile(y, reps)
    g = np.random.RandomState(reps).randn(y.size).astype(np.float32)
    for fn, keep in ((ops.relu_bwd, y > 0), (ops.relu6_bwd, (y > 0) & (y < 6))):
        guard = torch.full((y.size + 64,), SENT, dtype=torch.float32, device=dev)
        gd = guard[:y.size]
        gd.copy_(T(g, dev))
        fn(gd, T(y, dev))
        want = np.where(keep, g, np.float32(0))
        got = gd.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fn.__name__, got, want)
        assert bool((guard[y.size:] == SENT).all())
        with pytest.raises(FrcnnHipError):
            fn(guard[:y.size - 1], T(y[:-1], dev))


@pytest.mark.parametrize("N,OH,OW,C,stride,H,W,acc", [
    (1, 37, 63, 64, 1, 37, 63, True),         # an identity shortcut's gradient added into dX
    (2, 17, 26, 128, 2, 34, 51, False),       # subsample gradient: every second pixel of an even x odd map
    (1, 19, 32, 32, 2, 37, 63, True),         # odd x odd, accumulate
    (1, 9, 13, 256, 2, 17, 26, False),
])
def test_add_strided(dev, N, OH, OW, C, stride, H, W, acc):
    from frcnn_hip import ops
    rng = np.random.RandomState(OH * OW + C)
    src = rng.randn(N, OH, OW, C).astype(np.float32)
    dst0 = rng.randn(N, H, W, C).astype(np.float32)
    guard, dst = _guarded((N, H, W, C), dev, T(dst0, dev))
    ops.add_strided(T(src, dev), dst, stride, acc)
    torch.cuda.synchronize()
    assert _tail_ok(guard, (N, H, W, C))
    want = dst0.copy()
    sl = (slice(None), slice(0, (OH - 1) * stride + 1, stride), slice(0, (OW - 1) * stride + 1, stride))
    want[sl] = want[sl] + src if acc else src                             # float32 adds: exact rounding, so bit equality
    assert np.array_equal(dst.cpu().numpy(), want)


@pytest.mark.parametrize("R_", [1, 37, 256])
def test_spatial_mean_bwd_hw49(dev, R_):
    from frcnn_hip import ops
    rng = np.random.RandomState(R_)
    C = 2048
    g = (rng.randn(R_, C) * 2.0 ** rng.randint(-8, 9, size=(R_, 1))).astype(np.float32)
    guard, out = _guarded((R_, 7, 7, C), dev)
    ops.spatial_mean_bwd(T(g, dev), 49, out)
    torch.cuda.synchronize()
    assert _tail_ok(guard, (R_, 7, 7, C))
    want = np.broadcast_to((g.astype(np.float64) / 49.0)[:, None, None, :], (R_, 7, 7, C))
    got = out.cpu().numpy()
    assert np.all(np.abs(got - want) <= 2 * R.EPS * np.abs(want))           # g * fl(1/49): two roundings
    assert np.array_equal(got[:, 0, 0], got[:, 6, 6])


@pytest.mark.parametrize("case", [
    # id, N, H, W, Cin, Cout, k, stride, pad
    ("cls_score_R256", 256, 1, 1, 2048, 21, 1, 1, (0, 0, 0, 0)),
    ("rpn_cls_112x112", 1, 112, 112, 512, 18, 1, 1, (0, 0, 0, 0)),        # M = 12544
    ("rpn_bbox_37x63", 1, 37, 63, 512, 36, 1, 1, (0, 0, 0, 0)),           # M = 2331: a tail past the last 32
    ("k3s2_c20_c36", 1, 37, 63, 20, 36, 3, 2, (1, 1, 1, 1)),              # im2col_t at k = 3, stride 2 (wgrad_tn off)
    ("k3s2_M12544", 1, 223, 225, 12, 32, 3, 2, (1, 1, 1, 1)),             # M = 112 x 113 = 12656
])
def test_head_filter_gradient_fallback_vs_float64(dev, case):
    """The sweep's filter gradient (frcnn_hip/sweep.py filter_gradient) when conv2d_wgrad_supported is false or TrainState.wgrad_tn is off:
    transpose_pad of dY, transpose_pad / im2col_t of X, the forward MFMA kernel on the padded pair, colsum for the bias"""
    import types
    from frcnn_hip import ops, sweep
    _, N, H, W, Cin, Cout, k, stride, pad = case
    OH, OW = R.conv_out(H, k, stride, pad[0], pad[1]), R.conv_out(W, k, stride, pad[2], pad[3])
    M = N * OH * OW
    KK = k * k * Cin
    rng = np.random.RandomState(M + Cin)
    x = np.maximum(rng.randn(N, H, W, Cin), 0).astype(np.float32)
    gy = (rng.randn(N, OH, OW, Cout) * (rng.rand(N, OH, OW, Cout) < 0.5)).astype(np.float32)
    guard, gw = _guarded((Cout, KK), dev)
    gb_guard, gb = _guarded((Cout,), dev)
    scratch = Scratch(dev)
    sweep.filter_gradient(ops, scratch, "", T(gy, dev), T(x, dev), k, stride, pad, types.SimpleNamespace(grad_w=gw, K=KK, bias=gb, grad_b=gb), False, False)
    gyT, xT = scratch.handed["bwd/gyT"], scratch.handed["bwd/xT"]
    assert gyT.shape[1] == xT.shape[1] == (M + 31) // 32 * 32 and xT.shape[0] == KK
    assert bool((gyT[:, M:] == 0).all()) and bool((xT[:, M:] == 0).all()), "the pad columns must be zero"
    torch.cuda.synchronize()
    assert _tail_ok(guard, (Cout, KK)) and _tail_ok(gb_guard, (Cout,))
    want = R.wgrad64(gy, x, k, k, stride, pad).reshape(Cout, KK)
    B = R.wgrad64(np.abs(gy), x, k, k, stride, pad).reshape(Cout, KK)
    r = R.ratio(gw.cpu().numpy(), want, B)
    wb = gy.astype(np.float64).reshape(M, Cout).sum(0)
    Bb = np.abs(gy.astype(np.float64)).reshape(M, Cout).sum(0)
    rb = R.ratio(gb.cpu().numpy(), wb, Bb)
    print("head wgrad fallback %s: dW max |err| / (2^-23 B) = %.3f, db %.3f" % (case[0], r, rb))
    assert r <= R.ROUTE_C["flipped"], r
    assert np.all(np.abs(gb.cpu().numpy() - wb) <= R.EPS * np.abs(wb) + 1e-9 * R.EPS * Bb), "colsum: float64 sum, one rounding"
    # the bound sees one dropped output row of the product
    gy_cut = gy.copy()
    gy_cut[:, -1] = 0
    assert R.ratio(R.wgrad64(gy_cut, x, k, k, stride, pad).reshape(Cout, KK), want, B) > R.ROUTE_C["flipped"]
