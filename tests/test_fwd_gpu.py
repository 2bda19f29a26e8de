"""GPU: every forward convolution route at op level against the float64 statement of the same operation (oracle/fwd_ref.py): the direct
kernel under the automatic plan, under forced tile configurations, split along K and in the stem's fold_w form; the Winograd chains with
f32, h2 and x3 products; gemm_h2 and gemm_x3 as 1x1 convolutions; the depthwise 3x3 -- each with the bias, residual and activation the
launch fuses, on two operand kinds (fwd_ref.operands: random, and trunk-like with outlier channels and a 2^+-8 block spread).

Two bounds, both must hold: elementwise |got - want| <= c 2^-23 B with B the float64 operation on |x|, |W|, |bias| (+ |residual|) and c
per route and kind (fwd_ref.ROUTE_C); and for the routes that have a yardstick (fwd_ref.YARDSTICK) the f32 class: their max |got - want| /
(2^-23 B) is at most fwd_ref.CLASS_FACTOR times that of the yardstick route launched on the same operands, plus fwd_ref.FLOOR.  Every output
starts as NaN in front of a sentinel tail that must survive; operand planes a route emits equal the splitter's planes of its float32
result bit for bit.  tests/test_fwd_bounds_cpu.py proves, per case, that the bounds reject a missing border row or column, a shifted pad,
transposed taps, a missing bias and a late residual.  Each run prints its ratio: the largest per route and kind is recorded beside the
constant in oracle/fwd_ref.py."""
import numpy as np
import pytest
import torch

import fwd_ref as R

# fwd_ref.reference() hands out read-only arrays; torch only reads them
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

SENT = 12345.5


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan_guarded(shape, dev):
    """(whole buffer, the output view filled with NaN): 4096 sentinel floats behind the output must survive the launch"""
    n = int(np.prod(shape))
    g = torch.full((n + 4096,), SENT, dtype=torch.float32, device=dev)
    v = g[:n].view(shape)
    v.fill_(float("nan"))
    return g, v


def _result(guard, out, what):
    torch.cuda.synchronize()
    assert bool((guard[out.numel():] == SENT).all()), "%s wrote past the end of its output" % what
    return out.cpu().numpy()


def _fresh_planes(rows, K, dev):
    from frcnn_hip import ops
    p = ops.H2.empty(rows, K, dev)
    p.planes.fill_(0x5a), p.inv.fill_(-1.0)
    return p


def _planes_np(h2):
    raw = h2.planes.cpu().numpy().view(np.uint16).reshape(2, h2.rows, h2.K)
    return raw[0], raw[1], h2.inv.cpu().numpy()


def _same_planes(got, want):
    for g_, w_, name in zip(_planes_np(got), want, ("h", "l", "inv")):
        w_ = w_.view(np.uint16) if w_.dtype == np.float16 else w_
        assert np.array_equal(g_, w_), name


def _wino_out_groups(m, N, H, W):
    """row -> plane-scale group of the Winograd output transform: the pixels of one output row of one tile share a scale"""
    if m == 7:
        return np.arange(N * 49) // 7
    TW = (W + m - 1) // m
    img, rem = np.divmod(np.arange(N * H * W), H * W)
    oh, ow = np.divmod(rem, W)
    return (img * H + oh) * TW + ow // m


def _hwio(wf):
    return np.ascontiguousarray(np.asarray(wf).transpose(1, 2, 3, 0))


# ---- one launch per route: (dev, case, reference, ...) -> (float32 result on the host, emitted operand planes or None) --------------------
def launch_direct(dev, c, ref, cfg=-1, must_split=False):
    """ops.conv2d: automatic plan (cfg -1; must_split: the plan has to cut K), or frcnn_set_tuning(0, cfg); the stem through fold_w"""
    from frcnn_hip import lib, ops
    OH, OW = R.out_hw(c)
    stem = c.Cin == 4
    nb = lib().frcnn_conv2d_workspace_bytes(c.N, OH, OW, c.Cout, c.k, c.k, c.Cin, 1 if stem else 0)
    assert (nb > 0) or not must_split, "the plan does not split %s" % c.id
    wd = T(ops.pack_filter_foldw(_hwio(ref.wf)[:, :, :3, :]), dev) if stem else T(ref.wf, dev)
    guard, out = _nan_guarded((c.N, OH, OW, c.Cout), dev)
    try:
        if cfg >= 0:
            lib().frcnn_set_tuning(0, cfg)
        ops.conv2d(T(ref.x, dev), wd, T(ref.bias, dev), c.k, c.k, c.stride, c.pad, c.act, T(ref.res, dev), max(c.res, 1), fold_w=stem, out=out)
        got = _result(guard, out, "conv2d")
    finally:
        lib().frcnn_set_tuning(0, -1)
        ops.split_k = True
    return got, None


def launch_winograd(dev, c, ref, m, products="f32"):
    """F(m x m, 3x3) as the chain input transform -> `products` -> output transform.  f32: ops.conv3x3_winograd; h2: the same call with
    u_planes (winograd_input_transform_h2 -> gemm_h2 -> winograd_output_transform_h2, which also emits the result as operand planes);
    x3: winograd_input_transform -> gemm_x3 over the points -> winograd_output_transform"""
    from frcnn_hip import ops
    assert c.k == 3 and c.stride == 1 and c.pad == R.SAME3 and not c.res
    u = T(ops.winograd_filter_transform(_hwio(ref.wf), None, m), dev)
    xd, bd = T(ref.x, dev), T(ref.bias, dev)
    guard, out = _nan_guarded((c.N, c.H, c.W, c.Cout), dev)
    planes = None
    if products == "f32":
        ops.conv3x3_winograd(xd, u, bd, c.act, out=out)
    elif products == "h2":
        planes = _fresh_planes(c.N * c.H * c.W, c.Cout, dev)
        ops.conv3x3_winograd(xd, u, bd, c.act, out=out, u_planes=ops.h2_pack_w(u), out_planes=planes)
    else:
        G, tiles = ops.winograd_points(m), ops.winograd_tiles(c.N, c.H, c.W, m)
        v = torch.full((G, tiles, c.Cin), float("nan"), dtype=torch.float32, device=dev)
        ops.winograd_input_transform(xd, v, m)
        mm = torch.full((G, tiles, c.Cout), float("nan"), dtype=torch.float32, device=dev)
        ops.gemm_x3(v, ops.gemm_x3_pack(u), G, tiles, c.Cout, c.Cin, out=mm)
        ops.winograd_output_transform(mm, bd, c.act, out, m)
    return _result(guard, out, "winograd m = %d (%s)" % (m, products)), planes


def launch_h2(dev, c, ref, cfg=-1, res_planes=False):
    """a 1x1 convolution as h2_split -> ops.gemm_h2, asked for the float32 result and its operand planes; the residual as float32 or,
    res_planes, as the operand planes of h2_split"""
    from frcnn_hip import ops
    assert c.k == 1 and c.stride == 1 and c.pad == R.ZERO
    M = c.N * c.H * c.W
    xp, wp = ops.h2_split(T(ref.x.reshape(M, c.Cin), dev)), ops.h2_pack_w(T(ref.wf, dev))
    rd = None
    if c.res:
        rd = T(ref.res_raw.reshape(M, c.Cout), dev)
        rd = ops.h2_split(rd) if res_planes else rd
    guard, out = _nan_guarded((M, c.Cout), dev)
    planes = _fresh_planes(M, c.Cout, dev)
    ops.gemm_h2(xp, wp, 1, M, c.Cout, c.Cin, T(ref.bias, dev), rd, c.act, out=out, out_planes=planes, cfg=cfg)
    return _result(guard, out, "gemm_h2 cfg %d" % cfg).reshape(c.N, c.H, c.W, c.Cout), planes


def launch_x3(dev, c, ref):
    from frcnn_hip import ops
    assert c.k == 1 and c.stride == 1 and c.pad == R.ZERO
    M = c.N * c.H * c.W
    guard, out = _nan_guarded((M, c.Cout), dev)
    rd = T(ref.res.reshape(M, c.Cout), dev) if c.res else None
    ops.gemm_x3(T(ref.x.reshape(M, c.Cin), dev), ops.gemm_x3_pack(T(ref.wf, dev)), 1, M, c.Cout, c.Cin, T(ref.bias, dev), rd, c.act, out=out, cfg=-1)
    return _result(guard, out, "gemm_x3").reshape(c.N, c.H, c.W, c.Cout), None


def launch_dw(dev, c, ref):
    from frcnn_hip import ops
    OH, OW = R.out_hw(c)
    guard, out = _nan_guarded((c.N, OH, OW, c.Cout), dev)
    ops.dwconv3x3(T(ref.x, dev), T(ref.wf, dev), T(ref.bias, dev), c.stride, c.pad, c.act, out=out)
    return _result(guard, out, "dwconv3x3"), None


_YARD = {}              # (yardstick, case id, kind, res_planes) -> the yardstick route's result on the same operands


def _yardstick(dev, route, c, kind, ref, res_planes=False):
    """the route the class rule measures `route` against (fwd_ref.YARDSTICK), on the same operands: the direct kernel under the automatic
    plan, or the Winograd chain of the same m with f32 products"""
    which = R.YARDSTICK[route]
    key = (which, c.id, kind, res_planes)
    if key not in _YARD:
        _YARD[key] = launch_direct(dev, c, ref)[0] if which == "direct" else launch_winograd(dev, c, ref, R.wino_m(route, c))[0]
    return _YARD[key]


def _check(dev, route, c, kind, ref, got, tag="", res_planes=False):
    """isfinite, the elementwise constant and, where the route has one, the class rule; one printed line per run"""
    cc = R.ROUTE_C[kind][route]
    assert got.shape == ref.want.shape
    r = R.ratio(got, ref.want, ref.B)
    line = "fwd %-10s %-18s %-6s %-12s: max |err| / (2^-23 B) = %8.3f (c = %g)" % (route, c.id, kind, tag, r, cc)
    ok = bool(np.isfinite(got).all()) and r <= cc
    if route in R.YARDSTICK:
        ry = R.ratio(_yardstick(dev, route, c, kind, ref, res_planes), ref.want, ref.B)
        line += "; %s %8.3f, ratio %.2f (<= %g)" % (R.YARDSTICK[route], ry, r / max(ry, 1e-30), R.CLASS_FACTOR[route])
        ok = ok and r <= R.CLASS_FACTOR[route] * ry + R.FLOOR
    print(line)
    assert ok, line


def _params(routes, variants=(None,)):
    """(route, case, kind, variant) in an order that keeps the runs of one (case, kind) together: fwd_ref.reference is computed once for them"""
    out = [(r, c, kind, v) for r in routes for c in R.CASES[r] for kind in R.KINDS for v in (variants if not callable(variants) else variants(r))]
    return out, ["%s-%s-%s%s" % (r, c.id, kind, "" if v is None else "-" + "_".join(str(t) for t in (v if isinstance(v, tuple) else (v,)))) for r, c, kind, v in out]


DIRECT, DIRECT_IDS = _params(("direct", "direct_cfg", "splitk", "stem"), lambda r: R.DIRECT_CFGS if r == "direct_cfg" else (-1,))


@pytest.mark.parametrize("p", DIRECT, ids=DIRECT_IDS)
def test_direct_conv_vs_float64(dev, p):
    """frcnn_conv2d_nhwc[_ws]: the automatic plan (64-row and 128-row tiles, the streaming GEMM, Cout <= 32 tiles), the forced
    k_conv_igemm configurations, split-K with its finish kernel (the plan must really split) and the stem's fold_w form"""
    route, c, kind, cfg = p
    ref = R.reference(route, c.id, kind)
    got, _ = launch_direct(dev, c, ref, cfg, must_split=(route == "splitk"))
    _check(dev, route, c, kind, ref, got, "cfg %d" % cfg)


WINO, WINO_IDS = _params(R.WINO_ROUTES)


@pytest.mark.parametrize("p", WINO, ids=WINO_IDS)
def test_winograd_chain_vs_float64(dev, p):
    """F(2,3), F(4,3) and the 7x7 scheme with f32 products, and the chains with h2 and x3 products that no other op-level test compares
    with float64; B is the tile's maximum (the transforms' rounding is shared by a tile's outputs)"""
    route, c, kind, _ = p
    ref = R.reference(route, c.id, kind)
    m = R.wino_m(route, c)
    products = {"wino_h2": "h2", "wino_x3": "x3"}.get(route, "f32")
    got, planes = launch_winograd(dev, c, ref, m, products)
    _check(dev, route, c, kind, ref, got, "m %d %s" % (m, products))
    if planes is not None:
        import h2_ref
        _same_planes(planes, h2_ref.split_grouped(got.reshape(-1, c.Cout), _wino_out_groups(m, c.N, c.H, c.W)))


H2, H2_IDS = _params(("h2",), [(cfg, rp) for rp in R.H2_RES for cfg in R.H2_CFGS])


@pytest.mark.parametrize("p", H2, ids=H2_IDS)
def test_gemm_h2_vs_float64(dev, p):
    """frcnn_gemm_h2 with bias + residual + ReLU under the by-shape choice and cfgs 9, 12 and 21; the emitted planes are the splitter's
    planes of the float32 result"""
    from frcnn_hip import ops
    route, c, kind, (cfg, res_form) = p
    rp = res_form == "planes"
    ref = R.reference(route, c.id, kind, rp)
    got, planes = launch_h2(dev, c, ref, cfg, rp)
    _check(dev, route, c, kind, ref, got, "cfg %d %s" % (cfg, res_form), rp)
    _same_planes(planes, _planes_np(ops.h2_split(T(got.reshape(-1, c.Cout), dev))))


X3, X3_IDS = _params(("x3",))


@pytest.mark.parametrize("p", X3, ids=X3_IDS)
def test_gemm_x3_vs_float64(dev, p):
    route, c, kind, _ = p
    ref = R.reference(route, c.id, kind)
    got, _ = launch_x3(dev, c, ref)
    _check(dev, route, c, kind, ref, got)


DW, DW_IDS = _params(("dw",))


@pytest.mark.parametrize("p", DW, ids=DW_IDS)
def test_dwconv3x3_vs_float64(dev, p):
    """nine fmaf and a bias: c = 8 covers the proven gamma_10 = 5, on either operand kind"""
    route, c, kind, _ = p
    ref = R.reference(route, c.id, kind)
    got, _ = launch_dw(dev, c, ref)
    _check(dev, route, c, kind, ref, got)
