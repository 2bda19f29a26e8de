"""GPU: frcnn_conv2d_wgrad (csrc/wgrad_tn.hip, f32 matrix pipe), frcnn_conv2d_wgrad_h2 (csrc/wgrad_h2.hip, two-piece fp16 operands
split in registers) -- the filter gradient of slim.conv2d read straight from dY and X in NHWC -- and frcnn_dwconv3x3_wgrad against the
float64 statement of the same sum (oracle/wgrad_ref.py), over the layer kinds of the three backbones' reverse sweeps (pointwise, strided
shortcut, 3x3 SAME, 3x3 stride 2 with conv2d_same's explicit padding, the RoI tail's 7x7 maps, a fully connected layer as a 1x1
convolution) and the loop and slice edges of the kernels (a pixel count below one slab, one past a slab, an odd slab count, a shorter last
slice, an image boundary inside one thread's pixel run, taps that are padding everywhere, Cin = 192), both tile sizes, one slice and many,
on three operand sets (wgrad_ref.operands: random, shaped like the block4 tail, a per-pixel 2^+-12 spread).

Three bounds, all must hold: max |err| / max |dW| <= 2e-6; elementwise |got - want| <= c 2^-23 bound with bound = the float64 sum on |dY|, |X|
(for h2 plus the derived format floor, wgrad_ref.bound) and c = wgrad_ref.ROUTE_C; and for h2 the f32 class against the f32 kernel on
the same data.  tests/test_wgrad_bounds_cpu.py proves that the elementwise bound rejects one dropped pixel, a shifted pad and transposed
taps on every case.  Every output starts as NaN in front of a sentinel tail that must survive."""
import ctypes

import numpy as np
import pytest
import torch

import wgrad_ref as R

# wgrad_ref.reference() hands out read-only arrays; torch only reads them
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

CASES = R.CASES
SENT = 12345.5
BY_ID = {c[0]: c for c in CASES}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan_guarded(shape, dev):
    """(whole buffer, the output view filled with NaN): 4096 sentinel floats behind the output must survive the launch"""
    n = int(np.prod(shape))
    g = torch.full((n + 4096,), SENT, dtype=torch.float32, device=dev)
    v = g[:n].view(shape)
    v.fill_(float("nan"))
    return g, v


def _tail_ok(g, shape):
    return bool((g[int(np.prod(shape)):] == SENT).all())


def _geometry(case):
    _, N, H, W, Cin, Cout, k, stride, pad = case
    OH, OW = R.out_hw(case)
    return N * OH * OW, OH, OW


def _setter(h2):
    from frcnn_hip import lib
    return lib().frcnn_conv2d_wgrad_h2_set_plan if h2 else lib().frcnn_conv2d_wgrad_set_plan


def _launch(dev, case, gyd, xd, plan, h2, check_plan=True):
    """one filter gradient under `plan` -> float32 [Cout,k,k,Cin] on the host.  The restated plan must be the library's: S slices <=>
    S partial gradients of workspace (none when S == 1)."""
    from frcnn_hip import lib, ops
    _, N, H, W, Cin, Cout, k, stride, pad = case
    M, OH, OW = _geometry(case)
    guard, out = _nan_guarded((Cout, k, k, Cin), dev)
    setter = _setter(h2)
    setter(*plan)
    try:
        if check_plan:
            BT, S, chunk = R.plan("h2" if h2 else "tn", M, Cin, Cout, k * k * Cin, *plan)
            nb = (lib().frcnn_conv2d_wgrad_h2_workspace_bytes if h2 else lib().frcnn_conv2d_wgrad_workspace_bytes)(N, OH, OW, Cin, Cout, k, k)
            assert nb == (S * 4 * Cout * k * k * Cin if S > 1 else 0), (nb, S, BT, chunk)
        ops.conv2d_wgrad(gyd, xd, k, k, stride, pad, out, h2=h2)
        torch.cuda.synchronize()
    finally:
        setter(0, 0)
    got = out.cpu().numpy()
    assert _tail_ok(guard, out.shape)
    return got


_TN_AUTO = {}           # (case id, kind) -> the f32 kernel's result under the automatic plan, the yardstick of the h2 class assertion


def _tn_auto(dev, case, kind, gyd, xd):
    key = (case[0], kind)
    if key not in _TN_AUTO:
        _TN_AUTO[key] = _launch(dev, case, gyd, xd, (0, 0), False, check_plan=False)
    return _TN_AUTO[key]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("plan", R.PLANS, ids=R.PLAN_IDS)
@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
def test_conv2d_wgrad_vs_float64_autograd(dev, case, plan, h2):
    """every operand kind of wgrad_ref.KINDS in turn (the float64 side is computed once per (case, kind) and shared)"""
    from frcnn_hip import ops
    _, N, H, W, Cin, Cout, k, stride, pad = case
    assert ops.conv2d_wgrad_supported(Cin, Cout) and not ops.conv2d_wgrad_supported(Cin, 21) and not ops.conv2d_wgrad_supported(3, Cout)
    route = "h2" if h2 else "tn"
    failures = []
    for kind in R.KINDS:
        gy, x, want, B, F = R.reference(case[0], kind)
        Bd = B + 2.0 ** -16 * F if h2 else B
        gyd, xd = T(gy, dev), T(x, dev)
        got = _launch(dev, case, gyd, xd, plan, h2).astype(np.float64)
        err = np.abs(got - want).max() / np.abs(want).max()
        r = R.ratio(got, want, Bd)
        line = "wgrad route=%s kind=%s case=%s plan=%s: max err / max |dW| = %.2e, max |err| / (2^-23 bound) = %.3f" % (route, kind, case[0], plan, err, r)
        ok = bool(np.isfinite(got).all()) and err <= 2e-6 and r <= R.ROUTE_C[route]
        if h2:
            r32 = R.ratio(_tn_auto(dev, case, kind, gyd, xd), want, Bd)
            line += ", f32 TN %.3f, h2 / f32 = %.2f" % (r32, r / max(r32, 1e-30))
            ok = ok and r <= R.CLASS_FACTOR_H2 * r32 + R.CLASS_FLOOR
        print(line)
        if not ok:
            failures.append(line)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
def test_conv2d_wgrad_taps_that_are_padding_everywhere_are_exactly_zero(dev, h2):
    """row_1x40: a single pixel row under a 3x3 SAME filter -- the taps of filter rows 0 and 2 read padding for every pixel.  Their X slabs
    are all zeros (in k_wgrad_h2 they take the clamped scale 2^126) and dW there is +0.0 bit for bit, whatever dY holds"""
    case = BY_ID["row_1x40"]
    gy, x, want, B, F = R.reference(case[0], "spread")
    gyd, xd = T(gy, dev), T(x, dev)
    for plan in R.PLANS:
        got = _launch(dev, case, gyd, xd, plan, h2)
        assert not got[:, 0].view(np.uint32).any() and not got[:, 2].view(np.uint32).any(), plan
        assert got[:, 1].all()


@pytest.mark.parametrize("case", [BY_ID["pointwise"], BY_ID["m65"]], ids=["pointwise", "m65"])
@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
def test_conv2d_wgrad_nonfinite_operands_stay_nonfinite_and_stay_put(dev, case, h2):
    """The rule of csrc/common.h (no kernel turns inf / nan into finite garbage): one NaN in dY[m, n] makes row dW[n] entirely NaN, one
    +inf in X[m, c] makes column dW[:, 0, 0, c] entirely non-finite, and every other element keeps the bits of the clean run under the same
    plan.  Two launches of the clean run give the same bits (slices are added in a fixed order, no atomics in HBM).  The pixel is the last
    one: in a ragged last slab, beside the zero rows past M."""
    _, N, H, W, Cin, Cout, k, stride, pad = case
    M, OH, OW = _geometry(case)
    gy, x, _, _, _ = R.reference(case[0], "random")
    m, n, c = M - 1, 5, Cin - 3
    gy_nan = np.array(gy, copy=True)
    gy_nan.reshape(M, Cout)[m, n] = np.nan
    x_inf = np.array(x, copy=True)
    x_inf.reshape(M, Cin)[m, c] = np.inf
    gyd, xd, gnd, xid = T(gy, dev), T(x, dev), T(gy_nan, dev), T(x_inf, dev)
    for plan in R.PLANS:
        clean = _launch(dev, case, gyd, xd, plan, h2)
        assert np.isfinite(clean).all()
        assert np.array_equal(clean.view(np.uint32), _launch(dev, case, gyd, xd, plan, h2).view(np.uint32)), plan
        got = _launch(dev, case, gnd, xd, plan, h2)
        assert np.isnan(got[n]).all(), (plan, "row of the NaN")
        rest = np.arange(Cout) != n
        assert np.array_equal(got[rest].view(np.uint32), clean[rest].view(np.uint32)), (plan, "beside the NaN row")
        got = _launch(dev, case, gyd, xid, plan, h2)
        assert not np.isfinite(got[:, 0, 0, c]).any(), (plan, "column of the inf")
        rest = np.arange(Cin) != c
        assert np.array_equal(got[..., rest].view(np.uint32), clean[..., rest].view(np.uint32)), (plan, "beside the inf column")


@pytest.mark.parametrize("case", [BY_ID["pw_37x63"], BY_ID["roi37_3x3"], BY_ID["n3_s2_m60"]], ids=["pw_37x63", "roi37_3x3", "n3_s2_m60"])
@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
def test_conv2d_wgrad_is_deterministic(dev, case, h2):
    gy, x, _, _, _ = R.reference(case[0], "block4")
    gyd, xd = T(gy, dev), T(x, dev)
    for plan in R.PLANS:
        a, b = _launch(dev, case, gyd, xd, plan, h2), _launch(dev, case, gyd, xd, plan, h2)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), plan


@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
def test_conv2d_wgrad_without_its_workspace_is_refused_and_writes_nothing(dev, h2):
    """the raw ABI on a plan with S > 1 and ws = NULL (or one byte short): FRCNN_E_WS, and the NaN-filled output is untouched"""
    from frcnn_hip import lib
    case = BY_ID["pointwise"]
    _, N, H, W, Cin, Cout, k, stride, pad = case
    M, OH, OW = _geometry(case)
    gy, x, _, _, _ = R.reference(case[0], "random")
    gyd, xd = T(gy, dev), T(x, dev)
    guard, out = _nan_guarded((Cout, k, k, Cin), dev)
    fn = lib().frcnn_conv2d_wgrad_h2 if h2 else lib().frcnn_conv2d_wgrad
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    setter = _setter(h2)
    setter(128, 4096)
    try:
        BT, S, chunk = R.plan("h2" if h2 else "tn", M, Cin, Cout, k * k * Cin, 128, 4096)
        assert S > 1
        need = S * 4 * Cout * k * k * Cin
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        for wsp, nb in ((None, 0), (None, need), (ws, need - 1)):
            rc = fn(P(gyd), P(xd), N, H, W, Cin, OH, OW, Cout, k, k, stride, pad[0], pad[2], P(out), P(wsp), nb, stream)
            torch.cuda.synchronize()
            assert rc == -2, (rc, nb)                                                 # FRCNN_E_WS
            assert bool(torch.isnan(out).all()) and _tail_ok(guard, out.shape)
        rc = fn(P(gyd), P(xd), N, H, W, Cin, OH, OW, Cout, k, k, stride, pad[0], pad[2], P(out), P(ws), need, stream)
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isfinite(out).all()) and _tail_ok(guard, out.shape)
    finally:
        setter(0, 0)


@pytest.mark.parametrize("case", R.DW_CASES, ids=[c[0] for c in R.DW_CASES])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_dwconv3x3_wgrad_vs_float64(dev, case, scaled):
    """frcnn_dwconv3x3_wgrad (k_dwconv3x3_wgrad: pixel chunks of 4096 x channel groups of 64, partials added in order) with more than one
    chunk, a chunk edge inside an image, a ragged channel group, with and without the frozen-BN scale: elementwise
    |got - want| <= c 2^-23 B, and the sentinel behind dw survives"""
    from frcnn_hip import ops
    _, N, H, W, C, stride, pad = case
    g, x, scale = R.dw_operands(case)
    sc = scale if scaled else None
    want, B = R.dw_wgrad64(g, x, stride, pad, sc), R.dw_bound(g, x, stride, pad, sc)
    guard, dw = _nan_guarded((3, 3, C), dev)
    ops.dwconv3x3_wgrad(T(g, dev), T(x, dev), stride, pad, T(scale, dev) if scaled else None, dw)
    torch.cuda.synchronize()
    got = dw.cpu().numpy().astype(np.float64)
    r = R.ratio(got, want, B)
    print("wgrad route=dw kind=random case=%s %s: max err / max |dW| = %.2e, max |err| / (2^-23 bound) = %.3f"
          % (case[0], "scaled" if scaled else "plain", np.abs(got - want).max() / np.abs(want).max(), r))
    assert np.isfinite(got).all() and _tail_ok(guard, dw.shape)
    assert r <= R.ROUTE_C["dw"], r


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
