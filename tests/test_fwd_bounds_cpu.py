"""CPU: the elementwise bound of tests/test_fwd_gpu.py (oracle/fwd_ref.py) is sharp enough to matter and loose enough to be met.  For every
route, case and operand kind of fwd_ref.CASES: the float64 result rounded to float32 passes with ratio <= 1; a plain float32 statement of
the same convolution (torch on the CPU) passes with half the route's constant to spare; and every reference of fwd_ref.perturbed -- the
last input row or column read taken as zero, the pad shifted by one, the taps transposed, the bias left out, the residual read one pixel
late -- FAILS c 2^-23 B.  The constants themselves are checked against the rules they were set by."""
import numpy as np
import pytest

import dgrad_ref
import fwd_ref as R

# fwd_ref.reference() hands out read-only arrays; torch only reads them
pytestmark = pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")

ROUTE_CASES = [(r, c) for r in R.CASES for c in R.CASES[r]]
IDS = ["%s-%s" % (r, c.id) for r, c in ROUTE_CASES]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("rc", ROUTE_CASES, ids=IDS)
def test_bound_passes_float32_and_rejects_every_perturbed_reference(rc, kind):
    route, c = rc
    x, wf, bias, res, want, B, _ = R.reference(route, c.id, kind)
    dw, rs, cc = route == "dw", max(c.res, 1), R.ROUTE_C[kind][route]
    assert want.shape == (c.N,) + R.out_hw(c) + (c.Cout,) and B.shape == want.shape
    assert R.ratio(want.astype(np.float32), want, B) <= 1.0
    r32 = R.ratio(R.conv32(x, wf, bias, c.stride, c.pad, res, rs, c.act, dw), want, B)
    names, least = [], np.inf
    for name, ref in R.perturbed(x, wf, bias, c.stride, c.pad, res, rs, c.act, dw):
        names.append(name)
        r = R.ratio(ref, want, B)
        least = min(least, r)
        assert r > cc, (route, c.id, kind, name, r, cc)
    print("fwd bound %-10s %-18s %-6s: float32 statement %.2f (c / 2 = %g), least rejected perturbation %.3g" % (route, c.id, kind, r32, cc / 2, least))
    assert r32 <= cc / 2, (route, c.id, kind, r32, cc)
    single_pixel = c.H == 1 and c.W == 1
    assert len(names) == 4 + (c.k > 1 and not single_pixel) + bool(c.bias) + bool(c.res), names


def test_constants_follow_their_rules():
    assert set(R.ROUTE_C["random"]) == set(R.ROUTE_C["trunk"]) == set(R.CASES) == set(R.CAP)
    for route, c in R.ROUTE_C["random"].items():
        assert R.ROUTE_C["trunk"][route] == (c if route == "dw" else 4.0 * c), route
        assert R.ROUTE_C["trunk"][route] < R.CAP[route] and c < R.CAP[route], route
    assert R.CAP["direct"] == 2e-5 / R.EPS and R.CAP["wino4"] == 1e-4 / R.EPS
    for route in ("direct", "direct_cfg", "splitk", "stem"):
        assert R.ROUTE_C["random"][route] == dgrad_ref.ROUTE_C["flipped"]
    assert R.ROUTE_C["random"]["h2"] == dgrad_ref.ROUTE_C["h2"]
    for route in R.WINO_ROUTES:
        assert R.ROUTE_C["random"][route] == dgrad_ref.ROUTE_C["winograd"]
    assert R.ROUTE_C["random"]["x3"] == 3 * R.ROUTE_C["random"]["direct"]
    assert R.ROUTE_C["random"]["dw"] >= 5.0                                   # gamma_10: nine fmaf and a bias
    assert R.FLOOR == 1e-7 / R.EPS and R.EPS is dgrad_ref.EPS and R.ratio is dgrad_ref.ratio and R.tile_max is dgrad_ref.tile_max
    assert set(R.CLASS_FACTOR) == set(R.YARDSTICK) and R.CLASS_FACTOR["wino4"] == dgrad_ref.CLASS_FACTOR["winograd"]


def test_case_ids_are_unique_and_geometry_is_what_the_comments_say():
    ids = [c.id for r in R.CASES for c in R.CASES[r]]
    assert len(ids) == len(set(ids))
    by = {c.id: c for r in R.CASES for c in R.CASES[r]}
    assert R.out_hw(by["same_s2_37x63"]) == (19, 32) and R.out_hw(by["tfsame_s2_34x51"]) == (17, 25) and R.out_hw(by["stem_22x30"]) == (11, 15)
    c = by["tail27_37x63"]
    assert (c.N * c.H * c.W) % 128 == 27
    c = by["x3_3x43_k2048"]
    assert c.N * c.H * c.W == 129 and by["x3_37x63_k96"].Cin // 32 == 3 and by["x3_17x26_n192"].Cout % 128
    assert by["h2_long_k_17x26"].Cin // 128 == 8
    for c in R.CASES["wino7"]:
        assert c.H == 7 and c.W == 7
    for route in ("wino_h2", "wino_x3"):
        assert all(R.wino_m(route, c) in (2, 4, 7) for c in R.CASES[route])
    assert R.wino_m("wino2", by["pixel_m2"]) == 2 and R.wino_m("direct", by["valid_9x11"]) is None
    # every direct / h2 / x3 / Winograd launch needs Cin % 32 == 0 (the stem: 4), the h2 forms K % 128 == 0 and N % 128 == 0
    for route, c in ROUTE_CASES:
        assert c.Cin % 32 == 0 or route == "stem", c.id
        if route in ("h2", "wino_h2"):
            assert c.Cin % 128 == 0 and c.Cout % 128 == 0, c.id


def test_a_strided_shortcut_on_an_even_size_does_not_read_the_last_row():
    """why perturbed() zeroes the last row READ: zeroing the literal last row of a 1x1 stride-2 input of even height changes nothing"""
    c = R.find("direct", "shortcut_s2_34x51")
    assert R.last_read(c.H, 1, 2, 0, 0) == c.H - 2 and R.last_read(c.W, 1, 2, 0, 0) == c.W - 1
    x, wf, bias, res, want, B, _ = R.reference("direct", c.id, "random")
    z = np.array(x, copy=True)
    z[:, -1] = 0
    assert R.ratio(R.conv64(z, wf, bias, c.stride, c.pad, act=c.act), want, B) == 0.0
    assert R.last_read(37, 3, 2, 1, 1) == 36 and R.last_read(34, 3, 2, 1, 1) == 33 and R.last_read(34, 3, 2, 0, 1) == 33 and R.last_read(22, 7, 2, 3, 3) == 21


def test_conv64_statement():
    """conv64 == torch float64 conv2d at an asymmetric pad and stride 2 with a strided residual and ReLU6; the depthwise form likewise;
    a negative pad cuts rows off; trunk operands are what the docstring says"""
    import torch
    F = torch.nn.functional
    rng = np.random.RandomState(1)
    x, w, b = rng.randn(2, 9, 12, 6), rng.randn(5, 3, 3, 6), rng.randn(5)
    res = rng.randn(2, 8, 12, 5)
    y = F.conv2d(F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (0, 1, 1, 0)), torch.from_numpy(w).permute(0, 3, 1, 2), torch.from_numpy(b), stride=2)
    assert tuple(y.shape[2:]) == (4, 6)
    want = (y.permute(0, 2, 3, 1) + torch.from_numpy(res)[:, ::2, ::2]).clamp(0, 6).numpy()
    assert np.allclose(R.conv64(x, w, b, 2, (1, 0, 0, 1), res, 2, 2), want, rtol=1e-12, atol=1e-12)
    wd = rng.randn(3, 3, 6)
    y = F.conv2d(F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (0, 1, 0, 1)), torch.from_numpy(wd).permute(2, 0, 1)[:, None], None, stride=2, groups=6)
    assert np.allclose(R.conv64(x, wd, None, 2, (0, 1, 0, 1), depthwise=True), y.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.conv32(x, w, b, 2, (1, 0, 0, 1), res, 2, 2), want, rtol=1e-4, atol=1e-4)
    assert np.allclose(R.conv32(x, wd, None, 2, (0, 1, 0, 1), depthwise=True), y.permute(0, 2, 3, 1).numpy(), rtol=1e-4, atol=1e-4)
    # a bottom pad of -1 cuts the last row of x off: one output row fewer, the others as under a bottom pad of 0
    cut = R.conv64(x, w, None, 1, (2, -1, 1, 1))
    assert cut.shape[1] == 8 and np.array_equal(cut, R.conv64(x, w, None, 1, (2, 0, 1, 1))[:, :8])
    assert np.array_equal(R.conv64(x, w, None, 1, (2, 0, 1, 1))[:, 1:], R.conv64(x, w, None, 1, (1, 1, 1, 1))[:, :8])
    c = R.find("direct", "res2_20x24")
    xt, _, _, rt = R.operands("trunk", c)
    xr, _, _, rr = R.operands("random", c)
    assert rt.shape == rr.shape == (1, 20, 24, 128) and xt.dtype == np.float32 and xt.min() >= 0
    assert np.abs(xt).max() > 64 * np.abs(xr).max() and (xt == 0).any() and (xt == np.float32(1e-30)).any()
    img = R.operands("random", R.find("stem", "stem_21x29"))[0]
    assert not img[..., 3].any() and -110 <= img.min() < -100 and 135 < img.max() <= 145
