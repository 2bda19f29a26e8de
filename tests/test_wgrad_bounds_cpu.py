"""CPU: the elementwise bounds of tests/test_wgrad_gpu.py (oracle/wgrad_ref.py) are sharp enough to matter, and the case list runs the
edges it claims.  For every case of wgrad_ref.CASES and the operand kinds 'random' and 'block4', under the float32 bound (B) and the h2
bound (B + 2^-16 F): the true result rounded to float32 passes with ratio <= 1, while a float64 reference with the last output row,
column or pixel of dY dropped, pixel 64 dropped, the pad shifted by one or kh / kw transposed FAILS c 2^-23 bound.  ('spread' is left out
of this proof on purpose: a pixel 2^-24 below its neighbours is below float32 resolution by construction.)  The h2 format in numpy
(h2_ref.wgrad_terms, exact accumulation) stays within c under the h2 bound on all three kinds and does NOT under plain B -- the floor term
is needed, not decorative.  plan(), the restatement of the kernels' launch plans, puts every loop and slice edge into CASES x PLANS."""
import numpy as np
import pytest

import h2_ref
import wgrad_ref as R

# wgrad_ref.reference() hands out read-only arrays; torch only reads them
pytestmark = pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")

IDS = [c[0] for c in R.CASES]


def _bounds(case, kind):
    gy, x, want, B, F = R.reference(case[0], kind)
    return gy, x, want, {"tn": B, "h2": B + 2.0 ** -16 * F}


@pytest.mark.parametrize("kind", ["random", "block4"])
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bounds_reject_a_dropped_pixel_shifted_pad_or_transposed_taps(case, kind):
    _, N, H, W, Cin, Cout, k, stride, pad = case
    gy, x, want, bounds = _bounds(case, kind)
    assert np.array_equal(bounds["h2"], R.bound(gy, x, k, stride, pad, "h2")) and np.array_equal(bounds["tn"], R.bound(gy, x, k, stride, pad, "tn"))
    for route, Bd in bounds.items():
        assert R.ratio(want.astype(np.float32), want, Bd) <= 1.0, route
    names = []
    for name, dw in R.perturbed(gy, x, k, stride, pad):
        names.append(name)
        for route, Bd in bounds.items():
            r = R.ratio(dw, want, Bd)
            assert r > R.ROUTE_C[route], (case[0], kind, name, route, r)
    M = gy.shape[0] * gy.shape[1] * gy.shape[2]
    assert len(names) == 3 + (M > 64) + 3 * (k > 1), names


def _h2_format(gy, x, k, stride, pad):
    """k_wgrad_h2's arithmetic with exact accumulation, tap by tap"""
    N, OH, OW, Cout = gy.shape
    out = np.empty((Cout, k, k, x.shape[-1]))
    for kh, kw, xt in R._taps(x, k, k, stride, pad, OH, OW):
        out[:, kh, kw, :] = h2_ref.wgrad_terms(gy.reshape(-1, Cout), xt.astype(np.float32))
    return out


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_h2_format_stays_inside_the_h2_bound(case, kind):
    _, N, H, W, Cin, Cout, k, stride, pad = case
    gy, x, want, bounds = _bounds(case, kind)
    got = _h2_format(gy, x, k, stride, pad)
    r = R.ratio(got, want, bounds["h2"])
    print("h2 format %s %s: max |err| / (2^-23 (B + 2^-16 F)) = %.3f, against plain B %.3g" % (case[0], kind, r, R.ratio(got, want, bounds["tn"])))
    assert r <= R.ROUTE_C["h2"], r
    if case[0] == "m20" and kind == "block4":
        # x holds 1e-30 beside values of order 1 (dgrad_ref._edge_values): scaled by its slab's 2^e it lies below the remainder piece's
        # smallest subnormal and comes back 0 -- an error of the whole element where dY gates every other pixel of that channel out
        assert R.ratio(got, want, bounds["tn"]) > R.ROUTE_C["h2"]


def _launches(route):
    for case in R.CASES:
        _, N, H, W, Cin, Cout, k, stride, pad = case
        OH, OW = R.out_hw(case)
        M = N * OH * OW
        for pl in R.PLANS:
            BT, S, chunk = R.plan(route, M, Cin, Cout, k * k * Cin, *pl)
            yield case[0], pl, M, BT, S, R.slices(route, M, S, chunk)


@pytest.mark.parametrize("route", ["tn", "h2"])
def test_case_list_runs_every_loop_and_slice_edge(route):
    L = list(_launches(route))
    slab = R.SLAB[route]
    for _, _, M, BT, S, sl in L:
        assert len(sl) == S and sum(sl) == R.cdiv(M, slab) and min(sl) >= 1 and BT in (64, 128)
    assert any(S == 1 for _, _, _, _, S, _ in L)
    assert any(S > 1 for _, _, _, _, S, _ in L)
    assert any(1 in sl for _, _, _, _, _, sl in L)                                       # nloc == 1
    assert any(S > 1 and sl[-1] < sl[0] for _, _, _, _, S, sl in L)                      # a last slice shorter than the rest
    assert any(M < slab for _, _, M, _, _, _ in L)
    assert any(M % slab == 1 for _, _, M, _, _, _ in L)
    assert any(BT == 128 for _, _, _, BT, _, _ in L) and any(BT == 64 for _, _, _, BT, _, _ in L)
    if route == "h2":
        assert any(BT == 64 and any(n % 2 and n >= 3 for n in sl) for _, _, _, BT, _, sl in L)      # an odd count under two register sets
        # load_slab's incremental (img, oh, ow): a gathered launch whose images end inside a thread's run of 4 (BT 64) / 8 (BT 128) pixels,
        # at stride 1 and at stride 2
        geo = {c[0]: (c[1], R.out_hw(c)[0] * R.out_hw(c)[1], c[7]) for c in R.CASES if c[6] > 1 or c[7] > 1}
        for bt, run in ((64, 4), (128, 8)):
            for stride in (1, 2):
                assert any(BT == bt and cid in geo and geo[cid][0] > 1 and geo[cid][1] % run and geo[cid][2] == stride
                           for cid, _, _, BT, _, _ in L), (bt, stride)
    # Cin = 192: 128-wide tiles are refused even when asked for
    assert all(BT == 64 for cid, _, _, BT, _, _ in L if cid == "c192_3x3")
    by = {(cid, pl): (S, sl) for cid, pl, _, _, S, sl in L}
    S, sl = by[("pw_37x63", (128, 4096))]
    assert (S, sl[0], sl[-1]) == ((15, 5, 3) if route == "tn" else (13, 3, 1))


def test_case_geometry_is_what_the_comments_say():
    by = {c[0]: c for c in R.CASES}
    assert R.out_hw(by["n3_s2_m60"]) == (4, 5) and R.out_hw(by["n3_s2_m45"]) == (3, 5) and R.out_hw(by["n5_1x1s2"]) == (4, 4) and R.out_hw(by["row_1x40"]) == (1, 40)
    gy, x, want, B, F = R.reference("row_1x40", "random")
    assert not want[:, 0].any() and not want[:, 2].any() and not B[:, 0].any() and not F[:, 2].any() and want[:, 1].all(axis=(0, 2)).all()
    for case in R.DW_CASES:
        _, N, H, W, C, stride, pad = case
        M = N * R.conv_out(H, 3, stride, pad[0], pad[1]) * R.conv_out(W, 3, stride, pad[2], pad[3])
        assert {"two_chunks": M == 4160, "one_chunk_exact": M == 4096, "s2_three_images": M == 4218}.get(case[0], M < R.DW_CHUNK)


def test_dw_wgrad64_statement():
    """dw_wgrad64 == torch float64 autograd of the folded depthwise convolution, at an asymmetric pad and stride 2, w.r.t. the master filter"""
    import torch
    rng = np.random.RandomState(2)
    N, H, W, C, stride, pad = 2, 9, 12, 8, 2, (0, 1, 0, 1)
    x = rng.randn(N, H, W, C)
    scale = rng.rand(C) + 0.5
    wt = torch.from_numpy(rng.randn(3, 3, C)).requires_grad_(True)
    wf = (wt * torch.from_numpy(scale)[None, None, :]).permute(2, 0, 1)[:, None]
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, (pad[2], pad[3], pad[0], pad[1])), wf, stride=stride, groups=C)
    g = rng.randn(N, y.shape[2], y.shape[3], C)
    y.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
    assert tuple(y.shape[2:]) == (4, 6)
    assert np.allclose(R.dw_wgrad64(g, x, stride, pad, scale), wt.grad.numpy(), rtol=1e-12, atol=1e-12)
    for case in R.DW_CASES:
        g, x, scale = R.dw_operands(case)
        want, B = R.dw_wgrad64(g, x, case[5], case[6], scale), R.dw_bound(g, x, case[5], case[6], scale)
        assert R.ratio(want.astype(np.float32), want, B) <= 1.0
        M = g.size // g.shape[-1]
        for m in [M - 1] + ([R.DW_CHUNK] if M > R.DW_CHUNK else []):                       # the last pixel; the first of the second chunk
            g2 = g.copy()
            g2.reshape(M, -1)[m] = 0
            assert R.ratio(R.dw_wgrad64(g2, x, case[5], case[6], scale), want, B) > R.ROUTE_C["dw"], (case[0], m)


def test_wgrad64_statement():
    """wgrad64 == torch float64 autograd of the convolution at an asymmetric pad and stride 2"""
    import torch
    rng = np.random.RandomState(5)
    N, H, W, Cin, Cout, k, stride, pad = 2, 9, 12, 6, 5, 3, 2, (0, 1, 0, 1)
    x = rng.randn(N, H, W, Cin)
    w = torch.zeros((Cout, Cin, k, k), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (pad[2], pad[3], pad[0], pad[1])), w, stride=stride)
    g = rng.randn(N, y.shape[2], y.shape[3], Cout)
    y.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
    assert np.allclose(R.wgrad64(g, x, k, k, stride, pad), w.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
