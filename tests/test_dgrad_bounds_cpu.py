"""CPU: the elementwise bound of tests/test_dgrad_gpu.py is sharp enough to matter.  For every route shape of oracle/dgrad_ref.CASES, both
operand sets and both accumulate modes, a float64 reference with the last output row or column of dY dropped, or with the pad shifted by
one pixel, FAILS the route's bound c 2^-23 B against the true result -- while the true result rounded to float32 passes it."""
import numpy as np
import pytest

import dgrad_ref as R

ROUTE_CASES = [(r, c) for r in R.CASES for c in R.CASES[r]]


@pytest.mark.parametrize("kind", ["random", "block4"])
@pytest.mark.parametrize("had", [False, True], ids=["fresh", "had"])
@pytest.mark.parametrize("rc", ROUTE_CASES, ids=["%s-%s" % (r, c[0]) for r, c in ROUTE_CASES])
def test_bound_rejects_a_dropped_border_or_shifted_pad(rc, had, kind):
    route, case = rc
    _, N, H, W, Cin, Cout, k, stride, pad = case
    gy, wf, x, res = R.operands(kind, N, H, W, Cin, Cout, k, stride, pad, seed=N + H + W + Cin + Cout, with_res=had)
    # the masks the GPU test applies: none for the heads behind fc7, none where the Winograd route accumulates, none in the gather kernel
    masked = not ((route == "padded" and H == 1) or (route == "winograd" and had) or route == "gather")
    mk = x if masked else None
    m = (7 if H == 7 and W == 7 else 4) if route == "winograd" else None
    B = R.bound(gy, wf, stride, pad, H, W, res, wino_m=m)
    c = R.ROUTE_C[route]
    want = R.finish(R.dgrad64(gy, wf, stride, pad, H, W), res, mk)
    assert R.ratio(want.astype(np.float32), want, B) <= min(c, 1.0)
    for name, dx in R.perturbed(gy, wf, stride, pad, H, W):
        r = R.ratio(R.finish(dx, res, mk), want, B)
        assert r > c, (route, case[0], name, r, c)


def test_tile_max_and_dgrad64_statement():
    """dgrad64 == torch autograd (float64) at an asymmetric pad; tile_max covers each m x m tile, ragged edges included"""
    import torch
    rng = np.random.RandomState(1)
    x = torch.from_numpy(rng.randn(2, 5, 9, 8)).requires_grad_(True)
    w = torch.from_numpy(rng.randn(6, 5, 3, 3))
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (0, 1, 1, 1)), w, stride=2)
    g = torch.from_numpy(rng.randn(*y.shape))
    y.backward(g)
    got = R.dgrad64(g.permute(0, 2, 3, 1).numpy(), w.permute(0, 2, 3, 1).numpy(), 2, (1, 1, 0, 1), 9, 8)
    assert np.allclose(got, x.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    b = rng.rand(1, 5, 6, 1)
    t = R.tile_max(b, 4)
    assert t[0, 0, 0, 0] == b[0, :4, :4].max() and t[0, 4, 5, 0] == b[0, 4:, 4:].max() and t[0, 4, 0, 0] == b[0, 4:, :4].max()
