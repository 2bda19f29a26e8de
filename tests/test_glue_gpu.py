"""GPU: the bandwidth-bound kernels between the convolutions at op level against the float64 statements of oracle/glue_ref.py -- max pool
and its gradient, spatial mean, row and RPN-pair softmax, column copy, column sum, softmax cross-entropy (row and RPN addressing), smooth
L1, dropout, the depthwise refold and the single-tensor sum of squares -- at the smallest shapes that reach each code path (partly filled
last workgroups, a second trip of the lane loop, the unrolled row loop's tail, leading dimensions wider than the data).

Exact kernels are compared bit for bit; bounded ones by glue_ref.excess(got, want, bound) <= glue_ref.ROOM, the bound derived in glue_ref
from the kernel's arithmetic (tests/test_glue_bounds_cpu.py shows each bound holds for a float32 emulation and fails every planted
mistake).  Every output the caller owns starts as NaN in front of a sentinel tail that must survive; input columns a kernel must not read
hold NaN.  Every bounded run prints max |err| / bound; the largest per kernel is recorded in oracle/glue_ref.py."""
import numpy as np
import pytest
import torch

import glue_ref as G

pytestmark = pytest.mark.gpu

SENT = 12345.5
IDS = lambda v: "-".join(str(t) for t in v).replace(" ", "") if isinstance(v, tuple) else str(v)       # noqa: E731


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _held(what, got, want, bound, nan_where_want=False):
    r = G.excess(got, want, bound, nan_where_want)
    line = "glue %-44s: max |err| / bound = %.3f (<= %g)" % (what, r, G.ROOM)
    print(line)
    assert r <= G.ROOM, line
    return r


# ---- max pool ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.MAXPOOL_KINDS + G.MAXPOOL_NAN)
@pytest.mark.parametrize("case", G.MAXPOOL_CASES, ids=IDS)
def test_maxpool_exact_and_keeps_nan(dev, case, kind):
    """zero pad on all sides when the top / left is padded, TF SAME otherwise, on inputs whose maximum is negative (the pad decides), of
    mixed sign, and holding -inf; and the NaN rule: NaN iff an in-image tap is NaN"""
    from frcnn_hip import ops
    N, H, W, C, k, s, pad = case
    x = G.maxpool_input(case, kind)
    want = G.maxpool(x, k, s, pad)
    guard, out = _nan_guarded(want.shape, dev)
    ops.maxpool(T(x, dev), k, s, pad, out=out)
    got = _result(guard, out, "maxpool")
    assert np.isnan(want).any() == (kind in G.MAXPOOL_NAN)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN iff an in-image tap of the window is NaN"
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("kind", G.MAXPOOL_BWD_KINDS)
@pytest.mark.parametrize("case", G.MAXPOOL_BWD_CASES, ids=IDS)
def test_maxpool_bwd_first_maximum(dev, case, kind):
    """ties everywhere: the window's gradient goes to its first maximum in scan order; bit-exact at k == stride, EPS B and
    conservation per (image, channel) where windows overlap"""
    from frcnn_hip import ops
    N, H, W, C, k, s = case
    x, dy = G.maxpool_bwd_input(case, kind)
    y = G.maxpool(x, k, s, G.same_pad(H, W, k, s))
    assert y.shape == dy.shape
    want, bound = G.maxpool_bwd(x, dy, k, s), G.maxpool_bwd_bound(x, dy, k, s)
    guard, dx = _nan_guarded(x.shape, dev)
    ops.maxpool_bwd(T(x, dev), T(y, dev), T(dy, dev), k, s, dx)
    got = _result(guard, dx, "maxpool_bwd")
    if k == s:
        assert np.array_equal(got, want)
        return
    _held("maxpool_bwd %s %s" % (IDS(case), kind), got, want, bound)
    d64 = dy.astype(np.float64)
    cons = np.abs(got.astype(np.float64).sum(axis=(1, 2)) - d64.sum(axis=(1, 2)))
    _held("maxpool_bwd %s %s conservation" % (IDS(case), kind), cons, 0.0, G.maxpool_bwd_conservation(dy, k, s))


# ---- spatial mean -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.MEAN_KINDS)
@pytest.mark.parametrize("case", G.MEAN_CASES, ids=IDS)
def test_spatial_mean_vs_float64(dev, case, kind):
    from frcnn_hip import ops
    x = G.mean_input(case, kind)
    guard, out = _nan_guarded((case[0], case[2]), dev)
    ops.spatial_mean(T(x, dev), out=out)
    _held("spatial_mean %s %s" % (IDS(case), kind), _result(guard, out, "spatial_mean"), G.spatial_mean(x), G.spatial_mean_bound(x))


# ---- softmax ----------------------------------------------------------------------------------------------------------------------------
def _softmax_checks(what, kind, x, got, want, bound):
    """x: the logits the kernel may read.  -inf entries give exactly 0; a NaN poisons its own row (pair) and nothing else"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN exactly where the row holds one" % what
    assert np.isnan(want).any() == (kind == "nan_row")
    if kind == "neg_inf":
        assert np.isinf(x).any() and np.all(got[np.isinf(x)] == 0)
    _held(what, got, want, bound, nan_where_want=True)


@pytest.mark.parametrize("kind", G.SOFTMAX_KINDS + G.SOFTMAX_NONFINITE)
@pytest.mark.parametrize("case", G.SOFTMAX_CASES, ids=IDS)
def test_softmax_rows_vs_float64(dev, case, kind):
    """C = 2 .. 130 (one to three trips of the lane loop), R % 4 != 0, ld > C with NaN in the columns beyond C"""
    from frcnn_hip import ops
    R, C, ld = case
    x = G.softmax_rows_input(case, kind)
    guard, out = _nan_guarded((R, C), dev)
    ops.softmax_rows(T(x, dev), C=C, out=out)
    got = _result(guard, out, "softmax_rows")
    _softmax_checks("softmax_rows %s %s" % (IDS(case), kind), kind, x[:, :C], got, G.softmax_rows(x[:, :C]), G.softmax_bound(x[:, :C], G.softmax_depth(C)))


@pytest.mark.parametrize("kind", G.RPN_KINDS + G.SOFTMAX_NONFINITE)
@pytest.mark.parametrize("case", G.RPN_CASES, ids=IDS)
def test_rpn_softmax_vs_float64(dev, case, kind):
    """A = 1, 9, 12, 15 with ld == 2A and ld > 2A; the pairs (+88, -88), (-88, +88) and equal"""
    from frcnn_hip import ops
    H, W, A, ld = case
    x = G.rpn_input(case, kind)
    guard, out = _nan_guarded((1, H, W, 2 * A), dev)
    ops.rpn_softmax(T(x.reshape(1, H, W, ld), dev), A, out=out)
    got = _result(guard, out, "rpn_softmax").reshape(H * W, 2 * A)
    _softmax_checks("rpn_softmax %s %s" % (IDS(case), kind), kind, x[:, :2 * A], got, G.rpn_softmax(x, A), G.rpn_softmax_bound(x, A))


@pytest.mark.parametrize("case", G.COPY_CASES, ids=IDS)
def test_copy_cols_exact(dev, case):
    from frcnn_hip import ops
    R, ld, col0, cols = case
    src = np.full((R, ld), np.nan, np.float32)
    src[:, col0:col0 + cols] = np.random.RandomState(R + ld).randn(R, cols)
    guard, out = _nan_guarded((R, cols), dev)
    ops.copy_cols(T(src, dev), col0, cols, out=out)
    assert np.array_equal(_bits(_result(guard, out, "copy_cols")), _bits(G.copy_cols(src, col0, cols)))


# ---- reductions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.COLSUM_CASES, ids=IDS)
def test_colsum_vs_float64(dev, case):
    """M around the four-way unrolled loop's edges (m + 48 < M), M < 16, C on both sides of the 64-column workgroup"""
    from frcnn_hip import ops
    dy = G.colsum_input(case)
    want, bound = G.colsum(dy)
    guard, out = _nan_guarded((case[1],), dev)
    ops.colsum(T(dy, dev), out)
    _held("colsum %s" % IDS(case), _result(guard, out, "colsum"), want, bound)


@pytest.mark.parametrize("accumulate", (False, True), ids=("fresh", "accumulate"))
@pytest.mark.parametrize("n", G.SUMSQ_N)
def test_sumsq_vs_float64(dev, n, accumulate):
    from frcnn_hip import ops
    w = (np.random.RandomState(n).randn(n) * 0.05).astype(np.float32)
    prev = np.float32(0.37) if accumulate else None
    want, bound = G.sumsq(w, 0.5 * 1e-4, prev)
    guard, out = _nan_guarded((1,), dev)
    if accumulate:
        out.fill_(float(prev))
    ops.sumsq(T(w, dev), 0.5 * 1e-4, out, accumulate)
    _held("sumsq n %d %s" % (n, "accumulate" if accumulate else "fresh"), _result(guard, out, "sumsq"), want, bound)


# ---- losses -----------------------------------------------------------------------------------------------------------------------------
def _ce_checks(what, labels, got_loss, got_grad, x_rows, lab_rows, grad_rows):
    loss, grad, lb, gb = G.softmax_ce(x_rows, lab_rows)
    if labels == "ignored":                     # n == 0: the kernel's defined result, exactly
        assert got_loss == 0.0 and not got_grad.any() and not np.isnan(got_grad).any()
        return
    _held(what + " loss", got_loss, loss, lb)
    _held(what + " grad", grad_rows, grad, gb)


@pytest.mark.parametrize("logits", G.CE_LOGITS)
@pytest.mark.parametrize("labels", G.CE_LABELS)
@pytest.mark.parametrize("case", G.CE_ROW_CASES, ids=IDS)
def test_softmax_ce_rows_vs_float64(dev, case, labels, logits):
    """R on both sides of one and two workgroups, C = 2, 21, 81; labels all valid, half ignored, all ignored; a logit spread of 2 and of 30"""
    from frcnn_hip import ops
    x, lab = G.ce_row_input(case, labels, logits)
    loss, grad = ops.softmax_ce_loss(T(x, dev), T(lab, dev))
    torch.cuda.synchronize()
    g = grad.cpu().numpy()
    _ce_checks("softmax_ce %s %s %s" % (IDS(case), labels, logits), labels, float(loss.item()), g, x, lab, g)


@pytest.mark.parametrize("logits", G.CE_LOGITS)
@pytest.mark.parametrize("labels", G.CE_LABELS)
@pytest.mark.parametrize("case", G.CE_RPN_CASES, ids=IDS)
def test_softmax_ce_rpn_vs_float64(dev, case, labels, logits):
    """the RPN addressing: element (a, h, w) pairs channels a and A + a of pixel (h, w); A = 1, 9, 12, 15"""
    from frcnn_hip import ops
    A, H, W = case
    score, lab = G.ce_rpn_input(case, labels, logits)
    loss, grad = ops.softmax_ce_loss(T(score, dev), T(lab, dev), rpn_shape=(A, H, W))
    torch.cuda.synchronize()
    g = grad.cpu().numpy()
    assert g.shape == score.shape
    x_rows, lab_rows = G.rpn_ce_rows(score, lab, A, H, W)
    _ce_checks("softmax_ce rpn %s %s %s" % (IDS(case), labels, logits), labels, float(loss.item()), g, x_rows, lab_rows, G.rpn_ce_rows(g, lab, A, H, W)[0])


@pytest.mark.parametrize("sd", G.SL1_SIGMA_DIV, ids=IDS)
@pytest.mark.parametrize("n", G.SL1_N)
def test_smooth_l1_vs_float64(dev, n, sd):
    """one element and partly filled workgroups; |d| one float32 step either side of 1 / sigma^2; negative d in the linear branch"""
    from frcnn_hip import ops
    sigma, div = sd
    pred, tgt, iw, ow = G.smooth_l1_input(n, sigma, div)
    want_loss, want_grad, lb, gb = G.smooth_l1(pred, tgt, iw, ow, sigma, div)
    loss, grad = ops.smooth_l1_loss(T(pred, dev), T(tgt, dev), T(iw, dev), T(ow, dev), sigma, div)
    torch.cuda.synchronize()
    what = "smooth_l1 n %d sigma %g div %g" % (n, sigma, div)
    _held(what + " loss", float(loss.item()), want_loss, lb)
    _held(what + " grad", grad.cpu().numpy(), want_grad, gb)


# ---- bit-exact elementwise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", G.DROPOUT_SEEDS)
@pytest.mark.parametrize("keep", G.DROPOUT_KEEP)
@pytest.mark.parametrize("n", G.DROPOUT_N)
def test_dropout_is_the_restated_mask(dev, n, keep, seed):
    """the device mask equals the numpy restatement of dropout_keep bit for bit; y = fl(fl(x / keep) * mask); the mask does not depend on
    x; in-place equals out-of-place"""
    from frcnn_hip import ops
    rng = np.random.RandomState(n)
    mask = G.dropout_keep(seed, n, keep)
    guard, out = _nan_guarded((n,), dev)
    ops.dropout(torch.ones(n, dtype=torch.float32, device=dev), seed, keep, out=out)
    assert np.array_equal(_bits(_result(guard, out, "dropout")), _bits((np.float32(1) / np.float32(keep)) * mask))
    for x in (rng.randn(n).astype(np.float32), (rng.rand(n) * 100 + 1).astype(np.float32)):
        guard, out = _nan_guarded((n,), dev)
        xd = T(x, dev)
        ops.dropout(xd, seed, keep, out=out)
        got = _result(guard, out, "dropout")
        assert np.array_equal(_bits(got), _bits(G.dropout(x, seed, keep)))
        assert np.array_equal(got != 0, mask != 0)
        ops.dropout(xd, seed, keep, out=xd)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(xd.cpu().numpy()), _bits(got)), "in place"


@pytest.mark.parametrize("C", G.REFOLD_C)
def test_dw_refold_exact(dev, C):
    from frcnn_hip import ops
    rng = np.random.RandomState(C)
    w, scale = rng.randn(3, 3, C).astype(np.float32), (rng.rand(C) + 0.5).astype(np.float32)
    guard, wf = _nan_guarded((3, 3, C), dev)
    ops.dwconv3x3_refold(T(w, dev), T(scale, dev), wf)
    assert np.array_equal(_bits(_result(guard, wf, "dwconv3x3_refold")), _bits(G.dw_refold(w, scale)))
