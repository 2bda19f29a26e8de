"""CPU: the bounds tests/test_glue_gpu.py holds the bandwidth-bound kernels to (oracle/glue_ref.py) can be met and cannot be met by accident.
For every bounded kernel a float32 numpy emulation of the kernel's own order of operations stays inside the UN-doubled bound (the device
assertion doubles it) on every case and input kind the GPU test runs; and every planted mistake of glue_ref.MUTANTS exceeds the doubled
bound -- or breaks the equality an exact kernel is held to -- on every case it applies to.  The max-pool kernel before the NaN rule (plain
fmaxf) is kept as one more mutant: it fails both NaN kinds on every shape.  The dropout mask's numpy restatement is checked for its kept
fraction and for independence between adjacent seeds."""
import numpy as np
import pytest

import glue_ref as G

IDS = lambda v: "-".join(str(t) for t in v).replace(" ", "") if isinstance(v, tuple) else str(v)       # noqa: E731


def _applies(op, *args):
    return [name for name, pred in G.MUTANTS[op] if pred(*args)]


# ---- exact kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.MAXPOOL_KINDS)
@pytest.mark.parametrize("case", G.MAXPOOL_CASES, ids=IDS)
def test_maxpool_mutants_break_equality(case, kind):
    N, H, W, C, k, s, pad = case
    x = G.maxpool_input(case, kind)
    want = G.maxpool(x, k, s, pad)
    assert want.dtype == np.float32 and not np.isnan(want).any()
    assert np.array_equal(G.maxpool(x, k, s, pad, mutant="fmaxf"), want), "NaN-free input: the fmaxf form is the same function"
    names = _applies("maxpool", case)
    assert "shifted" in names and len(names) == 1 + G.maxpool_has_oob(H, W, k, s, pad)
    for name in names:
        assert not np.array_equal(G.maxpool(x, k, s, pad, mutant=name), want), (case, kind, name)


@pytest.mark.parametrize("kind", G.MAXPOOL_NAN)
@pytest.mark.parametrize("case", G.MAXPOOL_CASES, ids=IDS)
def test_maxpool_nan_rule_fails_the_fmaxf_kernel(case, kind):
    """NaN iff an in-image tap is NaN; the kernel of the parent commit (fmaxf from -inf, fmaxf(m, 0) under the zero pad) returns a finite
    number, -inf or 0 there"""
    N, H, W, C, k, s, pad = case
    x = G.maxpool_input(case, kind)
    want = G.maxpool(x, k, s, pad)
    old = G.maxpool(x, k, s, pad, mutant="fmaxf")
    assert np.isnan(want).any() and not np.isnan(old).any()
    assert not np.array_equal(old, want, equal_nan=True)
    assert np.array_equal(old[~np.isnan(want)], want[~np.isnan(want)])
    # the rule itself, window by window, against a direct statement
    for n, oh, ow, c in zip(*np.nonzero(np.ones(want.shape, bool))):
        r0, c0 = oh * s - pad[0], ow * s - pad[2]
        win = x[n, max(r0, 0):max(r0 + k, 0), max(c0, 0):max(c0 + k, 0), c]
        assert np.isnan(want[n, oh, ow, c]) == bool(np.isnan(win).any())
    if kind == "window_nan":
        assert np.isinf(old[np.isnan(want)]).any() or (old[np.isnan(want)] == 0).any()       # the all-NaN windows: -inf, or 0 under the pad
    else:
        assert np.isfinite(old[np.isnan(want)]).all()


def test_maxpool_statement_is_torch_max_pool():
    import torch
    F = torch.nn.functional
    rng = np.random.RandomState(0)
    x = rng.randn(2, 9, 11, 4).astype(np.float32)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    assert np.array_equal(G.maxpool(x, 3, 2, (1, 1, 1, 1)), F.max_pool2d(F.pad(xt, (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).numpy())
    assert np.array_equal(G.maxpool(x, 2, 2, (0, 1, 0, 1)), F.max_pool2d(xt, 2, 2, ceil_mode=True).permute(0, 2, 3, 1).numpy())
    assert G.same_pad(7, 9, 3, 2) == (0, 2, 0, 2) and G.same_pad(5, 7, 2, 2) == (0, 1, 0, 1) and G.same_pad(6, 6, 2, 2) == (0, 0, 0, 0)
    # the explicit loop of the gradient agrees with autograd where nothing ties
    for k, s in ((2, 2), (3, 2)):
        pad = G.same_pad(9, 11, k, s)
        xg = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
        y = F.max_pool2d(F.pad(xg, (0, pad[3], 0, pad[1]), value=-np.inf), k, s)
        dy = rng.randn(*y.permute(0, 2, 3, 1).shape).astype(np.float32)
        y.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
        assert np.array_equal(G.maxpool_bwd(x, dy, k, s), xg.grad.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("kind", G.MAXPOOL_BWD_KINDS)
@pytest.mark.parametrize("case", G.MAXPOOL_BWD_CASES, ids=IDS)
def test_maxpool_bwd_emulation_and_last_max_mutant(case, kind):
    N, H, W, C, k, s = case
    x, dy = G.maxpool_bwd_input(case, kind)
    want, bound = G.maxpool_bwd(x, dy, k, s), G.maxpool_bwd_bound(x, dy, k, s)
    emu = G.maxpool_bwd(x, dy, k, s, dtype=np.float32)
    mut = G.maxpool_bwd(x, dy, k, s, mutant="last_max")
    assert _applies("maxpool_bwd", case) == ["last_max"]
    cons = np.abs(emu.astype(np.float64).sum(axis=(1, 2)) - dy.astype(np.float64).sum(axis=(1, 2)))
    cons_bound = G.maxpool_bwd_conservation(dy, k, s)
    if k == s:
        assert not bound.any() and np.array_equal(emu, want) and not np.array_equal(mut, want)
        assert np.all(cons <= 1e-12 * np.abs(dy).sum())            # (only the float64 summation of this check itself)
    else:
        r = G.excess(emu, want, bound)
        print("maxpool_bwd %s %s: emulation / bound %.3f, conservation %.3f, mutant %.3g" % (case, kind, r, G.excess(cons, 0, cons_bound), G.excess(mut, want, bound)))
        assert r <= 1.0 and G.excess(mut, want, bound) > G.ROOM
        assert np.all(cons <= cons_bound)
    assert (G.maxpool_bwd(x, np.ones_like(dy), k, s) > 0).mean() < 0.5, "most elements win no window: the input ties"


@pytest.mark.parametrize("case", G.COPY_CASES, ids=IDS)
def test_copy_cols_and_refold_statements(case):
    R, ld, col0, cols = case
    src = np.arange(R * ld, dtype=np.float32).reshape(R, ld)
    got = G.copy_cols(src, col0, cols)
    assert got.shape == (R, cols) and got[0, 0] == col0 and got[-1, -1] == (R - 1) * ld + col0 + cols - 1
    w, sc = np.random.RandomState(1).randn(3, 3, 8).astype(np.float32), np.random.RandomState(2).rand(8).astype(np.float32)
    wf = G.dw_refold(w, sc)
    assert wf.dtype == np.float32 and np.array_equal(wf, (w.astype(np.float64) * sc.astype(np.float64)).astype(np.float32))


# ---- bounded kernels: the emulation inside the bound, the mutants outside ---------------------------------------------------------------
@pytest.mark.parametrize("kind", G.MEAN_KINDS)
@pytest.mark.parametrize("case", G.MEAN_CASES, ids=IDS)
def test_spatial_mean(case, kind):
    x = G.mean_input(case, kind)
    want, bound = G.spatial_mean(x), G.spatial_mean_bound(x)
    r = G.excess(G.spatial_mean(x, dtype=np.float32), want, bound)
    m = G.excess(G.spatial_mean(x, mutant="last_pixel_dropped"), want, bound)
    print("spatial_mean %s %s: emulation / bound %.3f, mutant %.3g" % (case, kind, r, m))
    assert _applies("spatial_mean", case) == ["last_pixel_dropped"]
    assert r <= 1.0 and m > G.ROOM


@pytest.mark.parametrize("kind", G.SOFTMAX_KINDS + G.SOFTMAX_NONFINITE)
@pytest.mark.parametrize("case", G.SOFTMAX_CASES, ids=IDS)
def test_softmax_rows(case, kind):
    R, C, ld = case
    x = G.softmax_rows_input(case, kind)
    assert np.isnan(x[:, C:]).all()
    x = x[:, :C]
    want, bound = G.softmax_rows(x), G.softmax_bound(x, G.softmax_depth(C))
    emu = G.softmax_rows_f32(x)
    r = G.excess(emu, want, bound, nan_where_want=True)
    assert r <= 1.0, (case, kind, r)
    if kind == "nan_row":
        assert np.isnan(want[R // 2]).all() and np.isnan(want).sum() == C
    elif kind == "neg_inf":
        assert np.isinf(x).any() and np.all(want[np.isinf(x)] == 0) and np.all(emu[np.isinf(x)] == 0)
    else:
        assert np.isfinite(want).all()
    assert abs(np.nansum(want) - (R - (kind == "nan_row"))) < 1e-9
    seen = []
    if kind in G.SOFTMAX_KINDS:
        for name in _applies("softmax_rows", case, kind):
            m = G.excess(G.softmax_rows_f32(x, mutant=name), want, bound)
            seen.append("%s %.3g" % (name, m))
            assert m > G.ROOM, (case, kind, name, m)
        assert len(seen) == (C > 64) + (kind in ("peak80", "constant_row"))
    print("softmax_rows %s %s: emulation / bound %.3f; mutants %s" % (case, kind, r, ", ".join(seen) or "-"))


@pytest.mark.parametrize("kind", G.RPN_KINDS + G.SOFTMAX_NONFINITE)
@pytest.mark.parametrize("case", G.RPN_CASES, ids=IDS)
def test_rpn_softmax(case, kind):
    H, W, A, ld = case
    x = G.rpn_input(case, kind)
    assert x.shape == (H * W, ld) and np.isnan(x[:, 2 * A:]).all()
    want, bound = G.rpn_softmax(x, A), G.rpn_softmax_bound(x, A)
    emu = G.rpn_softmax(x, A, dtype=np.float32)
    r = G.excess(emu, want, bound, nan_where_want=True)
    assert want.shape == (H * W, 2 * A) and r <= 1.0, (case, kind, r)
    if kind == "nan_row":
        assert np.isnan(want).sum() == 2
    elif kind == "neg_inf":
        assert np.all(emu[np.isinf(x[:, :2 * A])] == 0)
    elif kind == "pairs":
        assert want[0, 0] == 1.0 and emu[0, A] == 0.0
    ok = ~np.isnan(want[:, :A])
    assert np.allclose((want[:, :A] + want[:, A:])[ok], 1.0, rtol=0, atol=1e-12)
    seen = []
    if kind in G.RPN_KINDS:
        for name in _applies("rpn_softmax", case, kind):
            m = G.excess(G.rpn_softmax(x, A, mutant=name), want, bound)
            seen.append("%s %.3g" % (name, m))
            assert m > G.ROOM, (case, kind, name, m)
        assert len(seen) == (A > 1)
    print("rpn_softmax %s %s: emulation / bound %.3f; mutants %s" % (case, kind, r, ", ".join(seen) or "-"))


@pytest.mark.parametrize("case", G.COLSUM_CASES, ids=IDS)
def test_colsum(case):
    dy = G.colsum_input(case)
    want, bound = G.colsum(dy)
    r = G.excess(G.colsum_f32(dy), want, bound)
    m = G.excess(G.colsum(dy, mutant="last_16_rows_dropped")[0], want, bound)
    print("colsum %s: emulation / bound %.3f, mutant %.3g" % (case, r, m))
    assert _applies("colsum", case) == ["last_16_rows_dropped"]
    assert r <= 1.0 and m > G.ROOM
    # the mutant is seen in EVERY column, not in one lucky column
    assert np.all(np.abs(G.colsum(dy, mutant="last_16_rows_dropped")[0] - want) > G.ROOM * bound)


def _check_ce(tag, x, lab, labels):
    R = x.shape[0]
    loss, grad, lb, gb = G.softmax_ce(x, lab)
    el, eg = G.softmax_ce_f32(x, lab)
    if labels == "ignored":
        assert loss == 0.0 and not grad.any() and el == 0 and not eg.any() and lb == 0.0 and not gb.any()
        rl = rg = 0.0
    else:
        rl, rg = G.excess(el, loss, lb), G.excess(eg, grad, gb)
        assert (lab >= 0).any() and ((lab < 0).any() == (labels == "half" and R > 1))
    seen = []
    for name in _applies("softmax_ce", R, labels):
        ml, mg, _, _ = G.softmax_ce(x, lab, mutant=name)
        seen.append("%s loss %.3g grad %.3g" % (name, G.excess(ml, loss, lb), G.excess(mg, grad, gb)))
        assert G.excess(ml, loss, lb) > G.ROOM and G.excess(mg, grad, gb) > G.ROOM, (tag, seen)
    assert len(seen) == (labels == "half" and R > 1)
    print("softmax_ce %s: emulation / bound loss %.3f grad %.3f; mutants %s" % (tag, rl, rg, ", ".join(seen) or "-"))
    assert rl <= 1.0 and rg <= 1.0, (tag, rl, rg)


@pytest.mark.parametrize("logits", G.CE_LOGITS)
@pytest.mark.parametrize("labels", G.CE_LABELS)
@pytest.mark.parametrize("case", G.CE_ROW_CASES, ids=IDS)
def test_softmax_ce_rows(case, labels, logits):
    x, lab = G.ce_row_input(case, labels, logits)
    _check_ce("%s %s %s" % (case, labels, logits), x, lab, labels)


@pytest.mark.parametrize("logits", G.CE_LOGITS)
@pytest.mark.parametrize("labels", G.CE_LABELS)
@pytest.mark.parametrize("case", G.CE_RPN_CASES, ids=IDS)
def test_softmax_ce_rpn(case, labels, logits):
    A, H, W = case
    score, lab = G.ce_rpn_input(case, labels, logits)
    x, lab_rows = G.rpn_ce_rows(score, lab, A, H, W)
    assert set(np.unique(lab_rows)) <= {-1.0, 0.0, 1.0}
    # row (a, h, w) pairs channel a with A + a of pixel (h, w), and the inverse map puts it back
    a, h, w = A - 1, H - 1, W // 2
    assert np.array_equal(x[(a * H + h) * W + w], score[0, h, w, [a, A + a]])
    assert np.array_equal(G.rpn_ce_unrows(x, A, H, W), score)
    _check_ce("rpn %s %s %s" % (case, labels, logits), x, lab_rows, labels)


def test_softmax_ce_statement_is_torch_cross_entropy():
    import torch
    x, lab = G.ce_row_input((257, 21), "half", "randn2")
    loss, grad, _, _ = G.softmax_ce(x, lab)
    t = torch.from_numpy(x).double().requires_grad_(True)
    sel = torch.from_numpy(lab >= 0)
    ref = torch.nn.functional.cross_entropy(t[sel], torch.from_numpy(lab).long()[sel])
    ref.backward()
    assert abs(loss - ref.item()) < 1e-12 and np.allclose(grad, t.grad.numpy(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("sd", G.SL1_SIGMA_DIV, ids=IDS)
@pytest.mark.parametrize("n", G.SL1_N)
def test_smooth_l1(n, sd):
    sigma, div = sd
    pred, tgt, iw, ow = G.smooth_l1_input(n, sigma, div)
    loss, grad, lb, gb = G.smooth_l1(pred, tgt, iw, ow, sigma, div)
    el, eg = G.smooth_l1_f32(pred, tgt, iw, ow, sigma, div)
    rl, rg = G.excess(el, loss, lb), G.excess(eg, grad, gb)
    d = iw.astype(np.float64) * (pred.astype(np.float64) - tgt)
    thr = np.float32(1) / np.float32(sigma * sigma)
    if n >= 6:
        assert np.float32(d[1]) == np.nextafter(thr, np.float32(0)) and np.float32(d[2]) == np.nextafter(thr, np.float32(2)) and d[5] == -3
        assert (d[6:] < -1.0 / sigma ** 2).any() and set(np.unique(iw)) == {0.0, 1.0} and (ow == 0).any()
    seen = []
    for name in _applies("smooth_l1", sigma):
        ml, mg, _, _ = G.smooth_l1(pred, tgt, iw, ow, sigma, div, mutant=name)
        seen.append("%s loss %.3g grad %.3g" % (name, G.excess(ml, loss, lb), G.excess(mg, grad, gb)))
        assert G.excess(ml, loss, lb) > G.ROOM and G.excess(mg, grad, gb) > G.ROOM, seen
    assert len(seen) == (sigma != 1.0)
    print("smooth_l1 n %d sigma %g div %g: emulation / bound loss %.3f grad %.3f; mutants %s" % (n, sigma, div, rl, rg, ", ".join(seen) or "-"))
    assert rl <= 1.0 and rg <= 1.0


@pytest.mark.parametrize("n", G.SUMSQ_N)
def test_sumsq(n):
    w = (np.random.RandomState(n).randn(n) * 0.05).astype(np.float32)
    for prev in (None, np.float32(0.37)):
        want, bound = G.sumsq(w, 0.5 * 1e-4, prev)
        r = G.excess(G.sumsq_f32(w, 0.5 * 1e-4, prev), want, bound)
        cut, _ = G.sumsq(w[:-1], 0.5 * 1e-4, prev)
        print("sumsq n %d prev %s: emulation / bound %.3f; last element dropped %.3g" % (n, prev, r, G.excess(cut, want, bound)))
        assert r <= 1.0
        assert prev is not None or G.excess(cut, want, bound) > G.ROOM        # (against 0.37 one weight's square is below half an ulp)


# ---- dropout ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", G.DROPOUT_SEEDS)
@pytest.mark.parametrize("keep", G.DROPOUT_KEEP)
def test_dropout_restatement_statistics(keep, seed):
    n = 65536
    m = G.dropout_keep(seed, n, keep)
    assert m.dtype == np.float32 and set(np.unique(m)) == {0.0, 1.0}
    dev = abs(float(m.mean()) - keep)
    agree = float((m == G.dropout_keep(seed + 1, n, keep)).mean())
    print("dropout keep %g seed %d: |fraction - keep| = %.4f (<= %.4f); agreement with seed + 1: %.3f" % (keep, seed, dev, 5 * np.sqrt(keep * (1 - keep) / n), agree))
    assert dev <= 5 * np.sqrt(keep * (1 - keep) / n)
    # independent masks agree with probability keep^2 + (1 - keep)^2, 'about half' (0.5 / 0.58); 5 sigma
    p = keep * keep + (1 - keep) * (1 - keep)
    assert abs(agree - p) <= 5 * np.sqrt(p * (1 - p) / n)
    assert np.array_equal(G.dropout_keep(seed, 255, keep), m[:255]), "element i does not depend on n"


def test_dropout_restatement_first_values():
    """the finaliser by hand, in Python integers, for the first elements of two seeds"""
    M = (1 << 64) - 1
    for seed in (0, 2 ** 63 + 5):
        for i in range(4):
            z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            u = (z >> 40) / 16777216.0
            for keep in G.DROPOUT_KEEP:
                assert G.dropout_keep(seed, 4, keep)[i] == np.floor(np.float32(np.float32(keep) + np.float32(u)))
    x = np.array([3.0, -1.5, 0.1, 7.0], np.float32)
    y = G.dropout(x, 1, 0.3)
    k = G.dropout_keep(1, 4, 0.3)
    assert y.dtype == np.float32 and np.array_equal(y, (x / np.float32(0.3)) * k)
