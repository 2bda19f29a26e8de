"""TEST INFRASTRUCTURE ONLY -- float64 statements of the bandwidth-bound kernels between the convolutions (csrc/dense_misc.hip: k_maxpool,
k_spatial_mean, k_softmax_rows, k_rpn_softmax, k_copy_cols; csrc/backward_kernels.hip: k_maxpool_bwd, k_colsum, k_dropout, k_dw_refold,
k_sumsq; csrc/train_kernels.hip: k_softmax_ce, k_smooth_l1), the bound each is held to, a float32 emulation of each kernel's own order of
operations, and the planted mistakes (`mutant=`) the bound has to reject -- in the manner of oracle/fwd_ref.py.

Every bound is an ABSOLUTE array (or number) `bound` with |got - want| <= bound, derived below from one rounding (relative U = 2^-24) per
float32 + - * / and expf / logf within 1 ulp (relative 2 U = EPS).  The tests assert excess(got, want, bound) <= ROOM = 2 on the device (room
for 2-ulp library functions) and <= 1 for the emulations (tests/test_glue_bounds_cpu.py); no constant here comes from device output.  Beside
each bound: the largest excess the MI355X run of tests/test_glue_gpu.py printed.

Mutants are selected by name; MUTANTS lists, per operation, the names and a predicate that says which cases a mutant applies to (a case
that cannot show a mistake by construction -- sigma = 1 for a 1/sigma threshold, one anchor for a neighbouring-anchor pair -- is excluded
there, in one place, and nowhere skipped)."""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of float32
EPS = 2.0 ** -23
TINY = 2.0 ** -126              # smallest normal float32: absolute room where a result underflows
ROOM = 2.0                      # factor of every device assertion over the derived bound
F32 = np.float32


def excess(got, want, bound, nan_where_want=False):
    """max over elements of |got - want| / bound  (0 / 0 = 0, x / 0 = inf, a NaN on either side = inf -- unless nan_where_want: then an
    element counts 0 where both sides are NaN, and still inf where one is)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
    d = np.where(np.isnan(d), np.inf, d)
    if nan_where_want:
        d = np.where(np.isnan(got) & np.isnan(want), 0.0, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / np.asarray(bound, np.float64))
    return float(np.max(r)) if np.size(r) else 0.0


def pool_out(n, k, stride, lo, hi):
    return (n + lo + hi - k) // stride + 1


def same_pad(H, W, k, stride):
    """the pad lib/nets/network.py _max_pool hands to ops.maxpool: bottom / right only, out = ceil(n / stride)"""
    OH, OW = -(-H // stride), -(-W // stride)
    return (0, (OH - 1) * stride + k - H, 0, (OW - 1) * stride + k - W)


# ---- max pool ---------------------------------------------------------------------------------------------------------------------------
def _canvas(x, top, left, Hp, Wp):
    """x [N,H,W,C] placed at (top, left) (either may be negative) of a [N,Hp,Wp,C] canvas of -inf, and the mask of canvas pixels x covers"""
    N, H, W, C = x.shape
    xp = np.full((N, Hp, Wp, C), -np.inf, x.dtype)
    ins = np.zeros((Hp, Wp), bool)
    r0, r1, c0, c1 = max(top, 0), min(top + H, Hp), max(left, 0), min(left + W, Wp)
    if r1 > r0 and c1 > c0:
        xp[:, r0:r1, c0:c1] = x[:, r0 - top:r1 - top, c0 - left:c1 - left]
        ins[r0:r1, c0:c1] = True
    return xp, ins


def maxpool(x, k, stride, pad, mutant=None):
    """x [N,H,W,C] float32 -> float32 [N,OH,OW,C], exact (a maximum rounds nothing): compare with np.array_equal.
    Contract of ops.maxpool: pad = (top, bottom, left, right); any top or left pad means explicit zeros on all four sides (ResNet pool1:
    tf.pad then VALID), so a window with an out-of-image tap returns max(window, 0); pad at the bottom / right only means TF SAME:
    out-of-image taps are ignored.
    NaN rule: an output is NaN iff an in-image tap of its window is NaN; the zero pad does not clear it.
    mutants: 'neg_inf_pad' (the zero pad taken as -inf), 'clamp_in_same' (the zero clamp applied under SAME), 'shifted' (the window one
    pixel down and right), 'fmaxf' (the kernel before the NaN rule: fmaxf from -inf drops NaN -- one NaN gives the maximum of the others, an
    all-NaN window -inf, or 0 under the zero pad)."""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    pt, pb, pl, pr = pad
    OH, OW = pool_out(H, k, stride, pt, pb), pool_out(W, k, stride, pl, pr)
    shift = 1 if mutant == "shifted" else 0
    xp, ins = _canvas(x, pt - shift, pl - shift, (OH - 1) * stride + k, (OW - 1) * stride + k)
    m = np.full((N, OH, OW, C), -np.inf, F32)
    nan = np.zeros((N, OH, OW, C), bool)
    oob = np.zeros((OH, OW), bool)
    for dy in range(k):
        for dx in range(k):
            rows, cols = slice(dy, dy + (OH - 1) * stride + 1, stride), slice(dx, dx + (OW - 1) * stride + 1, stride)
            v = xp[:, rows, cols]
            m = np.fmax(m, v)                       # fmax from -inf: NaN taps lose, like fmaxf
            nan |= np.isnan(v)                      # (the canvas outside the image is -inf, never NaN)
            oob |= ~ins[rows, cols]
    zero = (pt > 0 or pl > 0)
    zero = {"neg_inf_pad": False, "clamp_in_same": True}.get(mutant, zero)
    if zero:
        m = np.where(oob[None, :, :, None] & (m < 0), F32(0), m)
    return m if mutant == "fmaxf" else np.where(nan, F32(np.nan), m)


def maxpool_has_oob(H, W, k, stride, pad):
    """some window of the geometry has an out-of-image tap"""
    OH, OW = pool_out(H, k, stride, pad[0], pad[1]), pool_out(W, k, stride, pad[2], pad[3])
    return pad[0] > 0 or pad[2] > 0 or (OH - 1) * stride + k - pad[0] > H or (OW - 1) * stride + k - pad[2] > W


def maxpool_bwd(x, dy, k, stride, mutant=None, dtype=np.float64):
    """Gradient of maxpool (bottom / right pad only: OH, OW are dy's) as an explicit loop over the windows: each window's gradient goes to
    its FIRST maximum in (row, column) scan order among its in-image taps.  dtype float64: the statement.  dtype float32: the kernel's
    arithmetic -- an input element adds the windows it wins in (oh, ow) order, which is the order of this loop.
    Bound (maxpool_bwd_bound): k == stride -- windows do not overlap, an element wins at most one, nothing is rounded: bit-exact.  k > stride:
    |got - want| <= EPS B, B the same routing of |dy|.  An element lies in at most w = ceil(k / stride)^2 windows; acc = 0 + g1 is exact and
    each further add rounds a partial sum of magnitude at most B: (w - 1) U B.  At 3x3 / 2 an element that wins all four of its windows
    rounds three times, 1.5 EPS B -- inside the asserted ROOM * EPS B, not inside EPS B itself; an element that wins up to three is.
    Conservation per (image, channel) (maxpool_bwd_conservation): every window has an in-image tap, so sum(want) = sum(dy); summing the
    element errors, |sum dx - sum dy| <= (w - 1) U sum B = (w - 1) U sum |dy|: 3 U sum |dy| at 3x3 / 2.
    mutant 'last_max': the LAST maximum takes the gradient."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    OH, OW = dy.shape[1], dy.shape[2]
    dx = np.zeros((N, H, W, C), dtype)
    ni, ci = np.arange(N)[:, None], np.arange(C)[None, :]
    for oh in range(OH):
        for ow in range(OW):
            r0, r1, c0, c1 = oh * stride, min(oh * stride + k, H), ow * stride, min(ow * stride + k, W)
            win = x[:, r0:r1, c0:c1].reshape(N, -1, C)
            T = win.shape[1]
            idx = (T - 1 - np.argmax(win[:, ::-1], axis=1)) if mutant == "last_max" else np.argmax(win, axis=1)     # argmax: the first
            rr, cc = r0 + idx // (c1 - c0), c0 + idx % (c1 - c0)
            dx[ni, rr, cc, ci] = dx[ni, rr, cc, ci] + dy[:, oh, ow].astype(dtype)       # (n, c) pairs are distinct: a plain add per window
    return dx


def maxpool_bwd_windows(k, stride):
    return (-(-k // stride)) ** 2


def maxpool_bwd_bound(x, dy, k, stride):
    """elementwise bound; all zeros (bit-exact) at k == stride.  measured on the MI355X: 0.48 (3x3 / 2)"""
    return (EPS if k > stride else 0.0) * maxpool_bwd(x, np.abs(dy), k, stride)


def maxpool_bwd_conservation(dy, k, stride):
    """bound on |sum dx - sum dy| per (image, channel).  measured on the MI355X: 0.059"""
    return (maxpool_bwd_windows(k, stride) - 1) * U * np.abs(np.asarray(dy, np.float64)).sum(axis=(1, 2))


# ---- spatial mean -----------------------------------------------------------------------------------------------------------------------
def spatial_mean(x, mutant=None, dtype=np.float64):
    """x [N,HW,C] -> [N,C].  float64: the statement.  float32: the kernel -- a sequential sum from 0, fl(1 / HW), one product.
    Bound: the sum rounds HW - 1 times (0 + x0 is exact), each at most U times a partial sum <= sum |x|; fl(1 / HW) and the product one
    rounding each: |got - want| <= (HW - 1 + 2) U sum |x| / HW = (HW + 1) / 2 * EPS * mean |x|, to first order (the second-order term is
    below (HW U)^2 = 2^-32 of it at HW = 196).
    mutant 'last_pixel_dropped': the sum stops one pixel early."""
    x = np.asarray(x)
    N, HW, C = x.shape
    n = HW - 1 if mutant == "last_pixel_dropped" else HW
    if dtype == np.float64:
        return x[:, :n].astype(np.float64).sum(axis=1) / HW
    s = np.zeros((N, C), F32)
    for i in range(n):
        s = s + x[:, i].astype(F32)
    return s * (F32(1) / F32(HW))


def spatial_mean_bound(x):
    """measured on the MI355X: 0.128"""
    HW = x.shape[1]
    return (HW + 1) / 2.0 * EPS * np.abs(np.asarray(x, np.float64)).mean(axis=1)


# ---- softmax (rows, RPN pairs) ----------------------------------------------------------------------------------------------------------
def _softmax_parts(x):
    """x [R,C] -> float64 (p, m [R,1], s [R,1], a = |x - m| (0 at -inf entries), D = sum p a [R,1]).  A row with a NaN is all NaN; -inf
    entries (never a whole row) have p = 0 exactly."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        m = x.max(axis=1, keepdims=True)
        e = np.exp(x - m)
        s = e.sum(axis=1, keepdims=True)
        p = e / s
        a = np.where(np.isinf(x), 0.0, np.abs(x - m))
    return p, m, s, a, (p * a).sum(axis=1, keepdims=True)


def softmax_rows(x):
    """float64 softmax over the last axis of x [R,C]"""
    return _softmax_parts(x)[0]


def softmax_depth(C):
    """adds on the path of k_softmax_rows' sum: ceil(C / 64) - 1 in a lane, 6 in the xor tree"""
    return 6 + -(-C // 64) - 1


def softmax_bound(x, depth):
    """y_i = fl(e_i / s), e_i = expf(fl(x_i - m)), s = the float32 sum of the e_j (m is exact).  In units of EPS = 2 U, relative to p_i:
      fl(x_i - m) errs by U |x_i - m|, which expf turns into a relative |x_i - m| / 2;  expf itself: 1;
      s: its terms carry (1 + |x_j - m| / 2) each, weighted by p_j: 1 + D / 2 with D = sum p_j |x_j - m|;  its adds: depth / 2;
      the division: 1 / 2.
    Sum: 2.5 + depth / 2 + (|x_i - m| + D) / 2.  The bound takes 4 for the 2.5 (the room covers the second-order terms, which at
    |x_i - m| = 100 and depth 8 are 2^-17 of the first-order ones) and adds TINY: an e_i below the normal range may be flushed to 0, which
    moves y_i by at most 2^-126 / s <= 2^-126.
    depth: softmax_depth(C) for k_softmax_rows, 1 for k_rpn_softmax (s = e0 + e1).
    measured on the MI355X: rows 0.823, pairs 0.88"""
    p, _, _, a, D = _softmax_parts(x)
    return EPS * (4.0 + depth / 2.0 + (a + D) / 2.0) * p + TINY


def _xor_tree(s):
    """s [..., 64] -> the wave sum every lane holds after `for (o = 32; o; o >>= 1) s += __shfl_xor(s, o)`"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    return s[..., 0]


def softmax_rows_f32(x, mutant=None):
    """k_softmax_rows in float32 numpy: lane l owns columns l, l + 64, ..; the maximum (exact); per-lane sequential sums of expf(x - m);
    the xor tree; e / s.  mutants: 'cols_ge_64_dropped' (the sum takes each lane's first column only), 'no_max' (m = 0: a sound algorithm
    while every |x| < 87, so it only applies to inputs that leave expf's range)."""
    x = np.asarray(x, F32)
    R, C = x.shape
    T = -(-C // 64)
    with np.errstate(over="ignore", invalid="ignore"):
        m = np.zeros((R, 1), F32) if mutant == "no_max" else np.fmax.reduce(x, axis=1, keepdims=True, initial=-np.inf)
        e = np.exp(x - m)
        lanes = np.zeros((R, T * 64), F32)
        lanes[:, :C] = e
        lanes = lanes.reshape(R, T, 64)
        s = np.zeros((R, 64), F32)
        for t in range(1 if mutant == "cols_ge_64_dropped" else T):
            s = s + lanes[:, t]                 # (a lane without a column at trip t adds nothing; + 0 is exact)
        return e / _xor_tree(s)[:, None]


def rpn_rows(score, A):
    """score [..., ld] -> [pixels * A, 2]: row pix * A + a holds (score[pix, a], score[pix, A + a]) (nets/network.py:68-86)"""
    s = np.asarray(score)
    s = s.reshape(-1, s.shape[-1])
    return np.stack([s[:, :A], s[:, A:2 * A]], axis=-1).reshape(-1, 2)


def rpn_unrows(rows, A):
    """[pixels * A, 2] -> [pixels, 2A]"""
    r = np.asarray(rows).reshape(-1, A, 2)
    return np.concatenate([r[:, :, 0], r[:, :, 1]], axis=1)


def rpn_softmax(score, A, mutant=None, dtype=np.float64):
    """score [pixels, ld] -> prob [pixels, 2A]; float32: k_rpn_softmax (max, two expf, one add, two divisions).
    mutant 'adjacent_pair': channel a paired with a + 1 in place of A + a (the same pair when A = 1)."""
    s = np.asarray(score)
    s = s.reshape(-1, s.shape[-1])
    if mutant == "adjacent_pair":
        s = np.concatenate([s[:, :A], s[:, 1:A + 1]], axis=1)
    rows = rpn_rows(s, A)
    if dtype == np.float64:
        return rpn_unrows(softmax_rows(rows), A)
    rows = rows.astype(F32)
    with np.errstate(invalid="ignore"):
        m = np.fmax(rows[:, :1], rows[:, 1:])
        e = np.exp(rows - m)
        return rpn_unrows(e / (e[:, :1] + e[:, 1:]), A)


def rpn_softmax_bound(score, A):
    return rpn_unrows(softmax_bound(rpn_rows(score, A), 1), A)


# ---- softmax cross-entropy --------------------------------------------------------------------------------------------------------------
def softmax_ce(logits, labels, mutant=None):
    """logits [R,C] float32, labels [R] (< 0: ignored) -> float64 (loss, grad [R,C], loss_bound, grad_bound [R,C]).
    loss = mean over the selected rows of l = log s + m - x_label; grad = (p - onehot) / n on selected rows, 0 elsewhere.  No selected row:
    loss 0 and grad 0 exactly -- the kernel's defined behaviour (TensorFlow's reduce_mean of nothing is NaN); bounds 0.
    Per selected row, in units of U: s sums C terms expf(fl(x_j - m)) sequentially -- each term |x_j - m| + 2 (expf 1 ulp), weighted D + 2, and
    C - 1 adds: s is relative C + 1 + D, which is log s's absolute error; logf 1 ulp: 2 |log s|; + m: |log s + m|; - x_label: |l|:
      E_row = U ((C + 1 + D) + 2 |log s| + |log s + m| + |l|)
    The row losses are summed and divided in float64 and rounded once: |loss - ref| <= mean_sel(E_row) + U |ref|.
    Gradient: p_i = fl(e_i / s) is relative (|x_i - m| + 2) + 1 + (C + 1 + D); fl(p_i - onehot), fl(1 / n) and the product round once each,
    relative to |p_i - onehot|: |g - ref| <= U ((C + 4 + D + |x_i - m|) p_i + 3 |p_i - onehot|) / n + TINY.
    mutant 'ignored_counted': one ignored row counted in n.
    measured on the MI355X: loss 0.672 (RPN addressing 0.257), gradient 0.841 (RPN 0.851)"""
    x = np.asarray(logits, np.float64)
    lab = np.asarray(labels).ravel()
    R, C = x.shape
    sel = lab >= 0
    n = int(sel.sum())
    if n == 0:
        return 0.0, np.zeros((R, C)), 0.0, np.zeros((R, C))
    li = np.where(sel, lab, 0).astype(np.int64)
    p, m, s, a, D = _softmax_parts(x)
    logs = np.log(s[:, 0])
    xl = x[np.arange(R), li]
    l = logs + m[:, 0] - xl
    onehot = np.zeros((R, C))
    onehot[np.arange(R), li] = 1.0
    div = n + 1 if mutant == "ignored_counted" else n
    loss = float(l[sel].sum() / div)
    grad = np.where(sel[:, None], (p - onehot) / div, 0.0)
    e_row = U * ((C + 1 + D[:, 0]) + 2 * np.abs(logs) + np.abs(logs + m[:, 0]) + np.abs(l))
    loss_bound = float(e_row[sel].mean() + U * abs(loss))
    grad_bound = np.where(sel[:, None], U * ((C + 4 + D + a) * p + 3 * np.abs(p - onehot)) / n + TINY, 0.0)
    return loss, grad, loss_bound, grad_bound


def softmax_ce_f32(logits, labels):
    """k_softmax_ce + k_ce_finish + k_scale_grad in float32 numpy: one thread per row, sequential max / sum over the classes, the row loss
    fl(fl(logf(s) + m) - x_label) summed in float64, loss = (float)(sum / n), grad = fl(fl(p - onehot) * (float)(1 / n))."""
    x = np.asarray(logits, F32)
    lab = np.asarray(labels).ravel()
    R, C = x.shape
    sel = lab >= 0
    n = int(sel.sum())
    li = np.where(sel, lab, 0).astype(np.int64)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = np.zeros(R, F32)
    for c in range(C):
        s = s + e[:, c]
    rowloss = (np.log(s) + m[:, 0]) - x[np.arange(R), li]
    assert rowloss.dtype == F32 and e.dtype == F32
    loss = F32(rowloss[sel].astype(np.float64).sum() / n) if n else F32(0)
    inv_n = F32(1.0 / n) if n else F32(0)
    onehot = np.zeros((R, C), F32)
    onehot[np.arange(R), li] = 1
    g = np.where(sel[:, None], e / s[:, None] - onehot, F32(0)) * inv_n
    return loss, g.astype(F32)


def rpn_ce_rows(score, labels, A, H, W):
    """the RPN form of the loss as rows: score [1,H,W,2A], labels [1,1,A*H,W] -> (logits [A*H*W, 2], labels [A*H*W]) in the labels'
    (a, h, w) order (nets/network.py:68-78, 282-288)"""
    s = np.asarray(score).reshape(H, W, 2 * A)
    pair = np.stack([s[:, :, :A].transpose(2, 0, 1).reshape(-1), s[:, :, A:].transpose(2, 0, 1).reshape(-1)], axis=1)
    return pair, np.asarray(labels).ravel()


def rpn_ce_unrows(g, A, H, W):
    """[A*H*W, 2] in (a, h, w) order -> [1,H,W,2A]"""
    g = np.asarray(g).reshape(A, H, W, 2)
    return np.concatenate([g[..., 0].transpose(1, 2, 0), g[..., 1].transpose(1, 2, 0)], axis=2)[None]


# ---- smooth L1 --------------------------------------------------------------------------------------------------------------------------
def smooth_l1(pred, tgt, in_w, out_w, sigma, div, mutant=None):
    """-> float64 (loss, grad, loss_bound, grad_bound): loss = sum(out_w f(in_w (pred - tgt))) / div,
    f(d) = sigma^2 d^2 / 2 if |d| < 1 / sigma^2 else |d| - 0.5 / sigma^2 (nets/network.py:264-277).  f and f' are continuous at the
    threshold, so an element whose float32 d falls on the other side of it stays inside the bounds.
    Per element, in units of U: d = fl(in_w fl(pred - tgt)) is relative 2.  Quadratic branch: fl(d d) carries 4 + 1, fl(sigma^2 / 2) and
    the product 2, the product with out_w 1: 8 f.  Linear branch: |d| carries 2 |d|, fl(0.5 / sigma^2) 0.5 / sigma^2, the subtraction and
    the product with out_w 2 f.  Both are inside E = U out_w (7 f + 2 |d| + 0.5 / sigma^2) (quadratic: f < |d| / 2, so 8 f <= 7 f + 2 |d|).
    The element losses are summed in float64, scaled and rounded once: |loss - ref| <= sum E / div + U |ref|.
    Gradient fl(fl(fl((1 / div) out_w) in_w) f'): f' = sigma^2 d is relative 3, 1 / div and three products 4, the threshold's own rounding
    under 1: |g - ref| <= 8 U |ref| + TINY.
    mutant 'threshold_1_over_sigma': the branch switches at 1 / sigma (the same threshold when sigma = 1).
    measured on the MI355X: loss 0.046, gradient 0.192"""
    p, t, iw, ow = (np.asarray(v, np.float64) for v in (pred, tgt, in_w, out_w))
    s2 = float(sigma) ** 2
    thr = 1.0 / float(sigma) if mutant == "threshold_1_over_sigma" else 1.0 / s2
    d = iw * (p - t)
    quad = np.abs(d) < thr
    f = np.where(quad, d * d * (s2 / 2.0), np.abs(d) - 0.5 / s2)
    loss = float((ow * f).sum() / div)
    grad = ow * iw * np.where(quad, s2 * d, np.sign(d)) / div
    e = U * np.abs(ow) * (7 * np.abs(f) + 2 * np.abs(d) + 0.5 / s2)
    return loss, grad, float(e.sum() / div + U * abs(loss)), 8 * U * np.abs(grad) + TINY


def smooth_l1_f32(pred, tgt, in_w, out_w, sigma, div):
    """k_smooth_l1 + k_sum_finish in float32 numpy"""
    p, t, iw, ow = (np.asarray(v, F32) for v in (pred, tgt, in_w, out_w))
    s2 = F32(sigma) * F32(sigma)
    d = iw * (p - t)
    ad = np.abs(d)
    quad = ad < F32(1) / s2
    f = np.where(quad, (d * d) * (s2 / F32(2)), ad - F32(0.5) / s2)
    loss = F32((ow * f).astype(np.float64).sum() * (1.0 / float(F32(div))))
    g = (F32(1) / F32(div)) * ow * iw * np.where(quad, s2 * d, np.sign(d))
    assert f.dtype == F32 and g.dtype == F32
    return loss, g


# ---- column sum, sum of squares ---------------------------------------------------------------------------------------------------------
def f64_sum_bound(want, terms_abs):
    """float64 accumulation, one rounding to float32: U |want| for the rounding; the float64 sum of n terms errs by at most n 2^-53 sum
    |terms|, under 1e-9 EPS sum |terms| for n < 2^20 (the form of the colsum assertion in tests/test_dgrad_gpu.py).
    measured on the MI355X: colsum 0.978, sumsq 0.674 (round to nearest reaches 1)"""
    return U * np.abs(want) + 1e-9 * EPS * terms_abs


def colsum(dy, mutant=None):
    """dy [M,C] -> (want [C] float64, bound).  mutant 'last_16_rows_dropped': the rows from the last multiple of 16 below M on are left out
    (the last, possibly partial, group of 16 rows: what a part loop that stops one trip early loses)."""
    d = np.asarray(dy, np.float64)
    M = d.shape[0]
    want = d[:(M - 1) // 16 * 16].sum(axis=0) if mutant == "last_16_rows_dropped" else d.sum(axis=0)
    return want, f64_sum_bound(d.sum(axis=0), np.abs(d).sum(axis=0))


def colsum_f32(dy):
    """k_colsum's order in float64, rounded once: 16 parts; part p walks rows p, p + 16, .. -- four at a time into s0..s3 while m + 48 < M,
    the rest into s0 -- then (s0 + s1) + (s2 + s3), then the parts in order"""
    d = np.asarray(dy, np.float64)
    M, C = d.shape
    tot = np.zeros(C)
    for part in range(16):
        s = [np.zeros(C) for _ in range(4)]
        m = part
        while m + 48 < M:
            for q in range(4):
                s[q] = s[q] + d[m + 16 * q]
            m += 64
        while m < M:
            s[0] = s[0] + d[m]
            m += 16
        tot = tot + ((s[0] + s[1]) + (s[2] + s[3]))
    return tot.astype(F32)


def sumsq(w, scale, prev=None):
    """-> (want, bound) of out = (prev if accumulating else 0) + (float)(scale * sum w^2).  Accumulating adds one float32 rounding of the
    result."""
    w = np.asarray(w, np.float64).ravel()
    v = float((w * w).sum() * scale)
    b = float(f64_sum_bound(v, abs(v)))
    if prev is None:
        return v, b
    want = float(prev) + v
    return want, b + U * (abs(want) + b)


def sumsq_f32(w, scale, prev=None):
    """k_sumsq + k_sumsq_finish: float64 grid-stride partial sums over min(ceil(n / 256), 256) workgroups of 256, the xor tree per wave, the
    four waves, the workgroups in order, times scale, rounded to float32 (+ prev in float32)"""
    w = np.asarray(w, np.float64).ravel()
    n = w.size
    nb = min(-(-n // 256), 256)
    T = nb * 256
    sq = np.zeros(-(-n // T) * T)
    sq[:n] = w * w
    s = np.zeros(T)
    for row in sq.reshape(-1, T):
        s = s + row
    waves = _xor_tree(s.reshape(nb, 4, 64))
    tot = 0.0
    for b in range(nb):
        tot = tot + (((waves[b, 0] + waves[b, 1]) + waves[b, 2]) + waves[b, 3])
    v = F32(tot * scale)
    return v if prev is None else F32(prev) + v


# ---- bit-exact: refold, column copy, dropout --------------------------------------------------------------------------------------------
def dw_refold(w, scale):
    """wf[tap][c] = fl(w[tap][c] * scale[c]), w [3,3,C] float32: one float32 product, bit-exact"""
    return np.asarray(w, F32) * np.asarray(scale, F32)[None, None, :]


def copy_cols(src, col0, cols):
    return np.ascontiguousarray(np.asarray(src)[..., col0:col0 + cols])


def dropout_keep(seed, n, keep_prob):
    """The mask of k_dropout (csrc/backward_kernels.hip dropout_keep) restated on numpy uint64, elements 0 .. n - 1 -> float32 0 / 1:
    z = seed + 0x9E3779B97F4A7C15 (i + 1) mod 2^64, the splitmix64 finaliser, u = (z >> 40) 2^-24 in [0, 1) (exact in float32: 24 bits),
    mask = floorf(fl(keep_prob + u)).
    keep_prob = 1 is not restated faithfully by 'always 1': fl(1 + u) rounds to 2 for the single value u = 1 - 2^-24.  No network uses it."""
    i = np.arange(n, dtype=np.uint64)
    z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15) * (i + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)
    return np.floor(F32(keep_prob) + u).astype(F32)


def dropout(x, seed, keep_prob):
    """y = fl(fl(x / keep_prob) * mask) in float32, bit for bit"""
    x = np.asarray(x, F32)
    return ((x.ravel() / F32(keep_prob)) * dropout_keep(seed, x.size, keep_prob)).reshape(x.shape)


# ---- the cases of tests/test_glue_gpu.py and tests/test_glue_bounds_cpu.py --------------------------------------------------------------
MAXPOOL_CASES = [(2, 7, 9, 4, 3, 2, (1, 1, 1, 1)), (1, 8, 10, 12, 3, 2, (1, 1, 1, 1)), (2, 5, 7, 8, 2, 2, (0, 1, 0, 1)),
                 (1, 6, 8, 4, 2, 2, (0, 0, 0, 0)), (1, 31, 45, 20, 3, 2, (1, 1, 1, 1))]        # the last: 16 * 23 * 5 = 1840 threads, 7.2 workgroups
MAXPOOL_KINDS = ("negative", "mixed", "neg_inf")
MAXPOOL_NAN = ("one_nan", "window_nan")
MAXPOOL_BWD_CASES = [(2, 5, 7, 8, 2, 2), (1, 6, 6, 4, 2, 2), (1, 7, 9, 20, 3, 2)]
MAXPOOL_BWD_KINDS = ("ties", "all_equal")
MEAN_CASES = [(1, 49, 4), (3, 49, 36), (5, 1, 8), (2, 196, 64), (37, 49, 28)]
MEAN_KINDS = ("randn", "positive_spread")
SOFTMAX_CASES = [(1, 2, 2), (5, 21, 21), (7, 21, 32), (3, 81, 81), (6, 81, 128), (9, 64, 64), (2, 65, 70), (5, 130, 130)]
SOFTMAX_KINDS = ("randn3", "randn30", "peak80", "constant_row")
SOFTMAX_NONFINITE = ("neg_inf", "nan_row")
RPN_CASES = [(1, 1, 1, 2), (3, 5, 9, 18), (3, 5, 9, 64), (2, 7, 12, 24), (4, 5, 15, 32), (17, 16, 15, 30)]
COPY_CASES = [(7, 54, 18, 36), (1, 5, 4, 1), (300, 64, 0, 64)]
COLSUM_CASES = [(M, 84) for M in (1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 2331)] + [(M, C) for M in (17, 65) for C in (1, 18, 64, 65)]
CE_ROW_CASES = [(1, 2), (7, 21), (255, 21), (257, 21), (300, 81), (513, 2)]
CE_RPN_CASES = [(1, 1, 1), (9, 3, 5), (15, 4, 5), (12, 5, 9)]
CE_LABELS = ("valid", "half", "ignored")
CE_LOGITS = ("randn2", "randn30")
SL1_N = (1, 255, 257, 540)
SL1_SIGMA_DIV = ((3.0, 1.0), (1.0, 256.0))
DROPOUT_N = (1, 255, 4097, 65536)
DROPOUT_KEEP = (0.5, 0.3)
DROPOUT_SEEDS = (0, 1, 12345, 2 ** 63 + 5)
REFOLD_C = (8, 32, 100)
SUMSQ_N = (1, 255, 257, 100003)

# operation -> [(mutant, applies(case...) )]: every mutant must fail on EVERY case it applies to
MUTANTS = {
    "maxpool": [("neg_inf_pad", lambda c: c[6][0] > 0 or c[6][2] > 0),
                ("clamp_in_same", lambda c: not (c[6][0] > 0 or c[6][2] > 0) and maxpool_has_oob(c[1], c[2], c[4], c[5], c[6])),
                ("shifted", lambda c: True)],
    "maxpool_bwd": [("last_max", lambda c: True)],
    "spatial_mean": [("last_pixel_dropped", lambda c: True)],
    "softmax_rows": [("cols_ge_64_dropped", lambda c, kind: c[1] > 64),
                     ("no_max", lambda c, kind: kind in ("peak80", "constant_row"))],
    "rpn_softmax": [("adjacent_pair", lambda c, kind: c[2] > 1)],
    "colsum": [("last_16_rows_dropped", lambda c: True)],
    "softmax_ce": [("ignored_counted", lambda R, labels: labels == "half" and R > 1)],
    "smooth_l1": [("threshold_1_over_sigma", lambda sigma: sigma != 1.0)],
}


def _rng(*key):
    """a generator seeded by the case alone (not by PYTHONHASHSEED)"""
    s = 17
    for ch in repr(key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return np.random.RandomState(s)


def maxpool_input(case, kind):
    """'negative': randn - 3 cut at -0.25 (no positive value: only the zero pad can give 0); 'mixed': randn; 'neg_inf': randn - 3 with one
    element in five -inf; 'one_nan' / 'window_nan': mixed with one NaN / the in-image taps of the output window nearest the centre all NaN
    (in every channel) -- window_nan picks a window next to the top-left corner too when the geometry pads, so a padded all-NaN window is
    met"""
    N, H, W, C, k, s, pad = case
    rng = _rng("maxpool", case, kind)
    x = rng.randn(N, H, W, C).astype(F32)
    if kind in ("negative", "neg_inf"):
        x = np.minimum(x - 3, F32(-0.25))
    if kind == "neg_inf":
        x[rng.rand(N, H, W, C) < 0.2] = -np.inf
    if kind == "one_nan":
        x[N - 1, H // 2, W // 2, C - 1] = np.nan
    if kind == "window_nan":
        OH, OW = pool_out(H, k, s, pad[0], pad[1]), pool_out(W, k, s, pad[2], pad[3])
        for oh, ow in ((OH // 2, OW // 2), (0, 0), (OH - 1, OW - 1)):
            r0, c0 = oh * s - pad[0], ow * s - pad[2]
            x[0, max(r0, 0):max(r0 + k, 0), max(c0, 0):max(c0 + k, 0)] = np.nan
    return x


def maxpool_bwd_input(case, kind):
    """(x, dy): x drawn from {0, 1, 2} (most windows tie) or all equal; dy randn"""
    N, H, W, C, k, s = case
    rng = _rng("maxpool_bwd", case, kind)
    x = rng.randint(0, 3, size=(N, H, W, C)).astype(F32) if kind == "ties" else np.full((N, H, W, C), 1.5, F32)
    pad = same_pad(H, W, k, s)
    dy = rng.randn(N, pool_out(H, k, s, 0, pad[1]), pool_out(W, k, s, 0, pad[3]), C).astype(F32)
    return x, dy


def mean_input(case, kind):
    N, HW, C = case
    rng = _rng("mean", case, kind)
    if kind == "randn":
        return rng.randn(N, HW, C).astype(F32)
    return ((rng.rand(N, HW, C) + 0.1) * 2.0 ** rng.randint(-8, 9, size=(N, 1, 1))).astype(F32)


def softmax_input(R, C, kind, rng):
    """[R,C] logits.  'randn3' / 'randn30': randn * 3 / * 30; 'peak80': randn * 3 + 15 with one logit per row 80 above the row's maximum
    (about 100: past expf's range without the max subtraction); 'constant_row': randn3 with row 0 constant at 100; 'neg_inf': randn3 with
    one entry in four -inf (never column 0: no row is all -inf); 'nan_row': randn3 with one NaN in row R // 2.  Where C > 64 every row's
    maximum is swapped into column C - 1."""
    x = rng.randn(R, C) * (30.0 if kind == "randn30" else 3.0)
    if kind == "peak80":
        x += 15.0
        x[np.arange(R), rng.randint(0, C, size=R)] = x.max(axis=1) + 80.0
    if C > 64:          # the row's maximum sits in the last column, which a lane's second trip reads: at a spread of 30 nothing else counts
        j = x.argmax(axis=1)
        x[np.arange(R), j], x[np.arange(R), C - 1] = x[np.arange(R), C - 1].copy(), x[np.arange(R), j].copy()
    if kind == "constant_row":
        x[0] = 100.0
    if kind == "neg_inf":
        mask = rng.rand(R, C) < 0.25
        mask[:, 0] = False
        mask[0, C - 1] = True
        x[mask] = -np.inf
    if kind == "nan_row":
        x[R // 2, C // 2] = np.nan
    return x.astype(F32)


def softmax_rows_input(case, kind):
    """[R, ld]: the logits of softmax_input, columns C .. ld - 1 NaN (never read)"""
    R, C, ld = case
    x = np.full((R, ld), np.nan, F32)
    x[:, :C] = softmax_input(R, C, kind, _rng("softmax", case, kind))
    return x


def rpn_input(case, kind):
    """[H*W, ld] scores: the pairs' logits by softmax_input over [HW * A, 2] rows (so 'constant_row' makes pair 0 equal, 'nan_row' poisons one
    pair, 'neg_inf' one side of some pairs); 'pairs': randn3 with the first pairs (+88, -88), (-88, +88) and (3, 3); columns 2A .. NaN"""
    H, W, A, ld = case
    rng = _rng("rpn", case, kind)
    rows = softmax_input(H * W * A, 2, "randn3" if kind == "pairs" else kind, rng)
    if kind == "pairs":
        extra = np.array([[88, -88], [-88, 88], [3, 3]], F32)[:min(3, rows.shape[0])]
        rows[:extra.shape[0]] = extra
    x = np.full((H * W, ld), np.nan, F32)
    x[:, :2 * A] = rpn_unrows(rows, A)
    return x


RPN_KINDS = SOFTMAX_KINDS + ("pairs",)


def colsum_input(case):
    M, C = case
    rng = _rng("colsum", case)
    return (rng.randn(M, C) * 2.0 ** rng.randint(-8, 9, size=(M, 1))).astype(F32)


def ce_labels(R, C, kind, rng):
    """'valid': uniform classes; 'half': about half -1, with at least one valid row and (R > 1) one ignored row; 'ignored': all -1"""
    lab = rng.randint(0, C, size=R).astype(F32)
    if kind == "half":
        lab[rng.rand(R) < 0.5] = -1
        lab[0] = 1
        if R > 1:
            lab[R - 1] = -1
    if kind == "ignored":
        lab[:] = -1
    return lab


def ce_row_input(case, labels, logits):
    R, C = case
    rng = _rng("ce", case, labels, logits)
    return (rng.randn(R, C) * (30.0 if logits == "randn30" else 2.0)).astype(F32), ce_labels(R, C, labels, rng)


def ce_rpn_input(case, labels, logits):
    """(score [1,H,W,2A], labels [1,1,A*H,W])"""
    A, H, W = case
    rng = _rng("ce_rpn", case, labels, logits)
    return ((rng.randn(1, H, W, 2 * A) * (30.0 if logits == "randn30" else 2.0)).astype(F32),
            ce_labels(A * H * W, 2, labels, rng).reshape(1, 1, A * H, W))


def smooth_l1_input(n, sigma, div):
    """(pred, tgt, in_w, out_w): d = randn * 2 (both branches, both signs); inside weights in {0, 1}; outside weights in (0, 1] with some
    zeros.  Element 0 has in_w = out_w = 1, tgt = 0 and d halfway between 1 / sigma^2 and 1 / sigma; elements 1 .. 4 (where n allows) sit one
    float32 step below / above the float32 threshold fl(1 / sigma^2), at either sign; element 5 is d = -3 (linear, negative)."""
    rng = _rng("sl1", n, sigma, div)
    pred, tgt = (rng.randn(n) * 2).astype(F32), rng.randn(n).astype(F32)
    iw = (rng.rand(n) < 0.7).astype(F32)
    ow = np.where(rng.rand(n) < 0.2, 0.0, rng.rand(n) * 0.9 + 0.1).astype(F32)
    thr = F32(1) / (F32(sigma) * F32(sigma))
    special = [F32(0.5 * (1.0 / sigma ** 2 + 1.0 / sigma)), np.nextafter(thr, F32(0)), np.nextafter(thr, F32(2)),
               -np.nextafter(thr, F32(0)), -np.nextafter(thr, F32(2)), F32(-3)][:n]
    for i, d in enumerate(special):
        pred[i], tgt[i], iw[i], ow[i] = d, 0, 1, 1
    return pred, tgt, iw, ow
