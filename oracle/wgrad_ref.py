"""TEST INFRASTRUCTURE ONLY -- the filter gradients of the reverse sweep (csrc/wgrad_tn.hip, csrc/wgrad_h2.hip, k_dwconv3x3_wgrad of
csrc/backward_kernels.hip) under the elementwise bound of oracle/dgrad_ref.py:

    |got - want| <= c * 2^-23 * bound,    B = the same float64 operation on |dY| and |X|  (floored at the smallest normal float32)

so a filter gradient that drops ONE pixel fails it -- on training-shaped operands (dgrad_ref.operands 'block4': RoIs of magnitudes
2^+-8, dY constant over 7x7 blocks) the max-relative 2e-6 of tests/test_wgrad_gpu.py does not see that.

bound() is B for the float32 routes ("tn", "dw").  For "h2" it is B + 2^-16 F, the format floor of k_wgrad_h2:
  The kernel gives every (channel, 64-pixel slab) segment of dY and of the X tap one power-of-two scale 2^e that puts the segment's
  largest magnitude into [2^14, 2^15), and stores v 2^e as h + l, two fp16 roundings.  The remainder piece l is exact to 2^-11
  relative while it is a normal fp16 number, and below that to half the smallest fp16 subnormal, 2^-25, absolute.  So
      |v 2^e - (h + l)| <= max(2^-22 |v 2^e|, 2^-25),
  and since max_slab |v| 2^e >= 2^14 the absolute part is, unscaled, at most 2^-25 2^-14 = 2^-39 = 2^-23 2^-16 of the SLAB MAXIMUM of
  that channel -- whatever the element itself is (an element 2^-40 of its slab's maximum comes back 0).  The relative part is what
  c 2^-23 B covers.  The absolute part of the slab's product sum_m dY[m,n] X[m,c] is therefore at most
      2^-39 ( max_m |dY[m,n]| sum_m |X[m,c]|  +  sum_m |dY[m,n]| max_m |X[m,c]| ),
  one term per operand, and F sums that over the slabs.  Slices are cut at slab granularity from pixel 0, so the slabs (and F) do not
  depend on the launch plan.  tests/test_wgrad_bounds_cpu.py shows the floor is needed (the format itself exceeds c under plain B on
  block4 / m20) and that it hides nothing: every perturbed() reference still fails the h2 bound.

CASES, PLANS and plan() say which loop and slice edges of the two kernels run (tests/test_wgrad_bounds_cpu.py asserts that the list
contains them); tests/test_wgrad_gpu.py ties plan() to the library through the workspace sizes."""
import functools

import numpy as np

from dgrad_ref import EPS, SAME3, ZERO, conv_out, operands as _dgrad_operands, ratio, wgrad64  # noqa: F401  (re-exported to the tests)

# c per route, in units of 2^-23 bound(): the numbers test_conv2d_wgrad_block4_conv3_structured_operands already holds.  16 2^-23 =
# 1.9e-6 stays under the 2e-6 max-relative gate of the same test.  Measured maxima on the MI355X over CASES x PLANS (DW_CASES with and
# without scale), max |got - want| / (2^-23 bound):
#            random   block4   spread
#   tn        2.42     6.46     7.63      (same3x3_s2 many slices; rpn3x3 one slice; rpn3x3 one slice)
#   h2        3.14     4.50     5.67      (n3_s2_m45; fc_as_1x1; same3x3 one slice)
#   dw        0.55                        (17x21_s2, plain; 0.28 on two_chunks)
#   h2 / tn   2.44     2.63     2.68      (largest r_h2 / r_tn on the same data, tn under the automatic plan: m33, m20, m20 -- the
#                                          shapes where 20 or 33 pixels leave the f32 kernel almost nothing to accumulate)
ROUTE_C = {"tn": 16.0, "h2": 16.0, "dw": 16.0}
# f32 class of k_wgrad_h2: its ratio is at most 3x that of k_wgrad_tn on the same data, plus a floor of 1e-7 of the scale
CLASS_FACTOR_H2 = 3.0
CLASS_FLOOR = 1e-7 / EPS

TINY = 2.0 ** -126                      # the smallest normal float32

SLAB = {"tn": 32, "h2": 64}             # pixels per slab: the unit slices are cut in, and for h2 the scale block

# (id, N, H, W, Cin, Cout, k, stride, pad (top, bottom, left, right))  (H, W: the input x of the forward convolution)
CASES = [
    ("pointwise", 1, 38, 63, 256, 128, 1, 1, ZERO),
    ("shortcut_s2", 1, 38, 63, 128, 256, 1, 2, ZERO),
    ("same3x3", 1, 20, 30, 64, 64, 3, 1, SAME3),
    ("same3x3_s2", 1, 21, 31, 128, 128, 3, 2, (0, 1, 0, 1)),
    ("roi_tail", 40, 7, 7, 128, 256, 3, 1, SAME3),
    ("fc_as_1x1", 96, 1, 1, 1024, 192, 1, 1, ZERO),
    ("rpn3x3", 1, 38, 63, 256, 512, 3, 1, SAME3),
    ("pw_37x63", 1, 37, 63, 128, 128, 1, 1, ZERO),             # M = 2331: many slices, the last one shorter (1 of 3 / 3 of 5 slabs)
    ("m20", 1, 4, 5, 64, 64, 1, 1, ZERO),                      # M below one slab: nloc = 1, shorter than the tn ring's prologue
    ("m33", 1, 3, 11, 64, 128, 1, 1, ZERO),                    # M = 32 + 1
    ("m64_3x3", 1, 8, 8, 128, 128, 3, 1, SAME3),               # exactly one h2 slab
    ("m65", 1, 5, 13, 128, 64, 1, 1, ZERO),                    # M = 64 + 1: a last slab of one pixel on both routes
    ("n3_s2_m60", 3, 9, 11, 64, 64, 3, 2, (0, 1, 0, 1)),       # 20 pixels per image, gathered at stride 2 (Cin = 64: 64-wide tiles only)
    ("row_1x40", 1, 1, 40, 64, 64, 3, 1, SAME3),               # six of nine taps are padding for every pixel: dW there is exactly 0
    ("n5_1x1s2", 5, 7, 7, 64, 128, 1, 2, ZERO),                # 16 pixels per image, gathered
    ("c192_3x3", 1, 10, 12, 192, 192, 3, 1, SAME3),            # column tiles three to a tap, 128-wide tiles refused
    ("roi37_3x3", 37, 7, 7, 128, 128, 3, 1, SAME3),
    # k_wgrad_h2's load_slab carries (img, oh, ow) along a thread's run of 4 (64-wide tiles) or 8 (128-wide) consecutive pixels that starts
    # at a multiple of the run: 20 pixels per image never put an image boundary inside one.  15 per image do, under both tile sizes
    ("n3_s2_m45", 3, 6, 10, 128, 128, 3, 2, (0, 1, 0, 1)),
]
PLANS = [(0, 0), (64, 1), (128, 4096)]                          # (tile, min_workgroups) of frcnn_conv2d_wgrad[_h2]_set_plan; 0 = automatic
PLAN_IDS = ["auto", "t64_one_slice", "t128_many_slices"]
KINDS = ["random", "block4", "spread"]

# depthwise 3x3: (id, N, H, W, C, stride, pad); k_dwconv3x3_wgrad cuts the pixels into chunks of 4096 and the channels into groups of 64
DW_CHUNK = 4096
DW_CASES = [
    ("two_chunks", 1, 65, 64, 128, 1, SAME3),                  # M = 4160: a second chunk of 64 pixels; two channel groups
    ("one_chunk_exact", 1, 64, 64, 72, 1, SAME3),              # M = 4096; C / 4 = 18: the second channel group is ragged
    ("s2_three_images", 3, 75, 77, 64, 2, (0, 1, 0, 1)),       # 37 x 38 outputs, M = 4218: the chunk edge falls inside image 2
    ("17x21_s1", 2, 17, 21, 32, 1, SAME3),                     # the shapes of test_maxpool_and_depthwise_gradients_vs_torch
    ("17x21_s2", 2, 17, 21, 32, 2, SAME3),
]


def cdiv(a, b):
    return -(-a // b)


def out_hw(case):
    _, N, H, W, Cin, Cout, k, stride, pad = case
    return conv_out(H, k, stride, pad[0], pad[1]), conv_out(W, k, stride, pad[2], pad[3])


def plan(route, M, Cin, Cout, Kf, tile=0, min_wgs=0):
    """(BT, S, chunk) of one launch: a restatement in Python of wgrad_plan (csrc/wgrad_tn.hip, route 'tn') and wgrad_h2_plan
    (csrc/wgrad_h2.hip, route 'h2') -- tile edge BT, S slices of `chunk` slabs each (the last one may be shorter).  tests/test_wgrad_gpu.py
    checks S against the library's workspace sizes."""
    auto_tiles, auto_wgs, keep = {"tn": (128, 512, 4), "h2": (32, 256, 2)}[route]
    nslabs = cdiv(M, SLAB[route])
    BT = 64
    ok128 = Cout % 128 == 0 and Cin % 128 == 0
    if ok128 and (Cout // 128) * (Kf // 128) >= auto_tiles:
        BT = 128
    if tile == 64 or (tile == 128 and ok128):
        BT = tile
    tiles = (Cout // BT) * (Kf // BT)
    want = cdiv(min_wgs if min_wgs > 0 else auto_wgs, tiles)
    want = max(1, min(want, nslabs // keep))
    chunk = cdiv(nslabs, want)
    return BT, cdiv(nslabs, chunk), chunk


def slices(route, M, S, chunk):
    """slab count of every slice of a launch"""
    nslabs = cdiv(M, SLAB[route])
    return [min(nslabs - s * chunk, chunk) for s in range(S)]


def operands(kind, case, seed=3):
    """(dY [N,OH,OW,Cout], X [N,H,W,Cin]) float32.  'random' and 'block4' are dgrad_ref.operands; 'spread' gives every pixel its own
    power-of-two magnitude: dY randn gated at 0.5 times 2^[-12, 12], X post-ReLU times 2^[-6, 6] -- inside a 64-pixel slab the elements
    of one channel then lie up to 2^24 (dY) below the maximum that sets the h2 scale.  For the accuracy assertion only: a pixel that far
    below its neighbours is below float32 resolution, so no bound can see it dropped."""
    _, N, H, W, Cin, Cout, k, stride, pad = case
    if kind != "spread":
        gy, _, x, _ = _dgrad_operands(kind, N, H, W, Cin, Cout, k, stride, pad, seed=seed)
        return gy, x
    OH, OW = out_hw(case)
    rng = np.random.RandomState(seed + 104729)
    gy = rng.randn(N, OH, OW, Cout) * (rng.rand(N, OH, OW, Cout) < 0.5) * 2.0 ** rng.randint(-12, 13, size=(N, OH, OW, 1))
    x = np.maximum(rng.randn(N, H, W, Cin), 0) * 2.0 ** rng.randint(-6, 7, size=(N, H, W, 1))
    return gy.astype(np.float32), x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(case_id, kind):
    """(dY, X, want, B, F) of one case and operand kind, computed once and shared read-only by every test that needs it"""
    case = next(c for c in CASES if c[0] == case_id)
    _, N, H, W, Cin, Cout, k, stride, pad = case
    gy, x = operands(kind, case)
    out = (gy, x, wgrad64(gy, x, k, k, stride, pad), bound(gy, x, k, stride, pad, "tn"), h2_floor(gy, x, k, stride, pad))
    for a in out:
        a.setflags(write=False)
    return out


def _taps(x, KH, KW, stride, pad, OH, OW):
    """(kh, kw, that tap's rows of x as [M, Cin], zeros where the tap is padding)"""
    x = np.asarray(x, np.float64)
    N, H, W, Cin = x.shape
    xp = np.zeros((N, max(pad[0] + H, KH + (OH - 1) * stride), max(pad[2] + W, KW + (OW - 1) * stride), Cin))
    xp[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W] = x
    for kh in range(KH):
        for kw in range(KW):
            yield kh, kw, xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride].reshape(-1, Cin)


def _slab_stats(a, slab):
    """a [M, C] >= 0 -> (max, sum) over each `slab`-row segment, [nslabs, C] each"""
    M, C = a.shape
    n = cdiv(M, slab)
    p = np.zeros((n * slab, C))
    p[:M] = a
    p = p.reshape(n, slab, C)
    return p.max(axis=1), p.sum(axis=1)


def h2_floor(gy, x, k, stride, pad):
    """F [Cout,k,k,Cin] of the module docstring: per tap, sum over the global 64-pixel slabs of
    max |dY| sum |X| + sum |dY| max |X|  (per output channel n and input channel c)"""
    g = np.abs(np.asarray(gy, np.float64))
    N, OH, OW, Cout = g.shape
    amax, asum = _slab_stats(g.reshape(-1, Cout), SLAB["h2"])
    F = np.zeros((Cout, k, k, x.shape[-1]))
    for kh, kw, xt in _taps(np.abs(x), k, k, stride, pad, OH, OW):
        xmax, xsum = _slab_stats(xt, SLAB["h2"])
        F[:, kh, kw, :] = amax.T @ xsum + asum.T @ xmax
    return F


def _normal(B):
    """B floored at the smallest normal float32 wherever anything was summed: below it a float32 rounding errs by up to 2^-150 absolute
    (2^-23 * 2^-126 is one subnormal step), not 2^-24 relative -- 'block4' x holds 1.18e-38, whose products are subnormal.  Elements with
    B = 0 (taps that are padding for every pixel) keep B = 0: there only an exact 0 passes."""
    return np.where(B > 0, np.maximum(B, TINY), 0.0)


def bound(gy, x, k, stride, pad, route):
    B = _normal(wgrad64(np.abs(gy), np.abs(x), k, k, stride, pad))
    if route == "h2":
        return B + 2.0 ** -16 * h2_floor(gy, x, k, stride, pad)
    assert route in ("tn", "dw"), route
    return B


def perturbed(gy, x, k, stride, pad):
    """references a wrong kernel could produce: the last output row / column / pixel of dY dropped, pixel 64 (the first of the second h2
    slab) dropped, the pad shifted by one, kh and kw transposed"""
    N, OH, OW, Cout = gy.shape

    def dropped(fn):
        g = np.array(gy, copy=True)
        fn(g)
        return wgrad64(g, x, k, k, stride, pad)

    def row(g): g[:, -1] = 0
    def col(g): g[:, :, -1] = 0
    def last(g): g.reshape(-1, Cout)[-1] = 0
    def p64(g): g.reshape(-1, Cout)[64] = 0
    yield "drop_last_row", dropped(row)
    yield "drop_last_col", dropped(col)
    yield "drop_last_pixel", dropped(last)
    if N * OH * OW > 64:
        yield "drop_pixel_64", dropped(p64)
    if k > 1:
        yield "pad_shift_h", wgrad64(gy, x, k, k, stride, (pad[0] + 1, pad[1] - 1, pad[2], pad[3]))
        yield "pad_shift_w", wgrad64(gy, x, k, k, stride, (pad[0], pad[1], pad[2] + 1, pad[3] - 1))
        yield "taps_transposed", np.ascontiguousarray(wgrad64(gy, x, k, k, stride, pad).transpose(0, 2, 1, 3))


def dw_operands(case, seed=3):
    """(g [N,OH,OW,C], x [N,H,W,C], scale [C]) float32: gated gradients, post-ReLU activations, a frozen-BN fold in [0.5, 1.5)"""
    _, N, H, W, C, stride, pad = case
    OH, OW = conv_out(H, 3, stride, pad[0], pad[1]), conv_out(W, 3, stride, pad[2], pad[3])
    rng = np.random.RandomState(seed + N + H + W + C)
    g = rng.randn(N, OH, OW, C) * (rng.rand(N, OH, OW, C) < 0.6)
    x = np.maximum(rng.randn(N, H, W, C), 0)
    return g.astype(np.float32), x.astype(np.float32), (rng.rand(C) + 0.5).astype(np.float32)


def dw_wgrad64(g, x, stride, pad, scale=None):
    """float64 filter gradient [3,3,C] of a depthwise 3x3 convolution whose forward filter is master * scale[c] (frozen-BN fold):
    dW[kh,kw,c] = scale[c] sum_pixels g[n,oh,ow,c] x[n, oh s - top + kh, ow s - left + kw, c]   (scale None: 1)"""
    g = np.asarray(g, np.float64)
    N, OH, OW, C = g.shape
    gm = g.reshape(-1, C)
    out = np.empty((3, 3, C))
    for kh, kw, xt in _taps(x, 3, 3, stride, pad, OH, OW):
        out[kh, kw] = (gm * xt).sum(axis=0)
    return out if scale is None else out * np.asarray(scale, np.float64)


def dw_bound(g, x, stride, pad, scale=None):
    return _normal(dw_wgrad64(np.abs(g), np.abs(x), stride, pad, None if scale is None else np.abs(scale)))
