"""The forward pass's convolutions, top to bottom: Plan, what the launch plan depends on besides shapes (the network hands it the switches;
nothing here reads a configuration); the route rules, WHICH pipe a convolution takes -- pure functions of a Plan, host integers and scope
strings, asked by the consumer ("do I run h2?") and, with the consumer's shape, by its producer ("will it read planes?"); Forms, the forms
(float32, operand planes) one build's activations exist in; one function per route, which makes that route's marks and launches and
tells the Forms what it wrote.  The reverse sweep's counterpart is frcnn_hip/sweep.py."""
import collections

from . import ACT_NONE, ACT_RELU

ZERO_PAD = (0, 0, 0, 0)
PLAN_IMAGES = 4                        # csrc/conv_igemm.hip PLAN_IMAGES: every launch-size rule is evaluated for a batch of this many images
H2_MIN_CHANNEL_RATIO = 2.0 ** -18      # see Session.h2_channel_spread


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
SWITCHES = (("mfma_h2", bool), ("h2_train", bool), ("h2_lazy_split", bool), ("h2_trunk_planes", bool), ("h2_tile_cfg", int), ("mfma_x3", bool),
            ("x3_tile_cfg", int), ("winograd", bool), ("winograd_train", bool), ("winograd_min_cin", int), ("winograd_m", int),
            ("winograd_7x7", bool), ("winograd_f2_scopes", tuple), ("winograd_direct_scopes", tuple), ("winograd_fused_f2", bool),
            ("fuse_tail_mean", bool))


class Plan(collections.namedtuple("Plan", ("mode", "plan_batch", "h2_min_tiles") + tuple(name for name, _ in SWITCHES))):
    """mode "TEST" / "TRAIN"; plan_batch: images per launch that TEST-mode launch-size rules see (0: the launch as it is); h2_min_tiles:
    the mode's threshold (h2_min_tiles()); then SWITCHES, the cfg.HIP switches of the same names.  Built once per graph build."""
    __slots__ = ()

    def key(self):
        """what a captured TEST-mode chain depends on: every field but the TRAIN-only Winograd switch"""
        return tuple(v for f, v in zip(self._fields, self) if f != "winograd_train")


def h2_min_tiles(mode, hip):
    """Tiles a launch must have to take frcnn_gemm_h2.  TEST: H2_MIN_TILES.  TRAIN (one image per step): H2_TRAIN_MIN_TILES, or -- when that is
    None -- the same knob as TEST mode (tests force the kernel onto toy TRAIN networks).  Each value means what it says: no comparison against a default."""
    if mode == "TRAIN" and hip["H2_TRAIN_MIN_TILES"] is not None:
        return int(hip["H2_TRAIN_MIN_TILES"])
    return int(hip["H2_MIN_TILES"])


def make_plan(mode, plan_batch, hip):
    """hip: the mapping of switches (cfg.HIP)"""
    return Plan(mode, int(plan_batch), h2_min_tiles(mode, hip), *(kind(hip[name.upper()]) for name, kind in SWITCHES))


# ---- the route rules -------------------------------------------------------------------------------------------------------------------
def plan_rows(plan, M):
    """Rows of a launch as they would be in a PLAN_IMAGES-image batch.  Which matrix pipe a GEMM runs on (>= 150 tiles: h2 / x3) and whether a
    convolution is cut along K change the bits of the result, so neither may depend on how many images share the launch: TEST-mode rules see
    per-image rows x PLAN_IMAGES whatever the batch is (the same image gives the same tensors at batch 1, in any slot of a batch of 4, or of 8)."""
    B = plan.plan_batch
    return M // B * PLAN_IMAGES if (B > 0 and M % B == 0) else M


def channel_spread(sess, plan, scope):
    """the h2 rule's `spread` argument for the filter of `scope`: static filters (TEST mode) only"""
    return sess.h2_channel_spread(scope) if plan.mode == "TEST" else 1.0


def h2_rule(plan, M, N, K, G=1, spread=1.0, planes=True):
    """Does G x [M,K] x [N,K]^T run in frcnn_gemm_h2?  K % 128 == 0 (scale blocks), N % 128 == 0 (tiles), enough tiles to fill the chip, the
    kernel's 32-bit offset limits.  TEST: static filters, split once; one whose entries for an input channel are < 2^-18 of the rest
    (spread) takes the exact x3 split instead.  TRAIN (h2_train): the solver re-splits the updated filters after every step (Session.
    h2_refresh).  planes: the left operand exists as operand planes or may be split by a separate pass (a producer asking: it will emit them)."""
    if plan.mode == "TEST" and spread < H2_MIN_CHANNEL_RATIO:
        return False
    return bool(planes and plan.mfma_h2 and (plan.mode == "TEST" or plan.h2_train) and K % 128 == 0 and N % 128 == 0
                and ((plan_rows(plan, M) + 127) // 128) * (N // 128) * G >= plan.h2_min_tiles
                and 4 * G * M * K < (1 << 32) and 4 * N * K < (1 << 32) and M * N < (1 << 29))


def x3_rule(plan, M, N, K, G=1):
    """frcnn_gemm_x3: TEST mode (static filters), N % 64 == 0, K % 32 == 0 and at least 150 tiles of 128 x 128 -- below that the
    split-K f32 launches are as fast (profiles/r02_m_x3_sweep.txt, single-image rows)."""
    return (plan.mfma_x3 and plan.mode == "TEST" and N % 64 == 0 and K % 32 == 0
            and ((plan_rows(plan, M) + 127) // 128) * ((N + 127) // 128) * G >= 150 and M * N < (1 << 31) and N * K < (1 << 28))


def winograd_scheme(plan, scope, H, W):
    """2 / 4 = F(m x m,3x3) tiles; 7 = the mixed F(4,3)+F(3,3) scheme for 7x7 maps (121 instead of 144 GEMM rows per RoI)."""
    if any(tok in scope for tok in plan.winograd_f2_scopes):
        return 2
    return 7 if (plan.winograd_m == 4 and H == 7 and W == 7 and plan.winograd_7x7) else plan.winograd_m


def conv_route(plan, scope, k, stride, pad, act, Cin, Cout, M, residual=False, res_stride=1, fold_w=False, out_affine=False, no_bias=False, spread=1.0, planes=True):
    """The key of CONV under which y[M,Cout] = conv(x[...,Cin], k, stride, pad) of `scope` runs.  residual / out_affine: the launch has
    one; spread, planes: see h2_rule.  One statement per route, in priority order."""
    pad = tuple(pad)
    if (plan.winograd and (plan.mode == "TEST" or plan.winograd_train) and k == 3 and stride == 1 and pad == (1, 1, 1, 1)
            and not residual and not fold_w and not out_affine and not no_bias and Cin % 32 == 0 and Cin >= plan.winograd_min_cin
            and act in (ACT_NONE, ACT_RELU) and not any(tok in scope for tok in plan.winograd_direct_scopes)):
        return "winograd"
    plain = k == 1 and stride == 1 and pad == ZERO_PAD and not fold_w and (not residual or res_stride == 1)
    if plain and h2_rule(plan, M, Cout, Cin, 1, spread, planes):
        return "h2"          # a plain GEMM on the fp16 matrix pipe, block-scaled two-piece operands
    if plain and x3_rule(plan, M, Cout, Cin, 1):
        return "x3"          # ... on the bf16 matrix pipe with exact bf16x3 operand splits
    return "direct"


def winograd_products(plan, T, Cout, Cin, G, m, pixels, spread=1.0):
    """The form of the G products [T,Cin] x [Cout,Cin]^T of a TEST-mode Winograd chain over `pixels` output pixels."""
    if plan.winograd_fused_f2 and m == 2 and Cin == 64 and Cout == 64 and x3_rule(plan, T, Cout, Cin, G) and pixels < (1 << 23):
        return "fused_x3"    # block1's conv2: transforms and products in one launch, the bits of the x3 chain (csrc/winograd2_fused.hip)
    if h2_rule(plan, T, Cout, Cin, G, spread):
        return "h2"
    return "x3" if x3_rule(plan, T, Cout, Cin, G) else "f32"


def emits_planes(plan, emit_h2, Cout):
    """Does a producer whose consumer reads operand planes (emit_h2) write them from its epilogue?"""
    return bool(emit_h2 and plan.mfma_h2 and Cout % 128 == 0)


def mean_fusable(plan, rows, cout, cin, group_rows=1, spread=1.0):
    """conv1x1_mean applies where the tail's last convolution runs in frcnn_gemm_h2 (TEST mode, h2-eligible shape and filter), the RoI
    rows split evenly over the images of the batch (whole groups of `group_rows` rows per image), and its input can exist as planes:
    emitted by the Winograd conv2, or split lazily."""
    G = max(1, plan.plan_batch)
    return bool(plan.fuse_tail_mean and plan.mode == "TEST" and rows % G == 0 and (rows // G) % max(1, int(group_rows)) == 0
                and h2_rule(plan, rows, cout, cin, 1, spread) and (plan.h2_lazy_split or plan.winograd))


# ---- the forms of the activations ------------------------------------------------------------------------------------------------------
class Forms(object):
    """Facts about ONE build's launches (buffers are reused across builds): `planes`, activation address -> the ops.H2 operand planes of
    that tensor, and `f32_missing`, the addresses of activations that exist ONLY as operand planes (never read as float32)."""
    __slots__ = ("ops", "sess", "tag", "lazy_split", "planes", "f32_missing")

    def __init__(self, ops, sess, tag, lazy_split):
        self.ops, self.sess, self.tag, self.lazy_split, self.planes, self.f32_missing = ops, sess, tag, lazy_split, {}, set()

    def wrote(self, t, planes=None, f32=True):
        """Every launch that writes activation t reports it: planes derived from an earlier write are dropped (buffers are static
        and sub-graphs may be re-run on new inputs), planes this launch emitted are registered."""
        k = t.data_ptr()
        if planes is None:
            self.planes.pop(k, None)
        else:
            self.planes[k] = planes
        (self.f32_missing.discard if f32 else self.f32_missing.add)(k)
        return t

    def need_f32(self, *tensors):
        if any(t is not None and t.data_ptr() in self.f32_missing for t in tensors):
            raise RuntimeError("graph construction error: a float32 consumer reads a tensor that was emitted as operand planes only")

    def has_planes(self, t):
        return t.data_ptr() in self.planes

    def planes_of(self, x):
        """Operand planes of activation x: those its producer emitted, else (lazy_split) a frcnn_h2_split pass, else None."""
        xp = self.planes.get(x.data_ptr())
        if xp is None and self.lazy_split:
            self.need_f32(x)
            K = x.shape[-1]
            xp = self.planes[x.data_ptr()] = self.sess.h2_buf(self.tag + "/split@%x" % x.data_ptr(), x.numel() // K, K)
            self.sess.mark("op:h2_split", 0, lambda: self.ops.h2_split(x, out=xp), nbytes=8 * x.numel())
        return xp

    def residual_operand(self, t):
        """what an h2 launch reads residual t from: its planes where the trunk exists as operand planes only (h2_trunk_planes)"""
        return self.planes[t.data_ptr()] if (t is not None and t.data_ptr() in self.f32_missing) else t


# ---- the routes ------------------------------------------------------------------------------------------------------------------------
# Every route: conv_<route>(ops, sess, plan, forms, tag, scope, x, k, stride, pad, act, bn_eps, residual, res_stride, fold_w, out_affine,
#                           real_cin, no_bias, emit_h2, want_f32) -> the output tensor
#   ops: the module of C-ABI entries the launches go through (the caller's, so that a test which replaces it by stand-ins replaces these
#   launches too); sess: buffers, packed / derived filters, mark; tag: the network's buffer prefix.  emit_h2 / want_f32 (mfma_h2): the
#   caller knows the consumers of the result -- emit_h2: a frcnn_gemm_h2 launch will read it, so the producer writes its operand planes
#   from its epilogue; want_f32 = False: nothing reads the float32 tensor (honoured only where the planes are emitted, TEST mode).
def _packed(ops, sess, tag, scope, x, k, stride, pad, bn_eps, fold_w, out_affine, real_cin, no_bias):
    """(w, b, out, flops) of a convolution that reads the packed filter"""
    w, b = sess.conv_params(scope, bn_eps=bn_eps, fold_w=fold_w, out_scale=None if out_affine is None else out_affine[0],
                            out_shift=None if out_affine is None else out_affine[1])
    N, H, W, Cin = x.shape
    out = sess.buf(tag + "/" + scope, (N, ops.conv_out_size(H, k, stride, pad[0], pad[1]), ops.conv_out_size(W, k, stride, pad[2], pad[3]), w.shape[0]))
    return w, None if no_bias else b, out, 2 * out.numel() * k * k * (Cin if real_cin is None else real_cin)


def conv_direct(ops, sess, plan, forms, tag, scope, x, k, stride, pad, act, bn_eps, residual, res_stride, fold_w, out_affine, real_cin, no_bias, emit_h2, want_f32):
    w, b, out, flops = _packed(ops, sess, tag, scope, x, k, stride, pad, bn_eps, fold_w, out_affine, real_cin, no_bias)
    forms.need_f32(x, residual)
    sess.mark("conv:" + scope, flops, lambda: ops.conv2d(x, w, b, k, k, stride, pad, act, residual, res_stride, fold_w, out=out),
              nbytes=4 * (x.numel() + w.numel() + out.numel() + (out.numel() if residual is not None else 0)))
    return forms.wrote(out)


def conv_x3(ops, sess, plan, forms, tag, scope, x, k, stride, pad, act, bn_eps, residual, res_stride, fold_w, out_affine, real_cin, no_bias, emit_h2, want_f32):
    w, b, out, flops = _packed(ops, sess, tag, scope, x, k, stride, pad, bn_eps, fold_w, out_affine, real_cin, no_bias)
    forms.need_f32(x, residual)
    Cout, Cin, planes = w.shape[0], x.shape[-1], sess.x3_planes(w)
    sess.mark("conv:x3:" + scope, flops, lambda: ops.gemm_x3(x, planes, 1, out.numel() // Cout, Cout, Cin, b, residual, act, out=out, cfg=plan.x3_tile_cfg),
              nbytes=4 * (x.numel() + out.numel() + (out.numel() if residual is not None else 0)) + 6 * w.numel())
    return forms.wrote(out)


def conv_h2(ops, sess, plan, forms, tag, scope, x, k, stride, pad, act, bn_eps, residual, res_stride, fold_w, out_affine, real_cin, no_bias, emit_h2, want_f32):
    w, b, out, flops = _packed(ops, sess, tag, scope, x, k, stride, pad, bn_eps, fold_w, out_affine, real_cin, no_bias)
    Cout, Cin = w.shape[0], x.shape[-1]
    M = out.numel() // Cout
    xp, wp = forms.planes_of(x), sess.h2_planes(w)
    yp = sess.h2_buf(tag + "/" + scope, M, Cout) if emit_h2 else None
    y = out if (want_f32 or yp is None or plan.mode == "TRAIN") else None
    res = forms.residual_operand(residual)
    sess.mark("conv:h2:" + scope, flops, lambda: ops.gemm_h2(xp, wp, 1, M, Cout, Cin, b, res, act, out=y, out_planes=yp, want_f32=False, cfg=plan.h2_tile_cfg),
              nbytes=4 * M * Cin + 4 * w.numel() + (4 * out.numel() if y is not None else 0)
              + (4 * out.numel() if yp is not None else 0) + (4 * out.numel() if residual is not None else 0))
    return forms.wrote(out, yp, y is not None)


def conv_winograd(ops, sess, plan, forms, tag, scope, x, k, stride, pad, act, bn_eps, residual, res_stride, fold_w, out_affine, real_cin, no_bias, emit_h2, want_f32):
    """3x3 / stride 1 / SAME convolution as Winograd F(m x m,3x3): input transform -> (m+2)^2 GEMMs in ONE launch -> output transform with bias
    + ReLU.  Exact algebra in f32; m = 2 (2.25x fewer multiplications, rounding like the direct kernel) or m = 4 (4x fewer; one layer rounds
    ~10x worse than direct, through the full ResNet-101 the outputs move by ~1e-6 relative, profiles/r01_e_winograd_error.txt).  TEST: the static
    transformed filter, the products in the form winograd_products names (h2: the input transform emits V as operand planes); emit_h2: the output
    transform emits the next 1x1's operand planes.  TRAIN: the live (folded) device filter is transformed, then the same chain in one call."""
    forms.need_f32(x)
    N, H, W, Cin = x.shape
    m = winograd_scheme(plan, scope, H, W)
    T = ops.winograd_tiles(N, H, W, m)
    if plan.mode == "TRAIN":
        w, b, out, _ = _packed(ops, sess, tag, scope, x, k, stride, pad, bn_eps, fold_w, out_affine, real_cin, no_bias)
        G, Cout = ops.winograd_points(m), w.shape[0]
        # (weight-only: after the first step the solver has it re-run beside the forward pass, frcnn_hip/runtime.py PreparedFilters)
        u = sess.prepared.get(("fwd", "wino_u", tag, scope, m), lambda: ops.winograd_filter_transform_device(
            w, m, False, out=sess.buf(tag + "/wino_u/" + scope, (G, Cout, Cin))))
        mm, v = sess.buf(tag + "/wino_m", (G, T, Cout)), sess.buf(tag + "/wino_v", (G, T, Cin))
        # emit_h2: the output transform writes the float32 tensor (the tape needs it) AND the operand planes of the 1x1 that follows
        yp = sess.h2_buf(tag + "/" + scope, N * H * W, Cout) if emits_planes(plan, emit_h2, Cout) else None
        sess.mark("conv:" + scope, 2 * G * T * Cout * Cin, lambda: ops.conv3x3_winograd(x, u, b, act, out=out, v_buf=v, m_buf=mm, out_planes=yp),
                  nbytes=4 * (v.numel() + u.numel() + mm.numel()))
        return forms.wrote(out, yp)
    u, b = sess.winograd_params(scope, bn_eps=bn_eps, m=m)
    G, Cout = u.shape[0], u.shape[1]
    out = sess.buf(tag + "/" + scope, (N, H, W, Cout))
    flops = 2 * G * T * Cout * Cin
    products = winograd_products(plan, T, Cout, Cin, G, m, N * H * W, channel_spread(sess, plan, scope))
    if products == "fused_x3":
        planes = sess.x3_planes(u)
        sess.mark("conv:x3:" + scope, flops, lambda: ops.winograd2_conv_x3(x, planes, b, act, out), nbytes=4 * (x.numel() + out.numel()) + 6 * u.numel())
        return forms.wrote(out)
    mm = sess.buf(tag + "/wino_m", (G, T, Cout))
    if products == "h2":
        vp, wp = sess.h2_buf(tag + "/wino_v", G * T, Cin), sess.h2_planes(u)
        sess.mark("op:wino_in", 0, lambda: ops.winograd_input_transform_h2(x, vp, m), nbytes=4 * (x.numel() + G * T * Cin))
        sess.mark("conv:h2:" + scope, flops, lambda: ops.gemm_h2(vp, wp, G, T, Cout, Cin, out=mm, cfg=plan.h2_tile_cfg),
                  nbytes=4 * (G * T * Cin + mm.numel()) + 4 * u.numel())
    else:
        v = sess.buf(tag + "/wino_v", (G, T, Cin))
        sess.mark("op:wino_in", 0, lambda: ops.winograd_input_transform(x, v, m), nbytes=4 * (x.numel() + v.numel()))
        if products == "x3":
            planes = sess.x3_planes(u)
            sess.mark("conv:x3:" + scope, flops, lambda: ops.gemm_x3(v, planes, G, T, Cout, Cin, out=mm, cfg=plan.x3_tile_cfg),
                      nbytes=4 * (v.numel() + mm.numel()) + 6 * u.numel())
        else:
            sess.mark("conv:" + scope, flops, lambda: ops.gemm_batched_nt(v, u, mm), nbytes=4 * (v.numel() + u.numel() + mm.numel()))
    if emits_planes(plan, emit_h2, Cout):
        yp = sess.h2_buf(tag + "/" + scope, N * H * W, Cout)
        y = out if want_f32 else None
        sess.mark("op:wino_out", 0, lambda: ops.winograd_output_transform_h2(mm, b, act, (N, H, W, Cout), m, yp, y),
                  nbytes=4 * (mm.numel() + out.numel() * (2 if want_f32 else 1)))
        return forms.wrote(out, yp, y is not None)
    sess.mark("op:wino_out", 0, lambda: ops.winograd_output_transform(mm, b, act, out, m), nbytes=4 * (mm.numel() + out.numel()))
    return forms.wrote(out)


CONV = dict(direct=conv_direct, x3=conv_x3, h2=conv_h2, winograd=conv_winograd)


def conv1x1_mean(ops, sess, plan, forms, tag, scope, x, group_rows, act, bn_eps, residual, name="fc7"):
    """The tail's last 1x1 convolution fused with reduce_mean over the P*P positions of every RoI (resnet_v1.py:115-125), TEST mode:
    frcnn_gemm_h2_mean -- the [R*P*P, Cout] tensor is never written.  One batch entry per IMAGE: a RoI's rows are added in an order that depends on
    its index inside its image only, so batch slots and sizes do not change a bit of fc7 (the caller checks mean_fusable, and that x has planes)."""
    w, b = sess.conv_params(scope, bn_eps=bn_eps)
    Cin, Cout = x.shape[-1], w.shape[0]
    rows = x.numel() // Cin
    G = max(1, plan.plan_batch)
    assert rows % G == 0 and (rows // G) % group_rows == 0
    out = sess.buf(tag + "/" + name, (rows // group_rows, Cout))
    xp, wp, res = forms.planes[x.data_ptr()], sess.h2_planes(w), forms.residual_operand(residual)
    sess.mark("conv:h2:" + scope, 2 * rows * Cout * Cin, lambda: ops.gemm_h2_mean(xp, wp, G, rows // G, Cout, Cin, b, res, act, group_rows, out=out, cfg=plan.h2_tile_cfg),
              nbytes=4 * (rows * Cin + w.numel() + out.numel() + (rows * Cout if residual is not None else 0)))
    return forms.wrote(out)
