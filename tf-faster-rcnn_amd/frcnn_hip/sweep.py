"""The reverse sweep of a training step (TrainState._sweep), top to bottom: dgrad_route, WHICH of the six forms a convolution's data
gradient takes (host integers and three switches only); one function per form and for the filter gradient, making that form's launches
from tensors, an allocator (buf / h2_buf / buf_pair: the session) and prepared(key, fn) -- tests/test_dgrad_gpu.py holds these very
functions to float64; and Sweep, the per-call bookkeeping of the walk over the tape (nothing per-call lives on the TrainState)."""
import bisect

import torch

from . import ACT_NONE, ACT_RELU, ACT_RELU6

ZERO_PAD = (0, 0, 0, 0)


# ---- the route rule --------------------------------------------------------------------------------------------------------------------
def h2_form(k, stride, pad, Cin, Cout, M, h2_train):
    """Does a data gradient of this shape run as frcnn_gemm_h2 (dX = dY W, K = Cout)?  (cfg.HIP.H2_TRAIN)"""
    if k != 1 or stride != 1 or tuple(pad) != ZERO_PAD or h2_train is None:
        return False
    return (Cout % 128 == 0 and Cin % 128 == 0 and ((M + 127) // 128) * (Cin // 128) >= h2_train
            and 4 * M * Cout < (1 << 32) and M * Cin < (1 << 29))


def upsampled_geometry(k, stride, pad, H, W, OH, OW):
    """(up_h, up_w, up_pad): dY spread out on the input grid and the pads of the stride-1 convolution that turns it into dX"""
    up_h, up_w = (OH - 1) * stride + 1, (OW - 1) * stride + 1
    return up_h, up_w, (k - 1 - pad[0], H - up_h - (k - 1 - pad[0]) + k - 1, k - 1 - pad[2], W - up_w - (k - 1 - pad[2]) + k - 1)


def dgrad_route(k, stride, pad, Cin, Cout, H, W, N, OH, OW, ydim, has_grad, pipe_dgrads, winograd, h2_train):
    """(route, m) of the data gradient of y[N,OH,OW,Cout] = conv(x[N,H,W,Cin], k, stride, pad): route is a key of DGRAD (and of
    oracle/dgrad_ref.CASES), m the Winograd tile (None for every other route).  has_grad: the target already holds a gradient.
    pipe_dgrads: strided 3x3 / odd-width 1x1 data gradients on the matrix pipe (False: the gather kernel).  winograd: (m, min
    channels[, 7x7]) or None; h2_train: frcnn_gemm_h2 from so many tiles, or None.  One statement per route, in priority order."""
    pad = tuple(pad)
    # (a tensor that already holds a gradient -- the RPN's 3x3 behind the crop's: Winograd into a scratch tensor + one add pass
    # instead of the direct kernel with its residual epilogue: 4608-deep float32 products, 490 us, r04_aj_train_streams.txt)
    if (winograd is not None and (not has_grad or pipe_dgrads) and k == 3 and stride == 1 and pad == (1, 1, 1, 1)
            and Cout % 32 == 0 and Cout >= winograd[1] and Cin % 4 == 0):
        return "winograd", 7 if (winograd[0] == 4 and len(winograd) > 2 and winograd[2] and OH == 7 and OW == 7) else winograd[0]
    if stride == 1 and Cout % 32 == 0:
        return ("h2" if h2_form(k, stride, pad, Cin, Cout, N * OH * OW, h2_train) else "flipped"), None
    if pipe_dgrads and k == 1 and stride == 1 and pad == ZERO_PAD and Cout % 32 != 0 and Cin % 4 == 0 and ydim == 4:
        return "padded", None
    if (pipe_dgrads and stride > 1 and k > 1 and Cout % 32 == 0 and Cin % 32 == 0
            and min(upsampled_geometry(k, stride, pad, H, W, OH, OW)[2]) >= 0):
        return "upsampled", None
    return "gather", None


# A borrowed buffer (an identity shortcut's gradient, waiting in somebody else's buffer) is consumed out of place -- read as the launch's
# residual, the result written to the record's own buffer -- only by these routes; winograd and gather accumulate in place on a private copy.
OUT_OF_PLACE = frozenset(("flipped", "h2", "padded", "upsampled"))


# ---- the data-gradient routes ----------------------------------------------------------------------------------------------------------
# Every route: dgrad_<route>(ops, alloc, prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit=False, m=None, gy_planes=None)
#   ops: the module of C-ABI entries the launches go through (frcnn_hip.ops -- the caller's, so that a test which replaces the
#   TrainState module's `ops` by stand-ins replaces these launches too);
#   gy [N,OH,OW,Cout], wf the packed forward filter [Cout,k,k,Cin], gx the target [N,H,W,Cin]; gres: what the launch adds to dX (gx
#   itself, or a borrowed buffer for the OUT_OF_PLACE routes), None = a fresh target; mk: x when it is a ReLU output (the gradient's
#   mask) or None; emit: the producer of x runs its own data gradient as frcnn_gemm_h2 and reads this result as operand planes;
#   gy_planes: operand planes of dY emitted by the launch that produced it.
# Returns (masked, planes, pipe, flops): is the WHOLE of gx masked now; the planes emitted or None; the matrix pipe and its FLOP count.
# Weight-only launches (transposed / flipped filters, their h2 split, the Winograd transform of the gradient filter) go through
# prepared(key, fn) (runtime.PreparedFilters.get): after the first step the solver re-runs them on a side stream right after its
# update, beside the next forward pass, and the sweep finds them done.
def _flipped_filter(ops, alloc, prepared, sc, wf, k, Cout):
    return prepared(("wflip", sc), lambda: ops.flip_transpose_filter(wf, out=alloc.buf("bwd/wflip/" + sc, (wf.shape[3], k, k, Cout))))


def dgrad_winograd(ops, alloc, prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit=False, m=None, gy_planes=None):
    # dX = conv(dY, flipped / transposed filter) is itself a 3x3 stride-1 SAME convolution: Winograd, with the
    # gradient filter transformed straight from the packed forward filter
    N, OH, OW, Cout = gy.shape
    Cin, had = wf.shape[3], gres is not None
    G = ops.winograd_points(m)
    T = ops.winograd_tiles(N, OH, OW, m)
    u = prepared(("wino_u", sc, m), lambda: ops.winograd_filter_transform_device(wf, m, True, out=alloc.buf("bwd/wino_u/" + sc, (G, Cin, Cout))))
    fused = mk is not None and m in (4, 7) and not had
    planes = None
    if fused and Cin % 128 == 0 and emit:
        planes = alloc.h2_buf("bwd/gyp/" + sc, gx.numel() // Cin, Cin)      # dY planes of the producer's dgrad GEMM
    dst = alloc.buf("bwd/wino_sum", gx.shape) if had else gx
    ops.conv3x3_winograd(gy, u, None, ACT_NONE, out=dst, v_buf=alloc.buf("bwd/wino_v", (G, T, Cout)),
                         m_buf=alloc.buf("bwd/wino_m", (G, T, Cin)), mask=mk if fused else None, out_planes=planes)
    if had:
        ops.add_strided(dst, gx, 1, True)
    return fused, planes, "f32", 2 * G * T * Cin * Cout


def dgrad_flipped(ops, alloc, prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit=False, m=None, gy_planes=None):
    N, OH, OW, Cout = gy.shape
    wd = _flipped_filter(ops, alloc, prepared, sc, wf, k, Cout)
    dpad = (k - 1 - pad[0], k - 1 - pad[1], k - 1 - pad[2], k - 1 - pad[3])
    ops.conv2d(gy, wd, None, k, k, 1, dpad, ACT_NONE, gres, 1, out=gx, mask=mk)
    return mk is not None, None, "f32", 2 * N * OH * OW * wf.shape[3] * Cout * k * k      # mask * (dX + what was there): the whole buffer


def dgrad_h2(ops, alloc, prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit=False, m=None, gy_planes=None):
    # dX = dY W: a plain GEMM with K = Cout -- frcnn_gemm_h2 on the split of dY and of the transposed filter
    # (cfg.HIP.H2_TRAIN; both change every step, so both are split here: 8 B per element of dY, a few MB of filter)
    N, OH, OW, Cout = gy.shape
    M, Cin = N * OH * OW, wf.shape[3]
    wd = _flipped_filter(ops, alloc, prepared, sc, wf, k, Cout)
    gp = gy_planes
    if gp is None:
        gp = ops.h2_split(gy.view(M, Cout), out=alloc.h2_buf("bwd/gy", M, Cout))
    wq = prepared(("wflip_h2", sc), lambda: ops.h2_pack_w(wd.view(Cin, Cout), out=alloc.buf_pair("bwd/wflip_h2/" + sc, Cin, Cout)))
    planes = None
    if mk is not None and emit:                                  # the producer's own data gradient reads this result as planes
        planes = alloc.h2_buf("bwd/gyp/" + sc, M, Cin)
    ops.gemm_h2(gp, wq, 1, M, Cin, Cout, None, None if gres is None else gres.view(M, Cin), ACT_NONE, out=gx.view(M, Cin),
                mask=None if mk is None else mk.view(M, Cin), out_planes=planes)
    return mk is not None, planes, "h2", 2 * M * Cin * Cout


def dgrad_padded(ops, alloc, prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit=False, m=None, gy_planes=None):
    # 1x1 heads whose output width is no multiple of 32 (cls_score 81, bbox_pred 324, the RPN's 2A / 4A): dX = dY W on the
    # matrix pipe with dY and the transposed filter zero-padded to the next multiple (the gather kernel: 60-120 us each)
    N, OH, OW, Cout = gy.shape
    Cin, Cp = wf.shape[3], (Cout + 31) // 32 * 32
    wdp = prepared(("wflip_pad", sc), lambda: ops.transpose_pad(wf.view(Cout, Cin), Cp, out=alloc.buf("bwd/wflip_pad/" + sc, (Cin, Cp))))
    gyp = alloc.buf("bwd/gypad/" + sc, (N, OH, OW, Cp), zero=True)      # columns >= Cout stay zero
    ops.t_copy(gyp[..., :Cout], gy)
    ops.conv2d(gyp, wdp.view(Cin, 1, 1, Cp), None, 1, 1, 1, ZERO_PAD, ACT_NONE, gres, 1, out=gx, mask=mk)
    return mk is not None, None, "f32", 2 * N * OH * OW * Cin * Cp


def dgrad_upsampled(ops, alloc, prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit=False, m=None, gy_planes=None):
    # A strided 3x3 (the last unit of a block, resnet_v1.py:80-113): dX = the stride-1 convolution of dY spread out on the
    # input grid (zeros between its pixels) with the flipped / transposed filter -- the matrix pipe on a 75 % empty operand
    # (~45 us) instead of the gather kernel's scalar FMAs (246 us, profiles/r04_ac_train_kernels_by_shape.txt).  The
    # buffer is zeroed once: only the pixels (oh * stride, ow * stride) are ever written.
    N, OH, OW, Cout = gy.shape
    up_h, up_w, up_pad = upsampled_geometry(k, stride, pad, gx.shape[1], gx.shape[2], OH, OW)
    wd = _flipped_filter(ops, alloc, prepared, sc, wf, k, Cout)
    up = alloc.buf("bwd/up/" + sc, (N, up_h, up_w, Cout), zero=True)
    ops.add_strided(gy, up, stride, False)
    ops.conv2d(up, wd, None, k, k, 1, up_pad, ACT_NONE, gres, 1, out=gx, mask=mk)
    return mk is not None, None, "f32", 2 * gx.shape[0] * gx.shape[1] * gx.shape[2] * wf.shape[3] * Cout * k * k


def dgrad_gather(ops, alloc, prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit=False, m=None, gy_planes=None):
    N, OH, OW, Cout = gy.shape
    ops.conv2d_dgrad_strided(gy, wf, stride, pad, gx.shape[1], gx.shape[2], gx, gres is not None)
    return False, None, "f32", 2 * N * OH * OW * Cout * k * k * wf.shape[3]


DGRAD = {"winograd": dgrad_winograd, "flipped": dgrad_flipped, "h2": dgrad_h2, "padded": dgrad_padded, "upsampled": dgrad_upsampled,
         "gather": dgrad_gather}


# ---- the filter gradient ---------------------------------------------------------------------------------------------------------------
def wgrad_tn(ops, gy, x, k, stride, pad, p, h2):
    """dW = dY^T X straight from the two tensors as they lie (csrc/wgrad_tn.hip): no transposed copies, no im2col"""
    ops.conv2d_wgrad(gy, x, k, k, stride, pad, p.grad_w, h2=h2)
    return "h2" if h2 else "f32", 2 * gy.numel() * p.K


def wgrad_fallback(ops, alloc, sfx, gy, x, k, stride, pad, p):
    """transposed, zero-padded copies of dY and of X (k > 1 or strided: its im2col) and the forward MFMA kernel on the pair; sfx: the
    side stream's own scratch"""
    N, OH, OW, Cout = gy.shape
    M, Cin = N * OH * OW, x.shape[-1]
    Mp = (M + 31) // 32 * 32
    gyT = ops.transpose_pad(gy.view(M, Cout), Mp, out=alloc.buf("bwd/gyT" + sfx, (Cout, Mp)))
    if k == 1 and stride == 1:
        xT = ops.transpose_pad(x.view(M, Cin), Mp, out=alloc.buf("bwd/xT" + sfx, (Cin, Mp)))
    else:
        xT = ops.im2col_t(x, k, k, stride, pad, OH, OW, Mp, out=alloc.buf("bwd/xT" + sfx, (k * k * Cin, Mp)))
    # dW_folded[n][(kh,kw,c)] = sum_m gyT[n][m] * xT[(kh,kw,c)][m]   -- the forward MFMA kernel
    ops.conv2d(gyT.view(1, 1, Cout, Mp), xT.view(xT.shape[0], 1, 1, Mp), None, 1, 1, out=p.grad_w.view(1, 1, Cout, p.K))
    return "f32", 2 * M * Cout * p.K


def filter_gradient(ops, alloc, sfx, gy, x, k, stride, pad, p, tn, h2):
    """dW (and the bias gradient) of one convolution record into p.grad_w / p.grad_b; tn / h2: TrainState.wgrad_tn / wgrad_h2.
    Returns (pipe, flops)."""
    Cout = gy.shape[3]
    if tn and ops.conv2d_wgrad_supported(x.shape[-1], Cout) and p.K == k * k * x.shape[-1]:
        counted = wgrad_tn(ops, gy, x, k, stride, pad, p, bool(h2))
    else:
        counted = wgrad_fallback(ops, alloc, sfx, gy, x, k, stride, pad, p)
    if p.bias is not None:
        ops.colsum(gy.view(-1, Cout), p.grad_b)
    return counted


# ---- the walk --------------------------------------------------------------------------------------------------------------------------
class Sweep(object):
    """One reverse sweep of a TrainState `ts` on the stream `main`: run(seeds) fills every Param.grad_* and returns
    {tensor address: gradient buffer}."""

    def __init__(self, ts, main, fuse_solver, caps, ops):
        """caps: train.exchange_caps of ts.all_reduce; ops: the entries every launch of the sweep goes through (train.py's frcnn_hip.ops)"""
        self.ts, self.sess, self.net, self.main, self.ops = ts, ts.sess, ts.net, main, ops
        self.grads, self.needs = None, ts.net._requires_grad
        self.ar = ts.all_reduce
        self.open_side_streams(*caps)
        self.open_solver(fuse_solver)
        self.pending = 0                                         # filter gradients enqueued since the last solver launch
        self.gs = 1.0 / float(ts.world_size) if ts.data_parallel() else 1.0     # the mean over replicas, folded into the update
        self.sess.prepared.enabled = bool(ts.prep_stream)
        self.prepared = self.sess.prepared.get
        # Elementwise passes of the chain rule folded into the launches on either side of them (cfg-free; `fuse_chain = False` keeps the
        # separate passes, for the bit-equality test):
        #  * ReLU gradient: the input x of a trunk convolution is a ReLU output, so the data gradient a record produces is masked by
        #    (x > 0) in the producing launch's epilogue (ops.*(mask=x)); `masked` = tensors whose gradient buffer holds ONLY masked
        #    contributions -- their producer record skips its relu_bwd pass (the select is idempotent and distributes over the sum, so a
        #    buffer that also received an unmasked contribution is simply masked again by the pass);
        #  * identity shortcut: the residual's gradient IS the masked dY of the unit's last convolution -- `borrowed` maps it to that
        #    buffer instead of copying it; the convolution that later adds its own data gradient reads it as the launch's residual and
        #    writes a fresh buffer (the borrowed one is still being read by the filter gradient on a side stream);
        #  * operand planes of dY for a following frcnn_gemm_h2 data gradient come out of the Winograd output transform (`emitted`).
        self.fuse, self.pipe = bool(ts.fuse_chain), bool(ts.pipe_dgrads)
        self.producer = {}
        if self.fuse:
            for r in self.net._tape:
                if r["kind"] not in ("mean", "crop", "roi_align", "maxpool", "dropout", "dwconv"):
                    self.producer[r["y"].data_ptr()] = r
        self.masked, self.borrowed, self.emitted = set(), set(), {}

    def open_side_streams(self, overlapped, multi_stream):
        # Filter gradients on side streams (cfg.HIP.WGRAD_STREAM = how many): a wgrad only feeds the solver, while the data-gradient
        # chain is what the next record waits for -- at one image per step neither fills 256 CUs, so they run side by side.  Each side
        # stream executes its wgrads in tape order with its OWN transposed-operand scratch and split-K workspace, sees dY through an
        # event recorded after the activation gradient, and is joined before backward() returns.  Data parallel: one side stream, so
        # that "everything behind this offset of the flat gradient is final" holds on the stream the collective is issued from.
        ts = self.ts
        nside = int(ts.wgrad_stream)
        self.dp = ts.data_parallel() and overlapped              # the bucketed, overlapped exchange (parallel.BucketedAllReduce)
        self.any_side = not ts.data_parallel() or (self.dp and multi_stream)    # may filter gradients (and the in-sweep solver) use every side stream?
        if not self.any_side:
            nside = min(nside, 1)                                # a plain all-reduce callable orders itself after ONE stream
        while len(ts._wgrad_stream_objs) < nside:
            ts._wgrad_stream_objs.append(torch.cuda.Stream(device=self.sess.device))
        self.sides = ts._wgrad_stream_objs[:nside]
        self.turn = 0
        if ts._wgrad_events is None:
            ts._wgrad_events = [torch.cuda.Event() for _ in range(16)]
        self.pins = [self.ops.pinned_stream(st) for st in self.sides]
        self.events = ts._wgrad_events

    def open_solver(self, fuse_solver):
        # The solver inside the sweep (single-GPU runs with side streams; from the second step on, when apply() has built its descriptor
        # table): the reverse sweep finishes the parameters from the END of the flat gradient backwards, so every SOLVER_CHUNK filter
        # gradients the solver stream updates that range -- frcnn_sgd_momentum_range -- behind (a) the side streams' filter gradients
        # enqueued so far and (b) the main stream's data gradients enqueued so far (the last readers of those filters in this step).
        # ~0.5 ms of memory-bound update leaves the tail of the step; apply() updates what is left (the first layers).  The L2
        # regulariser value reads the filters BEFORE any update: it opens the solver stream's step.
        ts = self.ts
        ts._sgd_done_from = None
        self.solver = None
        if (fuse_solver and self.sides and self.any_side and ts._sgd_table is not None and ts.lr is not None
                and ts.solver_in_sweep and not any(p.dw for p in ts.params.values())):
            if ts._solver_stream is None:
                ts._solver_stream = torch.cuda.Stream(device=self.sess.device)
            self.solver = ts._solver_stream
            self.ops.st_wait_stream(self.solver, self.main)           # (the previous step's apply() -- nothing else of this step matters to it)
            with self.ops.pinned_stream(self.solver):
                ts.regularization_loss(ts._reg_total())
            ts._reg_in_sweep = True
            ts._sgd_done_from = ts._sgd_count

    def run(self, seeds):
        self.grads = {t.data_ptr(): g for t, g in seeds}
        visit = {"mean": self.visit_mean, "crop": self.visit_crop, "roi_align": self.visit_roi_align, "maxpool": self.visit_maxpool, "dropout": self.visit_dropout,
                 "dwconv": self.visit_dwconv, "conv": self.visit_conv}
        for rec in reversed(self.net._tape):
            visit[rec["kind"]](rec)
        for side in self.sides:
            self.ops.st_wait_stream(self.main, side)  # the solver (and the next forward pass, which overwrites x) come after every wgrad
        if self.solver is not None:
            self.ops.st_wait_stream(self.main, self.solver)
        return self.grads

    # ---- the solver inside the sweep
    def solver_step(self, first):
        """update table[first, done_from) on the solver stream"""
        ts, solver = self.ts, self.solver
        while len(ts._solver_events) < 1 + len(self.sides):      # one per stream it waits for (cfg.HIP.WGRAD_STREAM is not bounded)
            ts._solver_events.append(torch.cuda.Event())
        for i, st in enumerate([self.main] + list(self.sides)):
            ev = ts._solver_events[i]
            self.ops.ev_record(ev, st)
            self.ops.st_wait_event(solver, ev)
        if self.dp:
            self.ar.wait_sent(solver)                            # ... and behind the all-reduces that sum these gradients over the replicas
        with self.ops.pinned_stream(solver):
            self.ops.sgd_momentum_range(ts._sgd_table, first, ts._sgd_done_from - first, ts.lr, ts.momentum, self.gs)
        ts._sgd_done_from = first
        self.pending = 0

    def dp_solver_step(self):
        """data parallel: every parameter whose gradient lies inside the range already handed to the all-reduce ([sent_from, end) of
        the flat buffer; the descriptor table is in the buffer's order) can be updated behind that collective"""
        if self.ar.sent_from is None:
            return
        first = bisect.bisect_left(self.ts._sgd_offsets, int(self.ar.sent_from))
        if first < self.ts._sgd_done_from:
            self.solver_step(first)

    def solver_tick(self, sc):
        """SOLVER_CHUNK trainable records' data gradients are enqueued: their filters have no reader left in this step"""
        ts = self.ts
        if self.dp:
            self.dp_solver_step()                                # (what the exchange has taken so far; pending counts on if nothing new was sent)
        else:
            first = ts._sgd_entry.get(sc)
            if first is not None and first < ts._sgd_done_from:
                self.solver_step(first)

    # ---- side streams and gradient buffers
    def on_side(self, p, fn):
        """p's filter gradient, fn(scratch suffix), on the next side stream in turn, behind what the main stream has enqueued so far"""
        sides = self.sides
        if not sides:
            fn("")
            if self.dp:
                self.filter_ready(p, None)
            return
        i = self.turn % len(sides)
        ev = self.events[self.turn % len(self.events)]           # a small ring: a wait captures the record that precedes it
        self.turn += 1
        side = sides[i]
        self.ops.ev_record(ev, self.main)
        self.ops.st_wait_event(side, ev)
        scope, self.ops.ws_scope = self.ops.ws_scope, self.ops.ws_scope + "/wgrad%d" % i
        try:
            with self.pins[i]:                                   # this module's launches go to `side` without a torch stream switch; a
                fn("/s%d" % i if i else "")                      # bucket that becomes ready is sent with `side` current (parallel.py)
                if self.dp:
                    self.filter_ready(p, side)
        finally:
            self.ops.ws_scope = scope

    def filter_ready(self, p, side):
        # data parallel: this parameter's gradient is enqueued, so everything from its offset to the end of the flat buffer is final
        # (the tape is walked backwards, the buffer is laid out in forward order; the collective orders itself after
        # every side stream a filter gradient may have been enqueued on)
        self.ar.ready(self.ts.flat, p.grad_w.data_ptr(), side, self.sides)

    def relu_mask(self, t):
        r = self.producer.get(t.data_ptr())
        return r["y"] if (r is not None and r["act"] == ACT_RELU) else None

    def runs_h2(self, r):
        """does the convolution record's own data gradient run as frcnn_gemm_h2?  (the rule dgrad_route reads)"""
        y, wf = r["y"], self.sess.conv_info[r["scope"]]["w"]
        return h2_form(r["k"], r["stride"], r["pad"], wf.shape[3], y.shape[-1], y.numel() // y.shape[-1], self.ts.h2_train)

    def accumulate_into(self, target, shape, name):
        grads, key = self.grads, target.data_ptr()
        if key in grads:
            self.emitted.pop(key, None)                      # (planes emitted with the first contribution would be stale)
            if key in self.borrowed:                         # an in-place accumulation is about to write it: take a private copy
                g = self.sess.buf("grad/" + name + "/own", shape)
                self.ops.t_copy(g, grads[key].view(shape))
                grads[key] = g
                self.borrowed.discard(key)
            self.masked.discard(key)                         # (callers that mask the whole sum add it again)
            return grads[key], True
        g = self.sess.buf("grad/" + name, shape)
        grads[key] = g
        self.masked.discard(key)
        return g, False

    def fresh_input_grad(self, rec, check_needs=True):
        """mean / maxpool / dropout: (dY, the fresh gradient buffer of the record's input), or None when nothing flows through it"""
        gy, x = self.grads.get(rec["y"].data_ptr()), rec["x"]
        if gy is None or (check_needs and x.data_ptr() not in self.needs):
            return None
        gx, had = self.accumulate_into(x, x.shape, rec["name"] + "/in")
        assert not had
        return gy, gx

    # ---- one visit per record kind
    def visit_mean(self, rec):
        g = self.fresh_input_grad(rec, check_needs=False)
        if g is not None:
            x = rec["x"]
            self.ops.spatial_mean_bwd(g[0].view(rec["y"].shape), x.shape[1] * x.shape[2], g[1])

    def visit_maxpool(self, rec):
        g = self.fresh_input_grad(rec)
        if g is not None:
            self.ops.maxpool_bwd(rec["x"], rec["y"], g[0].view(rec["y"].shape), rec["k"], rec["stride"], g[1])

    def visit_dropout(self, rec):
        g = self.fresh_input_grad(rec)
        if g is not None:
            self.ops.dropout(g[0].view(rec["x"].shape), rec["seed"], rec["keep"], out=g[1], step_mult=256)      # same mask, same 1 / keep_prob

    def visit_crop(self, rec):
        gy, feat = self.grads.get(rec["y"].data_ptr()), rec["feat"]
        if gy is None or feat.data_ptr() not in self.needs:
            return
        gx, had = self.accumulate_into(feat, feat.shape, "feat")
        if not had:
            self.ops.t_zero(gx)
        self.ops.crop_and_resize_bwd(gy.view(rec["y"].shape), rec["rois"], rec["stride"], gx)

    def visit_roi_align(self, rec):
        gy, feat = self.grads.get(rec["y"].data_ptr()), rec["feat"]
        if gy is None or feat.data_ptr() not in self.needs:
            return
        gx, had = self.accumulate_into(feat, feat.shape, "feat")
        if not had:
            self.ops.t_zero(gx)
        self.ops.roi_align_bwd(gy.view(rec["y"].shape), rec["rois"], rec["stride"], rec["samples"], gx)

    def visit_dwconv(self, rec):
        y, x, sc = rec["y"], rec["x"], rec["scope"]
        gy = self.grads.get(y.data_ptr())
        if gy is None:
            return
        gy = gy.view(y.shape)
        (self.ops.relu6_bwd if rec["act"] == ACT_RELU6 else self.ops.relu_bwd)(gy, y)
        p = self.ts.params.get(sc)
        if p is not None:
            self.on_side(p, lambda sfx: self.ops.dwconv3x3_wgrad(gy, x, rec["stride"], rec["pad"], p.scale, p.grad_w))
        if x.data_ptr() in self.needs:
            gx, had = self.accumulate_into(x, x.shape, sc + "/in")
            self.ops.dwconv3x3_dgrad(gy, self.sess.packed[("dw", sc)][0], rec["stride"], rec["pad"], gx, accumulate=had)

    def activation_gradient(self, rec):
        """dY of a convolution record with its activation's gradient applied (in place, on a private copy of a borrowed buffer), or None"""
        y, key = rec["y"], rec["y"].data_ptr()
        gy = self.grads.get(key)
        if gy is None:
            return None
        gy = gy.view(y.shape)
        if rec["act"] != ACT_NONE and key in self.borrowed:      # the activation gradient is applied in place
            gy = self.sess.buf("grad/" + rec["scope"] + "/own", y.shape)
            self.ops.t_copy(gy, self.grads[key].view(y.shape))
            self.grads[key] = gy
            self.borrowed.discard(key)
        if rec["act"] == ACT_RELU:
            if key not in self.masked:
                self.ops.relu_bwd(gy, y)
        elif rec["act"] == ACT_RELU6:
            self.ops.relu6_bwd(gy, y)
        return gy

    def residual_gradient(self, rec, gy):
        res = rec["residual"]
        if res.data_ptr() not in self.needs:
            return
        if self.fuse and rec["res_stride"] == 1 and res.data_ptr() not in self.grads:
            self.grads[res.data_ptr()] = gy                      # identity shortcut: no copy (see `borrowed` in __init__)
            self.borrowed.add(res.data_ptr())
            self.masked.discard(res.data_ptr())
            return
        gr, had = self.accumulate_into(res, res.shape, rec["scope"] + "/res")
        if rec["res_stride"] == 1 and not had:
            self.ops.t_copy(gr, gy)
        else:
            if not had:
                self.ops.t_zero(gr)
            self.ops.add_strided(gy, gr, rec["res_stride"], True)

    def target_buffer(self, x, sc, route):
        """(gx, gres): where the record's data gradient goes and what the launch adds to it (None: a fresh buffer)"""
        key = x.data_ptr()
        if key in self.borrowed and route in OUT_OF_PLACE:
            # an identity shortcut's gradient waits there, in somebody else's buffer -- out of place: residual = the borrowed buffer
            # (read only), result = this record's own buffer
            gres = self.grads[key]
            self.emitted.pop(key, None)
            gx = self.grads[key] = self.sess.buf("grad/" + sc + "/in", x.shape)
            self.borrowed.discard(key)
            self.masked.discard(key)
            return gx, gres
        gx, had = self.accumulate_into(x, x.shape, sc + "/in")   # (takes the private copy of a borrowed buffer)
        return gx, (gx if had else None)

    def visit_conv(self, rec):
        gy = self.activation_gradient(rec)
        if gy is None:
            return
        ts, y, x, sc = self.ts, rec["y"], rec["x"], rec["scope"]
        if rec["residual"] is not None:
            self.residual_gradient(rec, gy)
        k, stride, pad = rec["k"], rec["stride"], rec["pad"]
        p = ts.params.get(sc)
        if p is not None:
            self.on_side(p, lambda sfx: ts.count_flops(*filter_gradient(self.ops, self.sess, sfx, gy, x, k, stride, pad, p, ts.wgrad_tn, ts.wgrad_h2)))
        key = x.data_ptr()
        if key in self.needs:
            (N, OH, OW, Cout), (_, H, W, _) = y.shape, x.shape
            wf = self.sess.conv_info[sc]["w"]
            route, m = dgrad_route(k, stride, pad, wf.shape[3], Cout, H, W, N, OH, OW, y.dim(), key in self.grads, self.pipe, ts.winograd, ts.h2_train)
            mk = self.relu_mask(x) if self.fuse else None        # x itself when it is a ReLU output: the gradient's mask
            gx, gres = self.target_buffer(x, sc, route)
            emit = mk is not None and route in ("winograd", "h2") and self.runs_h2(self.producer[key])
            whole, planes, pipe_name, flops = DGRAD[route](self.ops, self.sess, self.prepared, sc, gy, wf, k, stride, pad, gx, gres, mk, emit, m,
                                                           self.emitted.pop(y.data_ptr(), None) if route == "h2" else None)
            if whole:
                self.masked.add(key)
            if planes is not None:
                self.emitted[key] = planes
            ts.count_flops(pipe_name, flops)
        self.emitted.pop(y.data_ptr(), None)
        if self.solver is not None and p is not None:
            self.pending += 1
            if self.pending >= ts.SOLVER_CHUNK:
                self.solver_tick(sc)
