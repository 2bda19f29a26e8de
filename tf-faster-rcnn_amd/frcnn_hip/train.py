"""Training step on the device chain (lib/model/train_val.py:116-153,
lib/nets/network.py:488-516): reverse sweep over the tape the Network records in TRAIN mode, parameter
gradients, momentum SGD with slim-style L2 regularisation, optional data-parallel gradient all-reduce.

Convolution gradients run on the SAME f32-MFMA implicit-GEMM kernel as the forward pass, on re-laid-out
operands (csrc/backward_kernels.hip).  BN is frozen in the reference (resnet_v1.py:22-44), so the
forward pass uses BN-folded filters; the master copy of every filter is kept un-folded on the device in
the packed layout [Cout][KH][KW][Cin], its gradient is dW_folded * scale[n] (chain rule through the
fold) and the folded copy is refreshed inside the SGD kernel.
"""
import numpy as np
import torch

from . import ops
from .sweep import Sweep


class Param(object):
    """One trainable filter (+ optional bias) on the device."""
    dw = False

    def __init__(self, scope, wf, bias, scale_np, bias_trainable, flat_w, flat_b, master_hwio=None):
        dev = wf.device
        self.scope = scope
        self.wf = wf                                            # folded filter used by the forward kernels
        self.K = wf[0].numel()
        self.scale = None if scale_np is None else torch.from_numpy(np.ascontiguousarray(scale_np, dtype=np.float32)).to(dev)
        if self.scale is None:
            self.w = wf                                         # no fold: master == forward filter
        elif master_hwio is not None and master_hwio.size == wf.numel():
            # the un-folded variable itself (exactly what a snapshot stores), and the folded copy recomputed from it with the
            # SGD kernel's own f32 product, so a resumed run starts from the very state the interrupted one had
            m = np.ascontiguousarray(master_hwio.reshape((wf.shape[1], wf.shape[2], wf.shape[3], wf.shape[0])).transpose(3, 0, 1, 2))
            self.w = torch.from_numpy(m.astype(np.float32)).to(dev)
            wf.copy_(self.w * self.scale.view(-1, 1, 1, 1))
        else:
            self.w = (wf / self.scale.view(-1, 1, 1, 1)).contiguous()
        self.acc_w = torch.zeros_like(self.w)
        self.grad_w = flat_w.view(wf.shape)                     # view into the flat gradient buffer (one all-reduce)
        self.bias = bias if bias_trainable else None
        self.acc_b = torch.zeros_like(bias) if bias_trainable else None
        self.grad_b = flat_b


class DwParam(object):
    """One trainable depthwise 3x3 filter (MobileNet): master copy [3,3,C] as in the variable `depthwise_weights` [3,3,C,1], the
    forward filter is master * scale[c] (frozen-BN fold, refreshed after every solver step); no bias (the BN shift is frozen)."""
    dw = True

    def __init__(self, scope, wf, scale_np, flat_w, master_np):
        dev = wf.device
        self.scope = scope
        self.wf = wf
        self.scale = torch.from_numpy(np.ascontiguousarray(scale_np, dtype=np.float32)).to(dev)
        self.w = torch.from_numpy(np.ascontiguousarray(master_np, dtype=np.float32)).to(dev)
        ops.dwconv3x3_refold(self.w, self.scale, self.wf)
        self.K = self.w.numel()
        self.acc_w = torch.zeros_like(self.w)
        self.grad_w = flat_w.view(self.w.shape)
        self.bias = self.acc_b = self.grad_b = None


def exchange_caps(ar):
    """(overlapped, multi_stream) of a gradient exchange, which is a foreign object: None, a plain callable f(flat) (parallel.py), a
    parallel.BucketedAllReduce or a test's stand-in.  overlapped: it has the bucketed interface (ready / wait_sent / finish) that the
    reverse sweep feeds range by range; multi_stream: its ready() orders a collective after EVERY stream it is given."""
    overlapped = ar is not None and hasattr(ar, "ready")
    return overlapped, overlapped and bool(getattr(ar, "multi_stream", False))


class TrainState(object):
    """Owns the parameters, their momentum buffers and ONE flat gradient buffer (so data-parallel
    training is a single RCCL all-reduce, or a few bucketed ones, over contiguous memory)."""

    def __init__(self, sess, net, momentum=0.9, weight_decay=1e-4, double_bias=False, bias_decay=False):
        self.sess, self.net = sess, net
        self.momentum, self.weight_decay = momentum, weight_decay
        self.double_bias, self.bias_decay = double_bias, bias_decay
        self.params, self.flat, self.reg_scopes = {}, None, []
        # ---- switches: what decides WHICH launches a step makes (SWITCHES names exactly this group; replay_signature carries it)
        self.fuse_chain = True                                  # see sweep.Sweep.__init__ (False: separate relu_bwd / copy / h2_split passes; tests)
        self.pipe_dgrads = True                                 # see sweep.dgrad_route (False: frcnn_conv2d_dgrad_strided for every strided / odd-width layer; tests)
        self.prep_stream = True                                 # sess.prepared: weight-only launches re-run by the solver on a side stream
        self.solver_in_sweep = True                             # see sweep.Sweep.open_solver (False: the whole update in apply(); tests)
        self.winograd, self.h2_train = None, None               # data gradients: Winograd (m, min channels, 7x7) / frcnn_gemm_h2 from so many tiles; None = off
        self.wgrad_tn, self.wgrad_h2, self.wgrad_stream = True, False, 0      # filter gradients: csrc/wgrad_tn.hip, its fp16 pipe, how many side streams
        self.world_size, self.force_dp, self.all_reduce = 1, False, None      # see data_parallel; the gradient exchange (see exchange_caps)
        # ---- per-run inputs: the step's learning rate, bench.py's ledger (count_flops), a resumed run's momentum slots (imported after build())
        self.lr, self.flop_ledger, self.pending_slots = None, None, None
        # ---- private state: apply()'s descriptor table, the regulariser's tables, streams and events (all made at their first use)
        self._sgd_table, self._sgd_count, self._sgd_done_from, self._sgd_offsets, self._sgd_entry = None, 0, None, None, {}
        self._reg_in_sweep, self._reg_buf, self._reg_tables, self._reg_keep = False, None, None, None
        self._solver_stream, self._solver_events, self._wgrad_stream_objs, self._wgrad_events = None, [], [], None

    SWITCHES = ("fuse_chain", "pipe_dgrads", "prep_stream", "solver_in_sweep", "winograd", "h2_train", "wgrad_tn", "wgrad_h2", "wgrad_stream",
                "world_size", "force_dp", "all_reduce")

    def build(self):
        """Call after one TRAIN forward (which packs every filter and fills net._tape)."""
        sess, net = self.sess, self.net
        scopes = []                                             # (kind, scope) in forward order: the flat buffer follows the tape
        for rec in net._tape:
            if rec["kind"] in ("conv", "dwconv") and net.trainable_scope(rec["scope"]):
                if (rec["kind"], rec["scope"]) in scopes:
                    # one tape record per trainable filter: the reverse sweep OVERWRITES grad_w per record, and the overlapped
                    # all-reduce (parallel.BucketedAllReduce) ships a gradient range as soon as its record has been visited
                    raise NotImplementedError("trainable scope %s is used by two layers of the TRAIN graph (shared filters)" % rec["scope"])
                scopes.append((rec["kind"], rec["scope"]))
        total = 0
        sizes = []
        for kind, sc in scopes:
            if kind == "dwconv":
                sizes.append((sess.packed[("dw", sc)][0].numel(), 0))
            else:
                info = sess.conv_info[sc]
                sizes.append((info["w"].numel(), info["b"].numel() if (info["b"] is not None and not info["bn"]) else 0))
            total += sum(sizes[-1])
        self.flat = torch.zeros((total,), dtype=torch.float32, device=sess.device)
        off = 0
        for (kind, sc), (nw, nb) in zip(scopes, sizes):
            fw = self.flat[off:off + nw]
            off += nw
            fb = self.flat[off:off + nb] if nb else None
            off += nb
            if kind == "dwconv":
                scale, _ = sess.fold_bn(sc, net.dw_bn_eps)
                self.params[sc] = DwParam(sc, sess.packed[("dw", sc)][0], scale, fw, sess.variables[sc + "/depthwise_weights"][:, :, :, 0])
            else:
                info = sess.conv_info[sc]
                self.params[sc] = Param(sc, info["w"], info["b"], info["scale"], nb > 0, fw, fb, sess.variables.get(sc + "/weights"))
        self.reg_scopes = [sc for sc in sess.conv_info]            # slim regularises every conv/fc weight, frozen or not
        return self

    # ---- gradients -----------------------------------------------------------------------------------
    def data_parallel(self):
        """True when the step runs under the data-parallel rules: more than one replica, or `force_dp` (bench.py --dp-constrained: one
        replica with everything a multi-GPU step does -- at most one filter-gradient side stream, the bucketed all-reduce issued from inside
        the sweep over a one-rank RCCL group, no captured sweep -- so that the step an 8-GPU run executes per GPU can be timed at N = 1)."""
        return int(self.world_size) > 1 or bool(self.force_dp)

    def count_flops(self, pipe, flops):
        """Ledger of the reverse sweep's matrix work per matrix pipe ("h2": frcnn_gemm_h2 / frcnn_conv2d_wgrad_h2, "f32": the f32-MFMA
        kernels); bench.py prices a training step per pipe with it (host arithmetic on launch shapes, nothing on the device)."""
        if self.flop_ledger is not None:
            self.flop_ledger[pipe] = self.flop_ledger.get(pipe, 0) + int(flops)

    def backward(self, seeds, fuse_solver=False):
        """seeds: list of (tensor, grad) for network outputs.  Fills every Param.grad_*.

        fuse_solver = True (what Network.train_step_async passes, and nobody else should): the sweep ALSO runs the solver for the tail of
        the parameter table on its own stream as the filter gradients finish (frcnn_sgd_momentum_range with TrainState.lr) -- weights and
        momentum of those parameters are updated when this returns, and the caller MUST complete the step with apply(self.lr, ...), which
        updates the rest.  With the default, backward() only computes gradients: calling it twice, inspecting gradients, accumulating
        them or skipping a step leaves the parameters alone."""
        if self._sgd_done_from is not None:
            raise RuntimeError("TrainState.backward: the previous sweep updated part of the parameters inside the sweep (fuse_solver=True) "
                               "and apply() never completed that step")
        main = torch.cuda.current_stream()
        with ops.pinned_stream(main):                 # ~1000 launches: one stream lookup instead of one per launch
            return self._sweep(seeds, main, bool(fuse_solver))

    def replay_signature(self):
        """Everything about this solver handle that decides WHICH launches a step makes (a recorded step is valid for one signature):
        the solver's constants and one value per name in SWITCHES (the exchange by identity)."""
        def value(name, v):
            if name == "all_reduce":
                return None if v is None else id(v)
            return tuple(v) if isinstance(v, (list, tuple)) else v
        return ((float(self.momentum), float(self.weight_decay), bool(self.double_bias), bool(self.bias_decay))
                + tuple(value(n, vars(self)[n]) for n in self.SWITCHES))

    def _sweep(self, seeds, main, fuse_solver=False):
        """One reverse sweep on `main` (sweep.Sweep: its per-call state lives there, never on this handle); returns {address: gradient}."""
        return Sweep(self, main, fuse_solver, exchange_caps(self.all_reduce), ops).run(seeds)

    SOLVER_CHUNK = 32

    def _reg_total(self):
        if self._reg_buf is None:
            self._reg_buf = torch.zeros((1,), dtype=torch.float32, device=self.sess.device)
        return self._reg_buf

    def regularization_value(self):
        """Device tensor [1]: the slim L2 term of this step's weights (network.py:315-317) -- computed by the sweep on the solver stream
        when that is active (before its first update), else here."""
        if not self._reg_in_sweep:
            self.regularization_loss(self._reg_total())
        self._reg_in_sweep = False
        return self._reg_total()

    # ---- solver --------------------------------------------------------------------------------------
    def apply(self, lr, world_size=1, all_reduce=None):
        """acc = m*acc + g ; w -= lr*acc (train_val.py:128-145) for every parameter in ONE launch.  Data parallel: the flat
        gradient is summed over the ranks (RCCL) -- bucket by bucket during the reverse sweep when `all_reduce` has the
        bucketed interface (parallel.BucketedAllReduce: backward() hands it every finished range), otherwise in one call
        here -- and the mean over replicas is folded into the SGD kernel (grad_scale = 1 / world_size)."""
        if all_reduce is not None and (world_size > 1 or self.data_parallel()):
            if exchange_caps(all_reduce)[0]:
                all_reduce.finish(self.flat)              # ranges not yet handed over + wait for the ones in flight
            else:
                all_reduce(self.flat)
        gs = 1.0 / float(world_size)
        self.sess.prepared.join()                    # (a step that used none of the side stream's buffers has not waited for it yet)
        if self._sgd_table is None:
            entries, self._sgd_entry = [], {}          # scope -> index of its first descriptor (filter, then bias)
            for p in self.params.values():
                self._sgd_entry[p.scope] = len(entries)
                if p.dw:          # gradient already carries the BN-fold scale; no L2 term (MOBILENET.REGU_DEPTH False)
                    entries.append((p.w, p.acc_w, None, p.grad_w, None, p.K, 1.0, 0.0))
                    continue
                wd = self._wd(p.scope)
                entries.append((p.w, p.acc_w, p.wf if p.scale is not None else None, p.grad_w, p.scale, p.K, 1.0, wd))
                if p.bias is not None:
                    entries.append((p.bias, p.acc_b, None, p.grad_b, None, p.bias.numel(), 2.0 if self.double_bias else 1.0,
                                    wd if self.bias_decay else 0.0))
            self._sgd_count = len(entries)
            self._sgd_table = ops.sgd_desc_table(entries, self.sess.device)
            # gradient offset of every descriptor inside the flat buffer (ascending: the table is in forward order like the buffer)
            self._sgd_offsets = None if self.flat is None else [(e[3].data_ptr() - self.flat.data_ptr()) // 4 for e in entries]
            assert self._sgd_offsets is None or self._sgd_offsets == sorted(self._sgd_offsets)
        left = self._sgd_count if self._sgd_done_from is None else self._sgd_done_from      # (the sweep updated the rest)
        if left != self._sgd_count and float(lr) != float(self.lr):
            raise RuntimeError("TrainState.apply(lr=%r): the reverse sweep already updated part of the parameters with TrainState.lr = %r"
                               % (lr, self.lr))
        self._sgd_done_from = None
        if left > 0:
            ops.sgd_momentum_range(self._sgd_table, 0, left, lr, self.momentum, gs)
        self.refresh_derived()

    def refresh_derived(self):
        """Everything computed FROM the trainable filters, after they changed (the solver's update; a caller that wrote Param.w / .wf
        itself): folded depthwise copies, then the derived filter images -- the operand planes of the forward pass's frcnn_gemm_h2
        launches and what a TEST-mode network on the same session reads: Winograd U of the 3x3 filters first (also with x3 / h2 off: a
        no-op when no ('wino', ...) entry is cached), then the pre-split planes of everything (x3 / h2) -- and the prepared gradient
        filters.  Weight-only launches: with cfg.HIP.PREP_STREAM they run on the side stream, beside the next forward pass
        (Session.h2_planes & co. wait for them at their first use: PreparedFilters.wait_planes)."""
        self.sess.device_filters_moved = True        # (Session.winograd_params: later first uses derive from the live device filters)
        for p in self.params.values():
            if p.dw:
                ops.dwconv3x3_refold(p.w, p.scale, p.wf)

        def derived():
            self.sess.wino_refresh()
            if self.sess.x3:
                self.sess.x3_refresh()
            if self.sess.h2:                         # the same for cfg.HIP.MFMA_H2
                self.sess.h2_refresh()
        self.sess.prepared.weights_changed()
        self.sess.prepared.refresh(pre=derived)

    def invalidate_prepared(self):
        self.sess.prepared.invalidate()

    def _wd(self, scope):
        wd = self.net.weight_decay_for(scope)
        return self.weight_decay if wd is None else wd

    # ---- checkpoint view (tf.train.Saver saves the variables AND the optimizer slots `<variable>/Momentum`) ----------
    def export_variables(self, slots=True):
        """{TF/slim variable name: ndarray in the variable's own layout (HWIO filters, [in,out] matrices)} of every TRAINED
        parameter, read back from the device master copies (packed [Cout][KH][KW][Cin]); with slots=True also the momentum
        accumulators under `<name>/Momentum` (MomentumOptimizer's slot name)."""
        out = {}
        for p in self.params.values():
            if p.dw:
                name = p.scope + "/depthwise_weights"
                for suffix, t in (("", p.w),) + ((("/Momentum", p.acc_w),) if slots else ()):
                    out[name + suffix] = t.detach().cpu().numpy().reshape(self.sess.variables[name].shape).copy()
                continue
            wname, bname = p.scope + "/weights", p.scope + "/biases"
            ref = self.sess.variables[wname]
            for suffix, t in (("", p.w),) + ((("/Momentum", p.acc_w),) if slots else ()):
                hwio = t.detach().cpu().numpy().transpose(1, 2, 3, 0)          # [O,KH,KW,I] -> [KH,KW,I,O]
                if hwio.size != ref.size:
                    raise ValueError("%s: device filter has %d values, variable %d (channel-folded stem filters are not exportable)"
                                     % (wname, hwio.size, ref.size))
                out[wname + suffix] = np.ascontiguousarray(hwio).reshape(ref.shape)
            if p.bias is not None:
                out[bname] = p.bias.detach().cpu().numpy().copy()
                if slots:
                    out[bname + "/Momentum"] = p.acc_b.detach().cpu().numpy().copy()
        return out

    def import_slots(self, reader_or_dict):
        """Restore the momentum accumulators written by export_variables(slots=True)."""
        get = reader_or_dict.get_tensor if hasattr(reader_or_dict, "get_tensor") else reader_or_dict.__getitem__
        for p in self.params.values():
            if p.dw:
                acc = np.asarray(get(p.scope + "/depthwise_weights/Momentum"), dtype=np.float32)
                p.acc_w.copy_(torch.from_numpy(np.ascontiguousarray(acc.reshape(tuple(p.w.shape)))))
                continue
            wname, bname = p.scope + "/weights", p.scope + "/biases"
            acc = np.asarray(get(wname + "/Momentum"), dtype=np.float32)
            kh, kw = p.w.shape[1], p.w.shape[2]
            acc = acc.reshape(kh, kw, p.w.shape[3], p.w.shape[0]).transpose(3, 0, 1, 2)
            p.acc_w.copy_(torch.from_numpy(np.ascontiguousarray(acc)))
            if p.bias is not None:
                p.acc_b.copy_(torch.from_numpy(np.asarray(get(bname + "/Momentum"), dtype=np.float32)))

    def regularization_loss(self, out):
        """slim l2_regularizer(WEIGHT_DECAY): wd * sum(w^2)/2 over every conv / fc weight (network.py:315-317), all tensors in
        two launches (the master tensors are static, so the pointer table is built once)."""
        if self._reg_tables is None:
            groups = {}                                              # L2 coefficient -> tensors (MobileNet: backbone vs heads)
            for sc in self.reg_scopes:
                p = self.params.get(sc)
                if p is not None:
                    t = p.w
                else:
                    info = self.sess.conv_info[sc]
                    if "w_master" not in info:
                        info["w_master"] = info["w"] if info["scale"] is None else \
                            (info["w"] / torch.from_numpy(info["scale"]).to(info["w"].device).view(-1, 1, 1, 1)).contiguous()
                    t = info["w_master"]
                groups.setdefault(self._wd(sc), []).append(t)
            dev = self.sess.device
            self._reg_keep = groups
            self._reg_tables = [(wd, torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=dev),
                                 torch.tensor([t.numel() for t in ts], dtype=torch.int64, device=dev)) for wd, ts in groups.items()]
        for i, (wd, ptrs, sizes) in enumerate(self._reg_tables):
            ops.sumsq_multi(ptrs, sizes, 0.5 * wd, out, i > 0)
        return out
