"""One training step as a flat launch list (the stand-in for the reference's ONE `sess.run` per step, lib/nets/network.py:488-498,
lib/model/train_val.py:260-300).

The step the Python host code enqueues is ~1 300 C-ABI launches + ~350 event records / waits over 4-5 HIP streams, and every argument
of every launch is a function of the image shape only: static session buffers, static arena buffers (below), constants.  What costs the
host 11 us per launch is not the launch but the Python around it -- dictionary lookups of buffers, shape arithmetic, ctypes argument
conversion, the sweep's bookkeeping.  A `Recording` is that step with the Python taken out: while ONE eager step runs, every `call()` of
the binding (frcnn_hip.call) and every stream-level operation of the step (ops.ev_record / st_wait_event / st_wait_stream / t_copy /
t_zero / host_op) is appended to a list; later steps of the same shape REPLAY the list -- the same launches with the same arguments on
the same streams in the same order, hence the same bits as the eager step by construction -- in one tight loop.

Streams are recorded as SLOTS (0 = the stream the step was started on, 1.. = helper streams in order of first use), so a recording can be
replayed with another assignment of physical streams to slots (`Recording.bind`): which hardware queue a helper stream lands on is worth
milliseconds per step, and `StreamPicker` chooses the assignment by timing real steps at start-up.

The few arguments that do change from step to step (the sampling seeds of the target layers, dropout seeds) are marked when they are
recorded (`patch_last`) and rewritten at replay from the step's seed counter.

The cache around it lives here too: `Session.graphs` holds one entry type (`Entry`: `CapturedGraph` for the TEST-mode hipGraphs, made and
launched by `launch_captured`; `RecordedStep` for the training steps of one key), and `StepReplayer` decides which step of a key runs
eagerly, which is recorded and which are replayed.
"""
import ctypes
import time

import torch

import frcnn_hip as _binding
from . import ops


class Arena(object):
    """Static result tensors for the wrappers in frcnn_hip.ops that allocate their outputs (`torch.empty` inside an op): while an arena
    is active (ops.arena), the n-th allocation of a step returns the session buffer ("arena", tag, n, shape, dtype) -- the same address
    every step, so a recorded launch that wrote it can be replayed, and a later eager step of the same shape reuses it."""

    def __init__(self, sess, tag):
        self.sess, self.tag, self.n = sess, tag, 0

    def reset(self):
        self.n = 0

    def take(self, shape, dtype, device):
        key = ("arena", self.tag, self.n, tuple(int(s) for s in shape), dtype)
        self.n += 1
        store = self.sess._store()                              # (per image shape inside Session.shape_scope)
        t = store.get(key)
        if t is None:
            t = store[key] = torch.empty(key[3], dtype=dtype, device=self.sess.device if device is None else device)
        return t


class Recording(object):
    CALL, OP = 0, 1

    def __init__(self, main_stream):
        self.main = main_stream
        self.slot_of = {int(main_stream.cuda_stream): 0}        # stream handle -> slot
        self.streams = [main_stream]                            # slot -> torch stream it was recorded on
        self.cmds = []                                          # (CALL, fn, [ctypes args], stream arg index or -1, slot) | (OP, closure(rec))
        self.patches = []                                       # (command index, argument index, variable, value at record time, multiplier, ctype)
        self.vars = dict(seed=0, gt=0)                          # the recorded step's own variables
        self.keep = []                                          # whatever the recorded arguments point to and nobody else holds
        self.bound = None                                       # slot -> torch stream of the compiled program
        self.prog = None
        self.n_calls = 0

    # ---- recording ---------------------------------------------------------------------------------------------------------------------
    def slot(self, stream):
        """slot of a torch stream (helper streams register themselves at first use)"""
        return self._slot_of_handle(int(stream.cuda_stream), stream)

    def _slot_of_handle(self, h, stream=None):
        s = self.slot_of.get(h)
        if s is None:
            s = self.slot_of[h] = len(self.streams)
            self.streams.append(torch.cuda.ExternalStream(h) if stream is None else stream)
        return s

    def add_call(self, fn, name, args):
        if name in HOST_ONLY:                                   # host arithmetic on host arrays: nothing a later step has to repeat
            return
        conv = []
        types = fn.argtypes or []
        for i, a in enumerate(args):
            if isinstance(a, ctypes._SimpleCData) or isinstance(a, ctypes.Array) or i >= len(types):
                conv.append(a)
            else:
                conv.append(types[i](a))
        si, slot = -1, -1
        if conv and isinstance(conv[-1], ctypes.c_void_p) and name not in NO_STREAM_ARG:
            h = int(conv[-1].value or 0)                        # every launch entry takes its stream last (include/frcnn_hip.h)
            if h or 0 in self.slot_of:                          # (0: the legacy default stream, when the step itself runs on it)
                si, slot = len(conv) - 1, self._slot_of_handle(h)
        self.cmds.append((self.CALL, fn, conv, si, slot, name))
        self.n_calls += 1

    def patch_last(self, arg_index, mult=1, var="seed"):
        """The last recorded call's argument `arg_index` changes from step to step.  var = "seed": a sampling seed, replay adds
        mult * (the step's seed - the recorded step's seed); var = "gt": the number of ground-truth boxes of the step's image."""
        i = len(self.cmds) - 1
        a = self.cmds[i][2][arg_index]
        self.patches.append((i, arg_index, var, int(a.value), int(mult), type(a)))

    def add_op(self, closure):
        """closure(rec): a stream-level operation of the step (event record / wait, tensor copy, collective); streams by rec.stream(slot)"""
        def op(rec, closure=closure):                           # (whatever the operation returns -- a tensor, a work handle -- is not a status code)
            closure(rec)
        self.cmds.append((self.OP, op))

    # ---- replay ------------------------------------------------------------------------------------------------------------------------
    def stream(self, slot):
        return self.bound[slot]

    def bind(self, streams):
        """compile the list for an assignment slot -> torch stream (slot 0 = the stream the step runs on)"""
        streams = list(streams)
        assert len(streams) == len(self.streams)
        self.bound = streams
        handles = [ctypes.c_void_p(int(s.cuda_stream)) for s in streams]
        prog = []
        for c in self.cmds:
            if c[0] == self.CALL:
                _, fn, conv, si, slot, _name = c
                if si >= 0:
                    conv = list(conv)
                    conv[si] = handles[slot]
                prog.append((fn, tuple(conv)))
            else:
                prog.append((c[1], (self,)))
        self.prog = prog
        return self

    def bound_to(self, main_stream):
        return self.bound is not None and int(self.bound[0].cuda_stream) == int(main_stream.cuda_stream)

    def default_binding(self, main_stream):
        return [main_stream] + list(self.streams[1:])

    def _patch(self, now):
        for i, ai, var, val, mult, typ in self.patches:
            fn, args = self.prog[i]
            a = list(args)
            a[ai] = typ(val + mult * (int(now["seed"]) - int(self.vars["seed"]))) if var == "seed" else typ(int(now[var]))
            self.prog[i] = (fn, tuple(a))

    def replay(self, now):
        """Enqueue the step.  now: this step's variables {"seed": Network._sample_seed, "gt": rows of gt_boxes}; torch's current stream
        must be the stream bound to slot 0."""
        if self.patches:
            self._patch(now)
        for fn, args in self.prog:
            rc = fn(*args)
            if rc:
                from . import check
                check(rc, getattr(fn, "__name__", "recorded call"))


class StreamPicker(object):
    """Which PHYSICAL stream each helper slot of a recorded step runs on, chosen by timing real steps.

    ROCm multiplexes HIP streams onto a few hardware queues (4 by default), and whether a helper stream of the step -- filter gradients,
    solver, filter preparation -- shares a queue with the data-gradient chain it is meant to run beside is decided by the order in which
    streams were created in the process: an RCCL process group that merely EXISTS moved the step from 19.4 to 23.4 ms in round 4
    (profiles/r04_ao_dp_pieces.txt), GPU_MAX_HW_QUEUES=8 gave that back and cost the single-GPU step 24 ms.  A recording names streams by
    slot, so the assignment can be searched instead of inherited: one pass of coordinate descent -- for every helper slot in turn, every
    stream of a small pool -- each candidate timed over a window of `window` real training steps between two device synchronisations, a
    candidate kept when it beats the best so far by more than 1 %.  Any binding is CORRECT (the list's events order the streams whatever
    they are; two slots on one stream merely serialise), so the search cannot change a bit of the result -- the steps it times are
    ordinary training steps."""

    def __init__(self, rec, main, pool, window=3, gain=0.01):
        self.rec, self.pool, self.window, self.gain = rec, list(pool), int(window), float(gain)
        self.best = rec.default_binding(main)
        self.best_s = None
        self.queue = [None]                                  # None = the inherited binding (the baseline), then (slot, pool index)
        self.queue += [(s, i) for s in range(1, len(self.best)) for i in range(len(self.pool))]
        self.left, self.t0, self.cur = 0, 0.0, None
        self.done = len(self.best) < 2
        self.log = []                                        # (what, seconds per step)

    def _binding(self, cand):
        b = list(self.best)
        if cand is not None:
            b[cand[0]] = self.pool[cand[1]]
        return b

    def before_step(self, main):
        if self.done or self.left:
            return
        while self.queue:
            self.cur = self.queue.pop(0)
            b = self._binding(self.cur)
            b[0] = main
            if self.cur is None or int(b[self.cur[0]].cuda_stream) != int(self.best[self.cur[0]].cuda_stream):
                break                                        # (a candidate equal to the slot's current stream was measured already)
        else:
            self._finish(main)
            return
        main.synchronize()
        self.rec.bind(b)
        self.left, self.t0 = self.window, time.perf_counter()

    def after_step(self, main):
        if self.done or not self.left:
            return
        self.left -= 1
        if self.left:
            return
        main.synchronize()
        s = (time.perf_counter() - self.t0) / self.window
        self.log.append(("inherited" if self.cur is None else "slot %d -> pool[%d]" % self.cur, s))
        if self.best_s is None or s < self.best_s * (1.0 - self.gain):
            self.best_s = s
            if self.cur is not None:
                self.best[self.cur[0]] = self.pool[self.cur[1]]
        if not self.queue:
            self._finish(main)

    def _finish(self, main):
        b = list(self.best)
        b[0] = main
        self.rec.bind(b)
        self.done = True


# ---- what Session.graphs holds -----------------------------------------------------------------------------------------------------------
# One entry per key: a captured TEST-mode chain (Network.forward_device under the shape's scope key, Network.propose_device under
# ("propose",) + that key) or the recorded training steps of one ("train_replay", ...) key.  Every entry names the shape scope whose
# buffers it addresses, and is dropped with it (Session.drop_scope); every path that drops entries goes through release_entries().
class Entry(object):
    __slots__ = ("scope",)

    def release(self, sess):
        """The entry is about to be forgotten, or its recording is: a stream search that runs on it ends here.  This is the one place
        that ends a search and clears sess.picking."""


class CapturedGraph(Entry):
    """A hipGraph of one image shape: the graph, the image buffer it reads, the forward pass's flop count, the rois per image and
    whatever else of the network the build left behind and a replay has to put back (`state`: the caller's own)."""
    __slots__ = ("graph", "image", "flops", "per", "state")

    def __init__(self, scope, graph, image, flops, per, state):
        self.scope, self.graph, self.image, self.flops, self.per, self.state = scope, graph, image, flops, per, state


class RecordedStep(Entry):
    """The training steps of one key: how many ran eagerly (`seen`), the LRU stamp (`used`), and once a steady step was recorded its
    Recording, the derived-set generation it covers, the network's result views of that step and -- while the session's stream search
    runs on this recording -- the StreamPicker."""
    __slots__ = ("seen", "used", "rec", "gen", "views", "acts", "picker")

    def __init__(self, scope):
        self.scope, self.seen, self.used = scope, 0, 0
        self.rec = self.gen = self.views = self.acts = self.picker = None

    def release(self, sess):
        """A finished search is published to the session (every recording with as many slots binds to its streams); one that was still
        running is abandoned -- sess.picking must not stay set, or no other recording could ever start a search."""
        pk, self.picker = self.picker, None
        if pk is not None:
            if pk.done:
                sess.picked_streams, sess.pick_log = list(pk.best[1:]), list(pk.log)
            sess.picking = False

    def forget(self, sess):
        """Drops the recording (kept: the `seen` count, so the next steady step records again)."""
        self.release(sess)
        self.rec = self.gen = self.views = self.acts = None


def release_entries(sess, keys=None):
    """Releases and deletes the entries of sess.graphs under `keys` (default: all of them)."""
    for k in list(sess.graphs) if keys is None else keys:
        sess.graphs.pop(k).release(sess)


def launch_captured(sess, key, scope, build, image, snapshot, restore):
    """A TEST-mode chain as one hipGraph per key.  First sight of the key: build() once on sess.stream as warm-up (allocates buffers,
    packs weights), then captured; snapshot(what the warm-up returned) -> (rois per image, state) is kept with the graph.  Always:
    restore(entry) puts the network's view of the results back, the image is copied to where the graph reads it when the caller staged
    it somewhere else (its own buffer, the session-wide staging buffer vs. the shape scope's: 4 B per pixel and channel, device to
    device, on the stream the graph is launched on), and the graph is launched on the current stream.  -> the entry"""
    ent = sess.graphs.get(key)
    if ent is None:
        cur = torch.cuda.current_stream(sess.device)
        with torch.cuda.stream(sess.stream):
            sess.stream.wait_stream(cur)
            sess.flops_last_forward = 0
            out = build()
            sess.stream.synchronize()
            flops = sess.flops_last_forward
            g = ops.Graph().capture(build)
            sess.stream.synchronize()
        per, state = snapshot(out)
        ent = sess.graphs[key] = CapturedGraph(scope, g, image, flops, per, state)
    restore(ent)
    if ent.image.data_ptr() != image.data_ptr():
        ent.image.copy_(image, non_blocking=True)
    ent.graph.launch()
    return ent


class StepReplayer(object):
    """Which training steps run eagerly, which one is recorded and which are replayed (Network.train_step_async under
    cfg.HIP.TRAIN_REPLAY), for one network: the first step of a key is eager, the next STEADY one is recorded while it runs (solver
    built, prepared filters current, nothing derived during the step), every later one replays the recording -- until the session's
    derived-filter set moves on (Session.derived_generation), which costs one eager-or-recorded step.  At most `cap` keys per session
    keep an entry, least recently used first out.  The network hands over the key, the shape scope the step's buffers live in, the step
    itself (`body(out)`: enqueues it eagerly, the five losses into `out`) and a pair for its host-side results: snapshot() -> (views,
    acts) after a recorded step, restore(views, acts) after a replayed one (which also owes the network the step's seed advance).
    Nothing here needs a GPU beyond what the streams, the session and the body it is given need."""

    def __init__(self):
        self.clock, self.arena = 0, None                        # LRU clock of the entries; the static results of the ops that allocate
        self.stats = dict(eager=0, recorded=0, replayed=0)

    new_stream = staticmethod(lambda device: torch.cuda.Stream(device=device))      # (the search's pool)

    def step(self, sess, main, name, key, scope, body, ready, snapshot, restore, now, hip, cap):
        """One step on `main`, torch's current stream.  name: prefix of the step's static buffers (losses, arena); ready(): the solver
        handle is built (asked only when a recording could start); now: the step's variables {"seed", "gt"} (Recording.replay); hip:
        cfg.HIP; cap: entries kept.  -> the five losses, a fresh device tensor"""
        ent = sess.graphs.get(key)
        if ent is None:
            ent = self._admit(sess, key, scope, cap)
        self.clock += 1
        ent.used = self.clock
        out = sess.buf(name + "/losses", (5,))
        rec = ent.rec
        if rec is not None and ent.gen == sess.derived_generation():
            self._replay(sess, main, ent, rec, now, restore, hip)
            return out.clone()
        if rec is not None:
            # the set of derived filter images changed after the recording (a TEST-mode network's first run on this session, another
            # shape's plan key): its refresh launches no longer cover the set -> this step runs eagerly (weights_changed + refresh see
            # everything) and the shape is recorded again at its next steady step
            ent.forget(sess)
        arena = self.arena
        if arena is None or arena.sess is not sess:
            arena = self.arena = Arena(sess, name)
        arena.reset()
        prep = sess.prepared
        steady = (ent.seen >= 1 and ready() and _binding.recorder is None
                  and (not hip.PREP_STREAM or (prep.ready_version == prep.version and len(prep.plan) > 0 and len(prep.ready) == len(prep.plan))))
        gen_before = sess.derived_generation()
        ops.arena = arena
        try:
            if steady:
                prep.forget_waits(main)                       # the recorded step carries every tier's wait at its first use
                rec = Recording(main)
                rec.vars = dict(now)
                _binding.recorder = rec
            body(out)
        finally:
            ops.arena = None
            _binding.recorder = None
        ent.seen += 1
        if steady and sess.derived_generation() == gen_before:     # (a filter image derived inline during the step = not the steady state yet)
            ent.rec, ent.gen = rec, gen_before
            ent.views, ent.acts = snapshot()
            self.stats["recorded"] += 1
        else:
            self.stats["eager"] += 1
        return out.clone()

    def _admit(self, sess, key, scope, cap):
        live = [k for k, e in sess.graphs.items() if type(e) is RecordedStep]
        if len(live) >= cap:
            release_entries(sess, [min(live, key=lambda k: sess.graphs[k].used)])
        ent = sess.graphs[key] = RecordedStep(scope)
        return ent

    def _replay(self, sess, main, ent, rec, now, restore, hip):
        # which physical stream every helper slot runs on: inherited from the recording, or (cfg.HIP.TRAIN_PICK_STREAMS = pool size)
        # searched once per session by timing real steps (StreamPicker) and then shared by every recording with the same slots
        picked = sess.picked_streams
        if ent.picker is None and picked is None and not sess.picking and int(hip.TRAIN_PICK_STREAMS) > 0:
            ent.picker = StreamPicker(rec, main, [self.new_stream(sess.device) for _ in range(int(hip.TRAIN_PICK_STREAMS))])
            sess.picking = True
        pk = ent.picker
        if pk is not None:
            pk.before_step(main)                              # (binds the recording to the candidate it times next)
            if pk.done:                                       # nothing to try
                ent.release(sess)
                pk = None
        if pk is None:
            helpers = picked if (picked is not None and len(picked) == len(rec.streams) - 1) else list(rec.streams[1:])
            if rec.bound is None or [int(x.cuda_stream) for x in rec.bound] != [int(x.cuda_stream) for x in [main] + helpers]:
                rec.bind([main] + helpers)
        prep = sess.prepared
        for h, st in list(prep.readers.items()):              # a TEST-mode network on another stream read the filter images since the
            if h != int(main.cuda_stream):                    # last refresh: the list's refresh waits for `main` only, so main waits for it
                main.wait_stream(st)
        prep.readers = {}
        rec.replay(now)
        prep.refreshed()                                      # (the replayed refresh re-recorded the tier events: every reader waits again)
        restore(ent.views, ent.acts)
        self.stats["replayed"] += 1
        if pk is not None:
            pk.after_step(main)
            if pk.done:
                ent.release(sess)


# Entries of include/frcnn_hip.h WITHOUT a trailing `void* stream` (tests/test_replay_cpu.py checks the two sets against the header):
# launch-context setters (thread-local state the following launches read: recorded, replayed in order) ...
NO_STREAM_ARG = frozenset(["frcnn_set_tuning", "frcnn_detect_set_tuning", "frcnn_conv2d_wgrad_set_plan", "frcnn_conv2d_wgrad_h2_set_plan"])
# ... and host functions on host memory (their pointer arguments do not outlive the call: never recorded)
HOST_ONLY = frozenset(["frcnn_generate_anchors", "frcnn_winograd_filter_transform", "frcnn_winograd7_filter_transform", "frcnn_pack_filter_hwio",
                       "frcnn_prep_image_shape", "frcnn_crc32c", "frcnn_snappy_uncompress", "_nms", "frcnn_graph_begin", "frcnn_graph_end",
                       "frcnn_graph_launch", "frcnn_graph_destroy", "frcnn_abi_version", "frcnn_build_info", "frcnn_sgd_desc_bytes",
                       "frcnn_conv2d_wgrad_supported", "frcnn_jpeg_info", "frcnn_jpeg_entropy_decode", "frcnn_jpeg_pixels_host", "frcnn_summary_limits",
                       "frcnn_jpeg_quant_tables", "frcnn_jpeg_coefs_host", "frcnn_jpeg_stream_bound", "frcnn_jpeg_entropy_encode",
                       "frcnn_draw_detections_host", "frcnn_proposal_recall_host", "frcnn_soft_nms_host",
                       "frcnn_box_vote_host", "frcnn_merge_flip_views_host",
                       "frcnn_roi_align_host", "frcnn_roi_align_bwd_host", "frcnn_roi_align_classify_host", "frcnn_ohem_select_host",
                       "frcnn_iou_loss_host"])
