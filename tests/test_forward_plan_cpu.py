"""CPU: the forward launch plan (frcnn_hip/forward.py: Plan, the route rules conv_route / winograd_products / mean_fusable, Forms and
one function per route, under lib/nets/network.py Network._conv and the three backbones).  The REAL resnetv1 / vgg16 / mobilenetv1
classes build their graphs on stand-ins: tensors are shape-only objects with distinct addresses (a ResNet-101 at 600 x 1000 in a batch of
8 is planned without allocating an activation), the session stand-in hands out such buffers, filters and operand planes and writes
down every mark, and a recording `ops` writes down every entry called inside a mark with the labels of its tensors and its scalars.
tests/golden/forward_plan_trace.json holds the ordered traces of the switch grid, a digest per entry, as fixtures/gen_forward_plan_trace.py wrote them from
the commit before the forward pass was split into frcnn_hip/forward.py; the rule tests below call the route rules directly.  No GPU (of
the library only the host-side anchor generator runs): tests/test_forward_plan_gpu.py ties these stand-ins to the real session."""
import copy
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tf-faster-rcnn_amd"), os.path.join(ROOT, "tf-faster-rcnn_amd", "lib")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "forward_plan_trace.json")
ACT_NONE, ACT_RELU = 0, 1


# ---- stand-ins -------------------------------------------------------------------------------------------------------------------------
class T(object):
    """a tensor's shape, name and address; a view shares the address and the name"""

    def __init__(self, name, shape, addr=None):
        self.name, self.shape = name, tuple(int(v) for v in shape)
        self.addr = (zlib.crc32(repr((name, self.shape)).encode()) + 1) << 8 if addr is None else addr

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return self.addr

    def view(self, *shape):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        assert int(np.prod(shape, dtype=np.int64)) == self.numel()
        return T(self.name, shape, self.addr)

    def __getitem__(self, i):
        assert isinstance(i, int)
        return T(self.name, self.shape[1:], self.addr)

    def label(self):
        return [self.name, list(self.shape)]


class Planes(object):
    """stand-in for ops.H2 and for the packed planes of a filter: a key"""

    def __init__(self, *key):
        self.key, self.rows, self.K = list(key), key[-2], key[-1]

    def label(self):
        return self.key


def lab(a):
    if isinstance(a, (T, Planes)):
        return a.label()
    if isinstance(a, (tuple, list)):
        return [lab(v) for v in a]
    if isinstance(a, np.ndarray):
        return ["ndarray", list(a.shape)]
    if isinstance(a, (np.floating, np.integer)):
        return a.item()
    assert a is None or isinstance(a, (bool, int, float, str)), a
    return a


class Sess(object):
    """Session stand-in: `trace` is the ordered list of marks [tag, flops, nbytes, [ops entries]] and of prepared.get keys"""
    profile = None

    def __init__(self, net, spreads=None):
        self.net, self.spreads, self.trace, self.cur = net, dict(spreads or {}), [], None
        self.bufs, self.packed, self.conv_info, self.by_addr, self.prepared = {}, {}, {}, {}, self
        for name, spec in net.variable_specs().items():          # mobilenetv1._dw_params: the folded depthwise filters are packed already
            if name.endswith("/depthwise_weights"):
                sc = name[:-len("/depthwise_weights")]
                self.packed[("dw", sc)] = (self._t("w:" + sc, spec.shape[:3]), self._t("b:" + sc, spec.shape[2:3]))

    def _t(self, name, shape):
        key = (name, tuple(int(v) for v in shape))
        t = self.bufs.get(key)
        if t is None:
            t = self.bufs[key] = T(name, shape)
            assert self.by_addr.setdefault(t.addr, key) == key, "address collision of the stand-ins"
        return t

    def buf(self, name, shape, dtype=None, zero=False):
        return self._t(name, shape)

    def h2_buf(self, name, rows, K):
        return Planes("h2", name, int(rows), int(K))

    def to_device(self, a, dtype=None):
        return self._t("host", np.asarray(a).shape)

    def _bias(self, scope, forced):
        has = forced or (scope + "/biases") in self.net.variable_specs()
        return self._t("b:" + scope, (self.net.variable_specs()[scope + "/weights"].shape[-1],)) if has else None

    def conv_params(self, scope, bn_eps=None, fold_w=False, out_scale=None, out_shift=None):
        key = (scope, bn_eps, fold_w, None if out_scale is None else tuple(out_scale))
        if key not in self.packed:
            s = tuple(self.net.variable_specs()[scope + "/weights"].shape)
            kh, kw, cin, cout = s if len(s) == 4 else (1, 1) + s
            w = self._t("w:" + scope + (":affine" if out_scale is not None else ""), (cout, kh, 8, 4) if fold_w else (cout, kh, kw, cin))
            self.packed[key] = (w, self._bias(scope, bn_eps is not None or out_scale is not None))
            self.conv_info[scope] = {"w": w, "b": self.packed[key][1], "bn": bn_eps is not None}
        return self.packed[key]

    def winograd_params(self, scope, bn_eps=None, m=2):
        kh, kw, cin, cout = self.net.variable_specs()[scope + "/weights"].shape
        G = 121 if m == 7 else (m + 2) ** 2
        return self._t("u:%s:%d" % (scope, m), (G, cout, cin)), self._bias(scope, bn_eps is not None)

    def h2_planes(self, w):
        return Planes("h2w", w.name, w.shape[0], w.numel() // w.shape[0])

    def x3_planes(self, w):
        return Planes("x3w", w.name, w.shape[0], w.numel() // w.shape[0])

    def h2_channel_spread(self, scope):
        return self.spreads.get(scope, 1.0)

    # sess.prepared
    def get(self, key, fn):
        self.trace.append(["prepared.get", lab(key)])
        return fn()

    def wait_planes(self):
        pass

    def mark(self, tag, flops, fn, nbytes=0):
        assert self.cur is None
        ent = [tag, int(flops), int(nbytes), []]
        self.trace.append(ent)
        self.cur = ent[3]
        try:
            return fn()
        finally:
            self.cur = None

    def label_of(self, addr):
        name, shape = self.by_addr[addr]
        return [name, list(shape)]


class RecOps(object):
    """the `ops` the nets.* modules see: every entry is written down (inside the mark that calls it, or as a mark-less entry) and returns
    its out= tensor; the pure host helpers stay the real ones"""

    def __init__(self, sess):
        from frcnn_hip import ops as real
        self._sess = sess
        self.conv_out_size, self.winograd_points, self.winograd_tiles = real.conv_out_size, real.winograd_points, real.winograd_tiles
        self.generate_anchors = real.generate_anchors

    def __getattr__(self, name):
        def entry(*a, **kw):
            ent = [name, [lab(v) for v in a]] + [[k, lab(kw[k])] for k in sorted(kw)]
            (self._sess.trace if self._sess.cur is None else self._sess.cur).append(ent)
            return kw.get("out")
        return entry


class _Lib(object):
    """frcnn_hip.lib(): the launch context is not set; the host entries (frcnn_generate_anchors) are the library's"""

    def __init__(self, real):
        self._real = real

    def frcnn_set_tuning(self, key, value):
        pass

    def __getattr__(self, name):
        return getattr(self._real(), name)


def _stub_layers(net, cfg):
    """the proposal and target layers are not part of the plan under test: buffers of the documented shapes, the nms layer's mark"""
    s, tag = net._sess, net._tag

    def proposal_layer(rpn_cls_prob, rpn_bbox_pred, name):
        post, B = int(cfg[net._mode].RPN_POST_NMS_TOP_N), rpn_cls_prob.shape[0]
        s.mark("op:proposal_layer", 0, lambda: None)
        net._num_rois, net._rois_per_image = s.buf(tag + "/num_rois", (B,)), post
        return s.buf(tag + "/rois", (B * post, 5)), s.buf(tag + "/roi_scores", (B * post, 1))

    def proposal_top_layer(rpn_cls_prob, rpn_bbox_pred, name):
        n = int(cfg.TEST.RPN_TOP_N)
        net._num_rois, net._rois_per_image = None, n
        return s.buf(tag + "/top_rois", (n, 5)), s.buf(tag + "/top_scores", (n, 1))

    def anchor_target_layer(rpn_cls_score, name):
        net._anchor_targets = {}

    def proposal_target_layer(rois, roi_scores, name):
        net._proposal_targets, net._num_rois = {}, None
        n = int(cfg.TRAIN.BATCH_SIZE)
        return s.buf(tag + "/" + name + "/rois", (n, 5)), s.buf(tag + "/" + name + "/scores", (n, 1))
    net._proposal_layer, net._proposal_top_layer = proposal_layer, proposal_top_layer
    net._anchor_target_layer, net._proposal_target_layer = anchor_target_layer, proposal_target_layer


def _make(net_name):
    from nets.mobilenet_v1 import mobilenetv1
    from nets.resnet_v1 import resnetv1
    from nets.vgg16 import vgg16
    return dict(res50=lambda: resnetv1(50), res101=lambda: resnetv1(101), vgg16=vgg16, mobile=mobilenetv1)[net_name]()


def plan_trace(net_name, mode="TEST", batch=1, hw=(600, 1000), switches=None, fuse_tail_entry=False, spreads=None):
    """The ordered trace of one graph build: create_architecture, _build_network on the stand-in session and image, graph_key -- the
    entry points the commit before the split has too.  switches: dotted configuration keys ("HIP.MFMA_H2", "TEST.MODE") -> values."""
    import frcnn_hip
    import model.config as C
    import nets.mobilenet_v1
    import nets.network
    import nets.resnet_v1
    import nets.vgg16
    cfg = C.cfg
    saved = copy.deepcopy(dict(cfg))
    try:
        cfg.USE_GPU_NMS = False                                      # (as tests/conftest.py pins it)
        for dotted, val in (switches or {}).items():
            node, parts = cfg, dotted.split(".")
            for p in parts[:-1]:
                node = node[p]
            assert parts[-1] in node, dotted
            node[parts[-1]] = val
        net = _make(net_name)
        net.create_architecture(mode, 21, tag="t")
        net._fuse_tail_entry = fuse_tail_entry
        sess = Sess(net, spreads)
        net._sess, net._image, net._im_info = sess, sess.buf("t/image", (batch, hw[0], hw[1], 4)), (float(hw[0]), float(hw[1]), 1.0)
        _stub_layers(net, cfg)
        rec = RecOps(sess)
        with pytest.MonkeyPatch.context() as mp:
            for mod in (nets.network, nets.resnet_v1, nets.vgg16, nets.mobilenet_v1, sys.modules.get("frcnn_hip.forward")):
                if mod is not None and hasattr(mod, "ops"):
                    mp.setattr(mod, "ops", rec)
            stub = _Lib(frcnn_hip.lib)
            mp.setattr(frcnn_hip, "lib", lambda: stub)
            net._build_network(mode == "TRAIN")
        trace = sess.trace
        if mode == "TRAIN":
            for r in net._tape:
                trace.append(["tape", r["kind"]] + [[k, lab(r[k])] for k in sorted(r) if k != "kind"])
            trace.append(["requires_grad", sorted(sess.label_of(a) for a in net._requires_grad)])
        trace.append(["graph_key", lab(net.graph_key(net._image.shape, net._im_info))])
        return json.loads(json.dumps(trace))
    finally:
        for k in list(cfg):
            cfg[k] = saved[k]


SPREAD_SCOPE = "resnet_v1_50/block3/unit_2/bottleneck_v1/conv1"
TEST_GRID = [
    ("defaults", {}),
    ("MFMA_H2 off", {"HIP.MFMA_H2": False}),
    ("MFMA_X3 off", {"HIP.MFMA_X3": False}),
    ("MFMA_H2 and MFMA_X3 off", {"HIP.MFMA_H2": False, "HIP.MFMA_X3": False}),
    ("WINOGRAD off", {"HIP.WINOGRAD": False}),
    ("WINOGRAD_M = 2", {"HIP.WINOGRAD_M": 2}),
    ("WINOGRAD_7X7 off", {"HIP.WINOGRAD_7X7": False}),
    ("WINOGRAD_FUSED_F2 off", {"HIP.WINOGRAD_FUSED_F2": False}),
    ("FUSE_TAIL_MEAN off", {"HIP.FUSE_TAIL_MEAN": False}),
    ("H2_TRUNK_PLANES off", {"HIP.H2_TRUNK_PLANES": False}),
    ("H2_LAZY_SPLIT off", {"HIP.H2_LAZY_SPLIT": False}),
    ("H2_LAZY_SPLIT off, block4 direct", {"HIP.H2_LAZY_SPLIT": False, "HIP.WINOGRAD_DIRECT_SCOPES": ("block4",)}),
    ("H2_MIN_TILES = 1", {"HIP.H2_MIN_TILES": 1}),
    ("H2_TILE_CFG = 9, X3_TILE_CFG = 1", {"HIP.H2_TILE_CFG": 9, "HIP.X3_TILE_CFG": 1}),
    ("POOLING_MODE align", {"POOLING_MODE": "align"}),
    ("RESNET.MAX_POOL", {"RESNET.MAX_POOL": True}),
    ("TEST.MODE top", {"TEST.MODE": "top"}),
]
TRAIN_GRID = [
    ("defaults", {}),
    ("H2_TRAIN off", {"HIP.H2_TRAIN": False}),
    ("WINOGRAD_TRAIN off", {"HIP.WINOGRAD_TRAIN": False}),
    ("H2_TRAIN_MIN_TILES = None, H2_MIN_TILES = 1", {"HIP.H2_TRAIN_MIN_TILES": None, "HIP.H2_MIN_TILES": 1}),
    ("POOLING_MODE align", {"POOLING_MODE": "align"}),
    ("RESNET.MAX_POOL", {"RESNET.MAX_POOL": True}),
]


def plan_traces():
    """{run: its ordered trace} of every run tests/golden/forward_plan_trace.json holds"""
    out = {}
    for B in (1, 4, 8):
        out["res101 TEST batch %d" % B] = plan_trace("res101", batch=B)
    for name, sw in TEST_GRID:
        out["res50 TEST " + name] = plan_trace("res50", switches=sw)
    out["res50 TEST fuse_tail_entry"] = plan_trace("res50", fuse_tail_entry=True)
    for e in (19, 17):
        out["res50 TEST spread 2^-%d" % e] = plan_trace("res50", spreads={SPREAD_SCOPE: 2.0 ** -e})
    for net in ("vgg16", "mobile"):
        out[net + " TEST defaults"] = plan_trace(net)
    for net in ("res50", "vgg16", "mobile"):
        for name, sw in TRAIN_GRID:
            out["%s TRAIN %s" % (net, name)] = plan_trace(net, "TRAIN", switches=sw)
    return out


def digest(entry):
    """40 bits of the SHA-1 of an entry's canonical JSON: any other tag, count, label, shape or scalar gives another digest"""
    return hashlib.sha1(json.dumps(entry, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:10]


def digest_traces(traces):
    """the golden file's form: per run the digest of every entry, in order, and the graph key in full (its fields are compared one by one)"""
    return {run: dict(entries=[digest(e) for e in tr[:-1]], graph_key=tr[-1][1]) for run, tr in traces.items()}


@pytest.fixture(scope="module")
def traces():
    return plan_traces()


@pytest.fixture(scope="module")
def golden_traces():
    with open(GOLDEN) as f:
        return json.load(f)


def tags(trace):
    return [e[0] for e in trace if len(e) == 4 and isinstance(e[3], list) and isinstance(e[1], int)]


def flat(key):
    """the fields of a graph key: its leaves, in order"""
    return [v for k in key for v in (flat(k) if isinstance(k, list) else [k])]


# ---- the ordered plan ------------------------------------------------------------------------------------------------------------------
def test_the_ordered_forward_plan_of_every_run_is_the_recorded_one(traces, golden_traces):
    """Every mark with its FLOP and byte counts, every entry called inside it with the labels of its tensors and planes and its scalar
    arguments, every prepared.get key, in TRAIN mode the tape and the set of tensors that take a gradient -- against the trace recorded
    from the forward pass as it was before the split, entry for entry by digest (the file would be 440 kB with the entries in full; the
    first entry that differs is printed with its neighbours, and fixtures/gen_forward_plan_trace.py --full run on the recorded commit
    prints the entries it is compared with).  The graph key is the one entry that may differ: it must still hold every field of the
    recorded one."""
    assert sorted(traces) == sorted(golden_traces)
    for run in sorted(golden_traces):
        got, want = traces[run], golden_traces[run]["entries"]
        assert len(got) > 30 and got[-1][0] == "graph_key"
        for i, (g, w) in enumerate(zip(got[:-1], want)):
            assert digest(g) == w, (run, i, "the entries around the first that differs:", got[max(0, i - 2):i + 2], "recorded digests:", want[max(0, i - 2):i + 2])
        assert len(got) - 1 == len(want), run
        have, fields = [repr(v) for v in flat(got[-1][1])], flat(golden_traces[run]["graph_key"])
        if " TRAIN " in run:
            # the recorded key held cfg.HIP.H2_MIN_TILES whatever the mode; a TRAIN-mode key holds the threshold its rules read instead
            # (forward.h2_min_tiles: H2_TRAIN_MIN_TILES, 320, unless that is None)
            tiles = 1 if "H2_MIN_TILES = 1" in run else 150
            fields.remove(tiles)
            have.remove(repr(tiles if "H2_TRAIN_MIN_TILES = None" in run else 320))
        for v in fields:
            assert repr(v) in have, (run, v)
            have.remove(repr(v))


def test_equal_graph_keys_mean_equal_plans(traces):
    """Two runs may share a captured graph only if they make the same launches.  (The two channel-spread runs are left out: the spread
    is a property of the session's weights, and graphs are kept per session.)  WINOGRAD_FUSED_F2 was not part of the key once."""
    by_key = {}
    for run, tr in traces.items():
        if " TEST " in run and "spread" not in run:
            by_key.setdefault(json.dumps(tr[-1]), []).append(run)
    assert len(by_key) > len(TEST_GRID)
    for runs in by_key.values():
        for run in runs[1:]:
            assert traces[run][:-1] == traces[runs[0]][:-1], (runs[0], run)
    key = {run: json.dumps(traces["res50 TEST " + run][-1]) for run in ("defaults", "WINOGRAD_FUSED_F2 off")}
    assert key["defaults"] != key["WINOGRAD_FUSED_F2 off"]
    assert traces["res50 TEST defaults"][:-1] != traces["res50 TEST WINOGRAD_FUSED_F2 off"][:-1]


def same_per_image(a, b, Ba, Bb):
    """a and b are the same once the batch dimension is stripped: integers agree as they are or per image"""
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same_per_image(x, y, Ba, Bb) for x, y in zip(a, b))
    if isinstance(a, int) and not isinstance(a, bool) and isinstance(b, int):
        return a == b or a * Bb == b * Ba
    if isinstance(a, str) and "/split@" in a:                # a split pass's planes are named after the address of the (batched) tensor
        return isinstance(b, str) and a.split("@")[0] == b.split("@")[0]
    return a == b


def test_the_per_image_plan_does_not_depend_on_the_batch(traces):
    """ResNet-101 at batch 1, 4 and 8: the same marks, entries, buffers and scalars once the batch dimension is stripped (rows, tiles,
    FLOPs and the leading dimension of every shape per image; the byte counts hold the filters once per launch and are left out)."""
    one = traces["res101 TEST batch 1"]
    assert len(tags(one)) > 150
    for B in (4, 8):
        many = traces["res101 TEST batch %d" % B]
        assert len(many) == len(one)
        for i, (a, b) in enumerate(zip(one[:-1], many[:-1])):
            a, b = (a[:2] + a[3:], b[:2] + b[3:]) if len(a) == 4 else (a, b)
            assert same_per_image(a, b, 1, B), (B, i, a, b)


def test_a_narrow_channel_spread_moves_that_layer_off_h2(traces):
    """Session.h2_channel_spread below 2^-18: that layer, and only that layer, leaves frcnn_gemm_h2 for the exact x3 split"""
    base, wide, narrow = (tags(traces["res50 TEST " + r]) for r in ("defaults", "spread 2^-17", "spread 2^-19"))
    assert wide == base and "conv:h2:" + SPREAD_SCOPE in base
    assert "conv:h2:" + SPREAD_SCOPE not in narrow and "conv:x3:" + SPREAD_SCOPE in narrow
    rest = [t for t in base if not t.endswith(SPREAD_SCOPE)]
    assert [t for t in narrow if not t.endswith(SPREAD_SCOPE) and t != "op:h2_split"] == [t for t in rest if t != "op:h2_split"]


def test_producers_and_consumers_agree_about_operand_planes(traces):
    """ResNet-101, defaults, every 1x1 convolution: where the producer of its input was told emit_h2 (it wrote operand planes: out_planes
    of a GEMM, the _h2 output transform) the consumer's mark is conv:h2: and it reads those very planes; the other way round, a conv:h2:
    1x1 reads planes its producer emitted, or the planes of a separate split pass."""
    emitted, split, told, ran = {}, set(), 0, 0
    for ent in traces["res101 TEST batch 1"]:
        if len(ent) != 4:
            continue
        tag, (op,) = ent[0], ent[3] or [[None, []]]
        kw = dict(p for p in op[2:])
        if op[0] == "h2_split":
            split.add(json.dumps(kw["out"]))
        if op[0] in ("gemm_x3", "conv2d") and (op[1][2] == 1 if op[0] == "gemm_x3" else op[1][3] == 1):       # a 1x1 off the h2 route
            assert op[1][0][0] not in emitted, (tag, "its producer emitted planes", emitted[op[1][0][0]])
        if op[0] in ("gemm_h2", "gemm_h2_mean") and (op[1][2] == 1 or op[0] == "gemm_h2_mean"):              # G = 1: a 1x1 on it
            planes = op[1][0]
            assert tag.startswith("conv:h2:") and planes[0] == "h2"
            assert json.dumps(planes) in split or emitted.get(planes[1]) == planes, (tag, planes)
            told, ran = told + (json.dumps(planes) not in split), ran + 1
        out_planes = kw.get("out_planes") if op[0] == "gemm_h2" else op[1][5] if op[0] == "winograd_output_transform_h2" else None
        if out_planes is not None:
            emitted[out_planes[1]] = out_planes                  # by the name of the producer's output buffer
    assert told > 50 and ran > told


# ---- the rules themselves --------------------------------------------------------------------------------------------------------------
HIP_KEYS = ("MFMA_H2", "H2_TRAIN", "H2_LAZY_SPLIT", "H2_TRUNK_PLANES", "H2_TILE_CFG", "MFMA_X3", "X3_TILE_CFG", "WINOGRAD", "WINOGRAD_TRAIN",
            "WINOGRAD_MIN_CIN", "WINOGRAD_M", "WINOGRAD_7X7", "WINOGRAD_F2_SCOPES", "WINOGRAD_DIRECT_SCOPES", "WINOGRAD_FUSED_F2",
            "FUSE_TAIL_MEAN", "H2_MIN_TILES", "H2_TRAIN_MIN_TILES")


def make_plan(mode="TEST", batch=1, **switches):
    """a Plan of the default switches with some replaced"""
    from frcnn_hip import forward
    from model.config import cfg
    hip = {k: cfg.HIP[k] for k in HIP_KEYS}
    assert all(k in hip for k in switches)
    hip.update(switches)
    return forward.make_plan(mode, batch, hip)


def test_the_plan_key_holds_every_field_a_test_mode_rule_reads():
    from frcnn_hip import forward
    p = make_plan()
    assert isinstance(p, tuple) and not hasattr(p, "__dict__") and len(p.key()) == len(p) - 1
    for k in HIP_KEYS:
        if k not in ("WINOGRAD_TRAIN", "H2_TRAIN_MIN_TILES"):
            flipped = {k: ("block9",) if k.endswith("SCOPES") else (not p._asdict()[k.lower()]) if isinstance(p._asdict()[k.lower()], bool) else 3}
            assert make_plan(**flipped).key() != p.key(), k
    assert make_plan(WINOGRAD_TRAIN=not p.winograd_train).key() == p.key() and make_plan(batch=4).key() != p.key()
    assert make_plan("TRAIN", 0).key() != make_plan("TEST", 0).key()
    with pytest.raises(AttributeError):
        p.mode = "TRAIN"
    with pytest.raises(KeyError):
        forward.make_plan("TEST", 1, {})


S50, S101 = "resnet_v1_50", "resnet_v1_101"
U = S101 + "/%s/unit_%d/bottleneck_v1/%s"
# (name, images, scope, k, stride, pad, act, Cin, Cout, H x W of the output, keywords of conv_route) of ResNet-101 at 600 x 1000: the stem
# 300 x 500, block1 150 x 250, block3 38 x 63, the 300 RoIs of an image 7 x 7
LAYERS = dict(
    direct=[("stem", 1, S101 + "/conv1", 7, 2, (3, 3, 3, 3), ACT_RELU, 4, 64, 300 * 500, dict(fold_w=True)),
            ("rpn_cls_score", 1, S101 + "/rpn_cls_score", 1, 1, (0, 0, 0, 0), ACT_NONE, 512, 18, 38 * 63, {}),
            ("cls_score", 1, S101 + "/cls_score", 1, 1, (0, 0, 0, 0), ACT_NONE, 2048, 21, 300, {}),
            ("bbox_pred", 1, S101 + "/bbox_pred", 1, 1, (0, 0, 0, 0), ACT_NONE, 2048, 84, 300, dict(out_affine=True)),
            ("block3 conv1, one image alone", 0, U % ("block3", 2, "conv1"), 1, 1, (0, 0, 0, 0), ACT_RELU, 1024, 256, 38 * 63, {})],
    x3=[("block1 conv1", 1, U % ("block1", 2, "conv1"), 1, 1, (0, 0, 0, 0), ACT_RELU, 256, 64, 150 * 250, {}),
        ("block1 conv3", 1, U % ("block1", 2, "conv3"), 1, 1, (0, 0, 0, 0), ACT_RELU, 64, 256, 150 * 250, dict(residual=True))],
    h2=[("block3 conv1", 1, U % ("block3", 2, "conv1"), 1, 1, (0, 0, 0, 0), ACT_RELU, 1024, 256, 38 * 63, {}),
        ("block3 conv3", 1, U % ("block3", 2, "conv3"), 1, 1, (0, 0, 0, 0), ACT_RELU, 256, 1024, 38 * 63, dict(residual=True)),
        ("block3 conv1, 4 images", 4, U % ("block3", 2, "conv1"), 1, 1, (0, 0, 0, 0), ACT_RELU, 1024, 256, 38 * 63, {}),
        ("block3 conv3, 4 images", 4, U % ("block3", 2, "conv3"), 1, 1, (0, 0, 0, 0), ACT_RELU, 256, 1024, 38 * 63, dict(residual=True)),
        ("tail-entry shortcut map", 1, U % ("block4", 1, "shortcut"), 1, 1, (0, 0, 0, 0), ACT_NONE, 1024, 2048, 38 * 63, dict(no_bias=True)),
        ("tail-entry conv1 map", 1, U % ("block4", 1, "conv1"), 1, 1, (0, 0, 0, 0), ACT_NONE, 1024, 512, 38 * 63, dict(no_bias=True))],
    winograd=[("block1 conv2", 1, U % ("block1", 2, "conv2"), 3, 1, (1, 1, 1, 1), ACT_RELU, 64, 64, 150 * 250, {}),
              ("block4 conv2", 1, U % ("block4", 2, "conv2"), 3, 1, (1, 1, 1, 1), ACT_RELU, 512, 512, 300 * 49, {}),
              ("rpn_conv/3x3", 1, S101 + "/rpn_conv/3x3", 3, 1, (1, 1, 1, 1), ACT_RELU, 1024, 512, 38 * 63, {})])
# the one switch that governs each route, and where the layers go without it
GOVERNS = dict(h2=(dict(MFMA_H2=False), "x3"), x3=(dict(MFMA_X3=False), "direct"), winograd=(dict(WINOGRAD=False), "direct"))


def route(layer, **switches):
    from frcnn_hip import forward
    name, B, scope, k, stride, pad, act, Cin, Cout, pixels, kw = layer
    return forward.conv_route(make_plan(batch=B, **switches), scope, k, stride, pad, act, Cin, Cout, max(1, B) * pixels, **kw)


def test_conv_route_answers_the_key_every_layer_is_listed_under():
    """The named layer shapes of ResNet-101 at 600 x 1000 against the route rule, under the defaults; flipping the one switch that
    governs a route moves exactly the layers listed under it; the planes, stride and spread arguments; TRAIN mode."""
    from frcnn_hip import forward
    assert sorted(LAYERS) == sorted(forward.CONV)
    for key, layers in LAYERS.items():
        for layer in layers:
            assert route(layer) == key, layer[0]
            for other, (switch, then) in GOVERNS.items():
                assert route(layer, **switch) == (then if other == key else key), (layer[0], switch)
    c1 = LAYERS["h2"][0]
    assert route(c1, H2_MIN_TILES=151) == "x3" and route(c1, H2_MIN_TILES=150) == "h2"        # 75 x 2 tiles in the 4-image plan
    assert route(c1[:10] + (dict(planes=False),)) == "x3"                                       # no planes and no lazy split
    assert route(c1[:10] + (dict(spread=2.0 ** -19),)) == "x3" and route(c1[:10] + (dict(spread=2.0 ** -18),)) == "h2"
    assert route(c1[:10] + (dict(residual=True, res_stride=2),)) == "direct"                    # a subsampled residual: the direct kernel's epilogue
    assert route(c1[:4] + (2,) + c1[5:]) == "direct"
    rpn = LAYERS["winograd"][2]
    assert route(rpn, WINOGRAD_DIRECT_SCOPES=("rpn_conv",)) == "direct" and route(rpn, WINOGRAD_MIN_CIN=2048) == "direct"
    assert route(rpn[:6] + (2,) + rpn[7:]) == "direct"                                          # ReLU6: not a Winograd epilogue
    # TRAIN mode, one image as it is: Winograd behind WINOGRAD_TRAIN, h2 behind H2_TRAIN and its own threshold, never x3
    name, B, scope, k, stride, pad, act, Cin, Cout, pixels, kw = rpn
    tr = lambda layer, **sw: forward.conv_route(make_plan("TRAIN", 0, **sw), *layer[2:9], layer[9], **layer[10])
    assert tr(rpn) == "winograd" and tr(rpn, WINOGRAD_TRAIN=False) == "direct"
    assert tr(c1) == "direct" and tr(c1, H2_TRAIN_MIN_TILES=38) == "h2" and tr(c1, H2_TRAIN_MIN_TILES=38, H2_TRAIN=False) == "direct"
    assert tr(c1, H2_TRAIN_MIN_TILES=None, H2_MIN_TILES=1) == "h2" and tr(LAYERS["x3"][0]) == "direct"


def test_winograd_products_answers_the_form_of_every_chain():
    from frcnn_hip import forward
    wp = forward.winograd_products
    b1 = (16 * 75 * 125, 64, 64, 16, 2, 150 * 250)               # block1 conv2: F(2,3), 75 x 125 tiles
    rpn = (36 * 10 * 16, 512, 1024, 36, 4, 38 * 63)              # F(4,3) on 38 x 63
    b4 = (300, 512, 512, 121, 7, 300 * 49)                        # the mixed 7 x 7 scheme: one tile per RoI
    p = make_plan()
    assert wp(p, *b1) == "fused_x3" and wp(p, *rpn) == "h2" and wp(p, *b4) == "h2"
    assert wp(make_plan(WINOGRAD_FUSED_F2=False), *b1) == "x3" and wp(make_plan(MFMA_X3=False), *b1) == "f32"
    assert wp(p, *b1[:5] + (1 << 23,)) == "x3"                    # the fused launch's 32-bit pixel index
    for chain in (rpn, b4):
        assert wp(make_plan(MFMA_H2=False), *chain) == "x3" and wp(make_plan(MFMA_H2=False, MFMA_X3=False), *chain) == "f32"
        assert wp(p, *chain, spread=2.0 ** -19) == "x3"
    assert forward.winograd_scheme(p, U % ("block1", 2, "conv2"), 150, 250) == 2 and forward.winograd_scheme(p, S101 + "/rpn_conv/3x3", 38, 63) == 4
    assert forward.winograd_scheme(p, U % ("block4", 2, "conv2"), 7, 7) == 7
    assert forward.winograd_scheme(make_plan(WINOGRAD_7X7=False), U % ("block4", 2, "conv2"), 7, 7) == 4
    assert forward.winograd_scheme(make_plan(WINOGRAD_M=2), S101 + "/rpn_conv/3x3", 38, 63) == 2


def test_mean_fusable_follows_the_h2_rule_and_the_image_split():
    from frcnn_hip import forward
    mf = forward.mean_fusable
    rows = 300 * 49
    assert mf(make_plan(), rows, 2048, 512, 49) and mf(make_plan(batch=4), 4 * rows, 2048, 512, 49)
    assert not mf(make_plan(batch=4), 4 * rows + 49, 2048, 512, 49)             # the RoI rows do not split evenly over the images
    assert not mf(make_plan(batch=2), 2 * 75, 2048, 512, 49)                     # ... not in whole RoIs
    assert not mf(make_plan(FUSE_TAIL_MEAN=False), rows, 2048, 512, 49) and not mf(make_plan(MFMA_H2=False), rows, 2048, 512, 49)
    assert not mf(make_plan("TRAIN", 0, H2_TRAIN_MIN_TILES=1), rows, 2048, 512, 49)
    assert not mf(make_plan(), rows, 2048, 512, 49, spread=2.0 ** -19)
    assert mf(make_plan(H2_LAZY_SPLIT=False), rows, 2048, 512, 49) and mf(make_plan(WINOGRAD=False), rows, 2048, 512, 49)
    assert not mf(make_plan(H2_LAZY_SPLIT=False, WINOGRAD=False), rows, 2048, 512, 49)       # nothing could make its input's planes


def test_forms_registry():
    from frcnn_hip import forward
    net = _make("res50")
    net.create_architecture("TEST", 21, tag="t")
    sess = Sess(net)
    ops = RecOps(sess)
    a, b = sess.buf("a", (1, 2, 2, 128)), sess.buf("b", (1, 2, 2, 128))
    for lazy in (False, True):
        f = forward.Forms(ops, sess, "t", lazy)
        assert not f.has_planes(a) and f.residual_operand(a) is a and f.residual_operand(None) is None
        f.need_f32(a, None, b)
        pl = Planes("h2", "a", 4, 128)
        assert f.wrote(a, pl, f32=False) is a and f.has_planes(a) and f.planes_of(a) is pl and f.residual_operand(a) is pl
        with pytest.raises(RuntimeError, match="graph construction error"):
            f.need_f32(b, a)
        f.wrote(a, pl)                                          # both forms: the float32 tensor is what a residual reads
        assert f.residual_operand(a) is a and f.planes_of(a) is pl
        f.wrote(a)                                              # written again without planes: the old ones are stale
        assert not f.has_planes(a)
        n = len(sess.trace)
        got = f.planes_of(b)
        if lazy:
            assert got.label() == ["h2", "t/split@%x" % b.data_ptr(), 4, 128] and f.planes_of(b) is got
            assert [e[0] for e in sess.trace[n:]] == ["op:h2_split"] and sess.trace[n][2] == 8 * b.numel()
        else:
            assert got is None and len(sess.trace) == n
