"""GPU: the solver and the regulariser against float64.  frcnn_sgd_momentum_multi / _range (MomentumOptimizer, train_val.py:128-145, as
TrainState.apply lays out its table: BN-folded filters with their folded copy refreshed, depthwise filters without scale or decay, biases
with DOUBLE_BIAS lr_mult 2 and no decay) over three steps from a non-zero momentum accumulator, grad_scale 0.5, sizes that are no
multiple of 256 or of SGD_BLOCKS * 256; frcnn_sumsq_multi over 1 .. 200 tensors of 1 .. 2.4M elements; TrainState.regularization_value()
against 0.5 wd sum(w^2) in float64 over the tensors regularization_loss collects.  The float64 recurrence is not bit-equal to the
kernel's float32 one (hipcc may contract to FMA): w, acc and wf are held to 4 ulp per step of the magnitudes that were summed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
LR, MOM, GS = 0.01, 0.9, 0.5


def _entries(dev, seed):
    """(tensors, table entries) shaped like TrainState.apply's: folded filter + bias, depthwise filter, plain filter + bias, a big folded
    filter"""
    rng = np.random.RandomState(seed)
    spec = [  # name, Cout, K, folded, lr_mult, wd
        ("conv_w", 130, 603, True, 1.0, 1e-4),
        ("conv_b", 130, 1, False, 2.0, 0.0),
        ("dw_w", 1, 405, False, 1.0, 0.0),
        ("head_w", 37, 1000, False, 1.0, 1e-4),
        ("head_b", 37, 1, False, 2.0, 0.0),
        ("big_w", 509, 4715, True, 1.0, 1e-4),          # 2 399 935 elements
    ]
    ts = []
    for name, Cout, K, folded, lrm, wd in spec:
        n = Cout * K
        d = dict(name=name, K=K, lrm=lrm, wd=wd,
                 w=rng.randn(n).astype(np.float32) * 0.05, acc=rng.randn(n).astype(np.float32) * 0.01,
                 s=(0.5 + rng.rand(Cout)).astype(np.float32) if folded else None)
        d["dev"] = {k: torch.from_numpy(d[k]).to(dev) for k in ("w", "acc")}
        d["dev"]["grad"] = torch.zeros(n, dtype=torch.float32, device=dev)
        d["dev"]["wf"] = torch.full((n,), 7.0, dtype=torch.float32, device=dev) if folded else None
        d["dev"]["s"] = torch.from_numpy(d["s"]).to(dev) if folded else None
        ts.append(d)
    entries = [(d["dev"]["w"], d["dev"]["acc"], d["dev"]["wf"], d["dev"]["grad"], d["dev"]["s"], d["K"], d["lrm"], d["wd"]) for d in ts]
    return ts, entries


class _Ref:
    """float64 recurrence + the magnitudes it summed (Sa, Sw: the error scale of acc and w)"""

    def __init__(self, d):
        self.w, self.a = d["w"].astype(np.float64), d["acc"].astype(np.float64)
        self.Sw, self.Sa = np.abs(self.w), np.abs(self.a)
        self.s = None if d["s"] is None else np.repeat(d["s"].astype(np.float64), d["K"])
        self.lr, self.wd = LR * d["lrm"], d["wd"]

    def step(self, grad):
        s = 1.0 if self.s is None else self.s
        g = GS * grad.astype(np.float64) * s + self.wd * self.w
        self.a = MOM * self.a + g
        self.Sa = MOM * self.Sa + np.abs(GS * grad * s) + self.wd * np.abs(self.w)
        self.w = self.w - self.lr * self.a
        self.Sw = self.Sw + self.lr * self.Sa


def _check(d, ref, steps, what):
    w = d["dev"]["w"].cpu().numpy().astype(np.float64)
    a = d["dev"]["acc"].cpu().numpy().astype(np.float64)
    c = 4.0 * steps * EPS
    assert np.all(np.abs(a - ref.a) <= c * ref.Sa), (what, d["name"], "acc", float(np.abs(a - ref.a).max()))
    assert np.all(np.abs(w - ref.w) <= c * ref.Sw), (what, d["name"], "w", float(np.abs(w - ref.w).max()))
    if d["dev"]["wf"] is not None:
        wf = d["dev"]["wf"].cpu().numpy().astype(np.float64)
        assert np.all(np.abs(wf - ref.w * ref.s) <= (c + EPS) * ref.Sw * ref.s), (what, d["name"], "wf")


@pytest.mark.parametrize("splits", [None, [(0, 2), (2, 3), (5, 1)], [(0, 1), (1, 5)], [(3, 3), (0, 3)]],
                         ids=["multi", "range_2_3_1", "range_1_5", "range_back_to_front"])
def test_sgd_momentum_three_steps_vs_float64(dev, splits):
    from frcnn_hip import ops
    ts, entries = _entries(dev, 1)
    table = ops.sgd_desc_table(entries, dev)
    refs = [_Ref(d) for d in ts]
    rng = np.random.RandomState(2)
    for step in range(1, 4):
        for d, ref in zip(ts, refs):
            g = (rng.randn(d["w"].size) * 0.1).astype(np.float32)
            d["dev"]["grad"].copy_(torch.from_numpy(g))
            ref.step(g)
        if splits is None:
            ops.sgd_momentum_multi(table, len(entries), LR, MOM, GS)
        else:
            for first, count in splits:
                ops.sgd_momentum_range(table, first, count, LR, MOM, GS)
        torch.cuda.synchronize()
        for d, ref in zip(ts, refs):
            _check(d, ref, step, "step %d" % step)


def test_sgd_momentum_range_leaves_other_entries_alone(dev):
    from frcnn_hip import ops
    ts, entries = _entries(dev, 3)
    table = ops.sgd_desc_table(entries, dev)
    rng = np.random.RandomState(4)
    before = []
    for d in ts:
        d["dev"]["grad"].copy_(torch.from_numpy((rng.randn(d["w"].size) * 0.1).astype(np.float32)))
        before.append({k: (None if v is None else v.clone()) for k, v in d["dev"].items()})
    ops.sgd_momentum_range(table, 1, 3, LR, MOM, GS)
    torch.cuda.synchronize()
    for i, (d, b) in enumerate(zip(ts, before)):
        if not 1 <= i < 4:                               # outside [first, first + count): not a bit changed
            assert all(b[k] is None or torch.equal(d["dev"][k], b[k]) for k in ("w", "acc", "wf")), (i, d["name"])
            continue
        ref = _Ref(d)
        ref.step(b["grad"].cpu().numpy())
        _check(d, ref, 1, "range")


@pytest.mark.parametrize("count", [1, 7, 200])
@pytest.mark.parametrize("accumulate", [False, True])
def test_sumsq_multi_vs_float64(dev, count, accumulate):
    from frcnn_hip import ops
    rng = np.random.RandomState(count)
    sizes = list(rng.randint(1, 20000, size=count))
    sizes[0] = 1
    if count > 1:
        sizes[1] = 2400001                               # 2.4M: a tail past every block stride
    if count > 2:
        sizes[2] = 64 * 256 + 3
    ts = [torch.from_numpy((rng.randn(n) * 2.0 ** rng.randint(-6, 7)).astype(np.float32)).to(dev) for n in sizes]
    ptrs = torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=dev)
    sz = torch.tensor(sizes, dtype=torch.int64, device=dev)
    scale = 0.5 * 1e-4
    v0 = 0.75
    out = torch.full((2,), v0 if accumulate else 123.0, dtype=torch.float32, device=dev)
    ops.sumsq_multi(ptrs, sz, scale, out[:1], accumulate)
    torch.cuda.synchronize()
    s = scale * sum(float((t.double() ** 2).sum()) for t in ts)
    want = s + (v0 if accumulate else 0.0)
    got = float(out[0])
    tol = EPS * abs(s) + (EPS * abs(want) if accumulate else 0.0)      # f32 rounding of the double sum (+ of the add)
    assert abs(got - want) <= tol, (got, want)
    assert float(out[1]) == (v0 if accumulate else 123.0)


def test_regularization_value_vs_float64(dev):
    """TrainState.regularization_value(): slim l2_regularizer(WEIGHT_DECAY) = 0.5 wd sum(w^2) over every conv / fc weights variable of the
    network (network.py:315-317), against float64 over the session's host variables"""
    from frcnn_hip.runtime import Session
    from frcnn_hip.train import TrainState
    from model.config import cfg
    from nets.resnet_v1 import resnetv1
    old = (cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO)
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO = 64, 0.0
    try:
        sess = Session(device=dev, seed=5)
        net = resnetv1(num_layers=50)
        net.create_architecture("TRAIN", 21, tag="reg_value", anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
        sess.init_variables(net.variable_specs())
        rng = np.random.RandomState(2)
        image = ((rng.rand(1, 128, 160, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)) * np.float32(1 / 256.0)
        gt = np.array([[16, 16, 79, 79, 3], [60, 30, 150, 110, 7]], dtype=np.float32)
        net.train_forward(sess, dict(data=image, im_info=np.array([128, 160, 1.0], dtype=np.float32), gt_boxes=gt))
        ts = TrainState(sess, net, momentum=0.9, weight_decay=1e-4).build()
        got = float(ts.regularization_value().cpu()[0])
        # independent of what regularization_loss collected: every slim weights variable of the network as the session holds it (host
        # float32, HWIO / [in, out], BN not folded), squared in float64
        names = [k for k in sess.variables if k.endswith("/weights")]
        want = sum(0.5 * ts._wd(k[:-len("/weights")]) * float((np.asarray(sess.variables[k], np.float64) ** 2).sum()) for k in names)
        assert len(names) == sum(len(v) for v in ts._reg_keep.values()) and len(names) > 50
        # the device's masters of folded filters are (w * scale) / scale in float32: two roundings per element, four per square
        assert want > 0 and abs(got - want) <= 8 * EPS * want, (got, want)
    finally:
        cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO = old
