"""RoIAlign (cfg.POOLING_MODE = 'align') without a GPU: the host statements frcnn_roi_align_host / frcnn_roi_align_bwd_host
(csrc/roialign_math.h, the bit-exact reference of the kernels) against the numpy / torch statements of fixtures/roi_align_ref.py and
the stored vectors tests/golden/roi_align.npz, and the configuration plumbing of lib/nets/network.py.

Error bounds (u = 2**-24, the unit roundoff of float32; the float64 statements share the float32 sample coordinates, so coordinates
add nothing; l = v - low is exact, h = 1 - l is exact for h <= 0.5 (Sterbenz) and has an absolute error <= u/2 otherwise):

  forward, one output, M = max |feature value|:
    a sample is 4 terms (w_y * w_x) * v.  The errors of hy and hx move the four weights by at most u/2 each in total (hy's error is
    shared by hy*hx and hy*lx, whose partners sum to 1): u * M.  The weight product and the product with v round once each:
    sum_i u * w_i * M = u * M.  Three additions of partial sums <= M: 1.5 u * M.  Per sample 3.5 u * M.
    S*S samples are added ((S*S - 1) roundings of partial sums <= S*S * M) and divided by S*S (one rounding of a value <= M):
    |host - float64| <= (3.5 + (S*S - 1) / 2 + 0.5) * u * M = (4 + (S*S - 1) / 2) * u * M, to first order; FWD_SLACK covers the rest.

  backward, one feature element with n contributions c_k = (dout_k / S^2) * w_k:
    h has a RELATIVE error <= u (exact below 0.5, u/2 absolute above), l none, so a weight product is within 2.5 u relative; the
    division and the product with it round once each: every c_k is within 3.5 u * |c_k|.  n - 1 additions of partial sums
    <= sum |c_k|: (n - 1) / 2 * u * sum |c_k|.  Together <= (n + 3) * u * sum |c_k| (n counts every tap addition, also those of weight
    0).  The sum is then added to the dfeat that was there: one more rounding, u/2 * |result|.
    |host - float64| <= (n + 3) * u * sum |c_k| + u * |result|."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import roi_align_ref as ref  # noqa: E402

U = 2.0 ** -24
FWD_SLACK = 1.01
H, W, STRIDE = ref.EDGE_H, ref.EDGE_W, ref.EDGE_STRIDE
CASES = [(7, 2), (7, 1), (7, 3), (2, 1), (14, 4)]
CHANNELS = [4, 64, 300 * 4]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def edge_rois_with_bad_images():
    return np.concatenate([ref.EDGE_ROIS, np.array([[7, 16, 16, 48, 48], [-1, 16, 16, 48, 48]], dtype=np.float32)]).astype(np.float32)


def random_rois(rng, n, images=1):
    """boxes around and beyond a H x W map at STRIDE: inside, hanging over every edge, some narrower than a feature cell"""
    x1 = rng.uniform(-48, W * STRIDE, n)
    y1 = rng.uniform(-48, H * STRIDE, n)
    w = rng.uniform(0, 1, n) ** 2 * (W * STRIDE + 40)
    h = rng.uniform(0, 1, n) ** 2 * (H * STRIDE + 40)
    return np.stack([rng.randint(0, images, n).astype(np.float64), x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)


@pytest.fixture(scope="module")
def ops():
    from frcnn_hip import ops
    return ops


def test_edge_rois_take_the_branches_they_are_there_for(ops):
    """the header's own classification of the 196 samples of each edge RoI at P = 7, S = 2: a fixture that stops exercising a branch fails"""
    counts = ops.roi_align_classify_host(H, W, ref.EDGE_ROIS, STRIDE, 7, 2)
    assert counts.shape == (6, 4)
    zero, low, high, integer = counts.T.tolist()
    assert zero == [0, 115, 160, 0, 0, 0]
    assert low == [0, 45, 0, 0, 0, 0]
    assert high == [0, 0, 27, 28, 64, 0]
    assert integer[2] == 6 and integer[0] == 0
    for k, want in enumerate(ref.EDGE_KINDS_7_2):
        assert tuple(counts[k][:3]) == want[:3]
    feat = np.random.RandomState(1).randn(2, H, W, 4).astype(np.float32)
    out = ops.roi_align_host(feat, edge_rois_with_bad_images(), STRIDE, 7, 2)
    assert out.shape == (8, 7, 7, 4) and not out[6:].any() and all(out[k].any() for k in range(6))
    # image 1 is really read: the sixth RoI on image 0 gives other values
    moved = edge_rois_with_bad_images()[5:6].copy()
    moved[0, 0] = 0
    assert not np.array_equal(ops.roi_align_host(feat, moved, STRIDE, 7, 2)[0], out[5])
    # forward(ones) == (number of non-zeroed samples) / S^2 per bin, exactly (the weights of a sample sum to 1 within rounding: allow 2 ulp)
    ones = ops.roi_align_host(np.ones((2, H, W, 1), np.float32), ref.EDGE_ROIS, STRIDE, 7, 2)[..., 0]
    want = ref.valid_samples(ref.EDGE_ROIS, STRIDE, H, W, 7, 2) / 4.0
    assert np.abs(ones - want).max() <= 4 * U


def test_forward_host_equals_the_golden_bytes(ops, golden):
    g = golden["roi_align"]
    rois, stride = g["rois"], float(g["stride"])
    seen = 0
    for key in g.files:
        if not key.endswith("/out"):
            continue
        c, case, _ = key.split("/")
        P, S = (int(v) for v in case[1:].split("s"))
        got = ops.roi_align_host(g[c + "/feat"], rois, stride, P, S)
        assert got.shape == g[key].shape and np.array_equal(bits(got), bits(g[key])), key
        seen += 1
    assert seen == 6


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("P,S", CASES)
def test_forward_host_equals_the_float32_statement_and_meets_the_float64_bound(ops, P, S, C, capsys):
    rng = np.random.RandomState(1000 * P + 10 * S + C)
    feat = (rng.randn(2, H, W, C) * rng.choice([0.01, 1.0, 30.0], size=(1, 1, 1, C))).astype(np.float32)
    rois = np.concatenate([edge_rois_with_bad_images(), random_rois(rng, 4, images=2)])
    got = ops.roi_align_host(feat, rois, STRIDE, P, S)
    assert np.array_equal(bits(got), bits(ref.align_f32(feat, rois, STRIDE, P, S)))
    want = ref.align_f64(feat, rois, STRIDE, P, S)
    bound = FWD_SLACK * (4 + (S * S - 1) / 2.0) * U * float(np.abs(feat).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    with capsys.disabled():
        print("\nroi_align forward P=%d S=%d C=%d: max |host - f64| = %.3e, bound %.3e, ratio %.3f" % (P, S, C, err, bound, err / bound))
    assert err <= bound
    # the bias + ReLU epilogue is the plain result, + bias, max(., 0)
    bias = rng.randn(C).astype(np.float32)
    fused = ops.roi_align_host(feat, rois, STRIDE, P, S, bias=bias, act=1)
    want_fused = got + bias
    want_fused = np.where(want_fused < 0, np.float32(0), want_fused)
    want_fused[6:8] = 0                                    # a row without an image is zero, bias or not (as in the crop kernel)
    assert np.array_equal(bits(fused), bits(want_fused))


def _scatter64(dout, rois, S, weight=True, absolute=False):
    """float64 scatter of (|dout| / S^2) * (weight or 1) over every tap addition the statement makes -> [H,W,C]; dout None: the count of
    additions per element [H,W,1]"""
    R, P = rois.shape[0], (dout.shape[1] if dout is not None else 7)
    r, ty, tx = ref._taps(rois, STRIDE, H, W, P, S)
    C = dout.shape[3] if dout is not None else 1
    acc = np.zeros((H, W, C))
    for k in range(R):
        ly = ty["v"][k].astype(np.float64) - ty["lo"][k]
        lx = tx["v"][k].astype(np.float64) - tx["lo"][k]
        for i in range(P * S):
            if not ty["valid"][k][i]:
                continue
            for j in range(P * S):
                if not tx["valid"][k][j]:
                    continue
                d = np.ones(C) if dout is None else dout[k, i // S, j // S].astype(np.float64) / (S * S)
                if absolute:
                    d = np.abs(d)
                for yy, wy in ((ty["lo"][k][i], 1 - ly[i]), (ty["hi"][k][i], ly[i])):
                    for xx, wx in ((tx["lo"][k][j], 1 - lx[j]), (tx["hi"][k][j], lx[j])):
                        acc[yy, xx] += d * (wy * wx if (weight and dout is not None) else 1.0)
    return acc


@pytest.mark.parametrize("C", [4, 64, 300])
@pytest.mark.parametrize("R", [0, 1, 6, 130])
def test_backward_host_matches_float64_autograd(ops, R, C, capsys):
    P, S = 7, 2
    rng = np.random.RandomState(7 * R + C)
    rois = np.concatenate([ref.EDGE_ROIS[:5], ref.EDGE_ROIS[5:] * np.float32([0, 1, 1, 1, 1]), random_rois(rng, max(R - 6, 0))])[:R]
    rois = rois.astype(np.float32).reshape(R, 5)
    dout = rng.randn(R, P, P, C).astype(np.float32)
    base = rng.randn(H, W, C).astype(np.float32)
    got = ops.roi_align_bwd_host(dout, rois, STRIDE, S, base.copy())
    if R == 0:
        assert np.array_equal(bits(got), bits(base))
        return
    feat = torch.zeros(1, C, H, W, dtype=torch.float64, requires_grad=True)
    out = ref.roi_align_torch(feat, rois, STRIDE, P, S)                                  # [R,C,P,P]
    (out * torch.from_numpy(dout).double().permute(0, 3, 1, 2)).sum().backward()
    grad = feat.grad[0].permute(1, 2, 0).numpy()                                         # [H,W,C]
    want = base.astype(np.float64) + grad
    n = _scatter64(None, rois, S)                                                        # additions per element
    mag = _scatter64(dout, rois, S, absolute=True)                                       # sum |c_k|
    assert np.abs(_scatter64(dout, rois, S) - grad).max() <= 1e-12 * max(1.0, np.abs(grad).max())      # the scatter helper states the same sum
    bound = (n + 3) * U * mag + U * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    with capsys.disabled():
        print("\nroi_align backward R=%d C=%d: max |host - f64| = %.3e, largest err / bound = %.3f, most additions per element %d"
              % (R, C, err.max(), float((err / np.maximum(bound, 1e-300)).max()), int(n.max())))
    assert np.all(err <= bound)
    # dout = 1: the gradient sums to the sum of all tap weights / S^2 (closed form from the taps alone), accumulated into zeros
    ones = ops.roi_align_bwd_host(np.ones((R, P, P, 1), np.float32), rois, STRIDE, S, np.zeros((H, W, 1), np.float32))
    total = ref.weight_sum(rois, STRIDE, H, W, P, S)
    assert abs(float(ones.astype(np.float64).sum()) - total) <= (float(_scatter64(None, rois, S).max()) + 3) * U * total + 1e-30
    # += and not =: the same call on zeros differs from the call on `base` by `base`
    zero = ops.roi_align_bwd_host(dout, rois, STRIDE, S, np.zeros((H, W, C), np.float32))
    assert np.abs(got.astype(np.float64) - (zero.astype(np.float64) + base)).max() <= U * np.abs(want).max() and np.abs(base).min() > 0


def test_host_entries_refuse_bad_arguments(ops):
    feat, rois = np.zeros((1, H, W, 4), np.float32), ref.EDGE_ROIS[:1]
    for P, S in ((7, 0), (7, 5), (0, 2)):
        with pytest.raises(Exception):
            ops.roi_align_host(feat, rois, STRIDE, P, S)
    assert ops.roi_align_host(feat, np.zeros((0, 5), np.float32), STRIDE, 7, 2).shape == (0, 7, 7, 4)
    assert ops.roi_align_host(np.zeros((1, H, W, 3), np.float32), rois, STRIDE, 7, 2).shape == (1, 7, 7, 3)       # the host takes any C


@pytest.fixture
def restore_cfg():
    from model.config import cfg
    saved = (cfg.POOLING_MODE, cfg.HIP.ROI_ALIGN_SAMPLES, cfg.RESNET.MAX_POOL)
    yield cfg
    cfg.POOLING_MODE, cfg.HIP.ROI_ALIGN_SAMPLES, cfg.RESNET.MAX_POOL = saved


def _nets():
    from nets.mobilenet_v1 import mobilenetv1
    from nets.resnet_v1 import resnetv1
    from nets.vgg16 import vgg16
    return [lambda: resnetv1(50), vgg16, mobilenetv1]


def test_align_mode_builds_and_other_values_are_refused(restore_cfg):
    import model.config as C
    cfg = restore_cfg
    assert cfg.POOLING_MODE == "crop" and cfg.HIP.ROI_ALIGN_SAMPLES == 2
    C.cfg_from_list(["POOLING_MODE", "align"])
    assert cfg.POOLING_MODE == "align"
    for make in _nets():
        for mode in ("TEST", "TRAIN"):
            make().create_architecture(mode, 21, tag="t")
    resnet = _nets()[0]
    for mode in ("pool", "pyramid"):
        cfg.POOLING_MODE = mode
        with pytest.raises(NotImplementedError, match="POOLING_MODE"):
            resnet().create_architecture("TEST", 21, tag="t")
    cfg.POOLING_MODE = "align"
    for s in (0, 5):
        cfg.HIP.ROI_ALIGN_SAMPLES = s
        with pytest.raises(NotImplementedError, match="ROI_ALIGN_SAMPLES"):
            resnet().create_architecture("TEST", 21, tag="t")
    cfg.HIP.ROI_ALIGN_SAMPLES = 2
    cfg.RESNET.MAX_POOL = True
    with pytest.raises(NotImplementedError, match="RESNET.MAX_POOL.*POOLING_MODE|POOLING_MODE.*RESNET.MAX_POOL"):
        resnet().create_architecture("TEST", 21, tag="t")
    cfg.POOLING_MODE = "crop"                              # MAX_POOL with the crop stays what it was
    resnet().create_architecture("TEST", 21, tag="t")
    cfg.HIP.ROI_ALIGN_SAMPLES = 0                          # only read in 'align' mode
    resnet().create_architecture("TEST", 21, tag="t")


def test_graph_key_tells_the_modes_and_sample_counts_apart(restore_cfg):
    cfg = restore_cfg
    net = _nets()[0]()
    net.create_architecture("TEST", 21, tag="t")
    keys = []
    for mode, s in (("crop", 2), ("align", 2), ("align", 1)):
        cfg.POOLING_MODE, cfg.HIP.ROI_ALIGN_SAMPLES = mode, s
        keys.append(net.graph_key((1, 128, 160, 4), (128.0, 160.0, 1.0)))
    assert len(set(keys)) == 3


class _Sess(object):
    """Session stand-in for building the pooling layer without a GPU: buffers are CPU tensors, marked launches are written down, not run"""

    def __init__(self):
        self.marks = []

    def buf(self, name, shape, **kw):
        return torch.zeros(shape)

    def mark(self, name, flops, fn, nbytes=0):
        self.marks.append(name)


@pytest.mark.parametrize("mode", ["align", "crop"])
def test_train_tape_holds_one_pooling_record_of_the_mode(restore_cfg, mode):
    from frcnn_hip import forward
    cfg = restore_cfg
    cfg.POOLING_MODE = mode
    for make in _nets():
        net = make()
        net.create_architecture("TRAIN", 21, tag="t")
        net._sess, net._tape, net._requires_grad = _Sess(), [], set()
        net._forms = forward.Forms(None, net._sess, "t", False)
        net._feat_stride = [16]
        bottom, rois = torch.zeros(1, H, W, 8), torch.zeros(6, 5)
        net._requires_grad.add(bottom.data_ptr())
        out = net._crop_pool_layer(bottom, rois, "pool5")
        kinds = [r["kind"] for r in net._tape]
        assert tuple(out.shape) == (6, 7, 7, 8) and out.data_ptr() in net._requires_grad
        if mode == "align":
            assert kinds == ["roi_align"] and net._sess.marks == ["op:roi_align"]
            rec = net._tape[0]
            assert rec["samples"] == 2 and rec["stride"] == 16.0 and rec["feat"] is bottom and rec["rois"] is rois and rec["y"] is out
        else:
            assert kinds.count("crop") == 1 and "roi_align" not in kinds and "op:roi_align" not in net._sess.marks


def test_sweep_routes_the_record_to_the_roi_align_backward():
    from frcnn_hip.sweep import Sweep
    assert callable(getattr(Sweep, "visit_roi_align"))
