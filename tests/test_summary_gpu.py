"""GPU: frcnn_summary_stats (csrc/summary_stats.hip) against the numpy statement of frcnn_hip/summary.py, and the TensorBoard summaries of
the training loop: a run with summaries + validation at every step leaves the same bits as a run without, its event files parse with the
independent reader of tests/test_summary_cpu.py, and the histograms it writes are those of the step's own tensors.

Bounds: counts, num, n_zero, n_nonfinite, min, max exactly; sum within n * 2^-53 * sum|x| and sum_squares within n * 2^-53 * sum(x^2) of
math.fsum -- the error bound of a length-n float64 summation in ANY order (every x and every x*x is exact in float64), nothing measured."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_summary_cpu import event_class, expand_buckets, parse_events

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _segments():
    """(name, host array to upload, slice of the uploaded tensor that is the segment)"""
    from frcnn_hip import ops
    rng = np.random.RandomState(7)
    limits = ops.summary_limits()
    f32 = np.float32
    segs = []
    for n in (1, 63, 64, 65, 257):
        segs.append(("n=%d" % n, (rng.randn(n) * 3).astype(f32), slice(None)))
    big = (rng.randn(1048579) * np.exp(rng.randn(1048579) * 4)).astype(f32)        # several workgroups, a grid-stride wrap, a tail of 3
    segs.append(("n=1048579", big, slice(None)))
    for off in (1, 2, 3):                                                          # views starting 1..3 floats past a 16-byte boundary
        segs.append(("offset %d" % off, rng.randn(4096 + 261 + off).astype(f32), slice(off, None)))
    segs.append(("offset 1, short", rng.randn(8).astype(f32), slice(1, 3)))         # shorter than the scalar head
    segs.append(("all zero", np.zeros(5000, dtype=f32), slice(None)))
    segs.append(("constant", np.full(5000, 0.37, dtype=f32), slice(None)))
    relu = np.maximum(rng.randn(70001), 0).astype(f32)
    relu[::7] = -0.0
    segs.append(("half zeros", relu, slice(None)))
    den = (rng.randint(1, 1 << 23, size=3001).astype(np.uint32) | (rng.randint(0, 2, size=3001).astype(np.uint32) << np.uint32(31))).view(f32)
    assert np.all(den != 0) and np.all(np.abs(den) < np.finfo(f32).tiny)
    segs.append(("denormals", den, slice(None)))
    bad = rng.randn(1000).astype(f32)
    bad[[3, 500, 999]] = [np.nan, np.inf, -np.inf]
    segs.append(("nan and inf", bad, slice(None)))
    inside = limits[(np.abs(limits) <= np.finfo(f32).max) & (limits != 0)]
    near = inside.astype(f32)
    below = np.where(near.astype(np.float64) < inside, near, np.nextafter(near, f32(-np.inf)))
    above = np.nextafter(below, f32(np.inf))
    assert np.all(below.astype(np.float64) < inside) and np.all(above.astype(np.float64) > inside)
    segs.append(("bracketing", np.stack([below, above], axis=1).reshape(-1).astype(f32), slice(None)))
    return segs, limits, inside


@pytest.fixture(scope="module")
def kernel_case(dev):
    from frcnn_hip import ops, summary
    segs, limits, inside = _segments()
    holders = [torch.from_numpy(a).to(dev) for _, a, _ in segs]
    views = [h[s] for h, (_, _, s) in zip(holders, segs)]
    plan = ops.SummaryPlan(views)
    got = plan.launch().read()
    raw1 = plan.out.cpu().numpy().tobytes()
    raw2 = ops.SummaryPlan(views).launch().out.cpu().numpy().tobytes()
    want = [summary.reference_stats(a[s], limits) for _, a, s in segs]
    return dict(segs=segs, got=got, want=want, raw=(raw1, raw2), limits=limits, inside=inside, views=views)


def test_kernel_counts_and_extrema_are_exact(kernel_case):
    for (name, a, s), g, w in zip(kernel_case["segs"], kernel_case["got"], kernel_case["want"]):
        bad = np.nonzero(g["counts"] != w["counts"])[0]
        assert bad.size == 0, (name, bad[:8], g["counts"][bad[:8]], w["counts"][bad[:8]])
        for k in ("num", "n_zero", "n_nonfinite", "min", "max"):
            assert g[k] == w[k], (name, k, g[k], w[k])
        assert g["counts"].sum() == g["num"] - g["n_nonfinite"] and g["counts"][776] >= g["n_zero"]
    by = {n: g for (n, _, _), g in zip(kernel_case["segs"], kernel_case["got"])}
    assert by["all zero"]["counts"][776] == 5000 == by["all zero"]["n_zero"] and by["constant"]["counts"].max() == 5000
    assert by["nan and inf"]["n_nonfinite"] == 3 and by["half zeros"]["n_zero"] > 35000 and by["denormals"]["n_zero"] == 0
    # every float32 pair around a limit lands in the two buckets that limit separates
    c = by["bracketing"]["counts"]
    idx = np.searchsorted(kernel_case["limits"], kernel_case["inside"])           # the limit's own index i: below -> bucket i, above -> i + 1
    want = np.zeros_like(c)
    np.add.at(want, idx, 1)
    np.add.at(want, idx + 1, 1)
    assert np.array_equal(c, want)


def test_kernel_sums_are_within_the_summation_bound_and_reproducible(kernel_case):
    for (name, a, s), g, w in zip(kernel_case["segs"], kernel_case["got"], kernel_case["want"]):
        x = a[s]
        d = x[np.isfinite(x)].astype(np.float64)
        n = max(1, d.size)
        e1, b1 = abs(g["sum"] - w["sum"]), n * U * math.fsum(np.abs(d).tolist())
        e2, b2 = abs(g["sum_squares"] - w["sum_squares"]), n * U * math.fsum((d * d).tolist())
        print("%-16s n %8d  sum err %.3e bound %.3e   sum_squares err %.3e bound %.3e" % (name, d.size, e1, b1, e2, b2))
        assert e1 <= b1 and e2 <= b2, (name, e1, b1, e2, b2)
    assert kernel_case["raw"][0] == kernel_case["raw"][1]                        # two calls: identical bytes, sums included


def test_kernel_argument_checks(dev, kernel_case):
    import frcnn_hip
    from frcnn_hip import ops
    L = frcnn_hip.lib()
    views = kernel_case["views"][:3]
    plan = ops.SummaryPlan(views)
    P = ctypes.c_void_p
    st = P(torch.cuda.current_stream().cuda_stream)
    need = L.frcnn_summary_stats_workspace_bytes(3)
    assert need >= 3 * 64 * 32 and L.frcnn_summary_stats_workspace_bytes(-1) == 0
    assert L.frcnn_summary_stats(P(plan.table.data_ptr()), 3, P(plan.out.data_ptr()), P(plan.ws.data_ptr()), need - 1, st) == -2      # FRCNN_E_WS
    assert L.frcnn_summary_stats(None, 0, None, None, 0, st) == 0                                                                       # empty table
    assert L.frcnn_summary_stats(None, 3, P(plan.out.data_ptr()), P(plan.ws.data_ptr()), need, st) == -1
    assert L.frcnn_summary_stats(P(plan.table.data_ptr()), 65536, P(plan.out.data_ptr()), P(plan.ws.data_ptr()), need, st) == -1
    assert ops.summary_stats([]) == []
    torch.cuda.synchronize()


# ---- training ------------------------------------------------------------------------------------------------------------------------
def _blob(seed):
    from model.config import cfg
    rng = np.random.RandomState(seed)
    image = ((rng.rand(1, 128, 160, 3) * 255.0).astype(np.float32) - cfg.PIXEL_MEANS.astype(np.float32)) * np.float32(1 / 256.0)
    gt = np.array([[16, 16, 79, 79, 3], [60, 30, 150, 110, 7], [5, 70, 60, 120, 12]], dtype=np.float32)
    gt[:, :4] += seed % 3
    return dict(data=image, im_info=np.array([128, 160, 1.0], dtype=np.float32), gt_boxes=gt)


def _layer(seed):
    blobs = [_blob(seed), _blob(seed + 10)]
    i = 0
    while True:
        yield blobs[i % 2]
        i += 1


class _small_cfg(object):
    KEYS = ("BATCH_SIZE", "BG_THRESH_LO", "LEARNING_RATE", "SUMMARY_INTERVAL", "DISPLAY")

    def __enter__(self):
        from model.config import cfg
        self.old = [cfg.TRAIN[k] for k in self.KEYS]
        cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.BG_THRESH_LO, cfg.TRAIN.LEARNING_RATE, cfg.TRAIN.SUMMARY_INTERVAL, cfg.TRAIN.DISPLAY = 64, 0.0, 2e-4, 0, 1000

    def __exit__(self, *exc):
        from model.config import cfg
        for k, v in zip(self.KEYS, self.old):
            cfg.TRAIN[k] = v
        return False


def _solver(dev, tag, **kw):
    from frcnn_hip.runtime import Session
    from model.train_val import SolverWrapper
    from nets.resnet_v1 import resnetv1
    sess = Session(device=dev, seed=5)
    net = resnetv1(num_layers=50)
    net.create_architecture("TRAIN", 21, tag=tag, anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
    sess.init_variables(net.variable_specs())
    return sess, net, SolverWrapper(sess, net, _layer(2), **kw)


LOSSES = ("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box", "total_loss")


def test_summaries_at_every_step_change_no_bit_of_training(dev, tmp_path):
    tb = str(tmp_path / "tb")
    with _small_cfg():
        _, net_a, sw_a = _solver(dev, "tbA", tb_dir=tb, data_layer_val=_layer(31))
        hist_a = sw_a.train_model(6, verbose=False)
        sw_a.close_writers()
        state_a = sw_a.state.export_variables(slots=True)
        _, net_b, sw_b = _solver(dev, "tbA")
        hist_b = sw_b.train_model(6, verbose=False)
        state_b = sw_b.state.export_variables(slots=True)
    assert [np.float32(v).tobytes() for v in hist_a] == [np.float32(v).tobytes() for v in hist_b], (hist_a, hist_b)
    assert sorted(state_a) == sorted(state_b) and any(k.endswith("/Momentum") for k in state_a)
    for k in state_a:
        assert state_a[k].tobytes() == state_b[k].tobytes(), k
    assert net_a._sample_seed == net_b._sample_seed == 12
    assert net_a.replay_stats == net_b.replay_stats and net_a.replay_stats["replayed"] >= 3, (net_a.replay_stats, net_b.replay_stats)
    assert sw_b.writer is None

    (train_file,) = [os.path.join(tb, f) for f in os.listdir(tb)]
    (val_file,) = [os.path.join(tb + "_val", f) for f in os.listdir(tb + "_val")]
    ev = parse_events(train_file)
    assert ev[0].file_version == "brain.Event:2" and [e.step for e in ev[1:]] == [1, 2, 3, 4, 5, 6]
    for e in ev[1:]:
        tags = [v.tag for v in e.summary.value]
        assert len(tags) == len(set(tags))
        for group in ("ACT/", "SCORE/", "TRAIN/", "GROUND_TRUTH"):
            assert any(t.startswith(group) for t in tags), (group, tags[:12])
        assert set(LOSSES) <= set(tags)
        assert sum(t.endswith("/zero_fraction") for t in tags) == 2 == sum(t.endswith("/activations") for t in tags)
        for key in ("rpn_cls_score", "rpn_cls_prob", "rpn_bbox_pred", "cls_score", "cls_prob", "bbox_pred", "rois", "rpn_labels", "rpn_bbox_targets",
                    "labels", "bbox_targets", "bbox_inside_weights"):
            assert "SCORE/%s/scores" % key in tags, key
        assert "TRAIN/resnet_v1_50/block3/unit_1/bottleneck_v1/conv2/weights" in tags and "TRAIN/resnet_v1_50/cls_score/biases" in tags
        assert not any(t.startswith("TRAIN/resnet_v1_50/conv1/") for t in tags)             # the frozen stem is no trainable variable
    totals = [[v.simple_value for v in e.summary.value if v.tag == "total_loss"][0] for e in ev[1:]]
    assert [np.float32(v).tobytes() for v in totals] == [np.float32(v).tobytes() for v in hist_a]
    evv = parse_events(val_file)
    assert [e.step for e in evv[1:]] == [1, 2, 3, 4, 5, 6]
    for e in evv[1:]:
        tags = [v.tag for v in e.summary.value]
        assert set(LOSSES) <= set(tags) and any(t.startswith("GROUND_TRUTH") for t in tags) and len(tags) == 6
        assert all(np.isfinite(v.simple_value) for v in e.summary.value if v.tag in LOSSES)
    img = [v for v in evv[1].summary.value if v.tag.startswith("GROUND_TRUTH")][0].image
    assert (img.height, img.width, img.colorspace) == (128, 160, 3)


def test_summary_histograms_are_those_of_the_steps_own_tensors(dev):
    """A REPLAYED step's ACT/* and SCORE/* histograms against numpy histograms of the tensors an eager train_forward computes from the
    same weights, blob and sampling seed; TRAIN/* against the solver's master copies after the update."""
    from frcnn_hip import ops, summary
    with _small_cfg():
        sess, net, sw = _solver(dev, "tbC")
        sw.train_model(4, verbose=False)                                              # eager, recorded, replayed, replayed
        assert net.replay_stats["replayed"] >= 2
        blob = _blob(2)                                                               # the layer's 5th minibatch
        seed = net._sample_seed
        net.train_forward(sess, blob)
        want = {}
        for name, t in zip(("head", "rpn_conv/3x3"), net._act_summaries):
            want["ACT/resnet_v1_50/%s/activations" % name] = t.cpu().numpy()
        for d in (net._anchor_targets, net._proposal_targets, net._predictions):
            for k, t in d.items():
                if torch.is_tensor(t) and t.dtype == torch.float32:
                    want["SCORE/%s/scores" % k] = t.cpu().numpy()
        net._sample_seed = seed
        sw.state.lr = 2e-4
        before = dict(net.replay_stats)
        out = net.train_step_with_summary(sess, blob, sw.state)
        assert net.replay_stats["replayed"] == before["replayed"] + 1 and net._sample_seed == seed + 2
        params = {}
        for p in sw.state.params.values():
            params["TRAIN/%s/weights" % p.scope] = p.w.cpu().numpy()
            if p.bias is not None:
                params["TRAIN/%s/biases" % p.scope] = p.bias.cpu().numpy()
    assert len(out) == 6 and all(np.isfinite(out[:5]))
    e = event_class()()
    e.ParseFromString(summary.event(0.0, 5, summary=out[5]))
    values = {v.tag: v for v in e.summary.value}
    limits = ops.summary_limits()
    assert len(want) == 2 + 15                                                      # 4 anchor targets, 5 RoI targets, 7 predictions, `rois` shared
    want.update(params)
    for tag, x in want.items():
        st = summary.reference_stats(x, limits)
        h = values[tag].histo
        dense = expand_buckets(list(h.bucket_limit), list(h.bucket), limits)
        assert np.array_equal(dense, st["counts"]), tag
        assert (h.min, h.max, h.num) == (st["min"], st["max"], float(st["num"])), tag
        assert abs(h.sum - st["sum"]) <= x.size * U * math.fsum(np.abs(x.astype(np.float64)).reshape(-1).tolist()), tag
        if tag.startswith("ACT/"):
            zf = values[tag[:-len("activations")] + "zero_fraction"].simple_value
            assert np.float32(zf) == np.float32(st["n_zero"] / st["num"]) and 0.05 < zf < 0.95, (tag, zf)
    assert [np.float32(v).tobytes() for v in out[:5]] == [np.float32(values[k].simple_value).tobytes() for k in LOSSES]


def test_trainval_net_tool_trains_vgg16_and_writes_one_event_file(dev, tmp_path):
    tb = str(tmp_path / "tb")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools", "trainval_net.py"), "--net", "vgg16", "--imdb", "synthetic",
                        "--iters", "2", "--tbdir", tb], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    (name,) = os.listdir(tb)
    assert name.startswith("events.out.tfevents.") and not os.path.exists(tb + "_val")
    ev = parse_events(os.path.join(tb, name))
    assert ev[0].file_version == "brain.Event:2" and len(ev) >= 2 and ev[1].step == 1
    tags = [v.tag for v in ev[1].summary.value]
    assert "total_loss" in tags and "TRAIN/vgg_16/conv3/conv3_1/weights" in tags and "ACT/vgg_16/head/activations" in tags
