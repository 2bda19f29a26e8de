"""GPU: proposal recall on the device -- frcnn_proposal_recall against tests/golden/recall.npz (the REFERENCE's own imdb.evaluate_recall
on the same inputs, fixtures/gen_golden_recall.py) bit for bit; Network.propose_device against forward_device; tools/rpn_recall.py at
TEST_BATCH_IMAGES 1 and 4, with and without the device JPEG decoder, and imdb.evaluate_recall reproducing its lines from its own pickle.
Reads only the golden file, never the reference tree."""
import contextlib
import io
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fixtures"), os.path.join(ROOT, "tf-faster-rcnn_amd", "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import recall_golden as rg  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ("hand", "empty", "large", "ties", "areas", "few", "scale16", "scale600", "many")
POISON = -12345.0


@pytest.fixture(scope="module")
def cases():
    return rg.load()


def launch(dev, cands, gts, limit=None, stride=4, scale=1.0, lead_gt=0):
    """one frcnn_proposal_recall launch with every output inside a larger poisoned buffer and the counts inside a larger poisoned array;
    lead_gt: that many unrelated gt rows in front, so gt_off[0] > 0.  -> (slots [n_gt] numpy incl. the leading ones, flags, pack)"""
    from datasets import recall
    from frcnn_hip import ops
    p = recall.pack(cands, gts, limit)
    boxes = p["boxes"]
    if stride == 5:
        boxes = np.concatenate([np.full((boxes.shape[0], 1), 99.0, dtype=np.float32), boxes], axis=1)
    gt = np.concatenate([np.full((lead_gt, 4), 3.0), p["gt"]])
    n_gt, n_img, pad = gt.shape[0], len(cands), 64
    big_out = torch.full((n_gt + 2 * pad,), POISON, dtype=torch.float64, device=dev)
    big_flag = torch.full((n_img + 2 * pad,), 77, dtype=torch.int32, device=dev)
    big_count = torch.full((n_img + 2 * pad,), 1 << 30, dtype=torch.int32, device=dev)           # a count read one slot off would be huge
    big_count[pad:pad + n_img] = torch.from_numpy(p["count"]).to(dev)
    out, flag, count = big_out[pad:pad + n_gt], big_flag[pad:pad + n_img], big_count[pad:pad + n_img]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = ops.proposal_recall(up(boxes), up(p["start"]), count, up(np.full(n_img, scale, dtype=np.float32)), up(gt), up(p["gt_off"] + lead_gt),
                              p["max_boxes"], limit, out=out, ran_out=flag)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is flag
    for big, n, v in ((big_out, n_gt, POISON), (big_flag, n_img, 77)):
        assert bool((big[:pad] == v).all()) and bool((big[pad + n:] == v).all()), "written outside the outputs"
    assert bool((out[:lead_gt] == POISON).all()), "written in front of gt_off[0]"
    return out.cpu().numpy(), flag.cpu().numpy(), p


def per_image(slots, p, lead_gt=0):
    off = p["gt_off"] + lead_gt
    return [slots[off[i]:off[i + 1]] for i in range(len(p["count"]))]


def check_run(case, run, slots, flags, p, lead_gt=0):
    from datasets import recall
    rows = per_image(slots, p, lead_gt)
    if run.raised:
        assert flags.any()
        for r, f, n, in zip(rows, flags, p["count"]):
            if f:                                          # the picks while candidates lasted, then -1.0 and nothing else
                n = n if run.limit is None else min(n, run.limit)
                assert np.all(r[:n] >= 0) and np.all(r[n:] == -1.0) and n < len(r)
        return
    assert not flags.any()
    kept = []
    for i, r in enumerate(rows):
        if p["count"][i] == 0:
            assert np.all(r == POISON), "an image without candidates writes nothing"
            assert len(run.per_image[i]) == 0
            continue
        assert np.all(np.diff(r) <= 0), "the picks of one image are non-increasing"
        assert rg.same(np.sort(r), run.per_image[i]), (case.name, i)
        kept.append(r)
    res = recall.summarise(np.concatenate(kept + [np.zeros(0)]), int(p["gt_off"][-1]))
    assert int(p["gt_off"][-1]) == run.num_pos
    for k in ("gt_overlaps", "recalls", "ar"):
        assert rg.same(res[k], getattr(run, k)), (case.name, run.area, run.limit, k)


@pytest.mark.parametrize("name", CASES)
def test_device_matcher_equals_the_reference(dev, cases, name):
    case = cases[name]
    for run in case.runs:
        if not run.use_cand:
            continue
        slots, flags, p = launch(dev, case.cands, case.gts(run.area), run.limit)
        check_run(case, run, slots, flags, p)
        slots5, flags5, _ = launch(dev, case.cands, case.gts(run.area), run.limit, stride=5, lead_gt=3)
        assert np.array_equal(slots5[3:], slots) and np.array_equal(flags5, flags), "stride 5 / an offset start: other bits"
        again, flags2, _ = launch(dev, case.cands, case.gts(run.area), run.limit)
        assert again.tobytes() == slots.tobytes() and np.array_equal(flags2, flags), "two runs differ"


@pytest.mark.parametrize("name", ("scale16", "scale600"))
def test_device_division_by_the_scale(dev, cases, name):
    """the candidates as rois = boxes * s, stride 5, scale s: the kernel's own float32 division gives the reference's rois / s"""
    case = cases[name]
    for run in case.runs:
        slots, flags, p = launch(dev, [case.rois[0][:, 1:]], case.gts(), run.limit, stride=5, scale=float(case.scale))
        check_run(case, run, slots, flags, p)
    assert not rg.same(case.runs[0].gt_overlaps, cases["large"].runs[0].gt_overlaps)


def test_cases_together_in_one_launch_equal_the_cases_alone(dev, cases):
    names = ("hand", "empty", "large", "ties", "areas")
    cands = [c for n in names for c in cases[n].cands]
    gts = [g for n in names for g in cases[n].gts()]
    slots, flags, p = launch(dev, cands, gts)
    rows, k = per_image(slots, p), 0
    for n in names:
        alone, alone_flags, q = launch(dev, cases[n].cands, cases[n].gts())
        for r, f in zip(per_image(alone, q), alone_flags):
            assert rows[k].tobytes() == r.tobytes() and flags[k] == f, (n, k)
            k += 1
    assert k == len(cands) == 7


def test_evaluate_recall_on_the_device_path(dev, cases):
    from datasets.imdb import imdb
    for name in ("empty", "areas"):
        case = cases[name]
        db = imdb("toy", ["__background__", "c1", "c2", "c3"])
        db._image_index, db._roidb = list(range(len(case.entries))), case.roidb()
        for run in case.runs:
            kw = dict(candidate_boxes=case.cands if run.use_cand else None, area=run.area, limit=run.limit)
            if run.raised:
                with pytest.raises(AssertionError):
                    db.evaluate_recall(**kw)
                continue
            res = db.evaluate_recall(**kw)
            for k in res:
                assert rg.same(res[k], getattr(run, k)), (name, run.area, run.use_cand, k)


# ---- propose_device against forward_device -----------------------------------------------------------------------------------------------
def _net(dev, kind, tag):
    from frcnn_hip.runtime import Session
    from nets.resnet_v1 import resnetv1
    from nets.vgg16 import vgg16
    sess = Session(device=dev, seed=9)
    net = resnetv1(num_layers=50) if kind == "res50" else vgg16()
    net.create_architecture("TEST", 21, tag=tag, anchor_scales=(4, 8, 16), anchor_ratios=(0.5, 1, 2))
    sess.init_variables(net.variable_specs())
    return sess, net


@pytest.fixture(scope="module")
def res50(dev):
    sess, net = _net(dev, "res50", "recall_res50")
    yield sess, net
    sess.close()


@pytest.fixture(scope="module")
def vgg(dev):
    sess, net = _net(dev, "vgg16", "recall_vgg16")
    yield sess, net
    sess.close()


@pytest.mark.parametrize("kind", ["res50", "vgg16"])
def test_propose_device_equals_forward_device(dev, res50, vgg, kind):
    sess, net = res50 if kind == "res50" else vgg
    for (h, w) in ((120, 160), (96, 160)):
        for B in (1, 3):
            rng = np.random.RandomState(h + B)
            image = torch.from_numpy((rng.rand(B, h, w, 3) * 255 - 110).astype(np.float32))
            im_info = np.array([h, w, 1.0], dtype=np.float32)
            img = net._stage_image(sess, image, im_info)

            def forward():
                p = net.forward_device(sess, img, im_info)
                with net.shape_scope(sess, img.shape, im_info):          # the proposal layer's score buffer of THIS shape
                    sc = sess.buf(net._tag + "/roi_scores", (B * net._rois_per_image, 1))
                torch.cuda.synchronize()
                return {k: v.clone() for k, v in p.items()}, sc.clone(), net._num_rois.clone()
            before, sc0, num0 = forward()
            rois, scores, num = net.propose_device(sess, img, im_info)
            torch.cuda.synchronize()
            assert rois.shape == before["rois"].shape and rois.shape[1] == 5 and num.shape == (B,) and num.dtype == torch.int32
            assert torch.equal(rois, before["rois"]) and torch.equal(scores, sc0) and torch.equal(num, num0), (kind, h, w, B)
            assert int(num.min()) > 0
            rois_c, scores_c, num_c = rois.clone(), scores.clone(), num.clone()
            after, sc1, num1 = forward()                   # the captured chain still returns what it returned before
            assert sorted(after) == sorted(before)
            for k in before:
                assert torch.equal(after[k], before[k]), (kind, h, w, B, k)
            assert torch.equal(sc1, sc0) and torch.equal(num1, num0)
            r2, s2, n2 = net.propose_device(sess, img, im_info)          # and propose_device after a replay gives its bits again
            torch.cuda.synchronize()
            assert torch.equal(r2, rois_c) and torch.equal(s2, scores_c) and torch.equal(n2, num_c)
            key = ("propose",) + net.graph_key(img.shape, im_info)
            assert key in sess.graphs and net.graph_key(img.shape, im_info) in sess.graphs           # its own key beside forward_device's
            r3, s3, n3 = net.propose_device(sess, img, im_info, use_graph=False)                     # the eager launches: the same bits
            torch.cuda.synchronize()
            assert torch.equal(r3, rois_c) and torch.equal(s3, scores_c) and torch.equal(n3, num_c)
            again, _, _ = forward()
            assert all(torch.equal(again[k], before[k]) for k in before)


def test_the_two_captured_chains_of_a_shape_name_one_scope_and_leave_together(dev):
    """forward_device and propose_device of one shape each keep an entry in sess.graphs (replay.CapturedGraph), under their own keys and
    naming the same shape scope: drop_scope of that key removes both, running them again captures afresh and gives the bits from before
    the drop, and with one shape cached a second shape evicts the first one's two entries together.  (A session of its own at the toy
    size of tests/test_streaming_shapes_gpu.py: the test above shares its sessions and shapes with the rest of this module.)"""
    from frcnn_hip import replay
    from model.config import cfg
    old = (cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.GRAPH_CACHE_SHAPES)
    cfg.TEST.RPN_POST_NMS_TOP_N = 48
    sess, net = _net(dev, "res50", "recall_scope")

    def both(h, w):
        rng = np.random.RandomState(h + w)
        image = torch.from_numpy((rng.rand(1, h, w, 3) * 255 - 110).astype(np.float32))
        im_info = np.array([h, w, 1.0], dtype=np.float32)
        img = net._stage_image(sess, image, im_info)
        p = net.forward_device(sess, img, im_info)
        torch.cuda.synchronize()
        out = [p[k].clone() for k in sorted(p)] + [net._num_rois.clone()]
        out += [t.clone() for t in net.propose_device(sess, img, im_info)]
        torch.cuda.synchronize()
        return net.graph_key(img.shape, im_info), out
    try:
        key, first = both(112, 144)
        fwd, prop = sess.graphs[key], sess.graphs[("propose",) + key]
        assert type(fwd) is type(prop) is replay.CapturedGraph and fwd.scope == prop.scope == key and fwd.graph is not prop.graph
        assert set(sess.graphs) == {key, ("propose",) + key} and list(sess.scopes) == [key] and int(first[-1].min()) > 0
        assert sess.drop_scope(key) and sess.graphs == {} and key not in sess.scopes
        key2, again = both(112, 144)
        assert key2 == key and set(sess.graphs) == {key, ("propose",) + key}
        assert sess.graphs[key].graph is not fwd.graph and sess.graphs[("propose",) + key].graph is not prop.graph      # captured afresh
        assert len(again) == len(first) and all(torch.equal(a, b) for a, b in zip(again, first))
        cfg.HIP.GRAPH_CACHE_SHAPES = 1
        other, _ = both(120, 160)
        assert other != key and set(sess.graphs) == {other, ("propose",) + other} and list(sess.scopes) == [other]
        assert sess.graphs[other].scope == sess.graphs[("propose",) + other].scope == other
    finally:
        cfg.TEST.RPN_POST_NMS_TOP_N, cfg.HIP.GRAPH_CACHE_SHAPES = old
        sess.close()


# ---- tools/rpn_recall.py on a toy devkit ------------------------------------------------------------------------------------------------
def test_rpn_recall_tool_batches_and_decoders_agree_and_evaluate_recall_reproduces_it(dev, res50, tmp_path, monkeypatch):
    import rpn_recall
    import test_batched_imdb_gpu as tb
    from datasets.factory import get_imdb
    from model.config import cfg
    data_dir = str(tmp_path / "data")
    tb.build_devkit(data_dir, "test", tb.SIZES, seed=41)
    limits = [1000, 300, 20]
    old = (cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES, cfg.TEST.RPN_POST_NMS_TOP_N)
    cfg.DATA_DIR, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE = data_dir, (120,), 160
    runs = {}
    try:
        for jpeg_device in (False, True):
            for batch in (1, 4):
                cfg.HIP.JPEG_DEVICE, cfg.HIP.TEST_BATCH_IMAGES = jpeg_device, batch
                out = str(tmp_path / ("out_%d_%d" % (jpeg_device, batch)))
                log = io.StringIO()
                with contextlib.redirect_stdout(log):
                    rc = rpn_recall.main(["--imdb", "voc_2007_test", "--limits"] + [str(v) for v in limits] +
                                         ["--areas", "all", "small", "medium", "large", "--out", out, "--save-proposals"], network=res50)
                assert rc == 0 and cfg.TEST.RPN_POST_NMS_TOP_N == old[5]
                with open(os.path.join(out, "recall.json")) as f:
                    js = json.load(f)
                with open(os.path.join(out, "proposals.pkl"), "rb") as f:
                    props = pickle.load(f)
                lines = [l for l in log.getvalue().splitlines() if l.startswith("limit ")]
                assert len(lines) == len(limits) * 4 == len(js["results"])
                runs[jpeg_device, batch] = (js, props, lines)
    finally:
        cfg.DATA_DIR, cfg.HIP.JPEG_DEVICE, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE, cfg.HIP.TEST_BATCH_IMAGES, cfg.TEST.RPN_POST_NMS_TOP_N = old
    for jpeg_device in (False, True):
        (js1, p1, l1), (js4, p4, l4) = runs[jpeg_device, 1], runs[jpeg_device, 4]
        assert js1 == js4 and l1 == l4, "TEST_BATCH_IMAGES 1 and 4 differ"
        assert len(p1) == len(p4) == len(tb.SIZES)
        for a, b in zip(p1, p4):
            assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.shape[1] == 4 and np.array_equal(a, b)
        assert sum(len(a) for a in p1) > 0

    # imdb.evaluate_recall from the tool's own pickle reproduces every line, on the device path and on the host path
    js, props, _ = runs[True, 4]
    cfg.DATA_DIR = data_dir
    try:
        imdb = get_imdb("voc_2007_test")
        for host in (False, True):
            if host:
                monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
            for r in js["results"]:
                res = imdb.evaluate_recall(candidate_boxes=props, area=r["area"], limit=r["limit"])
                assert rg.same(res["recalls"], r["recalls"]) and rg.same(res["ar"], r["ar"]), (host, r["limit"], r["area"])
                assert rg.same(res["thresholds"], r["thresholds"])
    finally:
        cfg.DATA_DIR = old[0]
    assert {r["num_pos"] for r in js["results"] if r["area"] == "all"} == {sum(1 + i % 2 for i in range(len(tb.SIZES)))}
