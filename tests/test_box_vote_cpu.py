"""CPU: bounding-box voting and the merge of two flip views on the host path -- frcnn_box_vote_host / frcnn_merge_flip_views_host
(csrc/boxvote_math.h) through ops.box_vote_host / ops.merge_flip_views_host -- against tests/golden/box_vote.npz and against the numpy
statement fixtures/box_vote_ref.py.  Both sides do the same IEEE operations in the same order (float32 IoU with one rounding per step,
sequential double sums in ascending candidate row, one double division, one rounding to float32), so every comparison is bit for bit.
Every equality test runs both thresholds and asserts that the vectors are not trivial: at 0.5, for n >= 63, more than half of the kept
detections have a second voter and at least one box changes its bits."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import box_vote_ref as ref  # noqa: E402
import gen_golden_box_vote as gen  # noqa: E402

SIZES = (1, 2, 63, 64, 65, 130, 300)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(gen.GOLD))


def assert_not_trivial(n, thresh, kept, out, voters):
    assert voters.min() >= 1
    if thresh == 0.5 and n >= 63:
        assert 2 * int((voters >= 2).sum()) > len(voters), (n, voters)
        assert out[:, :4].tobytes() != kept[:, :4].tobytes(), n


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("which", gen.LISTS)
def test_host_entry_equals_the_golden(gold, n, which):
    from frcnn_hip import ops
    assert tuple(gold["sizes"]) == SIZES
    cands, kept = gold["n%d/cands" % n], gold["n%d/%s/kept" % (n, which)]
    assert len(kept) == n or which == "hard"
    for tag, t in gen.THRESHOLDS:
        out = ops.box_vote_host(kept, cands, t)
        want, voters = gold["n%d/%s/t%d/out" % (n, which, tag)], gold["n%d/%s/t%d/voters" % (n, which, tag)]
        assert out.dtype == np.float32 and out.tobytes() == want.tobytes(), (n, which, tag)
        assert out[:, 4].tobytes() == kept[:, 4].tobytes()                                  # order and scores untouched
        assert_not_trivial(n, t, kept, out, voters)


def test_golden_is_what_the_numpy_statement_gives(gold):
    assert os.path.getsize(gen.GOLD) < 200 * 1024
    assert gen.compare(gen.generate(), gold) == []


@pytest.mark.parametrize("n", SIZES + (1024,))
def test_host_entry_equals_the_numpy_statement(n):
    """fresh boxes (another seed than the fixture's), kept lists from hard NMS under both rules and from Gaussian Soft-NMS with m = n"""
    from frcnn_hip import ops
    cands = ref.clustered(np.random.RandomState(500 + n), n)
    soft, sidx = ops.soft_nms_host(cands, 0.3, 0, 2, 0.5, 0.0)
    assert len(soft) == n
    for kept in (cands[ref.hard_nms(cands, 0.3, 0)], cands[ref.hard_nms(cands, 0.3, 1)], soft):
        for t in (0.8, 0.5):
            out = ops.box_vote_host(kept, cands, t)
            want, voters = ref.vote(kept, cands, t)
            assert out.tobytes() == want.tobytes(), (n, len(kept), t)
            assert out[:, 4].tobytes() == kept[:, 4].tobytes()
            assert np.array_equal(voters, ref.count_voters(kept, cands, t))
            assert_not_trivial(n, t, kept, out, voters)


def _grid(n, rng):
    """n distinct boxes of 51 x 51 on a grid of pitch 40 (neighbours overlap, no two share a box), scores in (0.01, 1)"""
    d = np.zeros((n, 5), dtype=np.float32)
    d[:, 0], d[:, 1] = (np.arange(n) % 16) * 40, (np.arange(n) // 16) * 40
    d[:, 2], d[:, 3] = d[:, 0] + 50, d[:, 1] + 50
    d[:, 4] = rng.uniform(0.01, 1, n).astype(np.float32)
    return d


def test_vote_thresh_one_returns_the_input_bits_on_duplicate_free_boxes():
    from frcnn_hip import ops
    for cands in (_grid(200, np.random.RandomState(1)), ref.clustered(np.random.RandomState(2), 300)):
        assert len(np.unique(cands[:, :4], axis=0)) == len(cands)
        for kept in (cands, cands[::-1], cands[ref.hard_nms(cands, 0.3)]):
            kept = np.ascontiguousarray(kept)
            assert ops.box_vote_host(kept, cands, 1.0).tobytes() == kept.tobytes()
    two = np.array([[10, 10, 50, 50, 0.75], [10, 10, 50, 50, 0.25], [10, 10, 50, 90, 0.5]], dtype=np.float32)
    assert ops.box_vote_host(two, two, 1.0).tobytes() == two.tobytes()                      # a shared box: the mean of equal values


def test_order_scores_and_the_weighted_mean():
    from frcnn_hip import ops
    pair = np.array([[0, 0, 99, 99, 0.75], [0, 0, 99, 79, 0.25]], dtype=np.float32)         # IoU 8000 / 10000
    out = ops.box_vote_host(pair[:1], pair, 0.8)
    assert out.tolist() == [[0.0, 0.0, 99.0, 94.0, 0.75]]                                   # (0.75 * 99 + 0.25 * 79) / 1
    assert ops.box_vote_host(pair[:1], pair, 0.81).tobytes() == pair[:1].tobytes()
    out = ops.box_vote_host(pair[::-1].copy(), pair, 0.8)                                   # the kept order is the output order
    assert out[:, 4].tolist() == [0.25, 0.75] and out[0, :4].tolist() == out[1, :4].tolist() == [0.0, 0.0, 99.0, 94.0]
    far = np.array([[5000, 5000, 5100, 5100, 0.5]], dtype=np.float32)                       # no voter at all: the row stays
    assert ops.box_vote_host(far, pair, 0.5).tobytes() == far.tobytes()
    assert ops.box_vote_host(np.zeros((0, 5), np.float32), pair, 0.5).shape == (0, 5)
    assert ops.box_vote_host(far, np.zeros((0, 5), np.float32), 0.5).tobytes() == far.tobytes()


def _views(rng, B, R, C, width=800.0):
    rows = 2 * B * R
    rois = np.zeros((rows, 5), dtype=np.float32)
    rois[:, 0] = np.arange(rows) // R
    rois[:, 1], rois[:, 2] = rng.uniform(0, width - 200, rows), rng.uniform(0, 400, rows)
    rois[:, 3], rois[:, 4] = rois[:, 1] + rng.uniform(1, 199, rows), rois[:, 2] + rng.uniform(1, 199, rows)
    return rng.uniform(0, 1, (rows, C)).astype(np.float32), (rng.randn(rows, 4 * C) * 0.1).astype(np.float32), rois


@pytest.mark.parametrize("B,R,C,nums", [(1, 1, 2, ([1, 1], [1, 0], [0, 1], [0, 0])), (2, 48, 3, ([48, 48, 48, 48], [0, 31, 17, 0], [48, 0, 0, 48])),
                                        (1, 512, 3, ([512, 512], [500, 7])), (2, 5, 21, ([-3, 9, 2, 5], None))])
def test_merge_host_twin_equals_the_numpy_statement(B, R, C, nums):
    from frcnn_hip import ops
    prob, pred, rois = _views(np.random.RandomState(B * 1000 + R), B, R, C)
    pred[0, 0] = 0.0                                                                        # -0.0 where a mirrored dx is 0
    for num in nums:
        for bp in (pred, None):
            got = ops.merge_flip_views_host(prob, bp, rois, num, 800.0, batch=B)
            want = ref.merge_flip_views(prob, bp, rois, num, 800.0, B)
            for g, w, name in zip(got, want, ("cls_prob", "bbox_pred", "rois", "num_rois")):
                assert (g is None and w is None) if (bp is None and name == "bbox_pred") else \
                    (g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()), (num, name)
            n0 = R if num is None else min(max(num[0], 0), R)
            n1 = R if num is None else min(max(num[1], 0), R)
            assert got[3][0] == n0 + n1 and not got[0][n0 + n1:2 * R].any() and not got[2][n0 + n1:2 * R].any()
            assert got[0][:n0].tobytes() == prob[:n0].tobytes() and got[2][:n0].tobytes() == rois[:n0].tobytes()
            if n1:
                assert np.array_equal(got[2][n0:n0 + n1, 1], np.float32(799) - rois[R:R + n1, 3])
                assert bp is None or np.array_equal(got[1][n0:n0 + n1, 4::4], -pred[R:R + n1, 4::4])


def test_error_codes():
    import frcnn_hip
    L = frcnn_hip.lib()
    E_ARG, E_UNSUPPORTED = -1, -3
    d = np.ascontiguousarray(ref.clustered(np.random.RandomState(2), 8))
    big = np.zeros((1025, 5), dtype=np.float32)
    out = np.full((1025, 5), 7, dtype=np.float32)

    def run(kept=d, m=8, cands=d, n=8, t=0.5, o=out):
        return L.frcnn_box_vote_host(None if kept is None else kept.ctypes.data, m, None if cands is None else cands.ctypes.data, n, t,
                                     None if o is None else o.ctypes.data)
    assert run() == 0 and not (out[:8] == 7).any()
    out[:] = 7
    for kw in (dict(t=0.0), dict(t=-0.5), dict(t=1.0000001), dict(t=float("nan")), dict(t=float("inf")), dict(kept=None), dict(cands=None),
               dict(o=None), dict(m=-1), dict(n=-1)):
        assert run(**kw) == E_ARG, kw
    assert run(kept=big, m=1025) == E_UNSUPPORTED and run(cands=big, n=1025) == E_UNSUPPORTED
    assert run(kept=big, m=1025, t=2.0) == E_ARG                                            # the argument check comes first
    assert (out == 7).all()                                                                 # nothing was written
    assert run(t=1.0) == 0 and run(kept=big, m=1024, cands=big, n=1024) == 0
    # the device entries refuse the same arguments before they launch anything (no GPU is touched)
    p = ctypes.c_void_p(64)

    def post(t=0.8, method=0, rule=0, sigma=0.5, min_score=0.001, R=8, cls=p, rois=p, o=p, cnt=p, ws=p):
        return L.frcnn_detect_post_vote_batched(cls, p, rois, None, 1, R, 3, 1.0, 100, 100, 0.3, rule, 0.0, 100, method, sigma, min_score, t,
                                                o, cnt, 128, 0, ws, 1 << 30, None)
    for kw in (dict(t=0.0), dict(t=-1.0), dict(t=1.5), dict(t=float("nan")), dict(method=3), dict(method=-1), dict(rule=2), dict(method=2, sigma=0.0),
               dict(method=1, min_score=float("nan")), dict(cls=None), dict(rois=None), dict(o=None), dict(cnt=None), dict(ws=None)):
        assert post(**kw) == E_ARG, kw
    assert post(R=1025) == E_UNSUPPORTED and post(R=1025, method=2) == E_UNSUPPORTED and post(R=1025, t=0.0) == E_ARG
    for t in (0.0, 1.5, float("nan")):
        assert L.frcnn_box_vote(p, 8, p, 8, t, p, None) == E_ARG
    assert L.frcnn_box_vote(None, 8, p, 8, 0.5, p, None) == E_ARG and L.frcnn_box_vote(p, 8, p, 8, 0.5, None, None) == E_ARG
    assert L.frcnn_box_vote(p, 1025, p, 8, 0.5, p, None) == E_UNSUPPORTED and L.frcnn_box_vote(p, 8, p, 1025, 0.5, p, None) == E_UNSUPPORTED
    assert L.frcnn_detect_post_vote_batched_workspace_bytes(2, 300, 21) == L.frcnn_detect_post_batched_workspace_bytes(2, 300, 21)
    for fn, tail in ((L.frcnn_merge_flip_views, (None,)), (L.frcnn_merge_flip_views_host, ())):
        assert fn(None, p, p, p, 1, 8, 3, 800.0, p, p, p, p, *tail) == E_ARG
        assert fn(p, p, None, p, 1, 8, 3, 800.0, p, p, p, p, *tail) == E_ARG
        assert fn(p, p, p, p, 1, 8, 3, 800.0, p, None, p, p, *tail) == E_ARG                # bbox_pred without a place for it
        assert fn(p, p, p, p, 1, 8, 3, 800.0, p, p, p, None, *tail) == E_ARG
        assert fn(p, p, p, p, 0, 8, 3, 800.0, p, p, p, p, *tail) == E_ARG
        assert fn(p, p, p, p, 1, 0, 3, 800.0, p, p, p, p, *tail) == E_ARG
        assert fn(p, p, p, p, 1, 8, 1, 800.0, p, p, p, p, *tail) == E_ARG
        assert fn(p, p, p, p, 1, 8, 3, 0.0, p, p, p, p, *tail) == E_ARG
    assert L.frcnn_mirror_views(None, 1, 8, 8, 4, p, None) == E_ARG and L.frcnn_mirror_views(p, 1, 8, 8, 4, None, None) == E_ARG
    assert L.frcnn_mirror_views(p, 0, 8, 8, 4, p, None) == E_ARG and L.frcnn_mirror_views(p, 1, 8, 0, 4, p, None) == E_ARG


def test_cfg_keys_defaults_and_refusals():
    from model.config import cfg
    from nets.network import Network
    assert (cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.HIP.BBOX_VOTE_THRESH) == (False, False, 0.8)
    Network._check_supported_cfg("TEST")
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        old, cfg.HIP.BBOX_VOTE_THRESH = cfg.HIP.BBOX_VOTE_THRESH, bad
        try:
            with pytest.raises(NotImplementedError, match="BBOX_VOTE_THRESH"):
                Network._check_supported_cfg("TEST")
        finally:
            cfg.HIP.BBOX_VOTE_THRESH = old
    for good in (1.0, 0.5, 1e-3):
        old, cfg.HIP.BBOX_VOTE_THRESH = cfg.HIP.BBOX_VOTE_THRESH, good
        try:
            Network._check_supported_cfg("TEST")
        finally:
            cfg.HIP.BBOX_VOTE_THRESH = old
    old = (cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.TEST.MODE)
    try:
        cfg.HIP.TEST_FLIP = cfg.HIP.BBOX_VOTE = True
        assert cfg.TEST.RPN_POST_NMS_TOP_N == 300
        Network._check_supported_cfg("TEST")                                                # 300 proposals: 600 rows
        cfg.TEST.RPN_POST_NMS_TOP_N = 512
        Network._check_supported_cfg("TEST")                                                # exactly 1024 rows
        for top_n in (513, 1000):
            cfg.TEST.RPN_POST_NMS_TOP_N = top_n
            with pytest.raises(NotImplementedError, match="TEST_FLIP.*1024"):                # refused, not truncated; the limit is named
                Network._check_supported_cfg("TEST")
        cfg.HIP.TEST_FLIP = False
        Network._check_supported_cfg("TEST")                                                # 1000 proposals without the flip: as before
        cfg.HIP.TEST_FLIP, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.TEST.MODE = True, 300, "top"
        with pytest.raises(NotImplementedError, match="TEST_FLIP.*top"):
            Network._check_supported_cfg("TEST")
    finally:
        cfg.HIP.TEST_FLIP, cfg.HIP.BBOX_VOTE, cfg.TEST.RPN_POST_NMS_TOP_N, cfg.TEST.MODE = old


def test_python_front_ends_without_a_gpu():
    from frcnn_hip import ops, replay
    sig = inspect.signature(ops.detect_post)
    assert sig.parameters["vote"].default == 0.0 and list(sig.parameters)[-1] == "vote"
    for name in ("box_vote", "box_vote_host", "merge_flip_views", "merge_flip_views_host", "mirror_views"):
        assert callable(getattr(ops, name)), name
    assert inspect.signature(ops.box_vote).parameters["vote_thresh"].default == 0.8
    assert {"frcnn_box_vote_host", "frcnn_merge_flip_views_host"} <= set(replay.HOST_ONLY)
    assert not {"frcnn_box_vote", "frcnn_merge_flip_views", "frcnn_mirror_views", "frcnn_detect_post_vote_batched"} & set(replay.HOST_ONLY)
    with pytest.raises(ValueError):
        ops.merge_flip_views_host(np.zeros((7, 3), np.float32), None, np.zeros((7, 5), np.float32), None, 800.0, batch=1)
    sys.path.insert(0, os.path.join(ROOT, "tf-faster-rcnn_amd", "tools"))
    import demo
    a = demo.parse_args(["--images", "a.jpg", "--flip", "--vote"])
    assert a.flip is True and a.vote == 0.8
    a = demo.parse_args(["--images", "a.jpg", "--vote", "0.6"])
    assert a.flip is False and a.vote == 0.6
    a = demo.parse_args(["--images", "a.jpg"])
    assert a.flip is False and a.vote is None
