"""GPU: the ordering machinery of csrc/detect_kernels.hip (proposal side) and csrc/detect_post.hip (per class, final cut) -- make_key, k_select_topk, k_rank / k_scatter_sorted, the rank sort of
k_perclass_nms, k_final_select -- under tied, saturated and non-finite scores (oracle/score_cases.py), through every entry point
that sorts or cuts: the proposal layers, the NMS entry points and detect_post.

Everything is compared with oracle/frcnn_oracle.py and with nothing else -- never with a golden recorded from the reference: the
reference's order among equal scores is whatever numpy's introsort leaves, while this project states (score descending, index
ascending; -0.0 == +0.0; every NaN above +inf and all NaNs equal -- include/frcnn_hip.h at frcnn_nms).  Every comparison is exact
(counts, keep lists, score bits, roi bits, zero-filled tails, sentinels); the one exception is the `overflow` case's coordinates,
whose deltas are not zero and which are held to the 2-ulp box_tol that tests/test_detect_gpu.py asserts.  Outputs start as NaN
inside a larger buffer whose sentinel tail must survive.  tests/test_select_cpu.py shows on the CPU which planted mistake each
case is there to catch."""
import numpy as np
import pytest
import torch

import frcnn_oracle as ora
import score_cases as sc
import select_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = 12345.5
ISENT = -77
PAD = 256
CASES = sc.cases()
POST = 300


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Guard:
    """float32 outputs of the given sizes laid out in ONE buffer, each filled with NaN and followed by PAD sentinel floats"""

    def __init__(self, dev, *shapes):
        sizes = [int(np.prod(s)) for s in shapes]
        self.buf = torch.full((sum(sizes) + PAD * len(sizes),), SENT, dtype=torch.float32, device=dev)
        self.views, self.pads, off = [], [], 0
        for s, n in zip(shapes, sizes):
            self.buf[off:off + n] = float("nan")
            self.views.append(self.buf[off:off + n].view(*s))
            self.pads.append((off + n, off + n + PAD))
            off += n + PAD

    def intact(self):
        h = self.buf.cpu().numpy()
        return all(bool((h[a:b] == f32(SENT)).all()) for a, b in self.pads)


def iguard(dev, n):
    """int32 [n] filled with a sentinel in front of PAD more"""
    buf = torch.full((n + PAD,), ISENT, dtype=torch.int32, device=dev)
    return buf, buf[:n]


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_rows(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope="module")
def base_d(dev):
    from frcnn_hip import ops
    return T(ops.generate_anchors(16), dev)


_ANCHORS = {}


def anchors_of(H, W):
    if (H, W) not in _ANCHORS:
        _ANCHORS[(H, W)] = ora.generate_anchors_pre(H, W, sc.FEAT_STRIDE)[0]
    return _ANCHORS[(H, W)]


def run_proposal(dev, base_d, prob_d, deltas_d, H, W, pre, post=POST):
    from frcnn_hip import ops
    g = Guard(dev, (post, 5), (post, 1))
    nbuf, num = iguard(dev, 1)
    ops.proposal_layer(prob_d, deltas_d, H * 16, W * 16, 16, base_d, pre, post, 0.7, rois=g.views[0], scores=g.views[1], num=num)
    assert g.intact() and bool((nbuf[1:] == ISENT).all())
    return g.views[0].cpu().numpy(), g.views[1].cpu().numpy(), int(num.item())


def check_proposal(got, want, what, exact_boxes=True):
    rois, scores, n = got
    wr, ws = want
    assert n == wr.shape[0], what
    assert ref.same_scores(scores[:n], ws), what
    if exact_boxes:
        assert same_rows(rois[:n], wr), what
    else:
        assert np.array_equal(rois[:n, 0], wr[:, 0]) and np.isfinite(rois[:n]).all(), what
        assert np.all(np.abs(rois[:n].astype(np.float64) - wr.astype(np.float64)) <= sc.box_tol(wr)), what
    assert not bits(rois[n:]).any() and not bits(scores[n:]).any(), what + ": the tail is not zero"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_proposal_layers_on_tied_and_saturated_scores(dev, base_d, case):
    """proposal_layer (TEST and TRAIN keys of the oracle, pre = every K of the case, post 300), proposal_top_layer (every K <= N) and
    proposal_layer_tf: count, score bits, roi bits, zero tails, sentinels."""
    from frcnn_hip import ops
    H, W, N = case.H, case.W, case.N
    prob, deltas, info, anchors = sc.prob_blob(case.scores, H, W), sc.zero_deltas(H, W), sc.im_info(H, W), anchors_of(H, W)
    prob_d, deltas_d = T(prob, dev), T(deltas, dev)
    for K in case.ks:
        got = run_proposal(dev, base_d, prob_d, deltas_d, H, W, K)
        for key in ("TEST", "TRAIN"):
            want = ora.proposal_layer(prob, deltas, info, key, 16, anchors, sc.A, K, POST, 0.7)
            check_proposal(got, want, "%s proposal_layer %s pre=%d" % (case.name, key, K))
        if K <= N:
            g = Guard(dev, (K, 5), (K, 1))
            ops.proposal_top_layer(prob_d, deltas_d, H * 16, W * 16, 16, base_d, K, rois=g.views[0], scores=g.views[1])
            wr, ws = ora.proposal_top_layer(prob, deltas, info, 16, anchors, sc.A, K)
            what = "%s proposal_top_layer top_n=%d" % (case.name, K)
            assert g.intact(), what
            assert ref.same_scores(g.views[1].cpu().numpy(), ws) and same_rows(g.views[0].cpu().numpy(), wr), what
    base_tf = np.trunc(ops.generate_anchors(16))
    anc_tf, _ = ora.generate_anchors_pre_tf(H, W, 16)
    g = Guard(dev, (POST, 5), (POST, 1))
    nbuf, num = iguard(dev, 1)
    ops.proposal_layer_tf(prob_d, deltas_d, H * 16, W * 16, 16, T(base_tf, dev), POST, 0.7, rois=g.views[0], scores=g.views[1], num=num)
    assert g.intact() and bool((nbuf[1:] == ISENT).all())
    want = ora.proposal_layer_tf(prob, deltas, info, anc_tf, sc.A, POST, 0.7)
    check_proposal((g.views[0].cpu().numpy(), g.views[1].cpu().numpy(), int(num.item())), want, case.name + " proposal_layer_tf")


def test_proposal_layer_overflowing_deltas(dev, base_d):
    """dw, dh of +89 / +100 / -100 / -104 and dx = +-1e30: inf and zero widths before the clip.  Scores are tie-free; the count and
    the score bits are exact, the coordinates are finite and within box_tol (the existing 2-ulp bound)."""
    case, deltas = sc.overflow()
    H, W = case.H, case.W
    prob, info, anchors = sc.prob_blob(case.scores, H, W), sc.im_info(H, W), anchors_of(H, W)
    prob_d, deltas_d = T(prob, dev), T(deltas, dev)
    for K in case.ks:
        with np.errstate(over="ignore"):
            want = ora.proposal_layer(prob, deltas, info, "TEST", 16, anchors, sc.A, K, POST, 0.7)
        assert np.isfinite(want[0]).all()
        check_proposal(run_proposal(dev, base_d, prob_d, deltas_d, H, W, K), want, "overflow pre=%d" % K, exact_boxes=False)


@pytest.mark.parametrize("N,K", [(9207, 6000), (4104, 2000)])
def test_batched_launch_equals_single_images(dev, base_d, N, K):
    """B = 3 images with DIFFERENT distributions (constant, trained, bucket_4097) in one launch: every slot equals its own
    single-image call bit for bit -- the select state is per workgroup and nothing leaks through the shared scratch."""
    from frcnn_hip import ops
    H, W = sc.MAPS[N]
    names = ("constant", "trained", "bucket_4097")
    probs = [sc.prob_blob(sc.case("%s_%d" % (d, N)).scores, H, W) for d in names]
    deltas_d = T(np.zeros((3, H, W, 4 * sc.A), dtype=f32), dev)
    g = Guard(dev, (3 * POST, 5), (3 * POST, 1))
    nbuf, num = iguard(dev, 3)
    ops.proposal_layer(T(np.concatenate(probs), dev), deltas_d, H * 16, W * 16, 16, base_d, K, POST, 0.7, rois=g.views[0], scores=g.views[1],
                       num=num)
    assert g.intact() and bool((nbuf[3:] == ISENT).all())
    rois, scores, nums = g.views[0].cpu().numpy().reshape(3, POST, 5), g.views[1].cpu().numpy().reshape(3, POST, 1), num.cpu().numpy()
    base_tf = T(np.trunc(ops.generate_anchors(16)), dev)
    tr, ts, tn = ops.proposal_layer_tf(T(np.concatenate(probs), dev), deltas_d, H * 16, W * 16, 16, base_tf, POST, 0.7)
    tr, ts, tn = tr.cpu().numpy().reshape(3, POST, 5), ts.cpu().numpy().reshape(3, POST, 1), tn.cpu().numpy()
    for b, name in enumerate(names):
        r1, s1, n1 = run_proposal(dev, base_d, T(probs[b], dev), deltas_d[:1].contiguous(), H, W, K)
        assert int(nums[b]) == n1 and np.array_equal(bits(scores[b]), bits(s1)), name
        assert np.array_equal(bits(rois[b][:, 1:]), bits(r1[:, 1:])) and np.all(rois[b][:, 0] == b), name
        r1, s1, n1 = ops.proposal_layer_tf(T(probs[b], dev), deltas_d[:1].contiguous(), H * 16, W * 16, 16, base_tf, POST, 0.7)
        assert int(tn[b]) == int(n1.item()) and np.array_equal(bits(ts[b]), bits(s1.cpu().numpy())), name + " tf"
        assert np.array_equal(bits(tr[b][:, 1:]), bits(r1.cpu().numpy()[:, 1:])) and np.all(tr[b][:, 0] == b), name + " tf"


@pytest.mark.parametrize("k", [65, 257, 4097])
def test_nms_entry_points_on_non_finite_and_tied_scores(dev, k):
    """ops.nms, ops.nms_sorted and ops.non_max_suppression with negatives, both zeros, +-inf, denormals, NaN of both signs and two
    payloads and heavy ties: the keep lists equal the oracle's."""
    from frcnn_hip import ops
    d = sc.zoo_dets(k)
    for thr in (0.5, 0.7):
        want = ora.cpu_nms(d, thr)
        for mk in (None, 64):
            kbuf, keep = iguard(dev, k if mk is None else mk)
            nbuf, num = iguard(dev, 1)
            ops.nms(T(d, dev), thr, max_keep=mk, keep=keep, num=num)
            n = int(num.item())
            assert keep[:n].cpu().numpy().tolist() == (want if mk is None else want[:mk]), (k, thr, mk)
            assert bool((kbuf[keep.numel():] == ISENT).all()) and bool((nbuf[1:] == ISENT).all())
    ds = np.ascontiguousarray(d[ora.order_desc(d[:, 4])])
    keep, num = ops.nms_sorted(T(ds, dev), 0.5)
    assert keep[:int(num.item())].cpu().numpy().tolist() == ora.cpu_nms(ds, 0.5)
    boxes, scores = np.ascontiguousarray(d[:, :4]), np.ascontiguousarray(d[:, 4])
    for m in (k, 64):
        sbuf, sel = iguard(dev, m)
        nbuf, num = iguard(dev, 1)
        ops.non_max_suppression(T(boxes, dev), T(scores, dev), m, 0.5, selected=sel, num=num)
        assert sel[:int(num.item())].cpu().numpy().tolist() == ora.tf_non_max_suppression(boxes, scores, m, 0.5).tolist(), (k, m)
        assert bool((sbuf[m:] == ISENT).all()) and bool((nbuf[1:] == ISENT).all())


MODES = {"hard": {}, "soft_linear": {"soft": 1}, "vote": {"vote": 0.5}}


def run_detect_post(dev, inputs, max_per_image=100, max_out=128, **mode):
    from frcnn_hip import ops
    prob, deltas, rois, (im_h, im_w), thresh = inputs
    buf = torch.full((max_out + 16, 6), SENT, dtype=torch.float32, device=dev)
    buf[:max_out] = float("nan")
    cbuf, count = iguard(dev, 1)
    ops.detect_post(T(prob, dev), T(deltas, dev), T(rois, dev), None, 1.0, im_h, im_w, nms_thresh=0.3, score_thresh=float(thresh),
                    max_per_image=max_per_image, max_out=max_out, out=buf[:max_out], count=count, **mode)
    assert bool((buf[max_out:] == SENT).all()) and bool((cbuf[1:] == ISENT).all()), "written past max_out"
    scores, boxes = ora.im_detect_post(prob, deltas, rois, 1.0, (im_h, im_w))
    want = ora.detections_to_records(ora.test_net_post(scores, boxes, prob.shape[1], 0.3, max_per_image, thresh))
    return buf[:max_out].cpu().numpy(), int(count.item()), want


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("t", [2, 28, 29, 60])
def test_detect_post_with_ties_at_the_max_per_image_cut(dev, t, mode):
    """t rows tie exactly at the max_per_image = 100 cut (max_out = 128, the default), scores are equal inside a class, some rows sit
    exactly at score_thresh and some are NaN; the rois are disjoint, so hard NMS, Soft-NMS and box voting all keep every row as it is.
    The count is the reference's (every row >= the cut: 99 + t), rows [:min(count, max_out)] are the oracle's first rows, the rest
    is zero and nothing past max_out is written.  t = 60: the count (159) exceeds max_out, as include/frcnn_hip.h says it may."""
    got, count, want = run_detect_post(dev, sc.detect_post_case(t), **MODES[mode])
    assert count == want.shape[0] == 99 + t
    n = min(count, 128)
    assert same_rows(got[:n], want[:n])
    assert not bits(got[n:]).any()
    assert (count > 128) == (t == 60)


def test_signed_zeros_are_equal_and_keep_their_bits(dev, base_d):
    """-0.0 and +0.0 are equal, so the index decides, and the score written out is the input's bits at that index: the sort (ops.nms:
    K = N), the radix select (proposal_top_layer: K < N) and the `>= cut` of k_final_select.
    Before sortable_u32 mapped both zeros to one key the device ranked every +0.0 above every -0.0 (scores [-0.0, +0.0]: oracle
    order [0, 1], device [1, 0])."""
    from frcnn_hip import ops
    d = np.array([[0, 0, 9, 9, -0.0], [100, 0, 109, 9, 0.0], [200, 0, 209, 9, -0.0], [300, 0, 309, 9, 0.0]], dtype=f32)
    keep, num = ops.nms(T(d, dev), 0.5)
    assert keep[:int(num.item())].cpu().numpy().tolist() == ora.cpu_nms(d, 0.5) == [0, 1, 2, 3]
    H, W = sc.MAPS[54]
    s = np.zeros(54, dtype=f32)
    s[::2] = -0.0
    s[[5, 17, 40]] = [0.25, -1.0, 0.5]
    prob, deltas, info = sc.prob_blob(s, H, W), sc.zero_deltas(H, W), sc.im_info(H, W)
    for K in (1, 2, 3, 4, 27, 52, 53, 54):
        rois, scores = ops.proposal_top_layer(T(prob, dev), T(deltas, dev), H * 16, W * 16, 16, base_d, K)
        wr, ws = ora.proposal_top_layer(prob, deltas, info, 16, anchors_of(H, W), sc.A, K)
        assert np.array_equal(bits(scores.cpu().numpy()), bits(ws)), K        # the zeros' sign bits too
        assert same_rows(rois.cpu().numpy(), wr), K
    inputs = sc.detect_post_case(28, score_thresh=-0.5, cut=(0.0, -0.0), low=-0.25, fill=-0.75)
    got, count, want = run_detect_post(dev, inputs)
    assert count == want.shape[0] == 127 and same_rows(got[:count], want)


def test_nans_rank_first_whatever_their_sign_or_payload(dev, base_d):
    """Every NaN ranks above +inf (the reference's `argsort()[::-1]`), all NaNs are equal (index ascending among them) and a NaN is
    written out as a NaN.  Before sortable_u32 mapped every NaN to one key the device put a positive-sign NaN first and a
    negative-sign NaN (what 0 / 0 gives on an x86 host) LAST, and ordered NaNs among themselves by payload."""
    from frcnn_hip import ops
    nan = np.array([0xffc00000, 0x7fc00123, 0x7fc00000, 0xffc00123], dtype=np.uint32).view(f32)
    d = np.array([[0, 0, 9, 9, 1.0], [100, 0, 109, 9, 0], [200, 0, 209, 9, np.inf], [300, 0, 309, 9, 0], [400, 0, 409, 9, 0],
                  [500, 0, 509, 9, -np.inf], [600, 0, 609, 9, 0]], dtype=f32)
    d[[1, 3, 4, 6], 4] = nan
    keep, num = ops.nms(T(d, dev), 0.5)
    assert keep[:int(num.item())].cpu().numpy().tolist() == ora.cpu_nms(d, 0.5) == [1, 3, 4, 6, 2, 0, 5]
    H, W = sc.MAPS[54]
    s = sc.zoo_scores(54)
    prob, deltas, info = sc.prob_blob(s, H, W), sc.zero_deltas(H, W), sc.im_info(H, W)
    n_nan = int(np.isnan(s).sum())
    assert n_nan >= 4
    for K in (1, n_nan - 1, n_nan, n_nan + 1, 53, 54):
        rois, scores = ops.proposal_top_layer(T(prob, dev), T(deltas, dev), H * 16, W * 16, 16, base_d, K)
        wr, ws = ora.proposal_top_layer(prob, deltas, info, 16, anchors_of(H, W), sc.A, K)
        got = scores.cpu().numpy()
        assert ref.same_scores(got, ws) and np.isnan(got[:min(K, n_nan)]).all(), K
        assert same_rows(rois.cpu().numpy(), wr), K
    # the per-class stage drops NaN with the rows at or below score_thresh (`scores > thresh`, test.py:163)
    prob, deltas, rois, shape, thresh = sc.detect_post_case(2)
    got, count, want = run_detect_post(dev, (prob, deltas, rois, shape, thresh))
    assert count == 101 and not np.isnan(got).any()
