"""The anchor target layer and the proposal target layer of csrc/train_kernels.hip held to their numpy restatement
(oracle/target_ref.py) on the border, tie, threshold, chunk-seam, mode and sampling-plan cases of oracle/target_cases.py, through the C
entries frcnn_anchor_target_layer, frcnn_anchor_target_layer_inject, frcnn_proposal_target_layer, frcnn_proposal_target_layer_dn and
frcnn_proposal_target_layer_inject, for the seeds 0, 1, 2^31, 2^63 - 1 and -1 (no sampling).  The sampler is a fixed hash, so the SUBSET is
compared, not its size: labels, inside and outside weights, the sampled rows (rois, roi_scores, labels, counts -- which rows, in which
order, the with-replacement draws included) bit for bit; regression targets within the bounds of tests/test_train_gpu.py (2e-6 anchor,
2e-5 normalised RoI targets: device logf against np.log; every case keeps its width / height ratios inside [1/32, 32],
tests/test_targets_cpu.py asserts that).  The injected entries reproduce the reference's own runs (tests/golden/targets_edges.npz) from
its recorded draws.  tests/test_targets_cpu.py shows on the CPU which planted mistake each case catches."""
import os

import numpy as np
import pytest
import torch

import target_cases as tc
import target_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
ACASES = tc.anchor_cases()
RCASES = tc.roi_cases()
C = tc.NUM_CLASSES
AT_TOL, PT_TOL = 2e-6, 2e-5


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "targets_edges.npz"))


def _at_args(c, dev):
    from frcnn_hip import ops
    return (T(c.gt, dev), c.im_h, c.im_w, c.H, c.W, T(c.base, dev)), dict(
        feat_stride=c.stride, rpn_batchsize=c.batch, fg_fraction=c.fg_fraction, pos_overlap=c.pos_ov, neg_overlap=c.neg_ov,
        opts=ops.rpn_target_opts(c.clobber, c.pos_weight, c.inside_w))


def _at_ref(c, **kw):
    return ref.anchor_target_layer(c.base, c.stride, c.H, c.W, c.im_h, c.im_w, c.gt, c.batch, c.fg_fraction, c.pos_ov, c.neg_ov,
                                   clobber=c.clobber, pos_weight=c.pos_weight, inside_w=c.inside_w, **kw)


def _check_at(got, want, what):
    lab, tg, iw, ow = [t.cpu().numpy() for t in got]
    assert lab.shape == want[0].shape and np.array_equal(bits(lab), bits(want[0])), (what, "labels", int((lab != want[0]).sum()))
    assert np.array_equal(bits(iw), bits(want[2])), (what, "inside weights")
    assert np.array_equal(bits(ow), bits(want[3])), (what, "outside weights")
    assert tg.shape == want[1].shape and np.abs(tg - want[1]).max() <= AT_TOL, (what, "targets", float(np.abs(tg - want[1]).max()))


@pytest.mark.parametrize("c", ACASES, ids=[c.name for c in ACASES])
def test_anchor_target_layer_is_the_restatement(dev, c, edges):
    from frcnn_hip import ops
    a, kw = _at_args(c, dev)
    for seed in tc.SEEDS:
        _check_at(ops.anchor_target_layer(*a, seed=seed, **kw), _at_ref(c, seed=seed), (c.name, seed))
    # the injected entry: no list = no sampling; the reference's recorded draws = the reference's run
    _check_at(ops.anchor_target_layer_inject(*a, torch.zeros((0,), dtype=torch.int32, device=dev), **kw), _at_ref(c, seed=-1), (c.name, "inject none"))
    if c.golden:
        dis = edges["at.%s.disable" % c.name]
        g = [edges["at.%s.%s" % (c.name, k)] for k in ("labels", "targets", "inside", "outside")]
        _check_at(ops.anchor_target_layer_inject(*a, T(dis, dev), **kw), g, (c.name, "inject reference draws"))


def _pt_kw(c):
    from frcnn_hip import ops
    return dict(batch_size=c.batch, fg_fraction=c.fg_fraction, fg_thresh=c.fg_thresh, bg_hi=c.bg_hi, bg_lo=c.bg_lo,
                opts=ops.roi_target_opts(c.use_gt, c.inside_w))


def _check_pt(got, want, what):
    got = [t.cpu().numpy() for t in got]
    for k, name in ((0, "rois"), (1, "roi_scores"), (2, "labels"), (4, "inside weights"), (5, "outside weights")):
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (what, name)
    if len(got) > 6 and want[6] is not None:
        assert got[6].tolist() == want[6].tolist(), (what, "counts", got[6].tolist(), want[6].tolist())
    assert np.abs(got[3] - want[3]).max() <= PT_TOL, (what, "targets", float(np.abs(got[3] - want[3]).max()))


@pytest.mark.parametrize("c", RCASES, ids=[c.name for c in RCASES])
def test_proposal_target_layer_is_the_restatement(dev, c, edges):
    from frcnn_hip import ops
    rois, sc, gt = T(c.rois, dev), T(c.scores, dev), T(c.gt, dev)
    N = c.rois.shape[0]
    num = None if c.num is None else torch.tensor([c.num], dtype=torch.int32, device=dev)
    for seed in tc.SEEDS:
        want = ref.proposal_target_layer(c.rois, c.scores, c.gt, C, c.batch, c.fg_fraction, c.fg_thresh, c.bg_hi, c.bg_lo, seed=seed,
                                         num=c.num, use_gt=c.use_gt, inside_w=c.inside_w)
        _check_pt(ops.proposal_target_layer(rois, sc, gt, C, seed=seed, num=num, **_pt_kw(c)), want, (c.name, seed))
        if c.num is None:             # the same rows through the device-resident count: *num = N, and a count past the buffer is clamped to N
            for n in (N, N + 5):
                _check_pt(ops.proposal_target_layer(rois, sc, gt, C, seed=seed, num=torch.tensor([n], dtype=torch.int32, device=dev), **_pt_kw(c)),
                          want, (c.name, seed, "_dn", n))
    if c.golden:
        n = N if c.num is None else c.num
        g = [edges["pt.%s.%s" % (c.name, k)] for k in ("rois", "scores", "labels", "targets", "inside", "outside")]
        got = ops.proposal_target_layer_inject(T(c.rois[:n], dev), T(c.scores[:n], dev), gt, C, T(edges["pt.%s.keep_inds" % c.name], dev),
                                               int(edges["pt.%s.n_fg" % c.name]), opts=ops.roi_target_opts(c.use_gt, c.inside_w))
        _check_pt(got, g + [None], (c.name, "inject reference draws"))


def test_target_layer_error_codes(dev):
    """N + G = 3073 candidates with USE_GT: FRCNN_E_UNSUPPORTED before any launch (the outputs keep their sentinel), from both sampled entries;
    a workspace one byte short: FRCNN_E_WS, and the exact size is accepted."""
    import frcnn_hip
    from frcnn_hip import ops
    u = tc.unsupported_roi_case()
    rois, sc, gt = T(u.rois, dev), T(u.scores, dev), T(u.gt, dev)
    for num in (None, torch.tensor([u.rois.shape[0]], dtype=torch.int32, device=dev)):
        with pytest.raises(frcnn_hip.FrcnnHipError, match="not supported"):
            ops.proposal_target_layer(rois, sc, gt, C, seed=0, num=num, **_pt_kw(u))
    ok = ops.proposal_target_layer(rois, sc, gt, C, seed=0, batch_size=u.batch)                   # without USE_GT the 3070 rows are supported
    assert ok[6].cpu().numpy()[:2].sum() == u.batch
    c = next(c for c in ACASES if c.name == "border")
    A, G = c.base.shape[0], c.gt.shape[0]
    need = int(frcnn_hip.lib().frcnn_anchor_target_workspace_bytes(c.H, c.W, A, G))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    gt_d, base_d = T(c.gt, dev), T(c.base, dev)
    lab = torch.full((1, 1, A * c.H, c.W), 7.0, dtype=torch.float32, device=dev)
    tg, iw, ow = (torch.full((1, c.H, c.W, 4 * A), 7.0, dtype=torch.float32, device=dev) for _ in range(3))

    def run(nbytes):
        frcnn_hip.call("frcnn_anchor_target_layer", ops._ptr(gt_d), G, c.im_h, c.im_w, c.H, c.W, A, c.stride, ops._ptr(base_d), c.batch,
                       c.fg_fraction, c.pos_ov, c.neg_ov, 0, None, ops._ptr(lab), ops._ptr(tg), ops._ptr(iw), ops._ptr(ow), ops._ptr(ws),
                       nbytes, ops._stream())
    with pytest.raises(frcnn_hip.FrcnnHipError, match="workspace too small"):
        run(need - 1)
    assert float(lab.min().item()) == 7.0 and float(ow.min().item()) == 7.0                         # refused before any launch
    run(need)
    _check_at((lab, tg, iw, ow), _at_ref(c, seed=0), "exact workspace")
