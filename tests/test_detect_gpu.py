"""GPU parity: HIP detection kernels (through the C ABI) vs the oracle and the golden vectors.
Bit-exact for indices / keep lists on identical inputs; 1e-4 on coordinates where a device expf
feeds the value (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

import frcnn_oracle as ora
import gen_golden_ref_gpu_nms as gen_ref
import synth
from score_cases import box_tol          # 2 ulp of the coordinate, per element (shared with tests/test_select_gpu.py)

pytestmark = pytest.mark.gpu
f32 = np.float32


BOX_TOL = float(box_tol(np.float32(1000.0)))            # scalar form for printouts: 1.22e-4 px


def boxes_close(got, want, what):
    if not np.size(want):
        return True
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    ulps = float((d / (box_tol(want) / 2.0)).max())
    print("%s: max |box - reference| = %.3g px = %.2f ulp of the coordinate (bound 2 ulp)" % (what, float(d.max()), ulps))
    return bool((d <= box_tol(want)).all())


def T(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


@pytest.mark.parametrize("scales,H,W", [((8, 16, 32), 38, 63), ((4, 8, 16, 32), 38, 63), ((2, 4, 8, 16, 32), 50, 84)])
def test_anchors_device_bit_exact(dev, scales, H, W):
    from frcnn_hip import ops
    base = ops.generate_anchors(16, (0.5, 1, 2), scales)
    got = ops.generate_anchors_pre(H, W, 16, T(base, dev)).cpu().numpy()
    want, _ = ora.generate_anchors_pre(H, W, 16, scales, (0.5, 1, 2))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("tag,k,thr,cl", [("u3000_t07", 3000, 0.7, 0), ("c3000_t03", 3000, 0.3, 12),
                                          ("c6000_t07", 6000, 0.7, 40), ("c700_t05", 700, 0.5, 5), ("one", 1, 0.3, 0)])
def test_nms_keep_bit_exact_vs_golden(dev, golden, tag, k, thr, cl):
    from frcnn_hip import ops
    d = synth.random_dets(k, seed=11, cluster=cl)
    keep, num = ops.nms(T(d, dev), thr)
    n = int(num.item())
    got = keep[:n].cpu().numpy()
    assert np.array_equal(got, golden["nms"][tag + "_keep"])          # the reference's own cpu_nms output
    assert got.tolist() == ora.cpu_nms(d, thr)


@pytest.mark.parametrize("k,thr,cl,seed", [(12000, 0.7, 200, 5), (16384, 0.5, 0, 6), (65, 0.3, 2, 7), (64, 0.3, 2, 8),
                                           (129, 0.9, 1, 9), (4097, 0.1, 30, 10)])
def test_nms_keep_bit_exact_vs_oracle(dev, k, thr, cl, seed):
    from frcnn_hip import ops
    d = synth.random_dets(k, seed=seed, cluster=cl)
    keep, num = ops.nms(T(d, dev), thr)
    assert keep[:int(num.item())].cpu().numpy().tolist() == ora.cpu_nms(d, thr)


def test_nms_max_keep_truncates_like_slicing(dev):
    from frcnn_hip import ops
    d = synth.random_dets(6000, seed=21, cluster=60)
    full = ora.cpu_nms(d, 0.7)
    for mk in (1, 63, 64, 65, 300):
        keep, num = ops.nms(T(d, dev), 0.7, max_keep=mk)
        assert keep[:int(num.item())].cpu().numpy().tolist() == full[:mk]


def test_nms_threshold_compared_in_double(dev):
    from frcnn_hip import ops
    d = np.array([[0, 0, 9, 9, 0.9], [0, 0, 9, 4, 0.8]], dtype=f32)        # IoU exactly 0.5
    for thr, want in ((0.5, [0]), (0.5000001, [0, 1]), (0.49999999, [0])):
        keep, num = ops.nms(T(d, dev), thr)
        assert keep[:int(num.item())].cpu().numpy().tolist() == want == ora.cpu_nms(d, thr)


def test_nms_ties_are_index_ascending_and_empty(dev):
    from frcnn_hip import ops
    d = synth.random_dets(500, seed=3, cluster=4)
    d[:, 4] = np.round(d[:, 4] * 8) / 8                                      # heavy ties
    keep, num = ops.nms(T(d, dev), 0.5)
    assert keep[:int(num.item())].cpu().numpy().tolist() == ora.cpu_nms(d, 0.5)   # oracle: (score desc, index asc)
    keep, num = ops.nms(torch.zeros((0, 5), device=dev), 0.3)
    assert int(num.item()) == 0                                                # nms_wrapper.py:18-19


def test_nms_sorted_and_host_compat__nms(dev):
    import ctypes
    import frcnn_hip
    from frcnn_hip import ops
    d = synth.random_dets(3000, seed=11, cluster=12)
    order = ora.order_desc(d[:, 4])
    ds = np.ascontiguousarray(d[order])
    want = ora.cpu_nms(ds, 0.3)                                                # indices into the sorted array
    keep, num = ops.nms_sorted(T(ds, dev), 0.3)
    assert keep[:int(num.item())].cpu().numpy().tolist() == want
    # `_nms` (lib/nms/gpu_nms.hpp:1-2): host pointers, float threshold
    keep_h = np.zeros(3000, dtype=np.int32)
    n_h = ctypes.c_int(0)
    frcnn_hip.lib()._nms(keep_h.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_h), ds.ctypes.data_as(ctypes.c_void_p),
                         3000, 5, ctypes.c_float(0.3), 0)
    assert keep_h[:n_h.value].tolist() == ora.gpu_nms(ds, 0.3)             # the CUDA kernel's rule (nms_kernel.cu:71), float threshold


def test_nms_under_the_reference_mangled_name(dev, golden):
    """The reference's `_nms` has C++ linkage (lib/nms/gpu_nms.hpp:1-2, bound by lib/nms/gpu_nms.pyx:13-31): libfrcnn_hip.so exports
    `_Z4_nmsPiS_PKfiifi` too, bound here exactly the way oracle/gen_golden_ref_gpu_nms.py binds the reference's own build -- same keep list as the
    extern "C" name and as the CUDA kernel's rule."""
    import ctypes
    import frcnn_hip
    d = synth.random_dets(3000, seed=11, cluster=12)
    ds = np.ascontiguousarray(d[ora.order_desc(d[:, 4])])
    fn = ctypes.CDLL(frcnn_hip.LIB_PATH)._Z4_nmsPiS_PKfiifi
    fn.restype = None
    keep = np.zeros(3000, dtype=np.int32)
    n = ctypes.c_int(0)
    fn(keep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), ds.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(3000), ctypes.c_int(5),
       ctypes.c_float(0.3), ctypes.c_int(0))
    assert keep[:n.value].tolist() == ora.gpu_nms(ds, 0.3)
    assert keep[:n.value].tolist() == _ref_gpu_nms_keep(golden, "plain", ds, 0.3)


def _ref_gpu_nms_keep(golden, key, ds, thresh, fma=False):
    """The keep list of the reference's CUDA kernel + host loop (lib/nms/nms_kernel.cu, hipified and compiled for gfx950 by
    oracle/build_ref.py::build_gpu_nms; FMA-contracted build with fma=True) on `ds`, as stored in tests/golden/ref_gpu_nms.npz by
    oracle/gen_golden_ref_gpu_nms.py.  The stored input digest must match `ds`.  Where that build is present under oracle/_ref/nms/,
    its live result must equal the stored one as well."""
    g = golden["ref_gpu_nms"]
    assert str(g["plain_sha1" if key == "plain" else "sha1_" + key]) == gen_ref.digest(ds), "inputs differ from the stored case " + key
    want = g[("fma_" if fma else "keep_") + key if key != "plain" else "plain_keep"].tolist()
    live = gen_ref.ref_lib("libref_gpu_nms_fma.so" if fma else "libref_gpu_nms.so")
    if live is not None:
        assert live(ds, thresh).tolist() == want, "oracle/_ref/nms build differs from tests/golden/ref_gpu_nms.npz"
    return want


@pytest.mark.parametrize("k,thr,cl,seed", [(3000, 0.3, 12, 11), (6000, 0.7, 40, 3), (12000, 0.7, 200, 5), (257, 0.5, 3, 2), (64, 0.3, 1, 9)])
def test_gpu_rule_bit_exact_vs_the_reference_cuda_kernel(dev, golden, k, thr, cl, seed):
    """FRCNN_NMS_RULE_GPU (`_nms`, what nms_wrapper picks under cfg.USE_GPU_NMS) against the reference's OWN CUDA kernel
    (lib/nms/nms_kernel.cu:24-144, hipified + compiled for gfx950 into oracle/_ref, separate roundings; its keep lists stored in
    tests/golden/ref_gpu_nms.npz): identical keep lists, incl. boxes engineered to sit on the threshold.  The FMA-contracted build of
    the same file (what nvcc's default -fmad=true may produce) is reported beside it: where it differs, the product follows the
    un-contracted arithmetic of lib/nms/py_cpu_nms.py:18-38."""
    import ctypes
    import frcnn_hip
    key = gen_ref.case_key(k, thr, cl, seed)
    # pairs exactly at the threshold: box j = box i shrunk so that IoU == thr in float32 for several i (synth.threshold_dets)
    ds = gen_ref.threshold_case(k, thr, cl, seed)
    keep_h = np.zeros(k, dtype=np.int32)
    n_h = ctypes.c_int(0)
    frcnn_hip.lib()._nms(keep_h.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_h), ds.ctypes.data_as(ctypes.c_void_p), k, 5,
                         ctypes.c_float(thr), 0)
    got = keep_h[:n_h.value].tolist()
    want = _ref_gpu_nms_keep(golden, key, ds, thr)
    fma = _ref_gpu_nms_keep(golden, key, ds, thr, fma=True)
    print("k %d thr %.1f: kept %d; reference CUDA kernel (contract off) %d, FMA-contracted build %d (differs in %d positions)"
          % (k, thr, len(got), len(want), len(fma), sum(1 for a, b in zip(want, fma) if a != b) + abs(len(want) - len(fma))))
    assert got == want
    assert got == ora.gpu_nms(ds, thr)


def _proposal_case(dev, H, W, scales, key, post, info, seed=3):
    from frcnn_hip import ops
    A = 3 * len(scales)
    prob, dl = synth.rpn_outputs(H, W, A, seed=seed)
    base = ops.generate_anchors(16, (0.5, 1, 2), scales)
    pre = {"TEST": 6000, "TRAIN": 12000}[key]
    rois, scores, num = ops.proposal_layer(T(prob, dev), T(dl, dev), info[0], info[1], 16, T(base, dev), pre, post, 0.7)
    return prob, dl, rois.cpu().numpy(), scores.cpu().numpy(), int(num.item())


@pytest.mark.parametrize("tag,H,W,scales,key,post,info", [
    ("test_38x63_a9", 38, 63, (8, 16, 32), "TEST", 300, (600, 1000, 1.6)),
    ("train_38x63_a9", 38, 63, (8, 16, 32), "TRAIN", 2000, (600, 1000, 1.6)),
    ("test_10x14_a9", 10, 14, (8, 16, 32), "TEST", 300, (160, 224, 1.0)),
    ("test_50x84_a15", 50, 84, (2, 4, 8, 16, 32), "TEST", 1000, (800, 1333, 1.6))])
def test_proposal_layer_vs_reference_golden(dev, golden, tag, H, W, scales, key, post, info):
    g = golden["proposal"]
    _, _, rois, scores, n = _proposal_case(dev, H, W, scales, key, post, info)
    want_r, want_s = g[tag + "_rois"], g[tag + "_scores"]
    assert n == want_r.shape[0]
    # scores are copied (bit-exact); boxes pass through the device expf: 1e-4
    # a 1-ulp decode difference may flip an IoU that sits on the threshold; such a flip would
    # change the kept set and show up as a score mismatch, so exact score equality is the
    # index-parity check.
    assert np.array_equal(scores[:n], want_s)
    assert boxes_close(rois[:n], want_r, "proposal_layer vs reference golden " + tag)
    assert np.all(rois[n:] == 0) and np.all(scores[n:] == 0)


def test_proposal_top_layer_vs_reference_golden(dev, golden):
    from frcnn_hip import ops
    g = golden["proposal"]
    prob, dl = synth.rpn_outputs(38, 63, 9, seed=3)
    base = ops.generate_anchors(16)
    rois, scores = ops.proposal_top_layer(T(prob, dev), T(dl, dev), 600, 1000, 16, T(base, dev), 5000)
    assert np.array_equal(scores.cpu().numpy(), g["top_38x63_a9_scores"])
    assert boxes_close(rois.cpu().numpy(), g["top_38x63_a9_rois"], "proposal_top_layer vs reference golden")


def test_proposal_layer_other_seeds_vs_oracle(dev):
    for seed in (4, 5):
        prob, dl, rois, scores, n = _proposal_case(dev, 38, 63, (8, 16, 32), "TEST", 300, (600, 1000, 1.6), seed=seed)
        anc, _ = ora.generate_anchors_pre(38, 63, 16)
        wr, ws = ora.proposal_layer(prob, dl, np.array([600, 1000, 1.6], dtype=f32), "TEST", [16], anc, 9)
        assert n == wr.shape[0] and np.array_equal(scores[:n], ws) and boxes_close(rois[:n], wr, "proposal_layer vs oracle")


@pytest.mark.parametrize("H,W,C,R,pool,mp", [(38, 63, 1024, 300, 7, False), (38, 63, 512, 64, 7, True), (50, 84, 256, 100, 7, False),
                                             (5, 6, 8, 9, 3, False)])
def test_crop_and_resize_vs_oracle(dev, H, W, C, R, pool, mp):
    from frcnn_hip import ops
    rng = np.random.RandomState(2)
    feat = rng.randn(H, W, C).astype(f32)
    d = synth.random_dets(R, seed=4, im_w=W * 16.0, im_h=H * 16.0)
    d[: R // 4, 2] = W * 16.0 - 1      # border-touching RoIs sample beyond the map -> zeros
    d[R // 4: R // 2, 3] = H * 16.0 - 1
    rois = np.hstack([np.zeros((R, 1), dtype=f32), d[:, :4]]).astype(f32)
    got = ops.crop_and_resize(T(feat, dev), T(rois, dev), 16.0, pool, max_pool=mp).cpu().numpy()
    want = ora.crop_and_resize(feat, rois, 16.0, pool, max_pool=mp)
    assert got.shape == want.shape
    assert np.array_equal(got, want)                                   # same f32 op order, no contraction
    assert (want == 0).any() and (want != 0).any()
    # both work splits of the kernel (round 5: one workgroup per (roi, slab); rounds 2-4: per (roi, output row, slab)) and other slab
    # counts: the same crop_sample per element -> the same bits
    import frcnn_hip
    L = frcnn_hip.lib()
    try:
        for form, slabs in ((1, -1), (0, 1), (0, 2), (1, 2)):
            L.frcnn_detect_set_tuning(5, form); L.frcnn_detect_set_tuning(4, slabs)
            alt = ops.crop_and_resize(T(feat, dev), T(rois, dev), 16.0, pool, max_pool=mp).cpu().numpy()
            assert np.array_equal(alt, want), (form, slabs)
    finally:
        L.frcnn_detect_set_tuning(5, 0); L.frcnn_detect_set_tuning(4, -1)


@pytest.mark.parametrize("tag,R,C,W,H", [("voc_300x21", 300, 21, 1000.0, 600.0), ("coco_1000x81", 1000, 81, 1333.0, 800.0)])
def test_detect_post_vs_reference_golden(dev, golden, tag, R, C, W, H):
    from frcnn_hip import ops
    prob, bp, rois = synth.rcnn_outputs(R, C, seed=7, im_w=W, im_h=H)
    im_h, im_w = int(H / 1.6), int(W / 1.6)
    dets, cnt = ops.detect_post(T(prob, dev), T(bp, dev), T(rois, dev), None, 1.6, im_h, im_w)
    n = int(cnt.item())
    want = golden["perclass"][tag + "_records"]
    got = dets[:n].cpu().numpy()
    assert n == want.shape[0]
    assert np.array_equal(got[:, 4:], want[:, 4:])                    # scores + classes: bit-exact => same keep sets
    assert boxes_close(got[:, :4], want[:, :4], "detect_post vs reference golden " + tag)


def test_detect_post_num_rois_and_no_cap(dev):
    from frcnn_hip import ops
    R, C = 300, 21
    prob, bp, rois = synth.rcnn_outputs(R, C, seed=9)
    nr = torch.tensor([120], dtype=torch.int32, device=dev)
    dets, cnt = ops.detect_post(T(prob, dev), T(bp, dev), T(rois, dev), nr, 1.6, 375, 625, max_per_image=0, max_out=4096)
    sc, boxes = ora.im_detect_post(prob[:120], bp[:120], rois[:120], 1.6, (375, 625, 3))
    want = ora.detections_to_records(ora.test_net_post(sc, boxes, C, max_per_image=0))
    n = int(cnt.item())
    got = dets[:n].cpu().numpy()
    assert n == want.shape[0] and np.array_equal(got[:, 4:], want[:, 4:]) and boxes_close(got[:, :4], want[:, :4], "detect_post (num_rois, no cap) vs oracle")


def _rows_u32(boxes):
    """[n,4] float32 -> the rows as uint32, sorted: a multiset of boxes compared bit for bit"""
    u = np.ascontiguousarray(boxes, dtype=f32).reshape(-1, 4).view(np.uint32)
    return u[np.lexsort(u.T[::-1])]


@pytest.mark.parametrize("regress", [True, False])
def test_detect_post_stages_exactly_the_im_detect_boxes(dev, regress):
    """One staging rule (csrc/detect_post.hip, stage_candidate): with nothing suppressed and no cut, the boxes every per-class stage --
    hard NMS, linear and Gaussian Soft-NMS -- emits for an (image, class) are, bit for bit, the rows of ops.im_detect_boxes for that
    class that pass r < num_rois and score > score_thresh (bbox_pred None: the un-clipped rois / im_scale); and the vote stage, given a
    class with ONE candidate, re-derives that same box and leaves it as it is.  (B, R, C) = (2, 65, 3): one row past a wave and past a
    Soft-NMS slot; the second image has rows past its count.  No row is excluded from the comparison."""
    from frcnn_hip import ops
    B, R, C, scale, im_h, im_w, thresh = 2, 65, 3, 1.6, 375, 625, 0.1
    num = np.array([65, 40], dtype=np.int32)
    parts = [synth.rcnn_outputs(R, C, seed=31 + b) for b in range(B)]
    prob, bp, rois = (np.concatenate([p[k] for p in parts]) for k in range(3))
    t_prob, t_bp, t_rois, t_num = T(prob, dev), (T(bp, dev) if regress else None), T(rois, dev), T(num, dev)
    want, passing = {}, {}
    for b in range(B):
        rows = slice(b * R, (b + 1) * R)
        if regress:
            boxes = ops.im_detect_boxes(T(rois[rows], dev), T(bp[rows], dev), scale, im_h, im_w).cpu().numpy().reshape(R, C, 4)
        else:
            boxes = np.repeat((rois[rows, 1:5].astype(np.float64) / scale).astype(f32)[:, None, :], C, axis=1)
        for j in range(1, C):
            ok = (np.arange(R) < num[b]) & (prob[rows, j] > f32(thresh))
            assert ok.sum() >= 10, "the comparison must not be vacuous"
            want[b, j], passing[b, j] = boxes[:, j], ok

    def run(soft, score_thresh, vote=0.0):
        # nms_thresh 1.5 under the CPU rule `ovr >= thresh`: no IoU reaches it, so hard NMS suppresses nothing and the linear weight is 1
        dets, cnt = ops.detect_post(t_prob, t_bp, t_rois, t_num, scale, im_h, im_w, nms_thresh=1.5, score_thresh=score_thresh,
                                    max_per_image=0, batch=B, soft=soft, min_score=0.0, vote=vote)
        dets, cnt = dets.cpu().numpy(), cnt.cpu().numpy()
        return {(b, j): dets[b, :cnt[b]][dets[b, :cnt[b], 5] == j][:, :4] for b in range(B) for j in range(1, C)}

    for soft in (0, 1, 2):
        got = run(soft, thresh)
        for key, ok in passing.items():
            assert np.array_equal(_rows_u32(got[key]), _rows_u32(want[key][ok])), ("soft", soft, "image, class", key)
        for (b, j), ok in passing.items():
            s = np.where(ok, prob[b * R:(b + 1) * R, j], -np.inf)
            top, second = np.argsort(-s, kind="stable")[:2]
            voted = run(soft, float(s[second]), vote=1.0)[b, j]                      # `>` the second score: one candidate in (b, j)
            assert voted.shape == (1, 4) and np.array_equal(voted.view(np.uint32), want[b, j][top:top + 1].view(np.uint32)), \
                ("vote", "soft", soft, "image, class", (b, j))


def test_bbox_overlaps_bit_exact(dev, golden):
    from frcnn_hip import ops
    d = synth.random_dets(600, seed=13)[:, :4].astype(np.float64)
    q = synth.gt_boxes(12, 21, seed=14).astype(np.float64)[:, :4]
    got = ops.bbox_overlaps(T(d, dev), T(q, dev)).cpu().numpy()
    assert np.array_equal(got, golden["targets"]["overlaps"])


def test_im_detect_boxes_vs_reference_golden(dev, golden):
    import hashlib
    from frcnn_hip import ops
    for tag, (R, C, W, H) in {"voc_300x21": (300, 21, 1000.0, 600.0), "coco_1000x81": (1000, 81, 1333.0, 800.0)}.items():
        prob, bp, rois = synth.rcnn_outputs(R, C, seed=7, im_w=W, im_h=H)
        got = ops.im_detect_boxes(T(rois, dev), T(bp, dev), 1.6, int(H / 1.6), int(W / 1.6)).cpu().numpy()
        _, want = ora.im_detect_post(prob, bp, rois, 1.6, (int(H / 1.6), int(W / 1.6), 3))
        # `want` is pinned to the reference through its sha in the golden file (test_oracle_golden.py)
        assert np.array_equal(np.frombuffer(hashlib.sha256(want.tobytes()).digest(), dtype=np.uint8), golden["perclass"][tag + "_boxes_sha"])
        assert boxes_close(got, want, "im_detect_boxes vs reference golden " + tag)     # device expf vs np.exp: <= 2 ulp of the coordinate


def test_host_mirror_seams_numpy_in_numpy_out(dev, golden):
    """The reference-named modules (nms.gpu_nms, model.nms_wrapper, utils.cython_bbox, layer_utils.*) are
    drop-ins: numpy in, numpy out, reference results."""
    from layer_utils.generate_anchors import generate_anchors
    from layer_utils.proposal_layer import proposal_layer
    from layer_utils.snippets import generate_anchors_pre
    from model.nms_wrapper import nms
    from utils.cython_bbox import bbox_overlaps
    d = synth.random_dets(3000, seed=11, cluster=12)
    assert np.array_equal(np.array(nms(d, 0.3), dtype=np.int32), golden["nms"]["c3000_t03_keep"])
    assert nms(np.zeros((0, 5), dtype=f32), 0.3) == []
    assert np.array_equal(generate_anchors(), ora.generate_anchors())
    anc, n = generate_anchors_pre(38, 63, [16, ], (8, 16, 32), (0.5, 1, 2))
    assert n == 21546 and np.array_equal(anc, ora.generate_anchors_pre(38, 63, 16)[0])
    q = synth.gt_boxes(12, 21, seed=14).astype(np.float64)
    bx = synth.random_dets(600, seed=13)[:, :4].astype(np.float64)
    assert np.array_equal(bbox_overlaps(bx, q), golden["targets"]["overlaps"])
    prob, dl = synth.rpn_outputs(38, 63, 9, seed=3)
    blob, sc = proposal_layer(prob, dl, np.array([600, 1000, 1.6], dtype=f32), b"TEST", [16, ], anc, 9)
    assert np.array_equal(sc, golden["proposal"]["test_38x63_a9_scores"])
    assert boxes_close(blob, golden["proposal"]["test_38x63_a9_rois"], "proposal_layer mirror vs reference golden")


# ------------------------------------------------------------------------------------------------ USE_E2E_TF graph
@pytest.mark.parametrize("k,thr,cl,seed,cap", [(3000, 0.7, 12, 21, 300), (400, 0.3, 8, 22, 400), (21546, 0.7, 300, 23, 300),
                                               (65536, 0.5, 2000, 24, 1000), (65, 0.5, 2, 25, 65), (1, 0.5, 0, 26, 5)])
def test_tf_non_max_suppression_bit_exact_vs_oracle(dev, k, thr, cl, seed, cap):
    """frcnn_non_max_suppression == the oracle's restatement of tf.image.non_max_suppression (r1.2): selected indices
    bit-exact, incl. k beyond the 16384 of the Cython-rule kernels, flipped corners and zero-area boxes."""
    from frcnn_hip import ops
    d = synth.random_dets(k, seed=seed, cluster=cl)
    boxes, scores = d[:, :4].copy(), d[:, 4].copy()
    if k > 8:
        boxes[5] = boxes[5][[2, 3, 0, 1]]
        boxes[7, 2] = boxes[7, 0]
    sel, num = ops.non_max_suppression(T(boxes, dev), T(scores, dev), cap, thr)
    n = int(num.item())
    want = ora.tf_non_max_suppression(boxes, scores, cap, thr)
    assert n == want.shape[0] and np.array_equal(sel[:n].cpu().numpy(), want)


def test_tf_non_max_suppression_rule_differs_from_cython_rule(dev):
    from frcnn_hip import ops
    b = np.array([[0, 0, 2, 2], [0, 0, 2, 1], [10, 10, 10, 30]], dtype=f32)       # IoU(0,1) = 0.5 exactly without the +1 rule
    s = np.array([0.9, 0.8, 0.7], dtype=f32)
    sel, num = ops.non_max_suppression(T(b, dev), T(s, dev), 10, 0.5)
    assert sel[:int(num.item())].cpu().tolist() == [0, 1, 2]                      # `>`: equality survives; zero-area box kept
    sel, num = ops.non_max_suppression(T(b, dev), T(s, dev), 10, 0.49)
    assert sel[:int(num.item())].cpu().tolist() == [0, 2]
    sel, num = ops.non_max_suppression(T(b, dev), T(s, dev), 1, 0.49)
    assert int(num.item()) == 1
    e, num = ops.non_max_suppression(torch.zeros((0, 4), device=dev), torch.zeros((0,), device=dev), 10, 0.5)
    assert int(num.item()) == 0


@pytest.mark.parametrize("tag,H,W,scales,post,info", [
    ("38x63_a9", 38, 63, (8, 16, 32), 300, (600, 1000, 1.6)),
    ("10x14_a9", 10, 14, (8, 16, 32), 300, (160, 224, 1.0)),
    ("50x84_a15", 50, 84, (2, 4, 8, 16, 32), 1000, (800, 1333, 1.6))])
def test_proposal_layer_tf_vs_reference_golden(dev, golden, tag, H, W, scales, post, info):
    """Goldens: the reference's proposal_layer_tf body (proposal_layer.py:56-84) on the numpy-backed tf shim."""
    from frcnn_hip import ops
    g = golden["proposal_tf"]
    A = 3 * len(scales)
    prob, dl = synth.rpn_outputs(H, W, A, seed=5)
    base = np.trunc(ops.generate_anchors(16, (0.5, 1, 2), scales))
    rois, scores, num = ops.proposal_layer_tf(T(prob, dev), T(dl, dev), info[0], info[1], 16, T(base, dev), post, 0.7)
    n = int(num.item())
    rois, scores = rois.cpu().numpy(), scores.cpu().numpy()
    want_r, want_s = g["tf_" + tag + "_rois"], g["tf_" + tag + "_scores"]
    assert n == want_r.shape[0]
    assert np.array_equal(scores[:n], want_s)                                     # same anchors selected, same order
    assert boxes_close(rois[:n], want_r, "proposal_layer_tf vs reference golden " + tag)
    assert np.all(rois[n:] == 0) and np.all(scores[n:] == 0)


def test_truncated_anchor_table_matches_generate_anchors_pre_tf(dev, golden):
    from frcnn_hip import ops
    base = np.trunc(ops.generate_anchors(16, (0.5, 1, 2), (3, 5, 7)))
    got = ops.generate_anchors_pre(7, 9, 16, T(base, dev)).cpu().numpy()
    want, _ = ora.generate_anchors_pre_tf(7, 9, 16, (3, 5, 7), (0.5, 1, 2))
    assert np.array_equal(got, want)
    assert np.array_equal(got[:64], golden["proposal_tf"]["anchors_odd_7x9_first"])
