"""CPU: proposal recall on the host path -- frcnn_proposal_recall_host through datasets.recall.match_host / summarise, select_gt and
imdb.evaluate_recall -- against tests/golden/recall.npz, the results of the REFERENCE's own imdb.evaluate_recall on the same inputs
(fixtures/gen_golden_recall.py).  Equality is exact: every recorded IoU is one float64 expression evaluated with one rounding per
operation on both sides, and everything after it is sorting and counting."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import recall_golden as rg  # noqa: E402

CASES = ("hand", "empty", "large", "ties", "areas", "few", "scale16", "scale600", "many")


@pytest.fixture(scope="module")
def cases():
    return rg.load()


def test_fixture_holds_every_case(cases):
    assert sorted(cases) == sorted(CASES)
    assert os.path.getsize(rg.GOLD) < 200 * 1024
    assert [r.raised for r in cases["few"].runs] == [True]
    hand = cases["hand"].runs[0]
    assert hand.gt_overlaps[0] == 0.0 and 0.5 < hand.gt_overlaps[1] < 1.0 and hand.num_pos == 2       # the uncovered gt is recorded as 0.0
    assert cases["empty"].runs[0].num_pos == 5 and len(cases["empty"].runs[0].gt_overlaps) == 2       # 3 gts without candidates still count


@pytest.mark.parametrize("name", CASES)
def test_host_statement_equals_the_reference(cases, name):
    from datasets import recall
    case = cases[name]
    for run in case.runs:
        if not run.use_cand:
            continue
        gts = case.gts(run.area)
        if run.raised:
            with pytest.raises(AssertionError):
                recall.match_host(case.cands, gts, run.limit)
            continue
        ov, num_pos = recall.match_host(case.cands, gts, run.limit)
        res = recall.summarise(ov, num_pos)
        assert num_pos == run.num_pos
        for k in ("gt_overlaps", "recalls", "ar", "thresholds"):
            assert rg.same(res[k], getattr(run, k)), (name, run.area, run.limit, k)
        pos = 0
        for i, (g, c) in enumerate(zip(gts, case.cands)):      # the picks of the images that have candidates, image after image
            picks = ov[pos:pos + (len(g) if len(c) else 0)]
            pos += len(picks)
            assert np.all(np.diff(picks) <= 0), "the picks of one image are non-increasing"
            assert rg.same(np.sort(picks), run.per_image[i]), (name, i)
        assert pos == len(ov)


def test_scaled_rois_give_the_candidates_divided_in_float32(cases):
    """stride 5 with a scale: the host entry's own division, not numpy's"""
    from frcnn_hip import ops
    for name in ("scale16", "scale600"):
        case = cases[name]
        gts = case.gts()
        for run in case.runs:
            n = case.rois[0].shape[0]
            ov, ran = ops.proposal_recall_host(case.rois[0], [0], [n], [case.scale], gts[0], [0, len(gts[0])], n, run.limit)
            assert not ran.any() and rg.same(np.sort(ov), run.gt_overlaps)
            assert not rg.same(run.gt_overlaps, cases["large"].runs[0].gt_overlaps)      # the rounding of * s then / s is visible


@pytest.mark.parametrize("name", ("empty", "areas"))
def test_imdb_evaluate_recall_on_the_host_path(cases, name, monkeypatch):
    import torch
    from datasets.imdb import imdb
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    case = cases[name]
    db = imdb("toy", ["__background__", "c1", "c2", "c3"])
    db._image_index = list(range(len(case.entries)))
    db._roidb = case.roidb()
    for run in case.runs:
        kw = dict(candidate_boxes=case.cands if run.use_cand else None, area=run.area, limit=run.limit)
        if run.raised:
            with pytest.raises(AssertionError):
                db.evaluate_recall(**kw)
            continue
        res = db.evaluate_recall(**kw)
        assert sorted(res) == ["ar", "gt_overlaps", "recalls", "thresholds"]
        for k in res:
            assert rg.same(res[k], getattr(run, k)), (name, run.area, run.use_cand, k)
    assert any(r.raised for r in cases["areas"].runs) and not all(r.raised for r in cases["areas"].runs if not r.use_cand)


def test_select_gt_for_all_eight_areas(cases):
    from datasets import recall
    case = cases["areas"]
    assert sorted(case.sel) == sorted(recall.AREAS) and len(recall.AREAS) == 8
    for area in recall.AREAS:
        got = recall.select_gt(case.roidb()[0], area)
        assert np.array_equal(got, case.sel[area][0]), area
    # the inclusive ends: 32^2 is small and medium, 96^2 medium and large and 96-128, ...
    sa = case.entries[0]["seg_areas"]
    for area, edge in (("small", 32 ** 2), ("medium", 32 ** 2), ("medium", 96 ** 2), ("96-128", 96 ** 2), ("96-128", 128 ** 2),
                       ("128-256", 128 ** 2), ("128-256", 256 ** 2), ("256-512", 256 ** 2), ("256-512", 512 ** 2), ("512-inf", 512 ** 2)):
        assert int(np.nonzero(sa == edge)[0][0]) in case.sel[area][0].tolist(), (area, edge)
    assert 12 not in case.sel["all"][0] and 13 not in case.sel["all"][0] and 14 not in case.sel["all"][0]      # crowd rows, class-0 rows
    with pytest.raises(AssertionError):
        recall.select_gt(case.roidb()[0], "huge")


def test_argument_checks():
    import frcnn_hip
    L = frcnn_hip.lib()
    E_ARG, OK = -1, 0
    boxes = np.array([[0, 0, 10, 10], [5, 5, 20, 20]], dtype=np.float32)
    rois = np.array([[9, 0, 0, 10, 10], [9, 5, 5, 20, 20]], dtype=np.float32)
    gt = np.array([[0, 0, 10, 10]], dtype=np.float64)
    scale = np.ones(1, dtype=np.float32)
    nbytes = L.frcnn_proposal_recall_workspace_bytes(1, 2, 1)
    assert nbytes >= 2 * 1 * 8
    ws = np.zeros(nbytes, dtype=np.uint8)

    def run(b=boxes, start=(0,), count=(2,), off=(0, 1), ws_bytes=nbytes, stride=None, n_images=1):
        out, flag = np.full(1, 7.0), np.full(max(n_images, 1), 7, dtype=np.int32)
        start, count, off = np.array(start, dtype=np.int64), np.array(count, dtype=np.int32), np.array(off, dtype=np.int64)
        rc = L.frcnn_proposal_recall_host(b.ctypes.data, b.shape[1] if stride is None else stride, b.shape[0], start.ctypes.data, count.ctypes.data,
                                          scale.ctypes.data, n_images, 2, 0, gt.ctypes.data, off.ctypes.data, 1, out.ctypes.data, flag.ctypes.data,
                                          ws.ctypes.data, ctypes.c_size_t(ws_bytes))
        return rc, out[0], flag[0]
    assert run() == (OK, 1.0, 0)
    assert run(b=rois) == (OK, 1.0, 0)                         # stride 5: column 0 is skipped
    assert run(count=(-1,)) == (E_ARG, 7.0, 7)
    for stride in (0, 3, 6, -4):
        assert run(stride=stride) == (E_ARG, 7.0, 7)
    assert run(off=(1, 0)) == (E_ARG, 7.0, 7)
    assert run(ws_bytes=nbytes - 1) == (E_ARG, 7.0, 7) and run(ws_bytes=0) == (E_ARG, 7.0, 7)
    assert run(start=(3,)) == (E_ARG, 7.0, 7) and run(n_images=-1)[0] == E_ARG
    assert run(n_images=0) == (OK, 7.0, 7)
    assert run(count=(0,)) == (OK, 7.0, 0)                     # no candidates: the flag is cleared, no slot is written
    # the device entry refuses what it can see without reading device memory, before any launch
    assert L.frcnn_proposal_recall(None, 3, 0, None, None, None, 1, 2, 0, None, None, 1, None, None, None, 0, None) == E_ARG
    assert L.frcnn_proposal_recall(boxes.ctypes.data, 4, 2, 1, 1, 1, 1, 2, 0, 1, 1, 1, 1, 1, 1, ctypes.c_size_t(nbytes - 1), None) == E_ARG
    assert L.frcnn_proposal_recall_workspace_bytes(1, -1, 1) == 0
