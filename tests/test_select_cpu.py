"""The ordering machinery of csrc/detect_kernels.hip (proposal side) and csrc/detect_post.hip (k_perclass_nms, k_final_select) on the
CPU: oracle/select_ref.py restates make_key, the radix select, the
compaction, the counting rank, the score recovery and k_final_select in numpy; oracle/score_cases.py states the tied, saturated
and non-finite score vectors.  Shown here:
  * the unmutated restatement equals oracle/frcnn_oracle.py (order_desc / proposal_layer / proposal_top_layer / test_net_post) on
    every case;
  * every planted mistake of select_ref.MUTANTS is INVISIBLE on the inputs the suite had before -- synth.rpn_outputs(38, 63, 9,
    seed=3) with K = 6000 and synth.rcnn_outputs(300, 21, seed=7), whose scores are unique -- which is the gap;
  * every planted mistake is caught by at least one of the new cases; the mutant x case table is printed (pytest -s).
The one exception is stated where it is asserted: `wave_order` in k_final_select reorders output rows, which the old rcnn input
already shows; in k_select_topk, where the compaction order is free, it is invisible on every input."""
import numpy as np
import pytest

import frcnn_oracle as ora
import score_cases as sc
import select_ref as ref
import synth

f32 = np.float32
CASES = sc.cases()
DETECT_T = (2, 28, 29, 60)


def _anchors(H, W):
    return ora.generate_anchors_pre(H, W, sc.FEAT_STRIDE)[0]


def _order_ok(scores, K, mutant=None):
    sidx, ss = ref.sort_topk(scores, K, mutant)
    want = ora.order_desc(scores)[:K]
    return np.array_equal(sidx, want) and ref.same_scores(ss, scores[want])


def _detect_inputs(name):
    """-> scores [R,C], decoded boxes [R,4C], score_thresh"""
    if name == "present_rcnn":
        prob, deltas, rois = synth.rcnn_outputs(300, 21, seed=7)
        thresh, shape = 0.0, (600, 1000)
    elif name == "detect_zero_cut":
        prob, deltas, rois, shape, thresh = sc.detect_post_case(28, score_thresh=-0.5, cut=(0.0, -0.0), low=-0.25, fill=-0.75)
    else:
        prob, deltas, rois, shape, thresh = sc.detect_post_case(int(name.rsplit("_", 1)[1]))
    scores, boxes = ora.im_detect_post(prob, deltas, rois, 1.0, shape)
    return scores, boxes, thresh


def _detect_ok(name, mutant=None):
    scores, boxes, thresh = _detect_inputs(name)
    want = ora.detections_to_records(ora.test_net_post(scores, boxes, scores.shape[1], 0.3, 100, thresh))
    got, count = ref.detect_post(scores, boxes, scores.shape[1], 0.3, 100, thresh, 128, mutant)
    return count == want.shape[0] and got.shape == want[:128].shape and np.array_equal(got.view(np.uint32), want[:128].view(np.uint32))


DETECT_CASES = ["detect_t_%d" % t for t in DETECT_T] + ["detect_zero_cut"]
ZOO_K = (65, 257, 4097)


def test_score_cases_are_what_they_claim():
    for c in CASES:
        assert c.H * c.W * sc.A == c.N and {k for k in (1, 63, 64, 65, c.N - 1, c.N, c.N + 1) if k <= c.N + 1} <= set(c.ks), c.name
        if c.N >= 6000:
            assert 6000 in c.ks
        if c.dist in ("constant", "untrained"):                         # all keys in one 16-bit bucket
            assert np.unique(ref.sortable_u32(c.scores) >> 16).size == 1, c.name
        if c.dist != "bucket_4096" and c.dist != "bucket_4097":
            assert sc.tie_blocks(c.scores), c.name                       # ties are present
    for dist, n_in, gathered in (("bucket_4096", 4096, True), ("bucket_4097", 4097, False)):
        for N in (4104, 9207):
            c = sc.case("%s_%d" % (dist, N))
            above = int((c.scores >= 0.75).sum())
            for K in (above + 1, above + n_in):
                info = {}
                ref.sort_topk(c.scores, K, info=info)
                assert info == {"bucket": n_in, "gathered": gathered}, (c.name, K, info)
    info = {}
    ref.sort_topk(sc.case("constant_9207").scores, 6000, info=info)
    assert info == {"bucket": 9207, "gathered": False}
    prob, _ = synth.rpn_outputs(38, 63, 9, seed=3)                      # the old input: the bucket always fits the list
    ref.sort_topk(np.ascontiguousarray(prob[..., 9:]).reshape(-1), 6000, info=info)
    assert info["gathered"] and info["bucket"] < 256
    z = sc.zoo_scores(257)
    assert np.isnan(z).sum() >= 16 and (z.view(np.uint32) == 0x80000000).any() and (z.view(np.uint32) == 0).any()
    for t in DETECT_T:
        prob, _, _, _, thresh = sc.detect_post_case(t)
        assert int((prob == f32(0.5)).sum()) == t and int((prob == thresh).sum()) == 40 and np.isnan(prob).sum() == 20


def test_key_round_trip_and_order_rules():
    z = sc.zoo_scores(4097)
    keys = ref.make_key(z)
    assert np.unique(keys).size == z.size                               # unique by the index alone
    assert np.array_equal(ref.key_index(keys), np.arange(z.size))
    back = ref.key_score(keys)
    nan = np.isnan(z)
    assert np.array_equal(back.view(np.uint32)[~nan], z.view(np.uint32)[~nan])         # bit for bit, a zero's sign included
    assert np.isnan(back[nan]).all()
    # the stated order: -0.0 == +0.0 (index decides); NaN above +inf, all NaNs equal
    s = np.array([-0.0, 0.0, np.inf, np.nan, 1.0, -np.nan, -np.inf, 0.0, -0.0], dtype=f32)
    s[5] = np.array([0xffc00123], dtype=np.uint32).view(f32)[0]
    assert ora.order_desc(s).tolist() == [3, 5, 2, 4, 0, 1, 7, 8, 6]
    sidx, ss = ref.sort_topk(s, s.size)
    assert sidx.tolist() == [3, 5, 2, 4, 0, 1, 7, 8, 6] and ref.same_scores(ss, s[sidx])
    assert np.signbit(ss[4]) and not np.signbit(ss[5]) and not np.signbit(ss[6]) and np.signbit(ss[7])
    # NaN-free input: order_desc is the stable argsort of the negated scores, as it always was
    for c in CASES:
        assert np.array_equal(ora.order_desc(c.scores), np.argsort(-c.scores.astype(np.float64), kind="stable")), c.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_restatement_equals_oracle_on_the_score_cases(case):
    anchors, info = _anchors(case.H, case.W), sc.im_info(case.H, case.W)
    prob, deltas = sc.prob_blob(case.scores, case.H, case.W), sc.zero_deltas(case.H, case.W)
    for K in case.ks:
        assert _order_ok(case.scores, K), (case.name, K)
        for key in ("TEST", "TRAIN"):
            want = ora.proposal_layer(prob, deltas, info, key, sc.FEAT_STRIDE, anchors, sc.A, K, 300, 0.7)
            got = ref.proposal_layer(prob, deltas, info, anchors, sc.A, K, 300, 0.7)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and ref.same_scores(got[1], want[1]), (case.name, K)
        if K <= case.N:
            want = ora.proposal_top_layer(prob, deltas, info, sc.FEAT_STRIDE, anchors, sc.A, K)
            got = ref.proposal_top_layer(prob, deltas, info, anchors, sc.A, K)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and ref.same_scores(got[1], want[1]), (case.name, K)


def test_restatement_equals_oracle_on_zoo_and_detect_cases():
    for k in ZOO_K:
        z = sc.zoo_scores(k)
        for K in sc.k_list(z, max_blocks=3):
            assert _order_ok(z, K), (k, K)
    for name in DETECT_CASES + ["present_rcnn"]:
        assert _detect_ok(name), name
    scores, boxes, thresh = _detect_inputs("detect_t_60")
    assert ref.detect_post(scores, boxes, 21, 0.3, 100, thresh, 128)[1] == 159        # the count exceeds max_out = 128


def test_every_mutant_hides_on_the_old_inputs_and_shows_on_the_new():
    prob, deltas = synth.rpn_outputs(38, 63, 9, seed=3)
    old_scores = np.ascontiguousarray(prob[..., 9:]).reshape(-1)
    anchors, info = _anchors(38, 63), np.array([600, 1000, 1.0], dtype=f32)
    old_layer = ora.proposal_layer(prob, deltas, info, "TEST", 16, anchors, 9, 6000, 300, 0.7)
    table, lines = {}, []
    for m in ref.MUTANTS:
        # the gap: the inputs the suite had
        assert _order_ok(old_scores, 6000, m), "%s shows on synth.rpn_outputs(38, 63, 9, seed=3), K = 6000" % m
        got = ref.proposal_layer(prob, deltas, info, anchors, 9, 6000, 300, 0.7, m)
        assert np.array_equal(got[0], old_layer[0]) and np.array_equal(got[1], old_layer[1]), m
        if m == "wave_order":
            # k_final_select's output order IS compared by the old tests, so this one mistake shows on the old rcnn input too
            assert not _detect_ok("present_rcnn", m)
        else:
            assert _detect_ok("present_rcnn", m), "%s shows on synth.rcnn_outputs(300, 21, seed=7)" % m
        # the new cases
        caught = []
        for c in CASES:
            hit = [K for K in c.ks if not _order_ok(c.scores, K, m)]
            if hit:
                caught.append("%s(K=%s%s)" % (c.name, hit[0], ",..." if len(hit) > 1 else ""))
        for k in ZOO_K:
            z = sc.zoo_scores(k)
            hit = [K for K in sc.k_list(z, max_blocks=3) if not _order_ok(z, K, m)]
            if hit:
                caught.append("zoo_%d(K=%s%s)" % (k, hit[0], ",..." if len(hit) > 1 else ""))
        caught += [name for name in DETECT_CASES if not _detect_ok(name, m)]
        table[m] = caught
        old = "rpn hidden, rcnn SHOWN" if m == "wave_order" else "hidden"
        lines.append("%-16s old inputs: %s   new cases that catch it (%d): %s" % (m, old, len(caught), " ".join(caught) or "NONE"))
    print("\nmutant x case\n" + "\n".join(lines))
    for m in ref.MUTANTS:
        assert table[m], "no new case catches " + m
    # what each case is there for
    assert any(s.startswith("bucket_4097") for s in table["gather_4097"]) and not any(s.startswith("bucket_4096") for s in table["gather_4097"])
    assert any(s.startswith("constant") for s in table["cut_hi32"]) and any(s.startswith("untrained") for s in table["cut_hi32"])
    assert any(s.startswith("zoo") for s in table["signed_zero_key"]) and "detect_zero_cut" in table["signed_zero_key"]
    assert any(s.startswith("zoo") for s in table["nan_key"])
    assert set(DETECT_CASES) <= set(table["final_gt"]) and set(DETECT_CASES) <= set(table["wave_order"])
