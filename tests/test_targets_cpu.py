"""The anchor target layer and the proposal target layer of csrc/train_kernels.hip on the CPU: oracle/target_ref.py restates both
kernels step by step in numpy; oracle/target_cases.py states the border, tie, threshold, chunk-seam, mode and sampling-plan inputs;
tests/golden/targets_edges.npz holds the reference's own runs on them (oracle/gen_golden_targets.py).  Shown here:
  * the cases are what they claim (which anchors sit on the border, which IoUs tie, which sampling branch runs, the rank launch's seams);
  * the unmutated restatement equals oracle/frcnn_oracle.py and the reference goldens on every case, bit for bit: labels, weights, sampled
    rows AND regression targets (both are numpy float32), with the sampling off or the recorded draws injected;
  * every planted mistake of target_ref.MUTANTS is checked against what the suite could see before -- the inputs of targets.npz,
    targets_modes.npz and test_target_layers_degenerate_samples under the assertions the old tests make (values without sampling, counts
    and subset membership with it, the injected draws) -- and against the new cases; the mutant x case table is printed (pytest -s).
    Ten of the seventeen are invisible on the old inputs; the seven that show (OLD_VISIBLE, each with the old assertion it breaks) are kept.
  * the sampler's distribution: inclusion and pair co-inclusion counts over 4096 seeds lie within 5 sigma of the uniform k-subset's."""
import os

import numpy as np
import pytest

import frcnn_oracle as ora
import target_cases as tc
import target_ref as ref

f32 = np.float32
ACASES = tc.anchor_cases()
RCASES = tc.roi_cases()
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C = tc.NUM_CLASSES
# planted mistakes the OLD inputs already show, and the old assertion each one breaks
OLD_VISIBLE = {
    "argmax_last": "targets: an inside anchor with IoU 0 against every gt box ties at 0; its regression target follows the arg-max",
    "clobber_order": "degenerate: the single gt box's arg-max anchors lie below RPN_NEGATIVE_OVERLAP and become background, no foreground is left",
    "rank_le": "targets / degenerate: the smallest key has rank 1, one anchor too few is kept in each class and the counts miss 256",
    "rank_tail": "degenerate: candidates among the last 1956 of the 21546 anchors are not counted, 258 anchors are kept "
                 "at seed 1 (on targets.npz the old test's seeds 3 and 4 happen to keep none of the uncounted ones)",
    "bg_from_num_fg": "targets / degenerate: fewer than 128 foreground candidates, so fg + 128 anchors are kept, not 256",
    "weights_presample": "targets: the outside weights are 1 / (candidates), not 1 / 256",
    "bg_lo_gt": "targets: RoIs with IoU exactly 0 at BG_THRESH_LO = 0 leave the background candidates, whose count the old test asserts",
}


def same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def at(c, seed=-1, mutant=None, **kw):
    return ref.anchor_target_layer(c.base, c.stride, c.H, c.W, c.im_h, c.im_w, c.gt, c.batch, c.fg_fraction, c.pos_ov, c.neg_ov, seed=seed,
                                   clobber=c.clobber, pos_weight=c.pos_weight, inside_w=c.inside_w, mutant=mutant, **kw)


def pt(c, seed=0, mutant=None, **kw):
    return ref.proposal_target_layer(c.rois, c.scores, c.gt, C, c.batch, c.fg_fraction, c.fg_thresh, c.bg_hi, c.bg_lo, seed=seed, num=c.num,
                                     use_gt=c.use_gt, inside_w=c.inside_w, mutant=mutant, **kw)


def acase(name):
    return next(c for c in ACASES if c.name == name)


def rcase(name):
    return next(c for c in RCASES if c.name == name)


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(GOLD, "targets_edges.npz"))


# ----------------------------------------------------------------------------- the cases
def test_anchor_cases_are_what_they_claim():
    info = {}
    c = acase("border")
    at(c, info=info)
    an = info["anchors"]
    on_edge = (an[:, 0] >= 0) & (an[:, 1] >= 0) & (an[:, 2] <= 111) & (an[:, 3] <= 79) & ((an[:, 2] == 111) | (an[:, 3] == 79))
    assert c.H * c.W * 3 == 105 and on_edge.sum() >= 10 and not info["inside"][on_edge].any()
    assert int((at(c, mutant="inside_le")[0] != at(c)[0]).sum()) >= 10
    c = acase("tie_zero")
    at(c, info=info)
    n = (2 * 7 + 2) * 3                                                   # the anchor (32,32,47,47)
    assert an[n].tolist() == [32, 32, 47, 47] and info["ov"][n, 0] == info["ov"][n, 1] > 0.5 and c.gt[0, 4] != c.gt[1, 4]
    assert info["gtmax"][2] == 0.0 and info["inside"].sum() == 81 and info["nfg"] == 81 and info["nbg"] == 0
    assert int((at(c, mutant="gtmax_no_zero")[0] != at(c)[0]).sum()) >= 70
    at(acase("tie_zero_b32"), seed=0, info=info)
    assert (info["nfg"], info["fg_keep"]) == (81, 16)                     # foreground subsampling drops anchors
    n, v = tc.threshold_value()
    at(acase("fractional"), info=info)
    assert info["maxov"][n] == v and info["inside"][n]
    d32 = ref.iou(info["anchors"][info["inside"]], tc.FRACTIONAL_GT, f32) != info["ov"][info["inside"]]
    assert d32.size == 81 * 6 and d32.sum() > 50                          # float32 arithmetic gives another IoU
    for tag, want in (("below", -1), ("at", -1), ("above", 0)):           # `mo < neg_ov`
        assert at(acase("threshold_neg_" + tag), info=info) and info["prelabel"][n] == want, tag
    for tag, want in (("below", 1), ("at", 1), ("above", -1)):            # `mo >= pos_ov`
        assert at(acase("threshold_pos_" + tag), info=info) and info["prelabel"][n] == want, tag
    for name, plan in (("chunks_2049", (9, 2, 1025)), ("chunks_2048", (8, 1, 2048)), ("chunks_4320", (17, 3, 1440))):
        c = acase(name)
        N = c.H * c.W * c.base.shape[0]
        assert ref.rank_plan(N) == plan, name
        at(c, seed=0, info=info)
        assert info["inside"].sum() >= 300 and info["fg_keep"] < info["nfg"] and info["bg_keep"] < info["nbg"], (name, info["nfg"], info["nbg"])
        cand = np.zeros(plan[0] * 256, dtype=bool)
        cand[:N] = info["prelabel"] >= 0
        assert (~cand.reshape(-1, 256).any(axis=1)).any(), name             # a whole 256-thread block without a candidate
    assert ref.rank_plan(38 * 63 * 9) == (85, 11, 1959)                    # the one N the suite had
    for name in ("modes_border", "modes_tie_zero"):
        at(acase(name), seed=0, info=info)
        assert info["fg_keep"] < info["nfg"] and info["nbg"] > 0, name
    assert acase("many_gt_1").gt.shape[0] == 1 and acase("many_gt_100").gt.shape[0] == 100
    for c in ACASES:
        assert np.all((c.gt[:, 4] >= 1) & (c.gt[:, 4] < C)), c.name
        at(c, info=info)
        ins = np.where(info["inside"])[0]
        g = c.gt[info["argmax"][ins]]
        a = info["anchors"][ins]
        rw, rh = (g[:, 2] - g[:, 0] + 1) / (a[:, 2] - a[:, 0] + 1), (g[:, 3] - g[:, 1] + 1) / (a[:, 3] - a[:, 1] + 1)
        assert rw.min() >= 1 / 32 and rw.max() <= 32 and rh.min() >= 1 / 32 and rh.max() <= 32, c.name


def test_roi_cases_are_what_they_claim():
    plan = {}
    for c in RCASES:
        info = {}
        out = pt(c, info=info)
        plan[c.name] = (out[6].tolist(), info["fg_repl"], info["bg_repl"])
        assert np.all((c.gt[:, 4] >= 1) & (c.gt[:, 4] < C)), c.name
        assert ref.supported(c.rois.shape[0], c.gt.shape[0], c.use_gt), c.name
    assert {c.rois.shape[0] for c in RCASES} >= {1, 63, 1025, 3072} and {c.gt.shape[0] for c in RCASES} >= {1, 3, 40}
    assert {c.batch for c in RCASES} >= {16, 256, 1030}
    assert plan["n1_fg_repl"] == ([16, 0, 1, 0], True, False) and plan["n1_bg_repl"] == ([0, 16, 0, 1], False, True)
    cnt, fr, br = plan["n63_g3_b16"]
    assert cnt[0] == 4 and cnt[2] > 4 and cnt[3] > 12 and not fr and not br          # nfg above fg_per_image: foreground subsampled
    cnt, fr, br = plan["n63_g3_b256_bg_repl"]
    assert 1 < cnt[2] < 64 and cnt[0] == cnt[2] and br and cnt[3] > 1                # nfg below fg_per_image; visible bg draw
    cnt, fr, br = plan["n1025_g40_b256"]
    assert cnt[0] == 64 and cnt[2] > 64 and not br
    cnt, fr, br = plan["n3072_g3_b1030"]
    assert cnt[0] == 258 and cnt[2] > 258 and cnt[1] == 772 and not br               # round(257.5) = 258, half to even
    cnt, fr, br = plan["fg_only_repl"]
    assert cnt == [16, 0, cnt[2], 0] and 1 < cnt[2] < 16 and fr
    cnt, fr, br = plan["bg_only_repl"]
    assert cnt == [0, 16, 0, 7] and br
    info = {}
    pt(rcase("exact_thresholds"), info=info)
    assert info["best"][:3].tolist() == [0.5, 0.1, 1.0] and info["kind"].tolist() == [1, 0, 1, -1, -1, 1, 0]
    pt(rcase("tied_gt"), info=info)
    assert info["assign"][:3].tolist() == [0, 2, 0] and info["kind"][:3].tolist() == [1, 1, 1]
    c = rcase("use_gt_3072")
    assert c.rois.shape[0] + c.gt.shape[0] == 3072
    u = tc.unsupported_roi_case()
    assert u.rois.shape[0] + u.gt.shape[0] == 3073 and not ref.supported(u.rois.shape[0], u.gt.shape[0], True)
    assert plan["dn_num_0"][0] == [0, 0, 0, 0] and plan["neither"][0] == [0, 0, 0, 0]
    for name in ("dn_num_0", "neither"):
        assert all(not np.any(o) for o in pt(rcase(name))), name
    for num in (1, 62):                                                   # rows past *num would be foreground
        c = rcase("dn_num_%d" % num)
        assert pt(c, mutant="num_ignored")[6][2] == pt(c)[6][2] + (63 - num)
    pt(rcase("nonfinite_bg_lo_0.1"), info=info)
    assert info["kind"][3] == -1 and info["kind"][7] == -1 and np.isnan(info["best"][3]) == False and info["best"][3] == -1.0
    for c in RCASES:                                                      # width / height ratios of every foreground pair
        pt(c, info=info)
        nv = c.rois.shape[0] if c.num is None else c.num
        for i in info["fg_list"]:
            b = (c.rois[i, 1:5] if i < nv else c.gt[i - nv, :4]).astype(np.float64)
            g = c.gt[info["assign"][i], :4].astype(np.float64)
            rw, rh = (g[2] - g[0] + 1) / (b[2] - b[0] + 1), (g[3] - g[1] + 1) / (b[3] - b[1] + 1)
            assert 1 / 32 <= rw <= 32 and 1 / 32 <= rh <= 32, (c.name, i)


# ----------------------------------------------------------------------------- restatement == oracle == reference
@pytest.mark.parametrize("c", ACASES, ids=[c.name for c in ACASES])
def test_anchor_restatement_equals_oracle_and_reference(c, edges):
    A = c.base.shape[0]
    anc = ref.anchor_f32(c.base, c.H, c.W, c.stride)
    score = np.zeros((1, c.H, c.W, 2 * A), dtype=f32)
    info = np.array([c.im_h, c.im_w, 1.0], dtype=f32)
    want = ora.anchor_target_layer(score, c.gt, info, [c.stride], anc, A, rng=np.random.RandomState(0), batchsize=10 ** 9,
                                   fg_fraction=c.fg_fraction, pos_ov=c.pos_ov, neg_ov=c.neg_ov, clobber_positives=c.clobber,
                                   positive_weight=c.pos_weight, inside_weights=c.inside_w)
    assert same(at(c, seed=-1), want)                                     # sampling off: all four outputs, targets included
    if c.golden:
        g = [edges["at.%s.%s" % (c.name, k)] for k in ("labels", "targets", "inside", "outside")]
        assert same(at(c, disable=edges["at.%s.disable" % c.name]), g)    # the reference's run, its draws injected
        kept = int((g[0] >= 0).sum())
        assert kept <= c.batch and int((g[0] == 1).sum()) <= int(c.fg_fraction * c.batch)
    else:
        assert "at.%s.labels" % c.name not in edges.files


class _Replay(object):
    """numpy's `choice` replaying the rows a device-sampled restatement drew"""

    def __init__(self, parts):
        self.parts = list(parts)

    def choice(self, a, size=None, replace=True):
        r = self.parts.pop(0)
        assert r.size == size and np.all(np.isin(r, a))
        return r


@pytest.mark.parametrize("c", RCASES, ids=[c.name for c in RCASES])
def test_roi_restatement_equals_oracle_and_reference(c, edges):
    n = c.rois.shape[0] if c.num is None else c.num
    rois, sc = c.rois[:n], c.scores[:n].reshape(-1, 1)
    kw = dict(batch_size=c.batch, fg_fraction=c.fg_fraction, fg_thresh=c.fg_thresh, bg_hi=c.bg_hi, bg_lo=c.bg_lo, use_gt=c.use_gt,
              inside_weights=c.inside_w)
    for seed in (0, 1):
        info = {}
        got = pt(c, seed=seed, info=info)
        nf, nb = int(got[6][0]), int(got[6][1])
        if nf + nb == 0:
            with pytest.raises((RuntimeError, ValueError)):
                ora.proposal_target_layer(rois, sc, c.gt, C, rng=_Replay([]), **kw)
            continue
        # the candidate sets: the oracle's, from its own IoU
        cand = np.vstack([rois[:, 1:5], c.gt[:, :4]]) if c.use_gt else rois[:, 1:5]
        mx = ora.bbox_overlaps(cand, c.gt[:, :4]).max(axis=1)
        kind = np.where(mx >= c.fg_thresh, 1, np.where((mx < c.bg_hi) & (mx >= c.bg_lo), 0, -1))
        differ = np.where(kind != info["kind"])[0]
        if c.name == "nan_rows_bg_lo_0":      # the stated departure: a NaN row is a background candidate of the reference at BG_THRESH_LO = 0
            assert differ.tolist() == [3] and kind[3] == 0 and info["kind"][3] == -1 and np.isnan(c.rois[3, 1])
        else:
            assert differ.size == 0
        parts = [p for p in (info["src"][:nf], info["src"][nf:]) if p.size]
        with np.errstate(invalid="ignore"):
            want = ora.proposal_target_layer(rois, sc, c.gt, C, rng=_Replay(parts), **kw)
        assert same(got[:6], want), seed                                  # the drawn rows through the oracle's own emit: targets bit-exact
    if c.golden:
        g = [edges["pt.%s.%s" % (c.name, k)] for k in ("rois", "scores", "labels", "targets", "inside", "outside")]
        got = ref.proposal_target_layer(rois, sc, c.gt, C, use_gt=c.use_gt, inside_w=c.inside_w, keep_inds=edges["pt.%s.keep_inds" % c.name],
                                        n_fg=int(edges["pt.%s.n_fg" % c.name]))
        assert same(got[:6], g) and g[0].shape[0] == c.batch
    else:
        assert "pt.%s.rois" % c.name not in edges.files


def test_bg_hi_above_fg_thresh_is_foreground_only():
    """The one decision in which k_proposal_target departs from the reference: a RoI with FG_THRESH <= IoU < BG_THRESH_HI is in both of the
    reference's index sets and in the kernel's foreground set only."""
    c = rcase("exact_thresholds")
    info = {}
    ref.proposal_target_layer(c.rois, c.scores, c.gt, C, 16, fg_thresh=0.5, bg_hi=0.7, bg_lo=0.1, info=info)
    mx = ora.bbox_overlaps(c.rois[:, 1:5], c.gt[:, :4]).max(axis=1)
    both = (mx >= 0.5) & (mx < 0.7)
    assert both.tolist() == [True, False, False, False, False, True, False] and np.all(info["kind"][both] == 1)


# ----------------------------------------------------------------------------- the planted mistakes
def _old_anchor_ok(inp, golden, m):
    """what the tests before this file assert on one old anchor input, evaluated on the (mutated) restatement"""
    name, base, H, W, im_h, im_w, gt, kw = inp
    run = lambda **k: ref.anchor_target_layer(base, 16, H, W, im_h, im_w, gt, mutant=m, **dict(kw, **k))
    clean = lambda **k: ref.anchor_target_layer(base, 16, H, W, im_h, im_w, gt, **dict(kw, **k))
    full = run(seed=-1)
    if not same(full, clean(seed=-1)):                                    # test_anchor_target_layer_deterministic_part_vs_oracle_and_reference
        return False
    fl = full[0].ravel()
    if name == "degenerate":                                              # test_target_layers_degenerate_samples
        l = run(seed=1)[0].ravel()
        return bool((l == 1).sum() >= 1 and (l == 1).sum() + (l == 0).sum() == 256)
    g = golden[name]
    if not same(run(disable=g["at_disable"]), [g[k] for k in ("at_labels", "at_targets", "at_inside", "at_outside")]):
        return False                                                      # test_injected_indices_from_the_reference_run / ..._other_modes
    if name == "targets":                                                 # test_anchor_target_layer_subsampling_contract
        outs = []
        for seed in (3, 3, 4):
            lab, tg, iw, ow = run(seed=seed)
            l = lab.ravel()
            nfg, nbg = int((l == 1).sum()), int((l == 0).sum())
            ok = nfg == min(int((fl == 1).sum()), 128) and nfg + nbg == 256 and np.all(fl[l == 1] == 1) and np.all(fl[l == 0] == 0)
            ok = ok and np.allclose(ow[ow > 0], 1.0 / 256) and int((ow > 0).sum()) == 4 * 256 and int((iw > 0).sum()) == 4 * nfg
            if not ok:
                return False
            outs.append(l)
        return bool(np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2]))
    return True


def _old_roi_ok(inp, golden, m):
    name, rois, sc, gt, kw = inp
    run = lambda **k: ref.proposal_target_layer(rois, sc, gt, 21, mutant=m, **dict(kw, **k))
    if name in ("targets", "targets_modes"):
        g = golden[name]
        inj = ref.proposal_target_layer(rois, sc, gt, 21, use_gt=kw.get("use_gt", False), inside_w=kw.get("inside_w", (1, 1, 1, 1)),
                                        keep_inds=g["pt_keep_inds"], n_fg=int(g["pt_n_fg"]), mutant=m)
        if not same(inj[:6], [g["pt_" + k] for k in ("rois", "scores", "labels", "targets", "inside", "outside")]):
            return False
    if name == "targets":                                                 # test_proposal_target_layer_contract_and_values
        o_rois, o_sc, labels, tg, iw, ow, counts = run(seed=5)
        nfg_s, nbg_s, nfg_c, nbg_c = counts.tolist()
        ov = ora.bbox_overlaps(rois[:, 1:5], gt[:, :4])
        mx, am = ov.max(axis=1), ov.argmax(axis=1)
        if not (nfg_c == int((mx >= 0.5).sum()) and nbg_c == int(((mx < 0.5) & (mx >= 0.0)).sum()) and nfg_s == min(64, nfg_c) and nfg_s + nbg_s == 256):
            return False
        idx = [int(np.where((rois == r).all(axis=1))[0][0]) for r in o_rois]
        want_labels = gt[am[idx], 4].copy()
        want_labels[nfg_s:] = 0
        ok = np.all(mx[idx[:nfg_s]] >= 0.5) and np.all(mx[idx[nfg_s:]] < 0.5) and len(set(idx[:nfg_s])) == nfg_s
        ok = ok and np.array_equal(o_sc, sc[idx]) and np.array_equal(labels.ravel(), want_labels)
        t = ((ora.bbox_transform(o_rois[:, 1:5], gt[am[idx], :4]) - np.zeros(4)) / np.array((0.1, 0.1, 0.2, 0.2))).astype(f32)
        want_t, want_i = np.zeros((256, 84), dtype=f32), np.zeros((256, 84), dtype=f32)
        for i in np.where(want_labels > 0)[0]:
            want_t[i, int(4 * want_labels[i]):int(4 * want_labels[i]) + 4] = t[i]
            want_i[i, int(4 * want_labels[i]):int(4 * want_labels[i]) + 4] = 1
        return bool(ok and np.array_equal(tg, want_t) and np.array_equal(iw, want_i) and np.array_equal(ow, want_i))
    if name == "targets_modes":                                           # test_target_layers_under_the_reference_s_other_modes
        d = run(seed=7)
        return bool(d[6][0] + d[6][1] == 256 and np.array_equal(np.unique(d[4]), np.array([0.0, 0.5, 1.0], dtype=f32)) and
                    any((np.abs(d[0][:, 1:5] - b).max(axis=1) == 0).any() for b in gt[:, :4]))
    out = run(seed=0)                                                     # test_target_layers_degenerate_samples
    if name == "degenerate_bg":
        return bool(out[6][0] == 0 and out[6][1] == 64 and np.abs(out[2]).sum() == 0.0)
    return bool(out[6][0] == 16 and out[6][1] == 0 and np.all(out[2] == 4))


def test_every_mutant_against_the_old_inputs_and_the_new_cases(golden):
    old_a = tc.old_anchor_inputs()
    old_r = tc.old_roi_inputs(golden["targets"])
    assert all(_old_anchor_ok(i, golden, None) for i in old_a) and all(_old_roi_ok(i, golden, None) for i in old_r)
    clean_a = {(c.name, s): at(c, seed=s) for c in ACASES for s in tc.SEEDS}
    clean_r = {(c.name, s): pt(c, seed=s) for c in RCASES for s in tc.SEEDS}
    table, lines, old_shown = {}, [], {}
    for m in ref.MUTANTS:
        shown = [i[0] for i in old_a if not _old_anchor_ok(i, golden, m)] + [i[0] for i in old_r if not _old_roi_ok(i, golden, m)]
        old_shown[m] = shown
        caught = []
        for c in ACASES:
            hit = [s for s in tc.SEEDS if not same(at(c, seed=s, mutant=m), clean_a[(c.name, s)])]
            if hit:
                caught.append(c.name)
        for c in RCASES:
            hit = [s for s in tc.SEEDS if not same(pt(c, seed=s, mutant=m)[:6], clean_r[(c.name, s)][:6]) or
                   not np.array_equal(pt(c, seed=s, mutant=m)[6], clean_r[(c.name, s)][6])]
            if hit:
                caught.append(c.name)
        table[m] = caught
        lines.append("%-18s old inputs: %-22s new cases that catch it (%2d): %s" % (m, "SHOWN " + ",".join(shown) if shown else "hidden",
                                                                                   len(caught), " ".join(caught) or "NONE"))
    print("\nmutant x case\n" + "\n".join(lines))
    assert len(table) == 17
    for m in ref.MUTANTS:                                                 # the gap: what the old inputs could not see
        assert bool(old_shown[m]) == (m in OLD_VISIBLE), "%s on the old inputs: %s" % (m, old_shown[m] or "hidden")
    for m in ref.MUTANTS:
        assert table[m], "no new case catches " + m
    # what each case is there for
    assert "border" in table["inside_le"] and "modes_border" in table["inside_le"]
    assert {"threshold_neg_at", "threshold_neg_above", "threshold_pos_at", "threshold_pos_above"} & set(table["iou_f32"])
    assert "threshold_neg_at" in table["neg_le"] and "threshold_pos_at" in table["pos_gt"]
    assert not {"threshold_neg_below", "threshold_neg_above"} & set(table["neg_le"])
    assert not {"threshold_pos_below", "threshold_pos_above"} & set(table["pos_gt"])
    assert "tie_zero" in table["gtmax_no_zero"] and "tie_zero" in table["argmax_last"] and "tied_gt" in table["argmax_last"]
    assert "modes_tie_zero" in table["clobber_order"]
    assert "chunks_2049" in table["rank_tail"] and "chunks_2048" not in table["rank_tail"]
    assert {"chunks_2049", "chunks_2048", "chunks_4320", "tie_zero_b32"} <= set(table["rank_le"])
    assert "tie_zero_b32" in table["fg_unsampled"] and "modes_border" in table["fg_unsampled"]
    assert "fractional" in table["bg_from_num_fg"]                        # nfg below num_fg, nbg above the rest of the batch
    assert {"modes_border", "modes_tie_zero"} <= set(table["weights_presample"])
    assert {"chunks_2049", "chunks_2048", "chunks_4320"} & set(table["bg_same_seed"])
    assert {"dn_num_1", "dn_num_62", "dn_num_0", "dn_num_40_use_gt"} <= set(table["num_ignored"]) and "dn_num_63" not in table["num_ignored"]
    assert {"fg_only_repl", "bg_only_repl", "n63_g3_b256_bg_repl"} <= set(table["repl_low_bits"])
    assert "exact_thresholds" in table["fg_thresh_gt"] and "exact_thresholds" in table["bg_lo_gt"]


# ----------------------------------------------------------------------------- the sampler's distribution
@pytest.mark.parametrize("idx,keep", [(np.arange(100, 140), 10), (5 + 9 * np.arange(37), 12), (np.arange(64), 63)], ids=["40c10", "37s12", "64c63"])
@pytest.mark.parametrize("first", [0, 1], ids=["anchor_seeds", "proposal_seeds"])
@pytest.mark.parametrize("bg", [False, True], ids=["fg_keys", "bg_keys"])
def test_sampler_is_a_uniform_k_subset(idx, keep, first, bg):
    """Seeds first, first + 2, ... (Network's sequence: even for the anchor layer, odd for the proposal layer), S = 4096.  For a uniform
    k-subset of n every candidate is included with p = k / n and every pair with q = k (k - 1) / (n (n - 1)); the counts over S
    independent seeds are binomial, so each lies within 5 sigma of S p (S q) -- conditions from the binomial, not measurements."""
    S, n = 4096, idx.size
    M = np.stack([ref.sample_keep(first + 2 * i, idx, keep, bg) for i in range(S)]).astype(np.float64)
    assert np.all(M.sum(axis=1) == keep)
    p = keep / n
    q = keep * (keep - 1) / (n * (n - 1))
    single = np.abs(M.sum(axis=0) - S * p) / np.sqrt(S * p * (1 - p))
    co = M.T @ M
    pair = np.abs(co[np.triu_indices(n, 1)] - S * q) / np.sqrt(S * q * (1 - q))
    print("largest deviation: single %.2f sigma, pair %.2f sigma" % (single.max(), pair.max()))
    assert single.max() <= 5.0 and pair.max() <= 5.0


@pytest.mark.skipif(not os.path.isdir("/root/reference/lib/layer_utils"), reason="reference tree only exists in the build container")
def test_pin_against_live_reference():
    """Runs the reference itself on every golden case (subprocess: its package names collide with the host mirror); oracle and
    restatement reproduce it bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "oracle", "gen_golden_targets.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "MISMATCH" not in r.stdout and r.stdout.count("bit-exact") == 2 * (sum(c.golden for c in ACASES) + sum(c.golden for c in RCASES))
