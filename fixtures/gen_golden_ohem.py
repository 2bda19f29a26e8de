#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for online hard example mining (frcnn_ohem_select_host / frcnn_ohem_select), produced by
the numpy float64 statement fixtures/ohem_ref.py; writes tests/golden/ohem.npz.

    python fixtures/gen_golden_ohem.py            # regenerate the fixture
    python fixtures/gen_golden_ohem.py --check    # regenerate in memory and compare with the stored fixture, exit 1 on mismatch

Per case `<case>/` the inputs (rois [N,5], scores [N], n, gt [G,5], cls [N,C], pred [N,4C], B, nms_thresh, rule, seed), what the statement
gives (keep_inds, labels, counts, targets, inside, outside, out_rois, out_scores, roi_loss in float64 with NaN for a non-finite loss) and its
margins.  RoIs are jittered copies of the gt boxes plus uniform background boxes; FG_THRESH 0.5, BG_THRESH_HI 0.5, BG_THRESH_LO 0.1, so
some rows are neither.  Every case puts exact duplicates of some rows in ON PURPOSE (same box, same logits, same predictions: the same
loss bits on any implementation), which tests the row tie rule.

Margins, asserted here and again by the test; a seed that misses one is redrawn (seed + 1000) and the seed used is recorded:
  loss_gap   >= 1e-5: every pair of DISTINCT candidate losses differs by that much relative -- an implementation within 2 float32 ulps
             (2.4e-7) of the statement orders the candidates the same way
  label_gap  >= 1e-6: no row's best IoU lies that close to FG_THRESH, BG_THRESH_HI or BG_THRESH_LO
  nms_gap    >= 1e-6: no IoU the greedy pass meets lies that close to nms_thresh (float32 IoU arithmetic is within 1e-6 of float64)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "ohem.npz")
sys.path.insert(0, HERE)
import ohem_ref as ref  # noqa: E402

FG, BG_HI, BG_LO = 0.5, 0.5, 0.1
MEANS, STDS, INSIDE = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2), (1.0, 1.0, 1.0, 1.0)
LOSS_GAP, LABEL_GAP, NMS_GAP = 1e-5, 1e-6, 1e-6
# name: N, n, C, B, G, nms_thresh, rule, kind
CASES = (("c21_cpu", 64, 64, 21, 16, 3, 0.7, 0, "plain"),                 # n = N
         ("c21_gpu", 64, 64, 21, 16, 3, 0.7, 1, "plain"),
         ("c81", 48, 37, 81, 24, 7, 0.7, 0, "plain"),
         ("n0", 64, 0, 21, 16, 3, 0.7, 0, "plain"),
         ("cycle", 64, 9, 21, 16, 3, 0.7, 0, "plain"),                    # fewer candidates than B: they repeat
         ("one_kept", 40, 40, 21, 8, 1, 0.7, 0, "stack"),                 # every RoI overlaps every other one: all suppressed but one
         ("no_nms", 64, 64, 21, 16, 3, 0.0, 0, "plain"),
         ("nan", 64, 64, 21, 16, 3, 0.7, 0, "nan"))                       # a NaN logit row ranks first


def draw(rng, N, n, C, G, kind):
    f32 = np.float32
    gt = np.zeros((G, 5), dtype=f32)
    for g in range(G):
        x, y, w, h = rng.uniform(20, 400), rng.uniform(20, 300), rng.uniform(60, 180), rng.uniform(60, 180)
        gt[g] = (np.round(x), np.round(y), np.round(x + w), np.round(y + h), rng.randint(1, C))
    rois = np.zeros((N, 5), dtype=f32)
    for r in range(N):
        if kind == "stack":
            b = gt[0, :4] + rng.uniform(-4, 4, 4)
        elif rng.rand() < 0.5:
            g = gt[rng.randint(G), :4]
            s = rng.choice([0.05, 0.15, 0.4])
            b = g + rng.uniform(-s, s, 4) * np.array([g[2] - g[0], g[3] - g[1]] * 2)
        else:
            x, y = rng.uniform(0, 500), rng.uniform(0, 400)
            b = np.array([x, y, x + rng.uniform(16, 200), y + rng.uniform(16, 200)])
        rois[r, 1:] = b.astype(f32)
    cls = (rng.randn(N, C) * 2.0).astype(f32)
    pred = (rng.randn(N, 4 * C) * 0.5).astype(f32)
    scores = rng.uniform(0, 1, N).astype(f32)
    if n >= 8:                                                             # exact duplicates: rows 5 and 6 repeat row 2, row n-1 repeats row 3
        for dst, src in ((5, 2), (6, 2), (n - 1, 3)):
            rois[dst], cls[dst], pred[dst] = rois[src], cls[src], pred[src]
    if kind == "nan":
        cls[n // 2, 4] = np.nan
    return rois, scores, gt, cls, pred


def generate():
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, N, n, C, B, G, thr, rule, kind in CASES:
        seed = sum(map(ord, name))
        while True:
            rois, scores, gt, cls, pred = draw(np.random.RandomState(seed), N, n, C, G, kind)
            res = ref.select(rois, scores, n, gt, C, cls, pred, B, FG, BG_HI, BG_LO, MEANS, STDS, INSIDE, thr, rule)
            ok = res["loss_gap"] >= LOSS_GAP and res["label_gap"] >= LABEL_GAP and res["nms_gap"] >= NMS_GAP
            if n >= 8:                                                     # the duplicates must be candidates, or they test nothing
                ok = ok and res["roi_loss"][2] != 0 and res["roi_loss"][3] != 0
            if kind == "nan":
                ok = ok and np.isnan(res["roi_loss"][n // 2])
            if kind == "stack":
                ok = ok and int(res["n_kept"]) == 1
            if ok:
                break
            seed += 1000
            assert seed < 100000, "no seed with the required margins"
        p = name + "/"
        for k, v in (("rois", rois), ("scores", scores), ("n", np.int64(n)), ("gt", gt), ("cls", cls), ("pred", pred), ("B", np.int64(B)),
                     ("C", np.int64(C)), ("nms_thresh", np.float64(thr)), ("rule", np.int64(rule)), ("seed", np.int64(seed))):
            out[p + k] = v
        for k in ("keep_inds", "labels", "counts", "targets", "inside", "outside", "roi_loss", "loss_gap", "label_gap", "nms_gap", "n_kept"):
            out[p + k] = res[k]
        out[p + "out_rois"], out[p + "out_scores"] = res["rois"], res["scores"]
    return out


def compare(a, b):
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b]
    for k in sorted(set(a) & set(b)):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or not (x.tobytes() == y.tobytes()):
            bad.append(k)
    return bad


def main():
    new = generate()
    if "--check" in sys.argv:
        bad = compare(new, dict(np.load(GOLD)))
        print("numpy statement vs fixture:", "bit-exact" if not bad else "MISMATCH %s" % bad[:8])
        return 1 if bad else 0
    np.savez_compressed(GOLD, **new)
    for c in CASES:
        p = c[0] + "/"
        print("%-9s seed %5d: counts %s kept %d; gaps loss %.2g label %.2g nms %.2g" % (
            c[0], new[p + "seed"], new[p + "counts"].tolist(), new[p + "n_kept"], new[p + "loss_gap"], new[p + "label_gap"], new[p + "nms_gap"]))
    print("wrote %s (%.1f KB, %d arrays)" % (GOLD, os.path.getsize(GOLD) / 1024, len(new)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
