#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for the IoU-family box regression losses (frcnn_iou_loss_host / frcnn_iou_loss), produced by
the float64 statement fixtures/iou_loss_ref.py; writes tests/golden/iou_loss.npz.

    python fixtures/gen_golden_iou_loss.py            # regenerate the fixture
    python fixtures/gen_golden_iou_loss.py --check    # regenerate in memory and compare with the stored fixture, exit 1 on mismatch

Per case `<case>/` the inputs (pred, targets, inside, outside [N,4K] float32, refs [N,ref_cols] float32, means, stds float32 [4], K, weight,
divisor) and per kind `<case>/<kind>/` what the statement gives: loss (float64), grad [N,4K] (float64) and the case's margin grad_gap.

Margin, asserted here and again by the test: grad_gap >= 1e-6 -- every gradient element of the statement that is not exactly zero (an
inactive slice, a clamped coordinate, the IoU term of a disjoint pair, a centre that does not move the loss of an identical pair) is at
least that fraction of the largest in its slice, for all four kinds.  A row of a drawn case that misses it is drawn again (the count is
stored as `redrawn`); the hand-made cases have no row that misses it.  With that margin float64 arithmetic rounded once stays within 2
float32 ulps of the statement: the terms of an element cancel to no less than 1e-6 of the largest, which costs 1e-16 / 1e-6 = 1e-10
relative, far below half a float32 ulp (6e-8); libm differences are another 1e-16."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "iou_loss.npz")
sys.path.insert(0, HERE)
import iou_loss_ref as ref  # noqa: E402

GRAD_GAP = 1e-6
ZERO4, ONE4 = (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)
HEAD_STDS = (0.1, 0.1, 0.2, 0.2)
# name: layout, N, K, ref_cols, means, stds, weight, divisor
DRAWN = (("head_5x3", "head", 5, 3, 5, ZERO4, HEAD_STDS, 1.0, 5.0),
         ("head_70x21", "head", 70, 21, 5, (0.0, 0.0, 0.0, 0.0), HEAD_STDS, 2.0, 70.0),
         ("rpn_3x5x3", "rpn", 45, 1, 4, ZERO4, ONE4, 1.0, 1.0),                  # H 3, W 5, A 3; non-uniform outside, non-unit inside weights
         ("blocks_257", "rpn", 257, 1, 4, ZERO4, ONE4, 0.5, 1.0),                # two blocks, a one-row tail
         ("wave_64", "rpn", 64, 1, 4, ZERO4, ONE4, 1.0, 1.0),
         ("wave_65", "rpn", 65, 1, 4, ZERO4, ONE4, 1.0, 1.0))
HAND = ("none_active", "disjoint", "identical", "enclosed", "clamped", "nan_active", "nan_inactive")


def draw_row(rng, layout, K, means, stds):
    """one row: (ref box [4], pred, targets, inside, outside [4K])"""
    f32 = np.float32
    x, y = rng.uniform(0, 500), rng.uniform(0, 350)
    a = np.array([x, y, x + rng.uniform(15, 250), y + rng.uniform(15, 250)]).astype(f32)
    pred, tg, iw, ow = (np.zeros(4 * K, dtype=f32) for _ in range(4))
    pred[:] = (rng.randn(4 * K) * 0.3).astype(f32)                             # every class predicts something; most slices are inactive
    if layout == "head":
        active = [int(rng.randint(1, K))] if rng.rand() < 0.45 else []
    else:
        active = [0] if rng.rand() < 0.5 else []
    m, s = np.asarray(means, f32).astype(np.float64), np.asarray(stds, f32).astype(np.float64)
    for k in active:
        d = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6)])
        t = ((d - m) / s).astype(f32)
        noise = rng.uniform(-1, 1, 4) * rng.choice([0.02, 0.2, 0.8]) / s * np.array([1, 1, 1, 1])
        tg[4 * k:4 * k + 4] = t
        pred[4 * k:4 * k + 4] = (t + noise).astype(f32)
        if layout == "head":
            iw[4 * k:4 * k + 4], ow[4 * k:4 * k + 4] = 1.0, 1.0
        else:
            iw[4 * k:4 * k + 4] = (1.0, 1.0, 0.5, 0.0)
            ow[4 * k:4 * k + 4] = f32(rng.uniform(0.002, 0.02))
    return a, pred, tg, iw, ow


def assemble(rows, ref_cols):
    a, pred, tg, iw, ow = (np.stack([r[i] for r in rows]) for i in range(5))
    refs = a if ref_cols == 4 else np.concatenate([np.zeros((a.shape[0], 1), np.float32), a], axis=1)
    return dict(pred=pred, targets=tg, inside=iw, outside=ow, refs=refs)


def gap_per_row(res_grad, K):
    """the smallest |g| / max|g| over the non-zero elements of each row's slices (inf where there are none)"""
    g = np.abs(res_grad.reshape(-1, 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where((g > 0) & np.isfinite(g), g / g.max(axis=1, keepdims=True), np.inf)
    return ratio.min(axis=1).reshape(-1, K).min(axis=1)


def statement(c, kind):
    return ref.loss_and_grad(c["pred"], c["targets"], c["inside"], c["outside"], c["refs"], c["means"], c["stds"], kind, c["weight"],
                             c["divisor"], c["K"])


def drawn_case(name, layout, N, K, ref_cols, means, stds, weight, divisor):
    rng = np.random.RandomState(sum(map(ord, name)))
    rows = [draw_row(rng, layout, K, means, stds) for _ in range(N)]
    redrawn = 0
    while True:
        c = assemble(rows, ref_cols)
        c.update(means=np.asarray(means, np.float32), stds=np.asarray(stds, np.float32), K=np.int64(K), weight=np.float32(weight),
                 divisor=np.float32(divisor))
        gap = np.min([gap_per_row(statement(c, kind)["grad"], K) for kind in ref.KINDS], axis=0)
        bad = np.where(gap < GRAD_GAP)[0]
        if not bad.size:
            break
        for r in bad:
            rows[r] = draw_row(rng, layout, K, means, stds)
        redrawn += int(bad.size)
        assert redrawn < 10 * N, "no draw with the required margin"
    c["redrawn"] = np.int64(redrawn)
    return c


def hand_case(name):
    """K = 1, anchors as references (ref_cols 4), means 0, stds 1, except none_active (K = 2, RoI references)"""
    f32 = np.float32
    box = np.array([100.0, 100.0, 150.0, 170.0], dtype=f32)
    t0 = np.array([0.05, -0.1, 0.2, -0.15], dtype=f32)
    # The identical pair sits on a reference box of one pixel and decodes to a box of about 0.05 x 0.08: at the optimum the GIoU gradient is
    # the difference of two terms that agree to eps / union.  On a RoI-sized box (union ~ 1e3) that is 1e-10, float64 keeps 1e-6 of the
    # difference and NO order of additions reproduces another's bits to 2 float32 ulps -- the statement itself is not determined there; on
    # this box eps / union is 2e-5 and float64 keeps 1e-11.  (tests/test_iou_loss_cpu.py holds a RoI-sized identical pair to what can be
    # asked of it: a loss below 1e-9, finite gradients, CIoU's bits equal to DIoU's.)
    tiny = np.array([0.05, -0.1, -3.0, -2.5], dtype=f32)
    rows = {"disjoint": [(t0 + f32([3.0, 0.05, 0.1, -0.1]), t0), (t0 + f32([0.1, -4.0, 0.3, 0.1]), t0), (t0 + f32([2.5, 2.5, -0.2, 0.2]), t0)],
            "identical": [(tiny, tiny), (tiny * f32(1.25), tiny * f32(1.25))],
            "enclosed": [(t0 + f32([0.02, 0.03, -1.0, -0.8]), t0), (t0 + f32([-0.03, 0.01, 0.9, 1.1]), t0)],       # P inside T, T inside P
            "clamped": [(f32([0.1, 0.0, 5.0, 0.3]), t0), (f32([0.0, 0.2, 0.1, 4.5]), t0), (f32([0.1, 0.1, 6.0, 7.0]), t0),
                        (f32([0.1, 0.0, 4.0, 0.3]), t0)],                                                           # the last one: below the clamp
            "nan_active": [(t0 + f32(0.1), t0), (f32([0.1, np.nan, 0.0, 0.2]), t0), (t0 - f32(0.1), t0), (t0, f32([np.nan, 0, 0, 0]))],
            "nan_inactive": [(t0 + f32(0.1), t0), (f32([np.nan, np.nan, 0.0, 0.2]), f32([0, np.nan, 0, 0])), (t0 - f32(0.1), t0)]}
    if name == "none_active":
        rng = np.random.RandomState(7)
        N, K = 7, 2
        c = dict(pred=rng.randn(N, 8).astype(f32), targets=rng.randn(N, 8).astype(f32), inside=np.zeros((N, 8), f32),
                 outside=np.ones((N, 8), f32), refs=np.concatenate([np.zeros((N, 1), f32), np.tile(box, (N, 1))], axis=1))
        c.update(means=f32(ZERO4), stds=f32(HEAD_STDS), K=np.int64(K), weight=f32(1.0), divisor=f32(N))
    else:
        rs = rows[name]
        N = len(rs)
        c = dict(pred=np.stack([r[0] for r in rs]).astype(f32), targets=np.stack([r[1] for r in rs]).astype(f32), inside=np.ones((N, 4), f32),
                 outside=np.full((N, 4), 0.25, f32), refs=np.stack([box + f32(7 * i) for i in range(N)]))
        if name == "identical":
            c["refs"][:, 2:] = c["refs"][:, :2]
        if name == "nan_inactive":
            c["inside"][1] = 0.0
        c.update(means=f32(ZERO4), stds=f32(ONE4), K=np.int64(1), weight=f32(1.0), divisor=f32(1.0))
    c["redrawn"] = np.int64(0)
    return c


def generate():
    out = {"cases": np.array([c[0] for c in DRAWN] + list(HAND)), "kinds": np.array(ref.KINDS)}
    for spec in DRAWN:
        _store(out, spec[0], drawn_case(*spec))
    for name in HAND:
        _store(out, name, hand_case(name))
    return out


def _store(out, name, c):
    for k, v in c.items():
        out[name + "/" + k] = v
    K = int(c["K"])
    for kind in ref.KINDS:
        res = statement(c, kind)
        gap = float(np.min(gap_per_row(res["grad"], K)))
        assert gap >= GRAD_GAP, "%s/%s: grad_gap %.3g" % (name, kind, gap)
        p = name + "/" + kind + "/"
        out[p + "loss"], out[p + "grad"], out[p + "grad_gap"] = res["loss"], res["grad"], np.float64(gap)


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
        print("statement vs fixture:", "bit-exact" if not bad else "MISMATCH %s" % bad[:8])
        return 1 if bad else 0
    np.savez_compressed(GOLD, **new)
    for name in new["cases"]:
        act = int((new[name + "/inside"].reshape(-1, 4) != 0).any(axis=1).sum())
        print("%-13s N %3d K %2d active %3d redrawn %d; grad_gap %s; loss %s" % (
            name, new[name + "/pred"].shape[0], new[name + "/K"], act, new[name + "/redrawn"],
            " ".join("%.2g" % new[name + "/" + k + "/grad_gap"] for k in ref.KINDS), " ".join("%.6g" % new[name + "/" + k + "/loss"] for k in ref.KINDS)))
    print("wrote %s (%.1f KB, %d arrays)" % (GOLD, os.path.getsize(GOLD) / 1024, len(new)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
