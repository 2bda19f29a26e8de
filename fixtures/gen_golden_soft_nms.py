#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for Soft-NMS (frcnn_soft_nms_host / frcnn_soft_nms), produced by the numpy statement
fixtures/soft_nms_ref.py; writes tests/golden/soft_nms.npz.

    python fixtures/gen_golden_soft_nms.py            # regenerate the fixture
    python fixtures/gen_golden_soft_nms.py --check    # regenerate in memory and compare with the stored fixture, exit 1 on mismatch

Inputs: clustered boxes (a few centres, jittered sizes, so that chains of decays occur) of n = 1, 2, 63, 64, 65, 130, 300 rows -- the wave
and per-lane boundaries of the kernel -- with scores in (0.001, 1); both methods and both rules at TEST.NMS = 0.3, sigma 0.5, min_score
0.001.  Per size `n<n>/dets` [n,5] and `n<n>/seed`; per (method m, rule r) `n<n>/m<m>r<r>/index` (emission order), `/scores` (the decayed
scores as emitted) and `/decays` (per input row the number of weights != 1 applied to it).

The generator asserts its own margins (soft_nms_ref.soft_nms reports the smallest slack): with bound = (k + 1) * 2^-23, k the largest
number of weights != 1 applied to either score involved, the relative gap between the best and the second-best current score exceeds the
bound at every selection, and every `score < min_score` and `ov` versus threshold comparison is at least that far from equality.  An
implementation whose Gaussian weights are within 1 float32 ulp of exp therefore emits the same rows in the same order.  A seed that fails
is redrawn (seed + 1000); the seed used is recorded."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "soft_nms.npz")
sys.path.insert(0, HERE)
import soft_nms_ref as ref  # noqa: E402

SIZES = (1, 2, 63, 64, 65, 130, 300)
THRESH, SIGMA, MIN_SCORE = 0.3, 0.5, 0.001
COMBOS = tuple((m, r) for m in (1, 2) for r in (0, 1))


def generate():
    out = {"sizes": np.array(SIZES, dtype=np.int64), "thresh": np.float64(THRESH), "sigma": np.float64(SIGMA),
           "min_score": np.float32(MIN_SCORE)}
    for n in SIZES:
        seed = n
        while True:
            dets = ref.clustered(np.random.RandomState(seed), n)
            res = {(m, r): ref.soft_nms(dets, THRESH, r, m, SIGMA, MIN_SCORE) for m, r in COMBOS}
            if all(v["slack"] > 0 for v in res.values()):
                break
            seed += 1000
            assert seed < 50000, "no seed with the required margins"
        out["n%d/dets" % n], out["n%d/seed" % n] = dets, np.int64(seed)
        for (m, r), v in res.items():
            p = "n%d/m%dr%d/" % (n, m, r)
            out[p + "index"], out[p + "scores"], out[p + "decays"] = v["index"], v["scores"], v["decays"]
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
    for n in SIZES:
        print("n = %3d seed %5d: emitted %s, most decays on one box %s" % (
            n, new["n%d/seed" % n], [len(new["n%d/m%dr%d/index" % (n, m, r)]) for m, r in COMBOS],
            [int(new["n%d/m%dr%d/decays" % (n, m, r)].max()) for m, r in COMBOS]))
    print("wrote %s (%.1f KB, %d arrays)" % (GOLD, os.path.getsize(GOLD) / 1024, len(new)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
