#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for RoIAlign (frcnn_roi_align_host / frcnn_roi_align_batched), produced by the numpy
float32 statement fixtures/roi_align_ref.py:align_f32; writes tests/golden/roi_align.npz.

    python fixtures/gen_golden_roi_align.py            # regenerate the fixture
    python fixtures/gen_golden_roi_align.py --check    # regenerate in memory and compare with the stored fixture, exit 1 on mismatch

Inputs: the edge map of the tests (two images of 5 x 6 at stride 16) and the six edge RoIs of roi_align_ref.EDGE_ROIS followed by a row
with image index 7 and a row with image index -1 (both: zero output).  `rois` [8,5]; per channel count `c<C>/feat` [2,5,6,C]
(RandomState(500 + C)); per case `c<C>/p<P>s<S>/out` [8,P,P,C].  Cases: C = 4 at (P, S) = (7,2), (7,1), (7,3), (2,1), (14,4) and C = 64 at
(2,1) -- the file stays under 200 KB; the larger channel counts are compared with align_f32 on fresh seeds by the tests.

The generator asserts that the edge RoIs still take the branches they are there for (roi_align_ref.EDGE_KINDS_7_2 against a count of its
own from the numpy taps)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "roi_align.npz")
sys.path.insert(0, HERE)
import roi_align_ref as ref  # noqa: E402

CASES = ((4, 7, 2), (4, 7, 1), (4, 7, 3), (4, 2, 1), (4, 14, 4), (64, 2, 1))


def all_rois():
    return np.concatenate([ref.EDGE_ROIS, np.array([[7, 16, 16, 48, 48], [-1, 16, 16, 48, 48]], dtype=np.float32)]).astype(np.float32)


def numpy_kinds(rois, P, S):
    """(zeroed, clamped-high) sample counts per RoI from the numpy taps, independent of the library"""
    r, ty, tx = ref._taps(rois, ref.EDGE_STRIDE, ref.EDGE_H, ref.EDGE_W, P, S)
    out = []
    for k in range(r.shape[0]):
        ok = ty["valid"][k][:, None] & tx["valid"][k][None, :]
        high = (ty["lo"][k] >= ref.EDGE_H - 1)[:, None] | (tx["lo"][k] >= ref.EDGE_W - 1)[None, :]
        out.append((int((~ok).sum()), int((ok & high).sum())))
    return out


def generate():
    rois = all_rois()
    for (zero, high), want in zip(numpy_kinds(ref.EDGE_ROIS, 7, 2), ref.EDGE_KINDS_7_2):
        assert (zero, high) == (want[0], want[2]), ("an edge RoI stopped exercising its branch", zero, high, want)
    out = {"rois": rois, "stride": np.float64(ref.EDGE_STRIDE)}
    for C, P, S in CASES:
        key = "c%d/feat" % C
        if key not in out:
            out[key] = np.random.RandomState(500 + C).randn(2, ref.EDGE_H, ref.EDGE_W, C).astype(np.float32)
        o = ref.align_f32(out[key], rois, ref.EDGE_STRIDE, P, S)
        assert o.dtype == np.float32 and not o[6:].any() and o[:6].any()
        out["c%d/p%ds%d/out" % (C, P, S)] = o
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
    print("wrote %s (%.1f KB, %d arrays)" % (GOLD, os.path.getsize(GOLD) / 1024, len(new)))
    assert os.path.getsize(GOLD) < 200 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
