#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for bounding-box voting (frcnn_box_vote_host / frcnn_box_vote), produced by the numpy
statement fixtures/box_vote_ref.py; writes tests/golden/box_vote.npz.

    python fixtures/gen_golden_box_vote.py            # regenerate the fixture
    python fixtures/gen_golden_box_vote.py --check    # regenerate in memory and compare with the stored fixture, exit 1 on mismatch

Inputs: the clustered boxes of the Soft-NMS fixture's generator (soft_nms_ref.clustered(RandomState(100 + n), n)) for n = 1, 2, 63, 64, 65,
130, 300 -- the candidates, in row order, with their original scores.  Two kept lists per size: `hard`, the rows greedy NMS keeps at 0.3
(Cython rule), and `soft`, all n rows in the emission order of linear Soft-NMS at min_score 0 with their decayed scores (m = n).  Both
vote thresholds 0.8 and 0.5.  Per size `n<n>/cands` [n,5]; per list `n<n>/<list>/kept` [m,5]; per threshold `n<n>/<list>/t<50|80>/out`
[m,5] and `/voters` [m].

The generator asserts that the vectors are not trivial: at 0.5, for n >= 63, more than half of the kept detections have at least two
voters and at least one box changes its bits; at either threshold every detection has at least one voter (itself)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "box_vote.npz")
sys.path.insert(0, HERE)
import box_vote_ref as ref  # noqa: E402
import soft_nms_ref  # noqa: E402

SIZES = (1, 2, 63, 64, 65, 130, 300)
NMS = 0.3
THRESHOLDS = ((80, 0.8), (50, 0.5))
LISTS = ("hard", "soft")


def kept_lists(cands):
    """-> dict(hard = the rows greedy NMS keeps, soft = every row in linear Soft-NMS's emission order with its decayed score)"""
    soft = soft_nms_ref.soft_nms(cands, NMS, 0, 1, 0.5, 0.0)
    assert len(soft["index"]) == len(cands)
    return dict(hard=cands[ref.hard_nms(cands, NMS)],
                soft=np.ascontiguousarray(np.hstack([cands[soft["index"], :4], soft["scores"][:, None]]), dtype=np.float32))


def assert_not_trivial(n, kept, out, voters, tag):
    assert voters.min() >= 1, (n, tag)
    if tag == 50 and n >= 63:
        assert 2 * int((voters >= 2).sum()) > len(voters), (n, "at 0.5 more than half of the kept detections must have two voters", voters)
        assert out[:, :4].tobytes() != kept[:, :4].tobytes(), (n, "at 0.5 at least one box must change")


def generate():
    out = {"sizes": np.array(SIZES, dtype=np.int64), "nms": np.float64(NMS)}
    for n in SIZES:
        cands = ref.clustered(np.random.RandomState(100 + n), n)
        out["n%d/cands" % n] = cands
        for name, kept in kept_lists(cands).items():
            out["n%d/%s/kept" % (n, name)] = kept
            for tag, t in THRESHOLDS:
                voted, voters = ref.vote(kept, cands, t)
                assert_not_trivial(n, kept, voted, voters, tag)
                out["n%d/%s/t%d/out" % (n, name, tag)], out["n%d/%s/t%d/voters" % (n, name, tag)] = voted, voters
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
        print("n = %3d: kept %s; with a second voter at 0.8 / 0.5: %s" % (
            n, [len(new["n%d/%s/kept" % (n, k)]) for k in LISTS],
            [[int((new["n%d/%s/t%d/voters" % (n, k, tag)] >= 2).sum()) for tag, _ in THRESHOLDS] for k in LISTS]))
    print("wrote %s (%.1f KB, %d arrays)" % (GOLD, os.path.getsize(GOLD) / 1024, len(new)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
