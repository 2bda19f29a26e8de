#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for proposal recall (datasets.recall, imdb.evaluate_recall, frcnn_proposal_recall),
produced by calling the REFERENCE's own imdb.evaluate_recall (lib/datasets/imdb.py:126-214, imported through oracle/ref_shim.py) on a
minimal subclass that only supplies _roidb, _classes and _image_index; writes tests/golden/recall.npz.  Must run in a process that has
not imported the host mirror (the package names collide).

    python fixtures/gen_golden_recall.py            # regenerate the fixture
    python fixtures/gen_golden_recall.py --check    # compare the live reference with the stored fixture, exit 1 on mismatch

The npz holds arrays only.  Per case `c`: c/n_images, and per image i the roidb entry (c/i/boxes uint16 [R,4], c/i/gt_classes int32,
c/i/overlaps float32 [R,C] dense, c/i/seg_areas float32) and its candidates (c/i/cand float32 [N,4]; case 7: c/i/rois [N,5] and c/scale,
the expected candidates being rois / scale in float32).  Per run r of a case (c/runs = how many): c/r/area (str), c/r/limit (-1 = None),
c/r/use_cand (0: candidate_boxes=None), c/r/raised (the reference's AssertionError), and unless it raised c/r/gt_overlaps, c/r/recalls,
c/r/ar, c/r/thresholds, c/r/num_pos and, for cases of several images, c/r/i/gt_overlaps, the sorted vector of image i alone (a one-image
imdb).  c/sel/<area>/i: the rows of image i the reference counts as positives for that area.

What the reference does not return is read off its behaviour, never restated: a row is a positive iff a one-row roidb holding it,
matched against its own box, gives recall 1 (an unselected row gives 0 / 0); num_pos is the number of such rows."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden", "recall.npz")
AREAS = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")
NUM_CLASSES = 4


def entry(boxes, classes=None, crowd=(), seg_areas=None):
    """a roidb entry as dense arrays: gt rows overlap their class with 1, crowd rows with -1, class-0 rows with nothing"""
    boxes = np.asarray(boxes, dtype=np.uint16).reshape(-1, 4)
    R = boxes.shape[0]
    classes = np.ones(R, dtype=np.int32) if classes is None else np.asarray(classes, dtype=np.int32)
    ov = np.zeros((R, NUM_CLASSES), dtype=np.float32)
    for r in range(R):
        if classes[r] > 0:
            ov[r, classes[r]] = -1.0 if r in crowd else 1.0
    if seg_areas is None:
        seg_areas = ((boxes[:, 2].astype(np.float32) - boxes[:, 0] + 1) * (boxes[:, 3].astype(np.float32) - boxes[:, 1] + 1))
    return dict(boxes=boxes, gt_classes=classes, overlaps=ov, seg_areas=np.asarray(seg_areas, dtype=np.float32))


def random_gts(rng, n, width, height, lo=20, hi=200):
    w, h = rng.randint(lo, hi, size=n), rng.randint(lo, hi, size=n)
    x, y = rng.randint(0, width - hi, size=n), rng.randint(0, height - hi, size=n)
    return np.stack([x, y, x + w, y + h], axis=1).astype(np.uint16)


def jittered(rng, gts, n, far, amp=12.0):
    """n candidates: gt boxes jittered by +-amp px (corners kept ordered), the last `far` of them moved where nothing overlaps; shuffled"""
    src = gts[np.arange(n) % len(gts)].astype(np.float32)
    c = src + (np.round(rng.uniform(-amp, amp, size=src.shape) * 16) / 16).astype(np.float32)      # sixteenths of a pixel: still not integers
    c[:, 2:] = np.maximum(c[:, 2:], c[:, :2] + 1)
    c[n - far:] += np.float32(5000)
    return np.ascontiguousarray(c[rng.permutation(n)], dtype=np.float32)


def cases():
    """-> {name: dict(entries=[...], cands=[...], runs=[(area, limit, use_cand)], [rois, scale])}"""
    out = {}
    # 1: gt B is covered by nothing; candidates 1 and 2 are identical (the first wins), the zero match consumes candidate 0
    out["hand"] = dict(entries=[entry([[10, 10, 50, 50], [200, 200, 240, 240]])],
                       cands=[np.array([[300, 300, 310, 310], [12, 12, 48, 48], [12, 12, 48, 48]], dtype=np.float32)],
                       runs=[("all", -1, 1)])
    # 2: no candidates / no gts / ordinary, in one call
    out["empty"] = dict(entries=[entry([[5, 5, 40, 60], [50, 20, 90, 80], [100, 100, 160, 150]]), entry(np.zeros((0, 4))),
                                 entry([[20, 30, 80, 90], [120, 40, 200, 140]])],
                        cands=[np.zeros((0, 4), dtype=np.float32), np.array([[1, 2, 30, 40], [5, 5, 50, 50]], dtype=np.float32),
                               np.array([[25, 28, 85, 95], [300, 300, 320, 320], [118, 44, 190, 150], [22, 30, 78, 88]], dtype=np.float32)],
                        runs=[("all", -1, 1), ("all", 2, 1)])
    # 3: more rows than a workgroup has threads, more columns than a wave has lanes
    rng = np.random.RandomState(3)
    gts = random_gts(rng, 70, 1000, 600)
    big = jittered(rng, gts, 2000, 200)
    out["large"] = dict(entries=[entry(gts)], cands=[big], runs=[("all", lim, 1) for lim in (-1, 1000, 300, 100)])
    # 4: exact ties in different rows and columns: 8 translated copies of one integer pattern
    pg = np.array([[10, 10, 40, 40], [30, 10, 60, 40], [10, 50, 30, 80]])
    pc = np.array([[10, 10, 40, 40], [20, 10, 50, 40], [30, 10, 60, 40], [12, 10, 42, 40], [28, 10, 58, 40], [10, 50, 30, 80], [10, 52, 30, 82],
                   [10, 48, 30, 78], [70, 70, 90, 90], [0, 0, 100, 100]])
    shifts = [(dx, dy) for dy in (0, 300) for dx in (0, 200, 400, 600)]
    tg = np.concatenate([pg + [dx, dy, dx, dy] for dx, dy in shifts])
    tc = np.concatenate([pc + [dx, dy, dx, dy] for dx, dy in shifts[::-1]]).astype(np.float32)
    out["ties"] = dict(entries=[entry(tg)], cands=[tc], runs=[("all", -1, 1), ("all", 40, 1)])
    # 5: seg_areas unrelated to the boxes, on the inclusive ends; two crowd rows, two class-0 rows
    rng = np.random.RandomState(5)
    sa = [32 ** 2 - 1, 32 ** 2, 32 ** 2 + 1, 96 ** 2, 96 ** 2 + 1, 128 ** 2, 128 ** 2 + 1, 256 ** 2, 256 ** 2 + 1, 512 ** 2, 512 ** 2 + 1, 100,
          5000, 70000, 7, 9]
    ab = random_gts(rng, 16, 900, 700)
    cls = np.array([1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3, 0, 0], dtype=np.int32)
    out["areas"] = dict(entries=[entry(ab, cls, crowd=(12, 13), seg_areas=sa)], cands=[jittered(rng, ab[:14], 60, 6)],
                        runs=[(a, -1, u) for u in (1, 0) for a in AREAS])
    # 6: fewer candidates than gts
    rng = np.random.RandomState(6)
    fg = random_gts(rng, 7, 600, 400)
    out["few"] = dict(entries=[entry(fg)], cands=[jittered(rng, fg, 5, 0)], runs=[("all", -1, 1)])
    # 7: case 3's candidates as rois * s; the expected candidates are rois / s in float32
    for name, s in (("scale16", np.float32(1.6)), ("scale600", np.float32(600.0 / 375.0))):
        rois = np.zeros((big.shape[0], 5), dtype=np.float32)
        rois[:, 1:] = big * s
        out[name] = dict(entries=[entry(gts)], cands=[rois[:, 1:] / s], rois=[rois], scale=s, runs=[("all", -1, 1), ("all", 300, 1)])
    # 8: more gts than the kernel keeps column state for in LDS
    rng = np.random.RandomState(8)
    mg = random_gts(rng, 1030, 4000, 3000, lo=10, hi=120)
    out["many"] = dict(entries=[entry(mg)], cands=[jittered(rng, mg, 1100, 40, amp=6.0)], runs=[("all", -1, 1)])
    return out


def reference_results():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shim
    ref_shim.load_reference()
    import scipy.sparse
    from datasets.imdb import imdb as ref_imdb

    class Toy(ref_imdb):
        def __init__(self, entries):
            ref_imdb.__init__(self, "toy", ["__background__"] + ["c%d" % k for k in range(1, NUM_CLASSES)])
            self._image_index = list(range(len(entries)))
            self._roidb = [dict(boxes=e["boxes"], gt_classes=e["gt_classes"], gt_overlaps=scipy.sparse.csr_matrix(e["overlaps"]),
                                seg_areas=e["seg_areas"], flipped=False) for e in entries]

    def run(entries, cands, area, limit, use_cand):
        try:
            return Toy(entries).evaluate_recall(candidate_boxes=cands if use_cand else None, area=area, limit=None if limit < 0 else limit)
        except AssertionError:
            return None

    def selected(e, area):
        rows = []
        for r in range(e["boxes"].shape[0]):
            one = {k: v[r:r + 1] for k, v in e.items()}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = run([one], [one["boxes"].astype(np.float32)], area, -1, 1)
            if res["recalls"][0] == 1.0:
                rows.append(r)
        return np.array(rows, dtype=np.int64)

    out = {"cases": np.array(list(cases()))}
    for c, case in cases().items():
        n = len(case["entries"])
        out[c + "/n_images"] = np.int64(n)
        for i, (e, cand) in enumerate(zip(case["entries"], case["cands"])):
            for k, v in e.items():
                out["%s/%d/%s" % (c, i, k)] = v
            if "rois" in case:
                out["%s/%d/rois" % (c, i)] = case["rois"][i]
            else:
                out["%s/%d/cand" % (c, i)] = cand
        if "scale" in case:
            out[c + "/scale"] = case["scale"]
        sel = {}
        for area in sorted(set(a for a, _, _ in case["runs"])):
            for i, e in enumerate(case["entries"]):
                sel[area, i] = out["%s/sel/%s/%d" % (c, area, i)] = selected(e, area)
        out[c + "/runs"] = np.int64(len(case["runs"]))
        for r, (area, limit, use_cand) in enumerate(case["runs"]):
            p = "%s/%d/" % (c, r)
            out[p + "area"], out[p + "limit"], out[p + "use_cand"] = np.array(area), np.int64(limit), np.int64(use_cand)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                      # num_pos == 0: the reference divides by zero and returns NaN recalls
                res = run(case["entries"], case["cands"], area, limit, use_cand)
                out[p + "raised"] = np.int64(res is None)
                if res is None:
                    continue
                for k in ("gt_overlaps", "recalls", "ar", "thresholds"):
                    out[p + k] = np.asarray(res[k], dtype=np.float64)
                out[p + "num_pos"] = np.int64(sum(len(sel[area, i]) for i in range(n)))
                for i in range(n if n > 1 else 0):                  # (one image: its vector is the whole result)
                    one = run(case["entries"][i:i + 1], case["cands"][i:i + 1], area, limit, use_cand)
                    out[p + "%d/gt_overlaps" % i] = np.asarray(one["gt_overlaps"], dtype=np.float64)
    return out


def compare(a, b):
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b]
    for k in sorted(set(a) & set(b)):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or not (x.tobytes() == y.tobytes()):
            bad.append(k)
    return bad


def main():
    ref = reference_results()
    if "--check" in sys.argv:
        bad = compare(ref, dict(np.load(GOLD)))
        print("live reference vs fixture:", "bit-exact" if not bad else "MISMATCH %s" % bad[:8])
        return 1 if bad else 0
    np.savez_compressed(GOLD, **ref)
    print("wrote %s (%.1f KB, %d arrays)" % (GOLD, os.path.getsize(GOLD) / 1024, len(ref)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
