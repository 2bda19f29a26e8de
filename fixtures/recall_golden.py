"""TEST INFRASTRUCTURE ONLY -- reads tests/golden/recall.npz (written by fixtures/gen_golden_recall.py, whose docstring states the
layout) back into cases; used by tests/test_recall_cpu.py and tests/test_recall_gpu.py.  Needs neither the reference nor a GPU."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "recall.npz")


class Run(object):
    """one call of the reference: area, limit (None or int), use_cand, raised, and unless it raised gt_overlaps / recalls / ar /
    thresholds / num_pos and per_image (list of sorted vectors)"""


class Case(object):
    """entries: roidb entries (gt_overlaps dense); cands: float32 [n,4] per image (what the reference was given); rois / scale: the
    [n,5] layout those candidates came from (scale cases), else None / 1.0; sel[area][i]: the rows the reference counts; runs"""

    def roidb(self):
        import scipy.sparse
        return [dict(e, gt_overlaps=scipy.sparse.csr_matrix(e["gt_overlaps"])) for e in self.entries]

    def gts(self, area="all"):
        """float64 [g,4] per image: the selected ground truth as the matcher takes it"""
        return [e["boxes"][self.sel[area][i]].astype(np.float64) for i, e in enumerate(self.entries)]


def load():
    z = dict(np.load(GOLD))
    out = {}
    for c in [str(v) for v in z["cases"]]:
        k = Case()
        k.name, n = c, int(z[c + "/n_images"])
        k.entries = [dict(boxes=z["%s/%d/boxes" % (c, i)], gt_classes=z["%s/%d/gt_classes" % (c, i)], gt_overlaps=z["%s/%d/overlaps" % (c, i)],
                          seg_areas=z["%s/%d/seg_areas" % (c, i)], flipped=False) for i in range(n)]
        k.scale = np.float32(z[c + "/scale"]) if c + "/scale" in z else np.float32(1.0)
        k.rois = [z["%s/%d/rois" % (c, i)] for i in range(n)] if c + "/scale" in z else None
        k.cands = [z["%s/%d/cand" % (c, i)] for i in range(n)] if k.rois is None else [r[:, 1:] / k.scale for r in k.rois]
        k.sel, k.runs = {}, []
        for r in range(int(z[c + "/runs"])):
            p = "%s/%d/" % (c, r)
            run = Run()
            run.area, run.use_cand, run.raised = str(z[p + "area"]), bool(z[p + "use_cand"]), bool(z[p + "raised"])
            run.limit = None if int(z[p + "limit"]) < 0 else int(z[p + "limit"])
            k.sel.setdefault(run.area, [z["%s/sel/%s/%d" % (c, run.area, i)] for i in range(n)])
            if not run.raised:
                run.gt_overlaps, run.recalls, run.ar, run.thresholds = z[p + "gt_overlaps"], z[p + "recalls"], z[p + "ar"], z[p + "thresholds"]
                run.num_pos = int(z[p + "num_pos"])
                run.per_image = [z[p + "%d/gt_overlaps" % i] for i in range(n)] if n > 1 else [run.gt_overlaps]
            k.runs.append(run)
        out[c] = k
    return out


def same(a, b):
    """bit-equal float64 arrays, NaN included (num_pos == 0 gives NaN recalls in the reference too)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
