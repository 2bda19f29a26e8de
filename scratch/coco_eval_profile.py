"""frcnn_coco_match on the minival-scale random set of tests/test_coco_gpu.py: HIP-event time of the entry (both kernels) over repeats,
groups/s, and the wall time of the numpy matcher (datasets.coco_eval.match_host) on the same CSR input.  python scratch/coco_eval_profile.py [out.txt]"""
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixtures"), os.path.join(ROOT, "tf-faster-rcnn_amd"), os.path.join(ROOT, "tf-faster-rcnn_amd", "lib")]
import coco_eval_cases as cases  # noqa: E402
from datasets import coco_eval  # noqa: E402
from frcnn_hip import ops  # noqa: E402

images, cats, gts, dts = cases.random_set(seed=2, n_images=200, n_cats=80, max_gt=90, fill=0.1)
g = cases.dataset(images, cats, gts)
p = coco_eval.Params()
csr = coco_eval.build_groups(g.dataset["annotations"], g.loadRes(dts).dataset["annotations"], images, cats, 100)
D, G = np.diff(csr["det_off"]), np.diff(csr["gt_off"])
lds = D * G * 8 + 68 * G <= 16384
dev = torch.device("cuda:0")
up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
args = (up(csr["det_xywh"], np.float64), csr["det_off"], up(csr["gt_xywh"], np.float64), up(csr["gt_area"], np.float64),
        up(csr["gt_crowd"], np.uint8), csr["gt_off"], up(p.iouThrs, np.float64), up(np.array(p.areaRng, dtype=np.float64), np.float64))
for _ in range(3):
    out = ops.coco_match(*args)
torch.cuda.synchronize()
ms = []
for _ in range(30):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = ops.coco_match(*args)
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
ms = np.array(ms)
t0 = time.perf_counter()
host = coco_eval.match_host(csr, p.iouThrs, p.areaRng)
host_s = time.perf_counter() - t0
same = all(np.array_equal(o.cpu().numpy(), h) for o, h in zip(out[:3], host[:3]))
lines = ["frcnn_coco_match, minival-scale random set (fixtures/coco_eval_cases.random_set(seed=2, n_images=200, n_cats=80, max_gt=90, fill=0.1))",
         "groups %d (LDS tiles %d, workspace tiles %d), detections %d, gts %d, pairs %d, A x T = 4 x 10"
         % (len(D), lds.sum(), (~lds).sum(), csr["det_off"][-1], csr["gt_off"][-1], coco_eval.n_pairs(csr)),
         "device: %s; HIP events around ops.coco_match (offset upload + output zero-fill + offsets kernel + match kernel), 30 repeats after 3 warm-up calls"
         % torch.cuda.get_device_name(0),
         "  ms per call: median %.3f  min %.3f  max %.3f  ->  %.0f groups/s (median)" % (np.median(ms), ms.min(), ms.max(), len(D) / (np.median(ms) * 1e-3)),
         "host numpy matcher (match_host) on the same input, one run: %.2f s wall  ->  %.0f groups/s; CPU %s, numpy %s, OMP_NUM_THREADS=%s (the matcher is single-threaded numpy)"
         % (host_s, len(D) / host_s, platform.processor() or platform.machine(), np.__version__, os.environ.get("OMP_NUM_THREADS", "unset")),
         "flags equal between the two: %s" % same]
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
