"""TEST INFRASTRUCTURE ONLY -- Soft-NMS (Bodla et al. 2017) as plain numpy, the second statement of the rule that
tf-faster-rcnn_amd/csrc/softnms_math.h holds for the kernels and the host entry.  Written from the rule's text, not from that header:

    IoU        float32 throughout, "+1" widths, one numpy operation (= one rounding) per step, the order of cpu_nms.pyx:57-64
    loop       pick the largest current score, the lower row among equal ones; stop when it is < min_score; emit it; multiply every
               other unselected score by its weight as ONE float32 product
    linear     1 - ov where the hard rule suppresses -- rule 0 (Cython): float64(ov) >= thresh; rule 1 (CUDA): ov > float32(thresh)
    gaussian   float32(numpy.exp(-(float64(ov) * float64(ov)) / sigma))   (libm's exp: the header's own exponential is allowed 1 ulp of
               float32 around it, hence the per-box bound below)

Besides the emission it reports what the fixture generator needs to assert its margins: per box the number of weights != 1 applied to it
(k), and the smallest slack of every comparison against `bound = (k + 1) * 2^-23` -- one weight that may differ by one float32 ulp plus one
product rounding per decay, relative.  A slack > 0 means the comparison cannot come out differently within that bound."""
import numpy as np

F = np.float32
ULP = 2.0 ** -23


def iou(a, b):
    """a float32 [4], b float32 [n,4] -> float32 [n]"""
    aa = ((a[2] - a[0]) + F(1)) * ((a[3] - a[1]) + F(1))
    ab = ((b[:, 2] - b[:, 0]) + F(1)) * ((b[:, 3] - b[:, 1]) + F(1))
    xx1, yy1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    xx2, yy2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    w = np.maximum(F(0), (xx2 - xx1) + F(1))
    h = np.maximum(F(0), (yy2 - yy1) + F(1))
    inter = w * h
    out = inter / ((aa + ab) - inter)
    assert out.dtype == np.float32
    return out


def soft_nms(dets, thresh, rule, method, sigma, min_score):
    """dets [n,5] float32 -> dict(index int32 [m], scores float32 [m], decays int32 [n], slack float: the smallest margin left over)"""
    dets = np.ascontiguousarray(dets, dtype=np.float32)
    n = dets.shape[0]
    boxes, cur = dets[:, :4], dets[:, 4].copy()
    alive = np.ones(n, dtype=bool)
    k = np.zeros(n, dtype=np.int32)
    index, scores = [], []
    slack = np.inf
    ms = float(min_score)
    while alive.any():
        rows = np.flatnonzero(alive)
        order = rows[np.lexsort((rows, -cur[rows].astype(np.float64)))]          # score descending, row ascending
        best = order[0]
        s1 = float(cur[best])
        if len(order) > 1:
            second = order[1]
            s2 = float(cur[second])
            slack = min(slack, (s1 - s2) / s1 - (max(k[best], k[second]) + 1) * ULP if s1 > 0 else -1.0)
        if ms > 0:
            # the only score compared with min_score is the best one; on a stop every remaining score is below it by the gap asserted above
            slack = min(slack, abs(s1 - ms) / ms - (k[best] + 1) * ULP)
        if cur[best] < F(min_score):
            break
        index.append(best), scores.append(cur[best])
        alive[best] = False
        rest = np.flatnonzero(alive)
        if rest.size == 0:
            break
        ov = iou(boxes[best], boxes[rest])
        if method == 1:
            hit = (ov.astype(np.float64) >= float(thresh)) if rule == 0 else (ov > F(thresh))
            w = np.where(hit, F(1) - ov, F(1)).astype(np.float32)
            t = float(thresh)
            slack = min(slack, float(np.min(np.abs(ov.astype(np.float64) - t) / t - (k[rest] + 1) * ULP)))
        else:
            o64 = ov.astype(np.float64)
            w = np.exp(-(o64 * o64) / float(sigma)).astype(np.float32)
        cur[rest] = cur[rest] * w
        k[rest] += (w != F(1))
    return dict(index=np.array(index, dtype=np.int32), scores=np.array(scores, dtype=np.float32), decays=k, slack=float(slack))


def clustered(rng, n, centres=None, width=800.0, height=600.0):
    """n boxes around a few centres with jittered position and size (chains of decays), scores in (0.001, 1); float32 [n,5]"""
    centres = max(1, min(8, n // 12 + 1)) if centres is None else centres
    cx, cy = rng.uniform(100, width - 100, centres), rng.uniform(100, height - 100, centres)
    bw, bh = rng.uniform(60, 220, centres), rng.uniform(60, 220, centres)
    c = rng.randint(0, centres, n)
    x = cx[c] + rng.uniform(-0.25, 0.25, n) * bw[c]
    y = cy[c] + rng.uniform(-0.25, 0.25, n) * bh[c]
    w = bw[c] * rng.uniform(0.7, 1.3, n)
    h = bh[c] * rng.uniform(0.7, 1.3, n)
    d = np.stack([x - w / 2, y - h / 2, x + w / 2, y + h / 2, rng.uniform(0.002, 0.999, n)], axis=1)
    d[:, 0], d[:, 1] = np.maximum(d[:, 0], 0), np.maximum(d[:, 1], 0)
    d[:, 2], d[:, 3] = np.minimum(d[:, 2], width - 1), np.minimum(d[:, 3], height - 1)
    return np.ascontiguousarray(d, dtype=np.float32)
