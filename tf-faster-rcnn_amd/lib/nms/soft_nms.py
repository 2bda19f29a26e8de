"""nms.soft_nms -- Soft-NMS (Bodla et al. 2017) with the signature of the `cpu_soft_nms` that the common forks of the reference carry
(lib/nms/cpu_nms.pyx of those forks; it is not part of this project's reference, so parity with it is unpinned).

The rule is csrc/softnms_math.h: pick the largest current score (ties: the lower row), stop below `threshold`, emit, multiply every
other unselected score by the weight of its IoU with the pick.  method 1 (linear): 1 - IoU where the net's hard rule would have
suppressed at `Nt`, else 1; method 2 (Gaussian): exp(-IoU^2 / sigma).  Two stated differences from the published code: its order among
equal scores depends on its in-place swaps (here: the lower row first), and its linear test is always `IoU > Nt` (here it follows
cfg.USE_GPU_NMS like every other NMS of the net: `>` with it, the Cython `>=` without).

Runs frcnn_soft_nms on the device when there is one, else frcnn_soft_nms_host -- the same bits either way.  At most 1024 boxes."""
import numpy as np

from frcnn_hip import NMS_RULE_CPU, NMS_RULE_GPU, ops


def _rule():
    from model.config import cfg
    return NMS_RULE_GPU if cfg.USE_GPU_NMS else NMS_RULE_CPU


def soft_nms(dets, method=1, sigma=0.5, Nt=0.3, threshold=0.001, rule=None):
    """dets [n,5] = x1,y1,x2,y2,score -> (dets_out f32 [m,5]: the emitted rows in emission order with their decayed scores,
    keep: their rows in `dets`)."""
    import torch
    dets = np.ascontiguousarray(dets, dtype=np.float32)
    if dets.ndim != 2 or dets.shape[1] != 5:
        raise ValueError("soft_nms: dets must be [n,5], got %r" % (dets.shape,))
    if method not in (1, 2):
        raise ValueError("soft_nms: method must be 1 (linear) or 2 (Gaussian), got %r" % (method,))
    rule = _rule() if rule is None else rule
    if dets.shape[0] == 0:
        return np.zeros((0, 5), dtype=np.float32), []
    if torch.cuda.is_available():
        out, index, count = ops.soft_nms(torch.from_numpy(dets).cuda(), Nt, rule, method, sigma, threshold)
        n = int(count.item())
        out, index = out[:n].cpu().numpy(), index[:n].cpu().numpy()
    else:
        out, index = ops.soft_nms_host(dets, Nt, rule, method, sigma, threshold)
    return out, index.astype(np.intp).tolist()


def cpu_soft_nms(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """The published signature: -> keep, the rows of `boxes` in emission order.  method 0 is the existing hard NMS at Nt."""
    if method == 0:
        from model.nms_wrapper import nms
        return nms(np.ascontiguousarray(boxes, dtype=np.float32), Nt)
    return soft_nms(boxes, method, sigma, Nt, threshold)[1]
