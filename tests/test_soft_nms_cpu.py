"""CPU: Soft-NMS on the host path -- frcnn_soft_nms_host (csrc/softnms_math.h) through ops.soft_nms_host and nms.soft_nms -- against
tests/golden/soft_nms.npz, the results of the numpy statement fixtures/soft_nms_ref.py on clustered boxes whose every comparison keeps
a margin of (k + 1) * 2^-23 (k = the weights != 1 applied to the scores involved; fixtures/gen_golden_soft_nms.py asserts it).  Emission
order is therefore exact for both methods; linear scores are the same float32 operations on both sides, hence bit-identical; Gaussian
scores may differ by one float32 ulp per weight (the header's own exponential against libm's) plus one product rounding per decay."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import gen_golden_soft_nms as gen  # noqa: E402
import soft_nms_ref as ref  # noqa: E402

SIZES = (1, 2, 63, 64, 65, 130, 300)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(gen.GOLD))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method,rule", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_host_entry_equals_the_golden(gold, n, method, rule):
    from frcnn_hip import ops
    assert tuple(gold["sizes"]) == SIZES
    dets, p = gold["n%d/dets" % n], "n%d/m%dr%d/" % (n, method, rule)
    out, index = ops.soft_nms_host(dets, float(gold["thresh"]), rule, method, float(gold["sigma"]), float(gold["min_score"]))
    assert index.dtype == np.int32 and np.array_equal(index, gold[p + "index"])
    assert np.array_equal(out[:, :4], dets[index, :4])
    want = gold[p + "scores"]
    if method == 1:
        assert out[:, 4].tobytes() == want.tobytes()
    else:
        rel = np.abs(out[:, 4].astype(np.float64) - want.astype(np.float64)) / want.astype(np.float64)
        bound = (gold[p + "decays"][index].astype(np.float64) + 1) * 2.0 ** -23
        print("n %d rule %d: largest relative distance %.3g, tightest bound %.3g, scores that differ %d of %d"
              % (n, rule, rel.max(), bound.min(), int((out[:, 4] != want).sum()), len(want)))
        assert np.all(rel <= bound)


def test_golden_is_what_the_numpy_statement_gives(gold):
    assert os.path.getsize(gen.GOLD) < 200 * 1024
    assert gen.compare(gen.generate(), gold) == []
    assert max(int(gold["n300/m2r%d/decays" % r].max()) for r in (0, 1)) >= 20            # chains of decays do occur
    assert all(len(gold["n300/m%dr0/index" % m]) < 300 for m in (1, 2))                   # ... and min_score drops rows


def _disjoint(n, rng):
    """n boxes of 20 x 20 on a grid of pitch 40: every IoU is 0"""
    d = np.zeros((n, 5), dtype=np.float32)
    d[:, 0], d[:, 1] = (np.arange(n) % 16) * 40, (np.arange(n) // 16) * 40
    d[:, 2], d[:, 3] = d[:, 0] + 20, d[:, 1] + 20
    d[:, 4] = rng.uniform(0.01, 1, n).astype(np.float32)
    return d


def test_linear_on_disjoint_boxes_is_a_sort_by_score_then_row():
    from frcnn_hip import ops
    d = _disjoint(100, np.random.RandomState(1))
    d[10:20, 4] = d[40, 4]                                                                 # equal scores: the lower row first
    for rule in (0, 1):
        out, index = ops.soft_nms_host(d, 0.3, rule, 1, 0.5, 0.001)
        want = np.lexsort((np.arange(100), -d[:, 4].astype(np.float64)))
        assert np.array_equal(index, want) and out.tobytes() == d[want].tobytes()
    out, index = ops.soft_nms_host(d, 0.3, 0, 2, 0.5, 0.001)                               # Gaussian: IoU 0 has weight exactly 1
    assert np.array_equal(index, want) and out.tobytes() == d[want].tobytes()


@pytest.mark.parametrize("method", [1, 2])
def test_properties_on_clustered_boxes(method):
    from frcnn_hip import ops
    d = ref.clustered(np.random.RandomState(7), 200)
    out, index = ops.soft_nms_host(d, 0.3, 0, method, 0.5, 0.0)
    assert len(index) == 200 and sorted(index.tolist()) == list(range(200))                # min_score = 0 emits all n
    assert index[0] == int(np.argmax(d[:, 4])) and out[0].tobytes() == d[index[0]].tobytes()
    assert np.all(np.diff(out[:, 4]) <= 0)                                                 # non-increasing
    assert np.all(out[:, 4] <= d[index, 4]) and np.any(out[:, 4] < d[index, 4])
    some, idx = ops.soft_nms_host(d, 0.3, 0, method, 0.5, 0.05)
    assert 0 < len(idx) < 200 and np.all(some[:, 4] >= np.float32(0.05)) and np.array_equal(idx, index[:len(idx)])
    assert some.tobytes() == out[:len(idx)].tobytes()                                      # a higher min_score only stops earlier


def test_error_codes():
    import frcnn_hip
    L = frcnn_hip.lib()
    d = np.ascontiguousarray(ref.clustered(np.random.RandomState(2), 8))
    big = np.zeros((1025, 5), dtype=np.float32)
    out, idx, cnt = np.zeros((1025, 5), dtype=np.float32), np.zeros(1025, dtype=np.int32), np.full(1, 77, dtype=np.int32)

    def run(dets=d, k=8, rule=0, method=1, sigma=0.5, min_score=0.001, o=out, i=idx, c=cnt):
        return L.frcnn_soft_nms_host(None if dets is None else dets.ctypes.data, k, 0.3, rule, method, sigma, min_score,
                                     None if o is None else o.ctypes.data, None if i is None else i.ctypes.data,
                                     None if c is None else c.ctypes.data)
    E_ARG, E_UNSUPPORTED = -1, -3
    assert run() == 0 and cnt[0] > 0
    cnt[0] = 77
    for kw in (dict(method=0), dict(method=3), dict(rule=2), dict(rule=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(min_score=float("nan")), dict(dets=None), dict(o=None), dict(i=None), dict(c=None), dict(k=-1)):
        assert run(**kw) == E_ARG, kw
    assert run(dets=big, k=1025) == E_UNSUPPORTED
    assert run(dets=big, k=1025, method=5) == E_ARG                                         # the argument check comes first
    assert cnt[0] == 77                                                                    # nothing was written
    assert run(dets=big, k=1024, min_score=0.0) == 0 and cnt[0] == 1024
    # the device entries refuse the same arguments before they launch anything (no GPU is touched)
    p = ctypes.c_void_p(64)
    for kw in (dict(method=0), dict(rule=2), dict(sigma=0.0), dict(sigma=float("nan")), dict(min_score=float("nan"))):
        a = dict(rule=0, method=1, sigma=0.5, min_score=0.001)
        a.update(kw)
        assert L.frcnn_soft_nms(p, 8, 0.3, a["rule"], a["method"], a["sigma"], a["min_score"], p, p, p, None) == E_ARG, kw
        assert L.frcnn_detect_post_soft_batched(p, p, p, None, 1, 8, 3, 1.0, 100, 100, 0.3, a["rule"], 0.0, 100, a["method"], a["sigma"],
                                                a["min_score"], p, p, 128, 0, p, 1 << 20, None) == E_ARG, kw
    assert L.frcnn_soft_nms(None, 8, 0.3, 0, 1, 0.5, 0.001, p, p, p, None) == E_ARG
    assert L.frcnn_soft_nms(p, 1025, 0.3, 0, 1, 0.5, 0.001, p, p, p, None) == E_UNSUPPORTED
    assert L.frcnn_detect_post_soft_batched(p, p, p, None, 1, 1025, 3, 1.0, 100, 100, 0.3, 0, 0.0, 100, 1, 0.5, 0.001, p, p, 128, 0, p,
                                            1 << 30, None) == E_UNSUPPORTED
    assert L.frcnn_detect_post_soft_batched_workspace_bytes(2, 300, 21) == L.frcnn_detect_post_batched_workspace_bytes(2, 300, 21)


def test_python_front_ends_without_a_gpu():
    """nms.soft_nms falls back to the host entry where there is no device; cpu_soft_nms has the published signature"""
    import torch
    from frcnn_hip import ops
    from nms.soft_nms import cpu_soft_nms, soft_nms
    sig = inspect.signature(cpu_soft_nms)
    assert list(sig.parameters) == ["boxes", "sigma", "Nt", "threshold", "method"]
    assert [sig.parameters[k].default for k in ("sigma", "Nt", "threshold", "method")] == [0.5, 0.3, 0.001, 0]
    assert list(inspect.signature(soft_nms).parameters)[:5] == ["dets", "method", "sigma", "Nt", "threshold"]
    sig = inspect.signature(ops.detect_post)
    assert [sig.parameters[k].default for k in ("soft", "sigma", "min_score")] == [0, 0.5, 0.001]
    if torch.cuda.is_available():
        return
    d = ref.clustered(np.random.RandomState(3), 90)
    for method in (1, 2):
        out, keep = soft_nms(d, method, 0.5, 0.3, 0.001)
        want, idx = ops.soft_nms_host(d, 0.3, 0, method, 0.5, 0.001)                       # the suite pins the Cython rule
        assert keep == idx.tolist() and out.tobytes() == want.tobytes()
        assert cpu_soft_nms(d, 0.5, 0.3, 0.001, method) == keep
    assert soft_nms(np.zeros((0, 5), dtype=np.float32), 1)[1] == []
    with pytest.raises(ValueError):
        soft_nms(d, 3)


def test_cfg_keys_defaults_and_refusals():
    from model.config import cfg
    from nets.network import Network
    assert (cfg.HIP.SOFT_NMS, cfg.HIP.SOFT_NMS_SIGMA, cfg.HIP.SOFT_NMS_MIN_SCORE) == (0, 0.5, 0.001)
    Network._check_supported_cfg("TEST")
    for key, bad in (("SOFT_NMS", 3), ("SOFT_NMS", -1), ("SOFT_NMS_SIGMA", 0.0), ("SOFT_NMS_SIGMA", -0.5), ("SOFT_NMS_SIGMA", float("nan")),
                     ("SOFT_NMS_MIN_SCORE", -0.001)):
        old = cfg.HIP[key]
        cfg.HIP[key] = bad
        try:
            with pytest.raises(NotImplementedError, match=key):
                Network._check_supported_cfg("TEST")
        finally:
            cfg.HIP[key] = old
    for key, good in (("SOFT_NMS", 1), ("SOFT_NMS", 2), ("SOFT_NMS_MIN_SCORE", 0.0), ("SOFT_NMS_SIGMA", 2.0)):
        old = cfg.HIP[key]
        cfg.HIP[key] = good
        try:
            Network._check_supported_cfg("TEST")
        finally:
            cfg.HIP[key] = old


def test_the_host_entry_is_never_recorded():
    from frcnn_hip import replay
    assert "frcnn_soft_nms_host" in replay.HOST_ONLY
    assert not {"frcnn_soft_nms", "frcnn_detect_post_soft_batched"} & set(replay.HOST_ONLY)
