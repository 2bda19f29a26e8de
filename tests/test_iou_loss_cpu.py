"""CPU: the IoU-family box regression losses on the host path -- frcnn_iou_loss_host (csrc/iouloss_math.h) through ops.iou_loss_host --
against tests/golden/iou_loss.npz, the results of the independently written float64 statement fixtures/iou_loss_ref.py (numpy forward,
torch float64 autograd for the gradient).  The fixture keeps a margin (fixtures/gen_golden_iou_loss.py): every gradient element that is
not exactly zero is >= 1e-6 of the largest in its slice, so float64 arithmetic rounded once stays within 2 float32 ulps of the statement;
that bound is asserted on every gradient element and on the loss, for all four kinds on every case."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import gen_golden_iou_loss as gen  # noqa: E402
import iou_loss_ref as ref  # noqa: E402

CSRC = os.path.join(ROOT, "tf-faster-rcnn_amd", "csrc")
CASES = tuple(c[0] for c in gen.DRAWN) + gen.HAND
KINDS = ref.KINDS


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(gen.GOLD))


def inputs(g, case):
    return tuple(g[case + "/" + k] for k in ("pred", "targets", "inside", "outside", "refs", "means", "stds"))


def run_host(g, case, kind):
    from frcnn_hip import ops
    return ops.iou_loss_host(*inputs(g, case), kind, g[case + "/weight"], g[case + "/divisor"], int(g[case + "/K"]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
def test_host_entry_within_two_ulps_of_the_statement(gold, case, kind):
    assert tuple(gold["cases"]) == CASES and tuple(gold["kinds"]) == KINDS
    p = case + "/" + kind + "/"
    assert gold[p + "grad_gap"] >= gen.GRAD_GAP                                          # the margin the bound rests on, as stored
    loss, grad = run_host(gold, case, kind)
    want = gold[p + "grad"]
    assert grad.dtype == np.float32 and grad.shape == want.shape and loss.shape == (1,)
    dg, dl = ref.ulps(grad, want), ref.ulps(loss, gold[p + "loss"])
    print("%s %s: largest distance gradient %d ulp, loss %d ulp; elements that differ %d of %d" % (
        case, kind, int(dg.max()), int(dl.max()), int((dg > 0).sum()), dg.size))
    assert dg.max() <= 2 and dl.max() <= 2
    # the structural zeros and the NaNs, exactly
    assert np.array_equal(grad == 0, want == 0) and np.array_equal(np.isnan(grad), np.isnan(want))
    assert np.all(grad[np.isnan(grad)].view(np.uint32) == 0x7fc00000)
    active = np.repeat((gold[case + "/inside"].reshape(-1, 4) != 0).any(axis=1), 4)
    assert np.all(grad.ravel()[~active].view(np.uint32) == 0)                            # +0, whatever the inactive slice holds


def test_golden_is_what_the_statement_gives(gold):
    assert gen.compare(gen.generate(), gold) == []
    assert os.path.getsize(gen.GOLD) < 400 * 1024
    assert ref.CLIP == 4.135166556742356                                                 # IOULOSS_CLIP of the header, digit for digit


def test_the_cases_are_the_ones_they_claim(gold):
    def decoded(case):
        p, t, iw, ow, refs, means, stds = inputs(gold, case)
        K = int(gold[case + "/K"])
        a = np.repeat(refs[:, -4:].astype(np.float64), K, axis=0)
        boxes = []
        for v in (p, t):
            d = v.reshape(-1, 4).astype(np.float64) * stds.astype(np.float64) + means.astype(np.float64)
            boxes.append((np.stack(ref._decode(np, a, v.reshape(-1, 4).astype(np.float64), means.astype(np.float64), stds.astype(np.float64),
                                               None, None, False), axis=1), d))
        return boxes, (iw.reshape(-1, 4) != 0).any(axis=1)
    shapes = {c[0]: (c[2], c[3], c[4]) for c in gen.DRAWN}
    assert shapes == {"head_5x3": (5, 3, 5), "head_70x21": (70, 21, 5), "rpn_3x5x3": (45, 1, 4), "blocks_257": (257, 1, 4),
                      "wave_64": (64, 1, 4), "wave_65": (65, 1, 4)}
    for case, (N, K, rc) in shapes.items():
        assert gold[case + "/pred"].shape == (N, 4 * K) and gold[case + "/refs"].shape == (N, rc)
        active = decoded(case)[1]
        assert 0 < active.sum() < active.size, case                                      # active and inactive slices in every drawn case
    assert tuple(gold["head_70x21/stds"]) == tuple(np.float32(gen.HEAD_STDS)) and float(gold["head_70x21/weight"]) == 2.0
    ow = gold["rpn_3x5x3/outside"][gold["rpn_3x5x3/inside"] != 0]
    assert len(np.unique(ow)) > 5 and set(np.unique(gold["rpn_3x5x3/inside"])) == {0.0, 0.5, 1.0}      # non-uniform outside, non-unit inside
    assert not decoded("none_active")[1].any() and gold["none_active/pred"].shape == (7, 8)
    (P, _), (T, _) = decoded("disjoint")[0]
    assert np.all((P[:, 0] >= T[:, 2]) | (P[:, 2] <= T[:, 0]) | (P[:, 1] >= T[:, 3]) | (P[:, 3] <= T[:, 1])) and len(P) == 3
    (P, _), (T, _) = decoded("identical")[0]
    assert np.array_equal(P, T) and len(P) == 2
    (P, _), (T, _) = decoded("enclosed")[0]
    inside = lambda a, b: np.all((a[0] > b[0]) & (a[1] > b[1]) & (a[2] < b[2]) & (a[3] < b[3]))
    assert inside(P[0], T[0]) and inside(T[1], P[1])
    (_, d), _ = decoded("clamped")[0]
    assert (d[:, 2:] > ref.CLIP).sum(axis=0).tolist() == [2, 2] and not (d[3] > ref.CLIP).any() and 4.0 < ref.CLIP
    for kind in KINDS:
        g = gold["clamped/%s/grad" % kind]
        # (the clamped boxes enclose their targets, so only the centre-distance kinds move with the centre)
        assert np.array_equal(g[:, 2:] == 0, d[:, 2:] > ref.CLIP) and np.all((g[:, :2] != 0) == (kind in ("diou", "ciou")))
        dj = gold["disjoint/%s/grad" % kind]
        assert np.all(dj == 0) if kind == "iou" else np.all((dj != 0).any(axis=1))       # only the penalty terms pull a disjoint box
        assert np.isnan(gold["nan_active/%s/loss" % kind]) and np.isfinite(gold["nan_inactive/%s/loss" % kind])
        assert np.isnan(gold["nan_active/%s/grad" % kind]).all(axis=1).tolist() == [False, True, False, True]
        assert np.all(gold["nan_inactive/%s/grad" % kind][1] == 0) and np.all(gold["none_active/%s/grad" % kind] == 0)
        assert gold["none_active/%s/loss" % kind] == 0 and not np.signbit(gold["none_active/%s/loss" % kind])
    assert np.isnan(gold["nan_inactive/pred"][1]).any() and np.isnan(gold["nan_inactive/targets"][1]).any()


def test_no_active_slice_gives_plus_zero_and_an_identical_roi_sized_pair_stays_finite(gold):
    from frcnn_hip import ops
    for kind in KINDS:
        loss, grad = run_host(gold, "none_active", kind)
        assert loss.view(np.uint32)[0] == 0 and not grad.view(np.uint32).any()
    # a RoI-sized identical pair: the loss is eps / (union + eps), v = alpha = 0 (CIoU's bits are DIoU's), nothing is NaN.  (Its GIoU gradient
    # is a difference of terms that agree to 1e-10, which float64 does not determine to 2 ulps: see fixtures/gen_golden_iou_loss.py.)
    t = np.float32([[0.05, -0.1, 0.2, -0.15]])
    a = np.float32([[100, 100, 150, 170]])
    one = np.ones((1, 4), np.float32)
    out = {k: ops.iou_loss_host(t, t, one, one, a, (0, 0, 0, 0), (1, 1, 1, 1), k, 1.0, 1.0, 1) for k in KINDS}
    for k in KINDS:
        assert 0 <= out[k][0][0] < 1e-9 and np.all(np.isfinite(out[k][1])) and np.all(out[k][1][0, :2] == 0)
    assert out["ciou"][0].tobytes() == out["diou"][0].tobytes() and out["ciou"][1].tobytes() == out["diou"][1].tobytes()


@pytest.mark.parametrize("case", ["head_5x3", "rpn_3x5x3"])
def test_statement_against_central_finite_differences(gold, case):
    """A third witness: the autograd gradient of the statement against (L(p + h) - L(p - h)) / 2h of its numpy forward, in float64, h = 1e-6.
    Tolerance: the truncation is h^2 / 6 |L'''| (1e-12 times third derivatives of the order of the gradient itself for deltas of order one),
    the roundoff 2^-52 |L| / h = 2e-10 |L| with |L| <= 3 -- so 1e-8 absolute plus 1e-6 of the case's largest gradient is ten times both."""
    p, t, iw, ow, refs, means, stds = inputs(gold, case)
    K, w, dv = int(gold[case + "/K"]), gold[case + "/weight"], gold[case + "/divisor"]
    h = 1e-6
    active = np.repeat((iw.reshape(-1, 4) != 0).any(axis=1), 4).reshape(p.shape)
    for kind in KINDS:
        g = gold[case + "/" + kind + "/grad"]
        tol = 1e-8 + 1e-6 * np.abs(g).max()
        worst = 0.0
        for idx in zip(*np.where(active)):
            lo, hi = p.astype(np.float64), p.astype(np.float64)
            lo[idx] -= h
            hi[idx] += h
            f = lambda x: ref.loss_only(x, t, iw, ow, refs, means, stds, kind, w, dv, K, alpha_at=p)      # CIoU's alpha held at p: the convention
            fd = (f(hi) - f(lo)) / (2 * h)
            worst = max(worst, abs(fd - g[idx]))
        print("%s %s: largest distance %.3g, tolerance %.3g" % (case, kind, worst, tol))
        assert worst <= tol


def test_every_mutant_of_the_statement_is_caught(gold):
    """each deliberately wrong variant of the statement is farther than 2 ulps from the golden on at least one case"""
    where = {"alpha_grad": ("ciou",), "plus_one": KINDS, "no_clamp": KINDS, "no_std": KINDS, "inside_w": KINDS}
    assert set(where) == set(ref.MUTANTS)
    for mutant in ref.MUTANTS:
        caught = []
        for case in CASES:
            for kind in where[mutant]:
                res = ref.loss_and_grad(*inputs(gold, case), kind, gold[case + "/weight"], gold[case + "/divisor"], int(gold[case + "/K"]), mutant=mutant)
                p = case + "/" + kind + "/"
                if max(ref.ulps(res["grad"].astype(np.float32), gold[p + "grad"]).max(), ref.ulps(np.float32(res["loss"]), gold[p + "loss"]).max()) > 2:
                    caught.append((case, kind))
        print(mutant, "caught by", len(caught), "case/kind pairs, e.g.", caught[:3])
        assert caught, mutant
    # and each by the case made for it
    far = lambda mutant, case, kind: ref.ulps(ref.loss_and_grad(*inputs(gold, case), kind, gold[case + "/weight"], gold[case + "/divisor"],
                                                                  int(gold[case + "/K"]), mutant=mutant)["grad"].astype(np.float32),
                                              gold[case + "/" + kind + "/grad"]).max()
    assert far("no_clamp", "clamped", "giou") > 2 and far("no_std", "head_70x21", "iou") > 2 and far("inside_w", "rpn_3x5x3", "diou") > 2
    assert far("plus_one", "enclosed", "iou") > 2 and far("alpha_grad", "head_5x3", "ciou") > 2


def test_error_codes():
    import frcnn_hip
    L = frcnn_hip.lib()
    E_ARG, E_WS, E_UNSUPPORTED = -1, -2, -3
    p = ctypes.c_void_p(64)
    f4 = lambda *v: (ctypes.c_float * 4)(*v)
    zero, one = f4(0, 0, 0, 0), f4(1, 1, 1, 1)

    def dev(N=5, K=3, rc=5, m=zero, s=one, kind=2, w=1.0, dv=5.0, ws=1 << 12, first=p, refs=p):
        return L.frcnn_iou_loss(first, p, p, p, N, K, refs, rc, m, s, kind, w, dv, p, p, p, ws, None)

    def host(N=5, K=3, rc=5, m=zero, s=one, kind=2, w=1.0, dv=5.0, first=p, refs=p, ws=None):
        return L.frcnn_iou_loss_host(first, p, p, p, N, K, refs, rc, m, s, kind, w, dv, p, p)
    # every refusal comes before anything is read, written or launched (no GPU is touched; the pointers are not dereferenced)
    for fn in (dev, host):
        for kw in (dict(first=None), dict(refs=None), dict(m=None), dict(s=None), dict(N=0), dict(N=-3), dict(K=0), dict(rc=3), dict(rc=6),
                   dict(kind=0), dict(kind=5), dict(s=f4(0.1, 0.1, 0.0, 0.2)), dict(s=f4(0.1, -0.1, 0.2, 0.2)), dict(s=f4(0.1, float("nan"), 0.2, 0.2)),
                   dict(dv=0.0), dict(dv=-1.0), dict(dv=float("nan")), dict(w=float("nan")), dict(w=float("inf"))):
            assert fn(**kw) == E_ARG, kw
        assert fn(N=1 << 31, K=1) == E_UNSUPPORTED and fn(N=1 << 20, K=1 << 12) == E_UNSUPPORTED
    assert dev(ws=0) == E_WS and dev(N=257, K=1, ws=8) == E_WS
    assert dev(ws=0, kind=9) == E_ARG                                                    # the argument check comes first
    wsb = L.frcnn_iou_loss_workspace_bytes
    assert wsb(1) >= 8 and wsb(256) >= 8 and wsb(257) >= 16 and wsb(300 * 81) >= 8 * 95 and wsb(0) > 0


def test_binding_refusals_without_a_gpu():
    from frcnn_hip import ops
    z = np.zeros((5, 12), np.float32)
    refs = np.zeros((5, 5), np.float32)
    refs[:, 3:] = 10
    args = lambda **kw: dict(dict(pred=z, targets=z, inside_w=z, outside_w=z, refs=refs, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), kind="giou",
                                  weight=1.0, mean_divisor=5.0, K=3), **kw)
    loss, grad = ops.iou_loss_host(**args())
    assert loss[0] == 0 and grad.shape == z.shape and not grad.any()
    for kw in (dict(kind="l2"), dict(K=5), dict(K=0), dict(refs=refs[:4]), dict(stds=(1, 1, 1)), dict(targets=z[:4])):
        with pytest.raises(ValueError):
            ops.iou_loss_host(**args(**kw))
    import frcnn_hip
    for kw in (dict(stds=(1, 0, 1, 1)), dict(mean_divisor=0.0), dict(weight=float("nan")), dict(kind=7), dict(refs=np.zeros((5, 3), np.float32))):
        with pytest.raises(frcnn_hip.FrcnnHipError, match="bad argument"):
            ops.iou_loss_host(**args(**kw))
    assert ops.IOU_LOSS_KINDS == {"iou": 1, "giou": 2, "diou": 3, "ciou": 4}
    assert [ops.iou_loss_host(**args(kind=k))[0][0] for k in (1, 2, 3, 4)] == [0, 0, 0, 0]


def test_header_binding_and_host_only_agree():
    import re
    import frcnn_hip
    from frcnn_hip import build, replay
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    for name in ("frcnn_iou_loss_workspace_bytes", "frcnn_iou_loss", "frcnn_iou_loss_host"):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, h)
        assert decl is not None and name in frcnn_hip.SIGNATURES
        assert len(decl.group(1).split(",")) == len(frcnn_hip.SIGNATURES[name][1])      # one ctypes entry an argument
        assert hasattr(frcnn_hip.lib(), name)
    assert "frcnn_iou_loss_host" in replay.HOST_ONLY and "frcnn_iou_loss" not in replay.HOST_ONLY
    assert re.search(r"#define\s+FRCNN_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read())
    assert "iou_loss.hip" in build.SOURCES


class _Keys(object):
    """cfg.HIP keys for the duration of a test"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from model.config import cfg
        self.old = {k: cfg.HIP[k] for k in self.kw}
        for k, v in self.kw.items():
            cfg.HIP[k] = v

    def __exit__(self, *exc):
        from model.config import cfg
        for k, v in self.old.items():
            cfg.HIP[k] = v
        return False


def test_cfg_keys_defaults_set_parsing_and_refusals():
    from model.config import BOX_LOSSES, box_loss_description, cfg, cfg_from_list
    from nets.network import Network
    h = cfg.HIP
    assert (h.BBOX_LOSS, h.RPN_BBOX_LOSS, h.BBOX_LOSS_WEIGHT, h.RPN_BBOX_LOSS_WEIGHT) == ("smooth_l1", "smooth_l1", 1.0, 1.0)
    assert box_loss_description() is None and BOX_LOSSES == Network.BOX_LOSSES == ("smooth_l1", "iou", "giou", "diou", "ciou")
    Network._check_supported_cfg("TRAIN")
    with _Keys(BBOX_LOSS="smooth_l1", RPN_BBOX_LOSS="smooth_l1", BBOX_LOSS_WEIGHT=1.0, RPN_BBOX_LOSS_WEIGHT=1.0):
        cfg_from_list(["HIP.BBOX_LOSS", "giou", "HIP.RPN_BBOX_LOSS", "diou", "HIP.BBOX_LOSS_WEIGHT", "2.5", "HIP.RPN_BBOX_LOSS_WEIGHT", "0.5"])
        assert (h.BBOX_LOSS, h.RPN_BBOX_LOSS, h.BBOX_LOSS_WEIGHT, h.RPN_BBOX_LOSS_WEIGHT) == ("giou", "diou", 2.5, 0.5)
        Network._check_supported_cfg("TRAIN")
        line = box_loss_description()
        assert "giou" in line and "diou" in line and "2.5" in line and "0.5" in line and "\n" not in line
        assert "snapshot does not record" in line and "BBOX_INSIDE_WEIGHTS only mark the active slices" in line
    with _Keys(RPN_BBOX_LOSS="ciou"):
        assert "head smooth_l1" in box_loss_description() and "RPN ciou" in box_loss_description()
    for name in BOX_LOSSES:
        with _Keys(BBOX_LOSS=name, RPN_BBOX_LOSS=name):
            Network._check_supported_cfg("TRAIN")
            Network._check_supported_cfg("TEST")
    for key in ("BBOX_LOSS", "RPN_BBOX_LOSS"):
        for bad in ("l2", "GIoU", "", None, 2):
            with _Keys(**{key: bad}):
                with pytest.raises(NotImplementedError, match="HIP." + key + " ="):
                    Network._check_supported_cfg("TRAIN")
        for bad in (0.0, -1.0, float("nan"), float("inf"), "1.0", None, True):
            with _Keys(**{key: "giou", key + "_WEIGHT": bad}):
                with pytest.raises(NotImplementedError, match=key + "_WEIGHT"):
                    Network._check_supported_cfg("TRAIN")
            with _Keys(**{key + "_WEIGHT": bad}):                                        # with smooth-L1 the weight is not read
                Network._check_supported_cfg("TRAIN")
    with _Keys(OHEM=True, BBOX_LOSS="giou"):
        with pytest.raises(NotImplementedError, match="HIP.OHEM with HIP.BBOX_LOSS"):
            Network._check_supported_cfg("TRAIN")
    with _Keys(OHEM=True, RPN_BBOX_LOSS="ciou"):                                         # mining ranks by the head's loss only
        Network._check_supported_cfg("TRAIN")


def test_recorded_step_key_changes_with_each_new_key():
    from nets.network import Network
    fake = types.SimpleNamespace(_tag="t", _image=np.zeros((1, 4, 4, 3)), _im_info=(4.0, 4.0, 1.0), _gt_boxes=types.SimpleNamespace(data_ptr=lambda: 64),
                                 _num_classes=21, _anchor_scales=(8,), _anchor_ratios=(1,))
    op = types.SimpleNamespace(lr=0.001, replay_signature=lambda: ("sig",))
    key = lambda: Network._replay_key(fake, op)
    base = key()
    assert base == key()
    seen = {base}
    for k, v in (("BBOX_LOSS", "giou"), ("RPN_BBOX_LOSS", "diou"), ("BBOX_LOSS_WEIGHT", 2.0), ("RPN_BBOX_LOSS_WEIGHT", 0.5)):
        with _Keys(**{k: v}):
            seen.add(key())
    assert len(seen) == 5 and key() == base


def test_train_state_has_no_new_switch():
    from frcnn_hip.train import TrainState
    assert len(TrainState.SWITCHES) == 12 and not [s for s in TrainState.SWITCHES if "loss" in s.lower()]


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/iou_loss_host_check.cc, built as its first lines say and run as a child process: iouloss_host on the edge cases, on heap blocks of
    exactly the size it may touch, and the exp / atan sweeps against libm"""
    exe = str(tmp_path / "iou_loss_host_check")
    src = os.path.join(CSRC, "iou_loss_host_check.cc")
    first = open(src).read().split("#include")[0]
    assert "-fsanitize=address,undefined" in first and "-ffp-contract=off" in first
    # (the sanitizer runtimes linked INTO the program: it runs in whatever environment the suite runs in, as it is)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-ffp-contract=off", "-I", CSRC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "iou_loss_host_check: ok" in r.stdout and "FAILED" not in r.stdout
