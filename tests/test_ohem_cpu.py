"""CPU: online hard example mining on the host path -- frcnn_ohem_select_host (csrc/ohem_math.h) through ops.ohem_select_host -- against
tests/golden/ohem.npz, the results of the independently written numpy float64 statement fixtures/ohem_ref.py (libm exp / log, argsort
and a loop).  The fixture keeps margins (fixtures/gen_golden_ohem.py): distinct losses differ by >= 1e-5 relative and no IoU lies within
1e-6 of a threshold, so an implementation whose per-RoI loss is within 2 float32 ulps of the statement -- double arithmetic rounded once
gives 1 -- selects exactly the same rows; exact duplicate rows are in every case on purpose and exercise the row tie rule."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import frcnn_oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fixtures"))
import gen_golden_ohem as gen  # noqa: E402

CSRC = os.path.join(ROOT, "tf-faster-rcnn_amd", "csrc")
CASES = tuple(c[0] for c in gen.CASES)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(gen.GOLD))


def run_host(g, p, **kw):
    from frcnn_hip import ops
    a = dict(batch_size=int(g[p + "B"]), fg_thresh=gen.FG, bg_hi=gen.BG_HI, bg_lo=gen.BG_LO, means=gen.MEANS, stds=gen.STDS,
             opts=ops.roi_target_opts(False, gen.INSIDE), nms_thresh=float(g[p + "nms_thresh"]), rule=int(g[p + "rule"]))
    a.update(kw)
    return ops.ohem_select_host(g[p + "rois"], g[p + "scores"], int(g[p + "n"]), g[p + "gt"], int(g[p + "C"]), g[p + "cls"], g[p + "pred"], **a)


def ulp_distance(a, b):
    """float32 ulps between a and b (same sign or zero)"""
    x, y = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(x - y)


@pytest.mark.parametrize("case", CASES)
def test_host_entry_equals_the_float64_statement(gold, case):
    p = case + "/"
    assert tuple(gold["cases"]) == CASES
    # the margins the selection's exactness rests on, as stored and as required
    assert gold[p + "loss_gap"] >= gen.LOSS_GAP and gold[p + "label_gap"] >= gen.LABEL_GAP and gold[p + "nms_gap"] >= gen.NMS_GAP
    rois, sc, labels, tg, iw, ow, counts, keep, loss = run_host(gold, p)
    want = gold[p + "roi_loss"]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(loss), nan)
    assert np.all(loss[nan].view(np.uint32) == 0x7fc00000)
    w32 = want[~nan].astype(np.float32)
    d = ulp_distance(loss[~nan], w32)
    print("%s: candidates %d, largest distance %d ulp, rows that differ %d" % (case, int((want != 0).sum()), int(d.max()) if d.size else 0, int((d > 0).sum())))
    assert np.all(d <= 2)
    assert np.array_equal(keep, gold[p + "keep_inds"]) and keep.dtype == np.int32
    assert np.array_equal(labels, gold[p + "labels"]) and np.array_equal(counts, gold[p + "counts"])
    assert rois.tobytes() == gold[p + "out_rois"].tobytes() and sc.tobytes() == gold[p + "out_scores"].tobytes()
    assert iw.tobytes() == gold[p + "inside"].tobytes() and ow.tobytes() == gold[p + "outside"].tobytes()
    # targets: what the numpy target layer (oracle/frcnn_oracle.py, proposal_target_layer.py:83-96) gives for those rows
    g, C = gold[p + "gt"], int(gold[p + "C"])
    exp = np.zeros_like(tg)
    for s, r in enumerate(keep):
        if r >= 0 and labels[s, 0] > 0:
            a = int(np.argmax(ora.bbox_overlaps(gold[p + "rois"][r:r + 1, 1:5], g[:, :4])[0]))
            t = ora.bbox_transform(gold[p + "rois"][r:r + 1, 1:5], g[a:a + 1, :4])
            c = int(labels[s, 0])
            exp[s, 4 * c:4 * c + 4] = ((t - np.array(gen.MEANS)) / np.array(gen.STDS)).astype(np.float32)[0]
    # dx, dy, every zero column: the same float32 operations, equal.  dw, dh: the numpy layer takes numpy's float32 log, a SIMD routine
    # whose documented error is below 4 ulp and whose bits depend on the CPU it runs on; the entry takes (float)log in double (host and
    # device agree on it byte for byte), which the golden targets state exactly.  4 ulp of the logarithm and one rounding of the division
    # by the std: 5 ulp of the normalised target.
    assert tg.tobytes() == gold[p + "targets"].tobytes()
    col = np.arange(tg.shape[1]) % 4
    assert np.array_equal(tg[:, col < 2], exp[:, col < 2]) and np.array_equal(tg == 0, exp == 0)
    d = ulp_distance(tg[:, col >= 2], exp[:, col >= 2])
    print("%s: dw / dh against numpy's float32 log: largest distance %d ulp" % (case, int(d.max())))
    assert np.all(d <= 5)


def test_golden_is_what_the_numpy_statement_gives(gold):
    assert os.path.getsize(gen.GOLD) < 400 * 1024
    assert gen.compare(gen.generate(), gold) == []


def test_the_cases_are_the_ones_they_claim(gold):
    k = lambda c, f: gold[c + "/" + f]
    assert k("n0", "counts").tolist() == [0, 0, 0, 0] and np.all(k("n0", "keep_inds") == -1) and not k("n0", "out_rois").any()
    m = int(k("cycle", "counts")[2] + k("cycle", "counts")[3])
    assert 0 < m < int(k("cycle", "B")) and len(set(k("cycle", "keep_inds").tolist())) == m                 # fewer candidates than B: all of them, repeated
    assert int(k("one_kept", "n_kept")) == 1 and int(k("one_kept", "B")) == 8
    assert int(k("c21_cpu", "n")) == k("c21_cpu", "rois").shape[0]                                           # n = N
    nan_row = int(k("nan", "n")) // 2
    assert np.isnan(k("nan", "roi_loss")[nan_row]) and nan_row in k("nan", "keep_inds").tolist()            # NaN ranks first: it is selected
    for c in ("c21_cpu", "c81", "no_nms"):                                                                   # the duplicates tie, the lower row first
        L, keep = k(c, "roi_loss"), k(c, "keep_inds").tolist()
        assert L[5] == L[2] == L[6] != 0
        if 2 in keep and 5 in keep:
            assert keep.index(2) < keep.index(5)
    # without NMS the selection is the B largest losses, duplicates side by side
    L = k("no_nms", "roi_loss")
    top = sorted(np.nonzero(L)[0], key=lambda r: (-L[r], r))[:int(k("no_nms", "B"))]
    assert sorted(k("no_nms", "keep_inds").tolist()) == sorted(top)


def test_nms_rules_differ_only_at_equality():
    """two identical background boxes and a threshold of exactly 1: IoU == 1 suppresses under `>=` (CPU rule) and not under `>` (GPU rule)"""
    from frcnn_hip import ops
    C = 21
    rois = np.array([[0, 100, 100, 140, 160], [0, 100, 100, 140, 160], [0, 300, 300, 340, 330]], dtype=np.float32)
    gt = np.array([[100, 100, 200, 200, 7]], dtype=np.float32)
    cls = np.zeros((3, C), dtype=np.float32)
    cls[2, 3] = 1.0                                                                                         # row 2 (IoU 0: background) loses most
    pred = np.zeros((3, 4 * C), dtype=np.float32)
    keep = {}
    for rule in (0, 1):
        keep[rule] = ops.ohem_select_host(rois, np.zeros(3), 3, gt, C, cls, pred, batch_size=2, bg_lo=0.0, nms_thresh=1.0, rule=rule)[7].tolist()
    assert keep == {0: [2, 0], 1: [2, 0]}
    cls[2, 3] = 0.0
    cls[:2, 3] = 1.0                                                                                         # now rows 0, 1 lead, equal: row order
    for rule in (0, 1):
        keep[rule] = ops.ohem_select_host(rois, np.zeros(3), 3, gt, C, cls, pred, batch_size=2, bg_lo=0.0, nms_thresh=1.0, rule=rule)[7].tolist()
    assert keep == {0: [0, 2], 1: [0, 1]}


def test_exp_and_log_against_libm_on_a_grid():
    """the two functions the loss is made of, through the loss itself: C equal logits give log C; two logits x apart give log(1 + exp(-x)).
    The stand-alone program sweeps 2^20 points each and the header records its maxima; this is the grid a test can afford."""
    from frcnn_hip import ops
    rois = np.array([[0, 300, 300, 340, 330]], dtype=np.float32)
    gt = np.array([[100, 100, 200, 200, 7]], dtype=np.float32)
    worst = 0
    for C in range(2, 82):
        cls, pred = np.zeros((1, C), dtype=np.float32), np.zeros((1, 4 * C), dtype=np.float32)
        got = ops.ohem_select_host(rois, np.zeros(1), 1, gt, C, cls, pred, batch_size=1, bg_lo=0.0)[8][0]
        worst = max(worst, int(ulp_distance(np.array([got]), np.array([np.log(np.float64(C))]))[0]))
    xs = np.linspace(0, 40, 1601).astype(np.float32)
    cls = np.zeros((len(xs), 2), dtype=np.float32)
    cls[:, 1] = xs                                                                                          # label 0: L = log(1 + exp(-x)) + x
    rois = np.tile(rois, (len(xs), 1))
    got = ops.ohem_select_host(rois, np.zeros(len(xs)), len(xs), gt, 2, cls, np.zeros((len(xs), 8), np.float32), batch_size=1, bg_lo=0.0, nms_thresh=0.0)[8]
    want = np.log1p(np.exp(-xs.astype(np.float64))) + xs.astype(np.float64)
    worst = max(worst, int(ulp_distance(got, want).max()))
    print("largest distance from libm on the grid: %d ulp" % worst)
    assert worst <= 1
    hdr = open(os.path.join(CSRC, "ohem_math.h")).read()
    assert "largest relative distance in double" in hdr and "0 of 3145731" in hdr                          # the measured maxima are written down


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """csrc/ohem_host_check.cc, built as its first lines say and run as a child process: the statement's edge cases on heap blocks of exactly
    the size it may touch, and the exp / log sweeps against libm"""
    exe = str(tmp_path / "ohem_host_check")
    # (the sanitizer runtimes linked INTO the program: it runs in whatever environment the suite runs in, as it is)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-ffp-contract=off", "-I", CSRC, os.path.join(CSRC, "ohem_host_check.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ohem_host_check: ok" in r.stdout and "more than 1 ulp away 0" in r.stdout


def test_error_codes():
    import frcnn_hip
    L = frcnn_hip.lib()
    E_ARG, E_WS, E_UNSUPPORTED = -1, -2, -3
    p = ctypes.c_void_p(64)
    m = (ctypes.c_double * 4)(0, 0, 0, 0)
    s = (ctypes.c_double * 4)(0.1, 0.1, 0.2, 0.2)
    use_gt = (ctypes.c_double * 5)(1, 1, 1, 1, 1)

    def dev(N=64, G=3, C=21, B=16, opts=None, thr=0.7, rule=0, ws=1 << 20, first=p):
        return L.frcnn_ohem_select(first, p, N, p, p, G, C, p, p, B, 0.5, 0.5, 0.0, m, s, opts, thr, rule, p, p, p, p, p, p, p, p, p, p, ws, None)

    def host(N=64, G=3, C=21, B=16, opts=None, thr=0.7, rule=0, first=p):
        return L.frcnn_ohem_select_host(first, p, N, p, p, G, C, p, p, B, 0.5, 0.5, 0.0, m, s, opts, thr, rule, p, p, p, p, p, p, p, p, p)
    # every refusal comes before anything is read, written or launched (no GPU is touched)
    for fn in (dev, host):
        for kw in (dict(thr=1.5), dict(thr=float("nan")), dict(rule=2), dict(N=0), dict(G=0), dict(C=1), dict(B=0), dict(first=None)):
            assert fn(**kw) == E_ARG, kw
        for kw in (dict(N=3073), dict(B=3073), dict(G=32768), dict(opts=use_gt)):
            assert fn(**kw) == E_UNSUPPORTED, kw
    assert dev(ws=64) == E_WS
    assert L.frcnn_ohem_workspace_bytes(3072, 81) >= 3072 * 16 and L.frcnn_ohem_workspace_bytes(1, 21) > 0


def test_cfg_keys_defaults_and_refusals():
    from model.config import cfg, ohem_description
    from nets.network import Network
    assert cfg.HIP.OHEM is False and cfg.HIP.OHEM_NMS_THRESH == 0.7 and ohem_description() is None
    Network._check_supported_cfg("TRAIN")
    saved = (cfg.HIP.OHEM, cfg.HIP.OHEM_NMS_THRESH, cfg.TRAIN.USE_GT, cfg.TRAIN.RPN_POST_NMS_TOP_N)
    try:
        cfg.HIP.OHEM = True
        Network._check_supported_cfg("TRAIN")
        assert "hard example mining" in ohem_description() and "NMS at 0.7" in ohem_description()
        for good in (0.0, -1.0, 1.0):
            cfg.HIP.OHEM_NMS_THRESH = good
            Network._check_supported_cfg("TRAIN")
        for holder, key, bad in ((cfg.HIP, "OHEM_NMS_THRESH", 1.5), (cfg.HIP, "OHEM_NMS_THRESH", float("nan")), (cfg.TRAIN, "USE_GT", True),
                                 (cfg.TRAIN, "RPN_POST_NMS_TOP_N", 3073)):
            old = holder[key]
            holder[key] = bad
            try:
                with pytest.raises(NotImplementedError, match=key):
                    Network._check_supported_cfg("TRAIN")
            finally:
                holder[key] = old
        cfg.HIP.OHEM = False                                                            # switched off, none of them is read
        cfg.TRAIN.USE_GT = True
        Network._check_supported_cfg("TRAIN")
    finally:
        cfg.HIP.OHEM, cfg.HIP.OHEM_NMS_THRESH, cfg.TRAIN.USE_GT, cfg.TRAIN.RPN_POST_NMS_TOP_N = saved


def test_header_binding_and_host_only_agree():
    import re
    import frcnn_hip
    from frcnn_hip import replay
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    for name in ("frcnn_ohem_workspace_bytes", "frcnn_ohem_select", "frcnn_ohem_select_host"):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, h)
        assert decl is not None and name in frcnn_hip.SIGNATURES
        assert len(decl.group(1).split(",")) == len(frcnn_hip.SIGNATURES[name][1])      # one ctypes entry an argument
        assert hasattr(frcnn_hip.lib(), name)
    assert "frcnn_ohem_select_host" in replay.HOST_ONLY and "frcnn_ohem_select" not in replay.HOST_ONLY
    assert re.search(r"#define\s+FRCNN_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read())
