"""TEST INFRASTRUCTURE ONLY -- the anchor target layer and the proposal target layer of csrc/train_kernels.hip restated step by step
in numpy: what the KERNELS do, in their order (anchor_f32, the strict inside test, ohem_iou_f64, the first-maximum arg-max, the per-gt
maximum over inside anchors, the label order, hash_key and the counting rank, fg_keep / bg_keep of k_at_finish, the weights, the three
layouts; the candidate set, kind / assign, fg_list / bg_list, the four-way sampling plan, the with-replacement draws and pt_emit_row of
k_proposal_target).  The sampler is a fixed splitmix64 finaliser, so WHICH rows a seed draws is stated here exactly, not only how many.

Where the kernel knowingly departs from the reference (layer_utils/proposal_target_layer.py:112-116): with BG_THRESH_HI > FG_THRESH the
reference puts a RoI whose maximum IoU lies in [FG_THRESH, BG_THRESH_HI) into BOTH index sets, so it can be drawn as foreground and
again as background; k_proposal_target decides `else if` and makes it foreground only.  No shipped configuration sets the thresholds that
way.  (Not a decision but a consequence of ohem_iou_f64's operand order, found by the `nan_rows_bg_lo_0` case: a RoI row with a NaN
coordinate has IoU NaN here and is neither foreground nor background at ANY BG_THRESH_LO; Cython's min / max in utils/bbox.pyx give such
a row IoU 0, so the reference agrees at BG_THRESH_LO > 0 and makes it a background candidate at BG_THRESH_LO = 0.  Rows with infinite
coordinates have IoU 0 in both.)  Everything else is the reference's rule: frcnn_oracle.anchor_target_layer / proposal_target_layer and the reference's own runs
recorded in tests/golden/targets_edges.npz (oracle/gen_golden_targets.py) agree with this file bit for bit once the draws are injected.

Regression targets are float32 numpy here (np.log), like the oracle; the device's logf is held to the oracle's bounds by the GPU test.

The `mutant` argument plants ONE mistake of the kind such code can carry.  tests/test_targets_cpu.py shows for each that the inputs the
suite had before oracle/target_cases.py do not see it, and which of the new cases do."""
import numpy as np

f32 = np.float32
u64 = np.uint64

MUTANTS = (
    "inside_le",          # inside test `<=` on x2 / y2
    "iou_f32",            # IoU in float32 arithmetic
    "argmax_last",        # the last maximum on ties
    "gtmax_no_zero",      # the gt-argmax rule skips gt boxes whose maximum is zero
    "pos_gt",             # `>` at the positive threshold
    "neg_le",             # `<=` at the negative threshold
    "clobber_order",      # negatives and positives applied in the other order
    "rank_le",            # k_key_rank counts `<=`
    "rank_tail",          # the last j-chunk's remainder is not counted
    "fg_unsampled",       # fg_keep = nfg
    "bg_from_num_fg",     # bg_keep = batch - num_fg
    "weights_presample",  # outside weights from the candidate counts
    "bg_same_seed",       # background keys use the foreground seed
    "num_ignored",        # rows past *num are candidates
    "repl_low_bits",      # the with-replacement draw uses the key's low word (the index)
    "fg_thresh_gt",       # `>` at FG_THRESH
    "bg_lo_gt",           # `>` at BG_THRESH_LO
)
NO_KEY = u64(0xFFFFFFFFFFFFFFFF)
BG_SEED_XOR = 0xA5A5A5A5DEADBEEF
FG_REPL_XOR, BG_REPL_XOR = 0x1234567, 0x7654321
PT_MAXN = 3072


# ----------------------------------------------------------------------------- shared pieces
def hash_key(seed, idx):
    """hash_key(seed, idx) of csrc/train_kernels.hip on uint64: splitmix64's finaliser, low word replaced by the index."""
    seed = u64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    idx = np.asarray(idx).astype(u64)
    with np.errstate(over="ignore"):
        z = seed + u64(0x9E3779B97F4A7C15) * (idx + u64(1))
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    z = z ^ (z >> u64(31))
    return (z & ~u64(0xFFFFFFFF)) | idx


def anchor_f32(base, H, W, stride):
    """anchor n = (h * W + w) * A + a: float64 base + shift, rounded to float32 -> [H*W*A, 4]"""
    base = np.asarray(base, dtype=np.float64)
    sx = (np.arange(W, dtype=np.int64) * int(stride)).astype(np.float64)
    sy = (np.arange(H, dtype=np.int64) * int(stride)).astype(np.float64)
    shift = np.stack([np.tile(sx, H), np.repeat(sy, W), np.tile(sx, H), np.repeat(sy, W)], axis=1)
    return (shift[:, None, :] + base[None, :, :]).reshape(-1, 4).astype(f32)


def iou(boxes, gt, dtype=np.float64):
    """ohem_iou_f64 (csrc/ohem_math.h) for every (box, gt) pair, its comparisons and operation order kept (so a NaN coordinate gives
    NaN, as there).  dtype float32 is the `iou_f32` mistake."""
    b = np.asarray(boxes, dtype=f32).astype(dtype)[:, None, :]
    q = np.asarray(gt, dtype=f32)[:, :4].astype(dtype)[None, :, :]
    one = dtype(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        area = (q[..., 2] - q[..., 0] + one) * (q[..., 3] - q[..., 1] + one)
        iw = np.where(b[..., 2] < q[..., 2], b[..., 2], q[..., 2]) - np.where(b[..., 0] > q[..., 0], b[..., 0], q[..., 0]) + one
        ih = np.where(b[..., 3] < q[..., 3], b[..., 3], q[..., 3]) - np.where(b[..., 1] > q[..., 1], b[..., 1], q[..., 1]) + one
        ua = (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one) + area - iw * ih
        o = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), o, dtype(0)).astype(np.float64)


def first_max(ov, mutant=None):
    """`best = -1, bi = 0; if (o > best) best = o, bi = g` over g: the FIRST maximum; a NaN never wins -> (best [N], bi [N])"""
    G = ov.shape[1]
    o = np.where(np.isnan(ov), -2.0, ov)
    if mutant == "argmax_last":
        bi = G - 1 - np.argmax(o[:, ::-1], axis=1)
    else:
        bi = np.argmax(o, axis=1)
    best = o[np.arange(o.shape[0]), bi]
    none = best < -1.0
    return np.where(none, -1.0, best), np.where(none, 0, bi).astype(np.int64)


def encode_box(ex, gt):
    """encode_box: bbox_transform for row pairs, float32, one rounding per operation"""
    ex, gt = np.asarray(ex, dtype=f32), np.asarray(gt, dtype=f32)
    one, half = f32(1), f32(0.5)
    ew, eh = (ex[:, 2] - ex[:, 0]) + one, (ex[:, 3] - ex[:, 1]) + one
    ecx, ecy = ex[:, 0] + half * ew, ex[:, 1] + half * eh
    gw, gh = (gt[:, 2] - gt[:, 0]) + one, (gt[:, 3] - gt[:, 1]) + one
    gcx, gcy = gt[:, 0] + half * gw, gt[:, 1] + half * gh
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([(gcx - ecx) / ew, (gcy - ecy) / eh, np.log(gw / ew), np.log(gh / eh)], axis=1).astype(f32)


def rank_plan(N):
    """launch_key_rank: (i-blocks of 256, j-chunks, keys per j-chunk)"""
    cdiv = lambda a, b: (a + b - 1) // b
    iblocks = cdiv(N, 256)
    js = max(1, min(cdiv(N, 2048), cdiv(4096, iblocks)))
    jchunk = cdiv(N, js)
    return iblocks, cdiv(N, jchunk), jchunk


def key_rank(keys, mutant=None):
    """k_key_rank: for every candidate (key != ~0) the number of keys smaller than its own; 0 elsewhere"""
    N = keys.shape[0]
    counted = keys
    if mutant == "rank_tail":
        jchunk = rank_plan(N)[2]
        counted = keys[:(N // jchunk) * jchunk]
    srt = np.sort(counted)
    rank = np.searchsorted(srt, keys, side="right" if mutant == "rank_le" else "left")
    return np.where(keys != NO_KEY, rank, 0).astype(np.int64)


def sample_keep(seed, idx, keep, bg=False):
    """The sampler alone: which of the candidate indices `idx` a seed keeps when `keep` of them are kept (the `keep` smallest keys)."""
    keys = hash_key(int(seed) ^ (BG_SEED_XOR if bg else 0), idx)
    return key_rank(keys) < keep


# ----------------------------------------------------------------------------- anchor target layer
def anchor_target_layer(base, stride, H, W, im_h, im_w, gt, batch=256, fg_fraction=0.5, pos_ov=0.7, neg_ov=0.3, seed=0, clobber=False,
                        pos_weight=-1.0, inside_w=(1.0, 1.0, 1.0, 1.0), disable=None, mutant=None, info=None):
    """anchor_target_impl.  seed < 0 or a `disable` list (frcnn_anchor_target_layer_inject, indices into ALL anchors): no device
    sampling.  -> labels [1,1,A*H,W], targets, inside, outside [1,H,W,4A]; `info` (a dict) receives the intermediate values."""
    base = np.asarray(base, dtype=np.float64)
    gt = np.asarray(gt, dtype=f32)
    A, N, G = base.shape[0], H * W * base.shape[0], gt.shape[0]
    an = anchor_f32(base, H, W, stride)
    # k_at_overlaps
    imw, imh = f32(im_w), f32(im_h)
    if mutant == "inside_le":
        inside = (an[:, 0] >= 0) & (an[:, 1] >= 0) & (an[:, 2] <= imw) & (an[:, 3] <= imh)
    else:
        inside = (an[:, 0] >= 0) & (an[:, 1] >= 0) & (an[:, 2] < imw) & (an[:, 3] < imh)
    ov = iou(an, gt, f32 if mutant == "iou_f32" else np.float64)
    best, bi = first_max(ov, mutant)
    maxov = np.where(inside, best, -1.0)
    argmax = np.where(inside, bi, -1)
    gtmax = np.where(inside[:, None], ov, 0.0).max(axis=0) if N else np.zeros(G)        # atomicMax from 0 over the inside anchors
    # k_at_labels
    hit = ov == gtmax[None, :]                                                          # ALL ties, zero maxima included
    if mutant == "gtmax_no_zero":
        hit = hit & (gtmax[None, :] > 0)
    is_gt_argmax = hit.any(axis=1)
    neg = (maxov <= neg_ov) if mutant == "neg_le" else (maxov < neg_ov)
    pos = (maxov > pos_ov) if mutant == "pos_gt" else (maxov >= pos_ov)
    negatives_first = (not clobber) != (mutant == "clobber_order")
    label = np.full(N, -1, dtype=np.int64)
    if negatives_first:
        label[neg] = 0
    label[is_gt_argmax] = 1
    label[pos] = 1
    if not negatives_first:
        label[neg] = 0
    label[~inside] = -1
    idx = np.arange(N)
    fgkey = np.where(label == 1, hash_key(seed, idx), NO_KEY)
    bgkey = np.where(label == 0, hash_key(int(seed) ^ (0 if mutant == "bg_same_seed" else BG_SEED_XOR), idx), NO_KEY)
    nfg, nbg = int((label == 1).sum()), int((label == 0).sum())
    do_sample = int(seed) >= 0 and disable is None
    fgrank, bgrank = (key_rank(fgkey, mutant), key_rank(bgkey, mutant)) if do_sample else (np.zeros(N, np.int64), np.zeros(N, np.int64))
    # k_at_disable
    if disable is not None:
        for n in np.asarray(disable, dtype=np.int64).ravel():
            if 0 <= n < N:
                if fgkey[n] != NO_KEY:
                    fgkey[n], nfg = NO_KEY, nfg - 1
                elif bgkey[n] != NO_KEY:
                    bgkey[n], nbg = NO_KEY, nbg - 1
    # k_at_finish
    num_fg = int(fg_fraction * batch)
    fg_keep = min(nfg, num_fg) if (do_sample and mutant != "fg_unsampled") else nfg
    bg_keep = min(nbg, batch - (num_fg if mutant == "bg_from_num_fg" else fg_keep)) if do_sample else nbg
    out_label = np.full(N, -1.0, dtype=f32)
    is_fg, is_bg = fgkey != NO_KEY, (fgkey == NO_KEY) & (bgkey != NO_KEY)
    out_label[is_fg & (fgrank < fg_keep)] = 1.0
    out_label[is_bg & (bgrank < bg_keep)] = 0.0
    targets = np.zeros((N, 4), dtype=f32)
    iw = np.zeros((N, 4), dtype=f32)
    ow = np.zeros((N, 4), dtype=f32)
    ins = np.where(argmax >= 0)[0]
    if ins.size:
        targets[ins] = encode_box(an[ins], gt[argmax[ins], :4])
    iw[inside & (out_label == 1.0)] = np.asarray(inside_w, dtype=np.float64).astype(f32)
    cf, cb = (nfg, nbg) if mutant == "weights_presample" else (fg_keep, bg_keep)
    with np.errstate(divide="ignore", invalid="ignore"):
        if pos_weight >= 0.0:
            vp, vn = np.float64(pos_weight) / np.float64(cf), (1.0 - np.float64(pos_weight)) / np.float64(cb)
        else:
            vp = vn = np.float64(1.0) / np.float64(cf + cb)
        ow[inside & (out_label == 1.0)] = f32(vp)
        ow[inside & (out_label == 0.0)] = f32(vn)
    if info is not None:
        info.update(anchors=an, inside=inside, maxov=maxov, argmax=argmax, gtmax=gtmax, ov=ov, prelabel=label, nfg=nfg, nbg=nbg,
                    fg_keep=fg_keep, bg_keep=bg_keep, fgrank=fgrank, bgrank=bgrank, flat_label=out_label)
    labels = out_label.reshape(1, H, W, A).transpose(0, 3, 1, 2).reshape(1, 1, A * H, W)
    return (np.ascontiguousarray(labels), targets.reshape(1, H, W, 4 * A), iw.reshape(1, H, W, 4 * A), ow.reshape(1, H, W, 4 * A))


# ----------------------------------------------------------------------------- proposal target layer
def supported(N, G, use_gt=False):
    """proposal_target_impl returns FRCNN_E_UNSUPPORTED before any launch otherwise"""
    return N + (G if use_gt else 0) <= PT_MAXN and G <= 32767


def proposal_target_layer(rois, scores, gt, num_classes, batch=256, fg_fraction=0.25, fg_thresh=0.5, bg_hi=0.5, bg_lo=0.0,
                          means=(0.0, 0.0, 0.0, 0.0), stds=(0.1, 0.1, 0.2, 0.2), seed=0, num=None, use_gt=False,
                          inside_w=(1.0, 1.0, 1.0, 1.0), keep_inds=None, n_fg=None, mutant=None, info=None):
    """k_proposal_target (num = *num_rois_d of the _dn entry, else every row), or k_proposal_target_inject when keep_inds / n_fg are
    given.  -> rois [B,5], scores [B], labels [B,1], targets, inside, outside [B,4C], counts int32 [4] (None for the injected entry)."""
    rois, gt = np.asarray(rois, dtype=f32), np.asarray(gt, dtype=f32)
    scores = np.asarray(scores, dtype=f32).reshape(-1)
    Nmax, G, C, B = rois.shape[0], gt.shape[0], int(num_classes), int(batch)
    Nv = Nmax if (num is None or mutant == "num_ignored") else max(0, min(int(num), Nmax))
    if keep_inds is not None:
        Nv = Nmax
    # PtCand: the proposal rows, then the gt boxes as rows (0, x1, y1, x2, y2) with score 0
    box = rois[:Nv, 1:5]
    image, score = rois[:Nv, 0], scores[:Nv]
    if use_gt:
        box = np.concatenate([box, gt[:, :4]], axis=0)
        image = np.concatenate([image, np.zeros(G, dtype=f32)])
        score = np.concatenate([score, np.zeros(G, dtype=f32)])
    N = box.shape[0]
    ov = iou(box, gt, f32 if mutant == "iou_f32" else np.float64) if N else np.zeros((0, G))
    best, assign = first_max(ov, mutant) if N else (np.zeros(0), np.zeros(0, np.int64))
    if keep_inds is None:
        is_fg_c = (best > fg_thresh) if mutant == "fg_thresh_gt" else (best >= fg_thresh)
        lo_ok = (best > bg_lo) if mutant == "bg_lo_gt" else (best >= bg_lo)
        kind = np.where(is_fg_c, 1, np.where((best < bg_hi) & lo_ok, 0, -1))
        key = hash_key(seed, np.arange(N))
        fg_idx, bg_idx = np.where(kind == 1)[0], np.where(kind == 0)[0]
        fg_list = fg_idx[np.argsort(key[fg_idx], kind="stable")]
        bg_list = bg_idx[np.argsort(key[bg_idx], kind="stable")]
        nfg, nbg = fg_list.size, bg_list.size
        fg_per_image = int(np.rint(fg_fraction * B))                       # nearbyint: half to even, like np.round
        fg_repl = bg_repl = False
        if nfg > 0 and nbg > 0:
            n_fg_out = min(fg_per_image, nfg)
            n_bg_out = B - n_fg_out
            bg_repl = nbg < n_bg_out
        elif nfg > 0:
            n_fg_out, n_bg_out, fg_repl = B, 0, nfg < B
        elif nbg > 0:
            n_fg_out, n_bg_out, bg_repl = 0, B, nbg < B
        else:
            n_fg_out = n_bg_out = 0
        counts = np.array([n_fg_out, n_bg_out, nfg, nbg], dtype=np.int32)
        s = np.arange(B)
        src = np.full(B, -1, dtype=np.int64)

        def draw(xor, n):
            k = hash_key(int(seed) ^ xor, s)
            word = (k & u64(0xFFFFFFFF)) if mutant == "repl_low_bits" else (k >> u64(32))
            return (word % u64(n)).astype(np.int64)
        if n_fg_out:
            pick = draw(FG_REPL_XOR, nfg) if fg_repl else s
            src[:n_fg_out] = fg_list[pick[:n_fg_out]]
        if n_bg_out:
            pick = draw(BG_REPL_XOR, nbg) if bg_repl else s - n_fg_out
            src[n_fg_out:n_fg_out + n_bg_out] = bg_list[pick[n_fg_out:n_fg_out + n_bg_out]]
        row_fg = s < n_fg_out
        if info is not None:
            info.update(kind=kind, assign=assign, best=best, fg_list=fg_list, bg_list=bg_list, fg_repl=fg_repl, bg_repl=bg_repl, src=src)
    else:
        src = np.asarray(keep_inds, dtype=np.int64).ravel().copy()
        B = src.size
        src[(src < 0) | (src >= N)] = -1
        row_fg = np.arange(B) < int(n_fg)
        counts = None
    # pt_emit_row
    out_rois = np.zeros((B, 5), dtype=f32)
    out_scores = np.zeros(B, dtype=f32)
    out_labels = np.zeros((B, 1), dtype=f32)
    tg = np.zeros((B, 4 * C), dtype=f32)
    iw = np.zeros((B, 4 * C), dtype=f32)
    ow = np.zeros((B, 4 * C), dtype=f32)
    ok = np.where(src >= 0)[0]
    if ok.size:
        sr = src[ok]
        out_rois[ok, 0], out_rois[ok, 1:5], out_scores[ok] = image[sr], box[sr], score[sr]
        g = gt[assign[sr]]
        lab = np.where(row_fg[ok], g[:, 4], f32(0))
        out_labels[ok, 0] = lab
        t = encode_box(box[sr], g[:, :4])
        tn = ((t.astype(np.float64) - np.asarray(means, dtype=np.float64)) / np.asarray(stds, dtype=np.float64)).astype(f32)
        inw = np.asarray(inside_w, dtype=np.float64).astype(f32)
        for r in np.where(lab > 0)[0]:
            c4 = 4 * int(lab[r])
            tg[ok[r], c4:c4 + 4] = tn[r]
            iw[ok[r], c4:c4 + 4] = inw
            ow[ok[r], c4:c4 + 4] = (inw > 0).astype(f32)
    return out_rois, out_scores, out_labels, tg, iw, ow, counts
