"""TEST INFRASTRUCTURE ONLY -- the score vectors that reach the ordering machinery of csrc/detect_kernels.hip and
csrc/detect_post.hip (make_key, k_select_topk, k_rank / k_scatter_sorted, the rank sort of k_perclass_nms, k_final_select) where oracle/synth.py's inputs do not:
synth makes every score unique (tie_free) and spreads them over (0, 1), so the K-th key is always decided by the score half alone,
its 16-bit bucket always fits the LDS list, and no two rows ever tie at a cut.  Shared by tests/test_select_cpu.py (the numpy
restatement oracle/select_ref.py and its planted mistakes) and tests/test_select_gpu.py (the kernels); stated once, here.

Everything derives from np.random.RandomState(seed).  A case is (distribution, N) with the list of K to run; the proposal-layer
inputs built from it carry ALL-ZERO deltas -- expf(0) = 1 and the decode is then the same float32 statements as numpy's, so rois
compare bitwise and no 1-ulp decode can flip an IoU at the NMS threshold -- except the one `overflow` case.

Map sizes, the smallest that still reach each path of k_select_topk (1024 threads, 8 keys a thread and trip, SEL_LIST = 4096):
   N = 54    2 x  3 x 9   less than one wave
   N = 4104  19 x 24 x 9  just above SEL_LIST when all keys share the cut's 16-bit bucket
   N = 9207  33 x 31 x 9  more than 8 * 1024: two trips of the unrolled scan; 9207 % 64 = 55: a ragged last wave
"""
import collections

import numpy as np

f32 = np.float32
A = 9
FEAT_STRIDE = 16
SEL_LIST = 4096
MAPS = collections.OrderedDict([(54, (2, 3)), (4104, (19, 24)), (9207, (33, 31))])      # N -> (H, W)

Case = collections.namedtuple("Case", "name dist N H W scores ks")


# ----------------------------------------------------------------------------------------------------- distributions
def constant(N, seed=0):
    """every score 0.5f: one tie block of N -- only the index half of the key tells rows apart"""
    return np.full(N, 0.5, dtype=f32)


def untrained(N, seed=0):
    """0.5 + U(0, 2^-9) in float32, NOT tie_free: an untrained RPN.  Sign, exponent and the top 7 mantissa bits are shared, so all
    N keys sit in one 16-bit bucket; duplicates are present (forced on the small map, where chance alone leaves none)."""
    rng = np.random.RandomState(100 + seed)
    s = (f32(0.5) + (rng.rand(N).astype(f32) * f32(2.0 ** -9))).astype(f32)
    src = rng.randint(0, N, size=N // 16 + 2)
    dst = rng.randint(0, N, size=N // 16 + 2)
    s[dst] = s[src]
    assert np.unique(s).size < N and s.min() >= 0.5 and s.max() < 0.5 + 2.0 ** -8
    return s


def _bucket(N, n_in, seed):
    """exactly n_in scores in [0.5, 0.5 + 2^-8) (one 16-bit bucket of the sort key: 0x3f00....), the rest split between [0.75, 1)
    and (0, 0.25), scattered by index"""
    assert N >= n_in
    rng = np.random.RandomState(200 + seed)
    s = np.empty(N, dtype=f32)
    where = rng.permutation(N)
    inside, rest = where[:n_in], where[n_in:]
    bits = np.uint32(0x3f000000) + rng.randint(0, 1 << 16, size=n_in).astype(np.uint32)
    s[inside] = bits.view(f32)
    hi = rng.rand(rest.size) < 0.5
    s[rest[hi]] = (0.75 + 0.25 * rng.rand(int(hi.sum()))).astype(f32).clip(0.75, np.nextafter(f32(1), f32(0)))
    s[rest[~hi]] = (0.25 * rng.rand(int((~hi).sum()))).astype(f32).clip(np.finfo(f32).tiny, np.nextafter(f32(0.25), f32(0)))
    assert int(((s >= 0.5) & (s < 0.5 + 2.0 ** -8)).sum()) == n_in
    return s


def bucket_4096(N, seed=0):
    return _bucket(N, SEL_LIST, seed)


def bucket_4097(N, seed=0):
    return _bucket(N, SEL_LIST + 1, seed)


def saturated(N, seed=0):
    """30 % exactly 1.0f, 30 % exactly +0.0f, the rest uniform; the two groups are interleaved by index, not contiguous"""
    rng = np.random.RandomState(300 + seed)
    s = rng.rand(N).astype(f32)
    u = rng.rand(N)
    s[u < 0.3] = f32(1.0)
    s[(u >= 0.3) & (u < 0.6)] = f32(0.0)
    return s


def quantised(N, seed=0):
    """round(p * 8) / 8: nine levels, heavy ties at every level"""
    rng = np.random.RandomState(400 + seed)
    return (np.round(rng.rand(N).astype(f32) * f32(8)) / f32(8)).astype(f32)


def trained(N, seed=0):
    """sigmoid(N(-6, 3^2)) in float32: scores over about twenty binades; plus 16 exact duplicates of interior values and 4 denormals"""
    rng = np.random.RandomState(500 + seed)
    z = (-6.0 + 3.0 * rng.randn(N)).astype(f32)
    s = (f32(1) / (f32(1) + np.exp(-z, dtype=f32))).astype(f32)
    pick = rng.choice(N, size=36, replace=False)
    s[pick[16:32]] = s[pick[:16]]
    s[pick[32:36]] = np.array([1, 2, 0x7fffff, 2], dtype=np.uint32).view(f32)        # denormals, two of them equal
    return s


DISTS = collections.OrderedDict([("constant", constant), ("untrained", untrained), ("bucket_4096", bucket_4096),
                                 ("bucket_4097", bucket_4097), ("saturated", saturated), ("quantised", quantised), ("trained", trained)])


# ----------------------------------------------------------------------------------------------------- K lists
def tie_blocks(scores):
    """[(start, end)] in descending-score order of every run of equal scores longer than 1 (ranks start .. end - 1 tie)"""
    v = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    v = v[~np.isnan(v)]                                                  # NaN rows are not a block here: no K is derived from them
    edge = np.flatnonzero(v[1:] != v[:-1]) + 1
    starts = np.concatenate([[0], edge])
    ends = np.concatenate([edge, [v.size]])
    return [(int(a), int(b)) for a, b in zip(starts, ends) if b - a > 1]


def k_list(scores, extra=(), max_blocks=None):
    """1, 63, 64, 65; every tie-block boundary and boundary +- 1 (`max_blocks`: only the longest so many blocks, for vectors with
    thousands of two-row blocks); N - 1, N, N + 1; the defaults 6000 / 12000 where N allows; `extra`."""
    N = int(np.size(scores))
    ks = {1, 63, 64, 65, N - 1, N, N + 1, 6000, 12000} | set(int(e) for e in extra)
    blocks = tie_blocks(scores)
    if max_blocks is not None:
        blocks = sorted(blocks, key=lambda ab: ab[0] - ab[1])[:max_blocks]
    for a, b in blocks:
        ks |= {a - 1, a, a + 1, b - 1, b, b + 1}
    return sorted(k for k in ks if 1 <= k <= N + 1)


def _case(dist, N, seed=0):
    H, W = MAPS[N]
    s = DISTS[dist](N, seed)
    assert s.dtype == f32 and s.shape == (N,)
    extra, max_blocks = (), 3
    if dist.startswith("bucket"):
        n_in = int(dist.split("_")[1])
        above = int((s >= 0.75).sum())                                   # K in (above, above + n_in]: the cut falls inside the bucket
        extra = (above + 1, above + 2, above + n_in // 2, above + n_in - 1, above + n_in)
    if dist == "quantised":
        max_blocks = None                                                # nine blocks: every boundary
    return Case("%s_%d" % (dist, N), dist, N, H, W, s, k_list(s, extra, max_blocks))


def cases():
    """every distribution x every N it fits (the buckets need N > SEL_LIST)"""
    out = []
    for dist in DISTS:
        for N in MAPS:
            if dist.startswith("bucket") and N <= SEL_LIST + 1:
                continue
            out.append(_case(dist, N))
    return out


def case(name):
    dist, N = name.rsplit("_", 1)
    return _case(dist, int(N))


# ----------------------------------------------------------------------------------------------------- proposal-layer inputs
def prob_blob(scores, H, W):
    """rpn_cls_prob [1,H,W,2A]: fg = the scores in anchor order (y, x, a), bg = 1 - p"""
    p = np.asarray(scores, dtype=f32).reshape(1, H, W, A)
    return np.ascontiguousarray(np.concatenate([(f32(1) - p).astype(f32), p], axis=-1))


def zero_deltas(H, W):
    return np.zeros((1, H, W, 4 * A), dtype=f32)


def im_info(H, W):
    return np.array([H * FEAT_STRIDE, W * FEAT_STRIDE, 1.0], dtype=f32)


def overflow(seed=0):
    """The one case with non-zero deltas: tie-free scores on the 19 x 24 map; a few anchors get dw, dh in {+89, +100, -100, -104}
    (exp overflows to inf above 88.7 and underflows to 0 below -103.9: inf and zero widths before the clip) and a few others
    dx = +-1e30.  No anchor gets both, so no box is NaN (inf - inf): NaN boxes are out of scope.  Coordinates are
    compared with box_tol, not bitwise: the deltas are no longer zero.  -> (Case, deltas [1,H,W,4A])"""
    import synth
    N = 4104
    H, W = MAPS[N]
    prob, deltas = synth.rpn_outputs(H, W, A, seed=600 + seed)
    s = np.ascontiguousarray(prob[..., A:]).reshape(-1)
    rng = np.random.RandomState(600 + seed)
    d = deltas.reshape(-1, 4).copy()
    pick = rng.choice(N, size=48, replace=False)
    big = np.array([89.0, 100.0, -100.0, -104.0], dtype=f32)
    for i, n in enumerate(pick[:16]):                                   # every (dw, dh) pair of the four values
        d[n, 2], d[n, 3] = big[i & 3], big[i >> 2]
    for i, n in enumerate(pick[16:32]):                                 # one of the two alone
        d[n, 2 + (i & 1)] = big[(i >> 1) & 3]
    for i, n in enumerate(pick[32:]):
        d[n, 0] = f32(1e30) if i & 1 else f32(-1e30)
    return Case("overflow_%d" % N, "overflow", N, H, W, s, [1, 64, 65, 300, 2000, N - 1, N]), d.reshape(1, H, W, 4 * A)


def box_tol(want):
    """2 ulp of the coordinate, per element: a decoded coordinate is pcx -+ 0.5 * pw (bbox_transform.py:58-65) evaluated at the
    magnitude of its TERMS, so coordinates below 512 px are held to 2 ulp at 512 px (1.22e-4 px); device expf vs np.exp is what
    differs.  (The bound tests/test_detect_gpu.py has always asserted; it lives here so that both test files share it.)"""
    mag = np.maximum(np.abs(np.asarray(want, dtype=np.float32)), np.float32(512.0))
    return 2.0 * np.spacing(mag).astype(np.float64)


# ----------------------------------------------------------------------------------------------------- NMS entry points
def zoo_scores(k, seed=0):
    """k scores for the NMS entry points: negatives, both zeros, +-inf, denormals, NaN of both signs and two payloads, heavy ties"""
    rng = np.random.RandomState(700 + seed + k)
    s = (np.round(rng.randn(k).astype(f32) * f32(4)) / f32(4)).astype(f32)            # quarter steps around 0: ties, negatives
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x7fc00000, 0xffc00000,
                        0x7fc00123, 0xffc00123, 0x7fe00001], dtype=np.uint32).view(f32)
    reps = 4 if k >= 64 else 1
    where = rng.choice(k, size=special.size * reps, replace=False)
    s[where] = np.tile(special, reps)
    return s


def zoo_dets(k, seed=0):
    """dets f32 [k,5]: clustered boxes (NMS suppresses a lot) with zoo_scores"""
    import synth
    d = synth.random_dets(k, seed=710 + seed, cluster=max(2, k // 40), unique=False)
    d[:, 4] = zoo_scores(k, seed)
    return d


# ----------------------------------------------------------------------------------------------------- detect_post
def detect_post_case(t, R=300, C=21, max_per_image=100, score_thresh=0.05, seed=0, cut=(0.5,), low=0.3, fill=0.01):
    """Inputs of the test-time post-processing whose max_per_image cut is tied: every roi is its own 30 x 20 px cell of a grid (no two
    overlap, so NMS keeps every row and Soft-NMS / box voting leave them as they are), bbox_pred is zero, and cls_prob holds
      (i)   max_per_image - 1 entries above the cut and exactly t entries AT the cut score 0.5, spread over classes and rows,
      (ii)  equal scores inside a class (the entries above the cut take one of three values),
      (iii) entries exactly at score_thresh (dropped: the comparison is a strict `>`), NaN entries (dropped) and entries below the cut.
    The reference keeps every row >= the cut (test.py:178): count = max_per_image - 1 + t.
    `cut`: the values the t tied entries take in turn -- (+0.0, -0.0) with a negative score_thresh, `low` and `fill` puts both zeros
    at the cut, where they are equal.
    -> cls_prob [R,C], bbox_pred [R,4C], rois [R,5], (im_h, im_w), score_thresh"""
    rng = np.random.RandomState(800 + seed + t)
    im_h, im_w = 600, 1000
    cols = 25
    r = np.arange(R)
    x1, y1 = (r % cols) * 40.0 + 2.0, (r // cols) * 30.0 + 2.0
    rois = np.stack([np.zeros(R), x1, y1, x1 + 29.0, y1 + 19.0], axis=1).astype(f32)
    prob = np.full((R, C), fill, dtype=f32)
    cells = rng.permutation(R * (C - 1))
    rows, cls = cells // (C - 1), cells % (C - 1) + 1
    n_hi = max_per_image - 1

    def take(a, b):
        return rows[a:b], cls[a:b]
    prob[take(0, n_hi)] = np.array([0.9, 0.8, 0.7], dtype=f32)[rng.randint(0, 3, size=n_hi)]
    prob[take(n_hi, n_hi + t)] = np.asarray(cut, dtype=f32)[np.arange(t) % len(cut)]
    o = n_hi + t
    prob[take(o, o + 40)] = f32(low)                                   # below the cut
    prob[take(o + 40, o + 80)] = f32(score_thresh)                     # exactly at the threshold: `>` drops them
    prob[take(o + 80, o + 100)] = np.array([0x7fc00000, 0xffc00000], dtype=np.uint32).view(f32)[rng.randint(0, 2, size=20)]
    return prob, np.zeros((R, 4 * C), dtype=f32), rois, (im_h, im_w), f32(score_thresh)
