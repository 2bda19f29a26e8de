"""The reduction order of frcnn_gemm_h2_mean (csrc/gemm_h2.hip: ep_mean + k_h2_mean_finish), stated in numpy float32.

A 32-row accumulator block (lane = row) adds, per column, the rows of the group its first row belongs to (slot 0) and of the next group
(slot 1); rows outside the group or past M count as +0.  The 32 lanes meet in five exchange steps.  The kernel runs them on the VALU
(four DPP adds inside a 16-lane row, then v_permlane16_swap between the two rows); the statement here shows that this gives every lane
the bits of the xor butterfly over offsets 1, 2, 4, 8, 16, which are the bits of a pairwise tree in row order.  k_h2_mean_finish then
adds a group's blocks in ascending order from 0.0f and multiplies by 1.0f / rows.

mean_emulate() is the host emulation the GPU test (test_h2_mean_valu_gpu.py) holds the kernel to, bit for bit."""
import numpy as np

LANES = np.arange(32)
# the partner lane of each exchange step: what the DPP controls / the row swap read
QUAD_1032 = (LANES & ~3) | np.array([1, 0, 3, 2])[LANES & 3]       # quad_perm:[1,0,3,2]
QUAD_2301 = (LANES & ~3) | np.array([2, 3, 0, 1])[LANES & 3]       # quad_perm:[2,3,0,1]
HALF_MIRROR = (LANES & ~7) | (7 - (LANES & 7))                     # row_half_mirror
ROW_MIRROR = (LANES & ~15) | (15 - (LANES & 15))                   # row_mirror
VALU_STEPS = (QUAD_1032, QUAD_2301, HALF_MIRROR, ROW_MIRROR)


def tree_valu(v):
    """v float32 [32, ...] (lane = row) -> [32, ...]: every lane's value after the kernel's five steps."""
    v = np.asarray(v, np.float32)
    for src in VALU_STEPS:
        v = v[src] + v                              # v_add_f32_dpp: the permuted operand + the lane's own
    # v_permlane16_swap_b32 of the value with a copy of itself: the first result keeps row 0 and takes row 0 into row 1, the second
    # takes row 1 into row 0 and keeps row 1; then one add of the two
    r0 = np.concatenate([v[:16], v[:16]])
    r1 = np.concatenate([v[16:], v[16:]])
    return r0 + r1


def tree_xor(v):
    """the same block through the butterfly v += v[lane ^ o], o = 1, 2, 4, 8, 16."""
    v = np.asarray(v, np.float32)
    for o in (1, 2, 4, 8, 16):
        v = v + v[LANES ^ o]
    return v


def tree_pairwise(v):
    """the pairwise tree in row order: [32, ...] -> [...]."""
    v = np.asarray(v, np.float32)
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def block_straddles(mb, rows):
    """whether the 32-row block starting at row mb can meet a second group (the kernel skips slot 1 when it cannot)."""
    return (mb % rows) + 31 >= rows


def block_partials(y, M, rows, shortcut=True):
    """y float32 [M, N] of ONE batch entry -> part float32 [ceil(M / 32)][2][N].  With `shortcut`, slot 1 of a block that cannot
    straddle is left NaN (the kernel does not write it); without, it is the sum of +0s like before."""
    y = np.asarray(y, np.float32)
    N = y.shape[1]
    nblk = (M + 31) // 32
    part = np.full((nblk, 2, N), np.nan, np.float32)
    for b in range(nblk):
        mb = 32 * b
        m = mb + LANES
        g0, gid = mb // rows, m // rows
        v = np.zeros((32, N), np.float32)
        live = m < M
        v[live] = y[m[live]]
        zero = np.zeros_like(v)
        part[b, 0] = tree_valu(np.where(((m < M) & (gid == g0))[:, None], v, zero))[0]
        if block_straddles(mb, rows) or not shortcut:
            part[b, 1] = tree_valu(np.where(((m < M) & (gid == g0 + 1))[:, None], v, zero))[0]
    return part


def finish(part, M, rows):
    """k_h2_mean_finish for one batch entry: part [nblk][2][N] -> [M / rows][N]."""
    N = part.shape[2]
    out = np.empty((M // rows, N), np.float32)
    inv = np.float32(1.0) / np.float32(rows)
    for r in range(M // rows):
        row0, row1 = r * rows, r * rows + rows - 1
        s = np.zeros(N, np.float32)
        for b in range(row0 >> 5, (row1 >> 5) + 1):
            which = 0 if (b << 5) // rows == r else 1
            s = s + part[b, which]
        out[r] = s * inv
    return out


def mean_emulate(y, G, M, rows):
    """y float32 [G * M, N] (the float32 result of frcnn_gemm_h2, G batch entries of M rows) -> [G * M / rows, N]: the bits
    frcnn_gemm_h2_mean gives."""
    y = np.asarray(y, np.float32).reshape(G, M, -1)
    return np.concatenate([finish(block_partials(y[g], M, rows), M, rows) for g in range(G)], axis=0)


def _vectors(rng, n):
    """[32, n] float32: 20 octaves of spread, both signs, a fifth of the entries exactly zero"""
    v = rng.standard_normal((32, n)) * np.exp2(rng.uniform(-10, 10, size=(32, n)))
    v[rng.random((32, n)) < 0.2] = 0.0
    return v.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_valu_steps_are_the_xor_butterfly_and_the_pairwise_tree_bit_for_bit():
    rng = np.random.default_rng(5)
    v = _vectors(rng, 2000)
    got, xor, pair = tree_valu(v), tree_xor(v), tree_pairwise(v)
    assert np.array_equal(_bits(got), _bits(xor))                               # every lane, not only the one that stores
    assert np.array_equal(_bits(got), np.broadcast_to(_bits(pair), (32, 2000)))


def test_masked_rows_count_as_plus_zero():
    """the group select: rows outside the group (or past M) enter the tree as +0, whatever they hold -- NaN and inf included"""
    rng = np.random.default_rng(6)
    v = _vectors(rng, 500)
    for first in (0, 1, 17, 31):                     # the group is rows [first, 32) or [0, first) of the block
        for keep in (LANES >= first, LANES < first):
            dirty = v.copy()
            dirty[~keep] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 1e30], np.float32), size=(int((~keep).sum()), 500))
            masked = np.where(keep[:, None], dirty, np.float32(0))
            want = tree_pairwise(np.where(keep[:, None], v, np.float32(0)))
            assert np.array_equal(_bits(tree_valu(masked)[0]), _bits(want))
            assert np.array_equal(_bits(tree_valu(masked)), _bits(tree_xor(masked)))


def test_no_straddle_shortcut_changes_nothing_the_finish_reads():
    rng = np.random.default_rng(7)
    for M, rows in ((92 * 49, 49), (30 * 49, 49), (37 * 49, 49), (40 * 32, 32), (24 * 64, 64), (5 * 33, 33), (3 * 100, 100), (96, 96)):
        y = (rng.standard_normal((M, 8)) * np.exp2(rng.uniform(-6, 6, size=(M, 8)))).astype(np.float32)
        cut, full = block_partials(y, M, rows, shortcut=True), block_partials(y, M, rows, shortcut=False)
        assert not np.isnan(full).any()
        skipped = np.isnan(cut[:, 1, 0])
        assert np.array_equal(skipped, np.array([not block_straddles(32 * b, rows) for b in range(cut.shape[0])]))
        if rows % 32 == 0:
            assert skipped.all()
        assert np.array_equal(_bits(cut[~np.isnan(cut)]), _bits(full[~np.isnan(cut)]))
        got = finish(cut, M, rows)                   # a NaN read from a skipped slot would surface here
        assert not np.isnan(got).any()
        assert np.array_equal(_bits(got), _bits(finish(full, M, rows)))


def test_mean_emulate_is_the_mean():
    rng = np.random.default_rng(8)
    G, R, rows, N = 2, 7, 49, 16
    y = rng.standard_normal((G * R * rows, N)).astype(np.float32)
    got = mean_emulate(y, G, R * rows, rows)
    want = y.astype(np.float64).reshape(G * R, rows, N).mean(axis=1)
    assert got.shape == (G * R, N) and got.dtype == np.float32
    assert float(np.abs(got - want).max()) <= 49 * 2.0 ** -24 * float(np.abs(y).max())      # 49 float32 additions at the data's scale
    # one batch entry per image: an entry's bits do not depend on its slot
    assert np.array_equal(_bits(mean_emulate(y[R * rows:], 1, R * rows, rows)), _bits(got[R:]))
