"""Cases and exact references for the construction kernels past one launch's worth of motions (NumPy, host only).

The construction kernels cut their work along the motion axis: launch loops that step by 65535 motions (grid.y, or grid.x
of the paths kernel) or by 2^22 workgroups, and reductions with a strided second leg once a block (256 lanes) or the
workgroup cap (1024 partials) is passed.  Everything here is tiny per motion (1 to 3 frames, one joint): the cost is the
count.  tests/test_motion_count_shapes_host.py keeps the constants below in step with the sources and asserts that every
case lies on the side of its cut it was written for; tests/test_gpu_motion_count_shapes.py runs the cases.

References
  * DTW (grids, paths, pair costs): J = 1, x = z = 0, y a small non-negative integer.  The fit is then the identity,
    S[i][j] = |a_i - b_j| exactly and every accumulated cost is an exact integer, so grids, D, totals, paths and warping
    functions are stated in vectorised integer NumPy (dp_tables / walk_back), the minimum taken as Python's min takes it
    (diagonal, (i-1, j), (i, j-1); the first of equals stays).
  * Spatial alignment: K = 64 distinct seeded motions and two long ones go through spatial_alignment.
    align_motions_spatially_host; every other motion n is motion n % K and must have its twin's bits.
  * Preparation: spatial_alignment.prepare_aligned_frames_host, in bits, with the three maxima planted where only the strided
    legs see them.
"""
import collections
import functools

import numpy as np

from morphablegraphs_amd import spatial_alignment as sa

# ---- the cuts, restated (kept in step with the sources by test_motion_count_shapes_host.py) ------------------------------------
GRID_Y = 65535                   # mg_spatial_align.hip, mg_dtw.hip, mg_dtw_pairs.hip: motions of one launch
PAIRS_MAX_WORKGROUPS = 1 << 22   # mg_dtw_pairs.hip: chunk_r = min(65535, 2^22 / nb)
SA_BLOCK, SA_FRAMES, SA_MAX_PARTIALS = 256, 32, 1024
PAIRS_STRIP, PAIRS_SUB, PAIRS_PASS_ROWS, PAIRS_MAX_FRAMES, DTW_MAX_JOINTS = 64, 16, 64, 1024, 64
PAIRS_LDS_BYTES = 152 * 1024
SENTINEL = -77.0


def launches(n_motions, chunk=GRID_Y):
    """[(n0, nb)] of `for (n0 = 0; n0 < n_motions; n0 += chunk)`."""
    return [(n0, min(chunk, n_motions - n0)) for n0 in range(0, n_motions, chunk)]


def pair_launches(n_motions, n_refs):
    """[(n0, nb, r0, rb)] of mg_dtw_pair_costs' two loops."""
    out = []
    for n0, nb in launches(n_motions):
        chunk_r = min(GRID_Y, PAIRS_MAX_WORKGROUPS // nb)
        out += [(n0, nb, r0, rb) for r0, rb in launches(n_refs, chunk_r)]
    return out


def pairs_lds_doubles(J, rows, bnd):
    """pairs_lds_doubles of mg_dtw_pairs.hip, term by term."""
    stride = (3 * J) | 1
    return (PAIRS_STRIP + PAIRS_SUB) * stride + DTW_MAX_JOINTS + 2 * PAIRS_STRIP + 2 * PAIRS_SUB + 1 + 2 * PAIRS_STRIP + bnd + rows * PAIRS_STRIP


def pass_rows(J, longest_ref):
    rows = PAIRS_PASS_ROWS
    while pairs_lds_doubles(J, rows, longest_ref) * 8 > PAIRS_LDS_BYTES:
        rows //= 2
    return rows


def first_halved_joint_count(longest_ref=PAIRS_MAX_FRAMES):
    """The smallest J whose 64-row pass does not fit beside a reference motion of `longest_ref` frames."""
    return next(J for J in range(1, DTW_MAX_JOINTS + 1) if pass_rows(J, longest_ref) < PAIRS_PASS_ROWS)


def n_partials(n_rows):
    """mg_prepare_aligned_frames: workgroups of pa_max_partial_kernel."""
    return min(SA_MAX_PARTIALS, (n_rows + SA_BLOCK - 1) // SA_BLOCK)


# ---- the counts ----------------------------------------------------------------------------------------------------------------
ALIGN_COUNTS = (SA_BLOCK - 1, SA_BLOCK, SA_BLOCK + 1, GRID_Y, GRID_Y + 1, GRID_Y + 2 + 2)
DTW_COUNTS = (GRID_Y, GRID_Y + 1, GRID_Y + 2 + 2)
DTW_REF_FRAMES = (1, 2, 3)
# (what, indices of the motions without a heading, n_motions, the motion the refusal names)
ALIGN_REFUSALS = [("a lane's second motion, minimum over lanes", (261, 700), 701, 261),
                  ("last lane's first against lane 0's second", (255, 256), 257, 255),
                  ("lane 0's 257th motion, alone", (65536,), GRID_Y + 2 + 2, 65536)]
PREPARE_SHAPES = [(1, 65536, 7), (1, 65537, 7), (4, 65536, 7), (5, 52429, 7)]
PAIRS_A = dict(n=GRID_Y + 2 + 2, refs=[0, GRID_Y, GRID_Y + 1, GRID_Y + 2 + 2 - 1])
PAIRS_B = dict(n=GRID_Y, n_refs=66)
PAIRS_C = dict(n=2049, refs=None)
PASS_LENGTHS = [1024, 3, 70]


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


# ---- DTW: integer motions and their exact tables -----------------------------------------------------------------------------------
def integer_motions(n_motions, seed=5):
    """(lengths cycling 1, 2, 3; offsets; the y value of every frame, integers 0 .. 3 as float64)."""
    lengths = 1 + np.arange(n_motions, dtype=np.int64) % 3
    off = offsets_of(lengths)
    ys = np.floor(np.random.default_rng(seed).uniform(0.0, 4.0, int(off[-1])))
    return lengths, off, ys


def integer_reference_motion(fr, seed=11):
    return np.floor(np.random.default_rng(seed + fr).uniform(0.0, 4.0, fr))


def clouds_of(ys):
    """(frames, 1, 3) clouds with x = z = 0."""
    out = np.zeros((len(ys), 1, 3))
    out[:, 0, 1] = ys
    return out


def dp_tables(S):
    """Accumulated cost and back-step codes of the grids S (..., Fr, F): one addition per cell, the minimum in the order
    diagonal, (i-1, j), (i, j-1) with strict comparisons (dtw.dtw_paths_host, vectorised over the leading axes)."""
    fr, f = S.shape[-2:]
    D, code = np.zeros(S.shape), np.full(S.shape, 2, dtype=np.int32)
    D[..., 0, 0] = S[..., 0, 0]
    for j in range(1, f):
        D[..., 0, j] = D[..., 0, j - 1] + S[..., 0, j]
    for i in range(1, fr):
        D[..., i, 0] = D[..., i - 1, 0] + S[..., i, 0]
        code[..., i, 0] = 1
        for j in range(1, f):
            m, c = D[..., i - 1, j - 1].copy(), np.zeros(S.shape[:-2], dtype=np.int32)
            up, left = D[..., i - 1, j], D[..., i, j - 1]
            take = up < m
            m, c = np.where(take, up, m), np.where(take, 1, c)
            take = left < m
            m, c = np.where(take, left, m), np.where(take, 2, c)
            D[..., i, j] = m + S[..., i, j]
            code[..., i, j] = c
    return D, code


def walk_back(code):
    """(paths (m, Fr + F - 1, 2) front to back with -1 behind each path's end, lengths (m,), warping (m, Fr)) of the back-step
    codes (m, Fr, F): find_path and get_warping_function."""
    m, fr, f = code.shape
    steps = fr + f - 1
    rows = np.arange(m)
    xi, yi = np.full(m, fr - 1), np.full(m, f - 1)
    back = np.full((m, steps, 2), -1, dtype=np.int32)
    length, live = np.zeros(m, dtype=np.int32), np.ones(m, dtype=bool)
    for k in range(steps):
        back[live, k, 0], back[live, k, 1] = xi[live], yi[live]
        length += live
        live = live & ((xi > 0) | (yi > 0))
        c = code[rows, xi, yi]                      # row 0 holds 2 and column 0 holds 1, as the walk wants them
        xi, yi = np.where(live & (c != 2), xi - 1, xi), np.where(live & (c != 1), yi - 1, yi)
    assert not live.any()
    k = np.arange(steps)[None, :]
    src = np.where(k < length[:, None], length[:, None] - 1 - k, k)
    paths = back[rows[:, None], src]
    warp = np.zeros((m, fr), dtype=np.int32)
    for k in range(steps):                          # the path rises in both indices: the last column of a row is its largest
        ok = k < length
        np.maximum.at(warp, (rows[ok], paths[ok, k, 0]), paths[ok, k, 1])
    return paths, length, warp


@functools.lru_cache(maxsize=None)
def dtw_case(n_motions, fr):
    """Inputs and every expected output of mg_dtw_distance_grids + mg_dtw_paths for n_motions integer motions against an
    integer reference motion of `fr` frames, in the layouts of include/mg_hip.h; room the kernels do not write holds the
    sentinel (-77, or -77 as an int32)."""
    lengths, off, ys = integer_motions(n_motions)
    a = integer_reference_motion(fr)
    total = int(off[-1])
    n_pairs = total + n_motions * (fr - 1)
    grids, acc = np.full(fr * total, SENTINEL), np.full(fr * total, SENTINEL)
    totals = np.full(n_motions, SENTINEL)
    paths = np.full((n_pairs, 2), int(SENTINEL), dtype=np.int32)
    path_len, warp = np.full(n_motions, int(SENTINEL), dtype=np.int32), np.full((n_motions, fr), int(SENTINEL), dtype=np.int32)
    for f in (1, 2, 3):
        idx = np.flatnonzero(lengths == f)
        if not len(idx):
            continue
        B = ys[off[idx][:, None] + np.arange(f)[None, :]]
        S = np.abs(a[None, :, None] - B[:, None, :])
        D, code = dp_tables(S)
        p, ln, w = walk_back(code)
        cells = (fr * off[idx])[:, None] + np.arange(fr * f)[None, :]
        grids[cells], acc[cells] = S.reshape(len(idx), -1), D.reshape(len(idx), -1)
        totals[idx], path_len[idx], warp[idx] = D[:, -1, -1], ln, w
        slot = (off[idx] + idx * (fr - 1))[:, None] + np.arange(fr + f - 1)[None, :]
        keep = np.arange(fr + f - 1)[None, :] < ln[:, None]
        paths[slot[keep]] = p[keep]
    for arr in (grids, acc, totals, paths, path_len, warp, ys, off):
        arr.setflags(write=False)
    return dict(lengths=lengths, off=off, ys=ys, ref=a, grids=grids, acc=acc, totals=totals, paths=paths, path_len=path_len, warp=warp, n_pairs=n_pairs)


def pair_costs_reference(lengths, off, ys, refs):
    """costs (len(refs), n_motions): the DTW total of motion refs[r] (rows) and motion n (columns) of the integer table."""
    refs = np.asarray(refs, dtype=np.int64)
    out = np.full((len(refs), len(lengths)), np.nan)
    for fr in (1, 2, 3):
        ri = np.flatnonzero(lengths[refs] == fr)
        if not len(ri):
            continue
        A = ys[off[refs[ri]][:, None] + np.arange(fr)[None, :]]
        for f in (1, 2, 3):
            ni = np.flatnonzero(lengths == f)
            if not len(ni):
                continue
            B = ys[off[ni][:, None] + np.arange(f)[None, :]]
            D, _ = dp_tables(np.abs(A[:, None, :, None] - B[None, :, None, :]))
            out[ri[:, None], ni[None, :]] = D[..., -1, -1]
    assert not np.isnan(out).any()
    return out


def pairs_b_refs():
    """66 reference indices of the 65535 motions: not in order, one repeated, 65534 among them, every length among them."""
    n, k = PAIRS_B["n"], PAIRS_B["n_refs"]
    refs = np.random.default_rng(66).permutation(n)[:k].astype(np.int64)
    refs[3], refs[40], refs[65] = n - 1, refs[7], 0
    return refs


# ---- spatial alignment ----------------------------------------------------------------------------------------------------------------
ALIGN_K, ALIGN_D = 64, 7
ALIGN_LONG = {0: SA_FRAMES + 1, GRID_Y: 2 * SA_FRAMES + 1}      # motion: frames (the second only where the table has it)
ALIGN_REF = (0.6, 1.7)


@functools.lru_cache(maxsize=None)
def align_distinct():
    """The K distinct motions (1, 2 or 3 frames, one joint) and the two long ones, seeded; their host alignment and transforms."""
    from test_spatial_alignment_host import random_motion
    rng = np.random.default_rng(640)
    motions = collections.OrderedDict(("k%d" % k, random_motion(rng, 1 + k % 3, 1)) for k in range(ALIGN_K))
    for n, frames in ALIGN_LONG.items():
        motions["long%d" % n] = random_motion(rng, frames, 1)
    host, transforms = sa.align_motions_spatially_host(motions, 0, ALIGN_REF, return_transforms=True)
    return motions, host, dict(zip(motions.keys(), transforms))


def align_key(n):
    return "long%d" % n if n in ALIGN_LONG else "k%d" % (n % ALIGN_K)


def align_twin(n):
    """The first motion of a table that is the same motion as motion n."""
    return n if n in ALIGN_LONG else (n % ALIGN_K if n % ALIGN_K not in ALIGN_LONG else n % ALIGN_K + ALIGN_K)


@functools.lru_cache(maxsize=None)
def align_table(n_motions):
    """(lengths, offsets, the (offsets[-1], 7) table): motion n is distinct motion n % K, except the long ones."""
    motions, _, _ = align_distinct()
    lengths = 1 + (np.arange(n_motions, dtype=np.int64) % ALIGN_K) % 3
    longs = [n for n in ALIGN_LONG if n < n_motions]
    for n in longs:
        lengths[n] = ALIGN_LONG[n]
    off = offsets_of(lengths)
    table = np.empty((int(off[-1]), ALIGN_D))
    plain = np.ones(n_motions, dtype=bool)
    plain[longs] = False
    for k in range(ALIGN_K):
        idx = np.flatnonzero(plain & (np.arange(n_motions) % ALIGN_K == k))
        m = motions["k%d" % k]
        table[off[idx][:, None] + np.arange(len(m))[None, :]] = m[None]
    for n in longs:
        table[off[n]:off[n + 1]] = motions["long%d" % n]
    for arr in (lengths, off, table):
        arr.setflags(write=False)
    return lengths, off, table


def no_heading(table, off, motions):
    """A copy of the table in which frame 0 of each of `motions` turns z onto the y axis: every statement exact, l = 0."""
    out = np.array(table)
    out[off[list(motions)], 3:7] = [1.0, 1.0, 1.0, -1.0]
    return out


# ---- preparation ---------------------------------------------------------------------------------------------------------------------------
PLANTED = (2.5, 3.75, 9.25)          # channel 2's with a negative sign; everything else is below 1 in magnitude


def planted_rows(n_rows):
    """Row of each channel's maximum: channel 0 in row 65536 (partial 256: the final kernel's lane 0, second visit), channel 1
    in row 262144 (workgroup 0, lane 0, second grid stride), channel 2 in the last row; a table without such a row has the
    maximum in row n_rows - 257 instead."""
    early = n_rows - SA_BLOCK - 1
    return (SA_BLOCK * SA_BLOCK if n_rows > SA_BLOCK * SA_BLOCK else early,
            SA_MAX_PARTIALS * SA_BLOCK if n_rows > SA_MAX_PARTIALS * SA_BLOCK else early, n_rows - 1)


@functools.lru_cache(maxsize=None)
def prepare_table(shape):
    """A seeded (N, F, 7) table: root positions in (-1, 1), unit quaternions, the three maxima planted."""
    rng = np.random.default_rng(sum(shape))
    x = rng.uniform(-1.0, 1.0, shape)
    x[:, :, 3:] /= np.linalg.norm(x[:, :, 3:], axis=2, keepdims=True)
    flat = x.reshape(-1, shape[2])
    r0, r1, r2 = planted_rows(len(flat))
    flat[r0, 0], flat[r1, 1], flat[r2, 2] = PLANTED[0], PLANTED[1], -PLANTED[2]
    x.setflags(write=False)
    return x


def prepare_reference(x):
    """(out (N, F, D), scale (3,)) of spatial_alignment.prepare_aligned_frames_host."""
    out, scale = sa.prepare_aligned_frames_host(collections.OrderedDict((i, x[i]) for i in range(len(x))))
    return np.array(list(out.values())), np.asarray(scale, dtype=np.float64)


# ---- the reductions as the kernels cut them (to show on the host what a dropped leg would answer) ---------------------------------------
def partial_maxima(flat, stride_leg=True):
    """pa_max_partial_kernel: partial[b][c] over the rows workgroup b visits (without the grid-stride leg: its first 256 only)."""
    mag, nb = np.abs(flat[:, :3]), n_partials(len(flat))
    out = np.zeros((nb, 3))
    for r0 in range(0, len(flat) if stride_leg else min(len(flat), nb * SA_BLOCK), nb * SA_BLOCK):
        chunk = mag[r0:r0 + nb * SA_BLOCK]
        full = len(chunk) // SA_BLOCK
        if full:
            out[:full] = np.maximum(out[:full], chunk[:full * SA_BLOCK].reshape(full, SA_BLOCK, 3).max(axis=1))
        if len(chunk) % SA_BLOCK:
            out[full] = np.maximum(out[full], chunk[full * SA_BLOCK:].max(axis=0))
    return out


def final_maxima(partial, second_leg=True):
    """pa_max_final_kernel (without `b += SA_BLOCK`: a lane's first partial only)."""
    return (partial if second_leg else partial[:SA_BLOCK]).max(axis=0)


def first_refused(bad, n_motions, second_leg=True):
    """sa_heading_check_kernel: the least refused motion over the lanes (without `n += SA_BLOCK`: a lane's first motion only)."""
    seen = [n for n in bad if second_leg or n < SA_BLOCK]
    return min(seen) if seen else n_motions
