"""Temporal alignment of motions on the device: the reference's construction/dtw.py (run_dtw, get_warping_function,
warp_motion, the find_optimal_dtw_async leg of find_optimal_dtw) and MotionModelConstructor's get_average_time_line,
_align_frames_temporally and _align_frames_temporally_split (motion_model_constructor.py:265-349), shaped like the
reference's module so that a construction script swaps an import.  The two results of align_frames_temporally are,
unchanged, the first two arguments of fpca.construct_motion_primitive_model.

The DTW is the exact one the reference's module carries (get_distgrid, find_path): D[i, j] = min(D[i-1, j-1], D[i-1, j],
D[i, j-1]) + S[i, j], back-steps to the first minimum of (diagonal, (i-1, j), (i, j-1)).  All N motions are warped against
one reference motion in ONE batched call (mg_dtw_distance_grids, mg_dtw_paths, mg_warp_motions).  For given grids S, the
accumulated cost D, the paths and the warping functions are the reference's bit for bit.  The cell distance is the mean
point distance after the weighted 2-D rigid fit (csrc/mg_dtw.hip states the formula and the order of its sums); the
reference's own, anim_utils' _transform_invariant_point_cloud_distance, is not available: PARITY UNPINNED for the grids.

The all-pairs search of the reference's find_optimal_dtw (dtw.py:125-146, and find_optimal_dtw_async without a mean_key)
averages, per candidate reference motion, the path costs of all motions against it and means to keep the least average; its
selection never updates best_d, so it returns the LAST key's paths whatever the costs.  The rule it means is here as
all_pairs_costs (mg_dtw_pair_costs: the (R, N) matrix of total costs, no grid or path in memory), reference_from_costs (the
means added in column order, the FIRST least mean) and select_reference_motion;
align_frames_temporally(reference_selection="least_mean_cost") uses it.  The matrix is, bit for bit, the `total` of dtw_batch
pair by pair.

Not reproduced:
  * the reference's behaviour of find_optimal_dtw without a key (the last key wins): find_optimal_dtw here takes the
    reference motion's key and raises KeyError without one; select_reference_motion finds the key the search means;
  * fastdtw's approximation (radius 1), which run_dtw_process calls in place of run_dtw: the paths here are the optimum it
    approximates.

distance_grid_host and dtw_paths_host restate the two device calls in NumPy / plain Python; they are the yardstick of the
CPU tests.  The device functions have no CPU fallback.
"""
import collections

import numpy as np

from . import _capi

MAX_FRAMES, MAX_JOINTS = _capi.MG_DTW_MAX_FRAMES, _capi.MG_DTW_MAX_JOINTS


# ---- host restatements ---------------------------------------------------------------------------------------------------
def distance_grid_host(a, b, weights=None):
    """S (Fr, F) of clouds a (Fr, J, 3) and b (F, J, 3) as mg_dtw_distance_grids computes it: every sum over the joints in
    index order, one product and one addition at a time."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n_joints = a.shape[1]
    w = np.ones(n_joints) if weights is None else np.asarray(weights, dtype=np.float64)
    ax, ay, az = (a[:, None, :, c] for c in range(3))
    bx, by, bz = (b[None, :, :, c] for c in range(3))
    sw = 0.0
    sax, saz, sbx, sbz = np.zeros(ax.shape[:2]), np.zeros(ax.shape[:2]), np.zeros(bx.shape[:2]), np.zeros(bx.shape[:2])
    num, den = np.zeros((len(a), len(b))), np.zeros((len(a), len(b)))
    for k in range(n_joints):
        sw = sw + w[k]
        sax, saz = sax + w[k] * ax[..., k], saz + w[k] * az[..., k]
        sbx, sbz = sbx + w[k] * bx[..., k], sbz + w[k] * bz[..., k]
        num = num + w[k] * (ax[..., k] * bz[..., k] - bx[..., k] * az[..., k])
        den = den + w[k] * (ax[..., k] * bx[..., k] + az[..., k] * bz[..., k])
    num = num - (sax * sbz - sbx * saz) / sw
    den = den - (sax * sbx + saz * sbz) / sw
    theta = np.arctan2(num, den)
    cs, sn = np.cos(theta), np.sin(theta)
    ox = ((sax - sbx * cs) - sbz * sn) / sw
    oz = ((saz + sbx * sn) - sbz * cs) / sw
    total = np.zeros((len(a), len(b)))
    for k in range(n_joints):
        dx = ax[..., k] - ((bx[..., k] * cs + bz[..., k] * sn) + ox)
        dy = ay[..., k] - by[..., k]
        dz = az[..., k] - (((-bx[..., k]) * sn + bz[..., k] * cs) + oz)
        total = total + np.sqrt((dx * dx + dy * dy) + dz * dz)
    return total / float(n_joints)


def dtw_paths_host(S):
    """What mg_dtw_paths returns for one grid: (D, path, warping_function), D an (Fr, F) array, path a list of (i, j), the
    warping function a list of Fr column indices.  Plain Python floats, one addition per cell."""
    S = np.asarray(S, dtype=np.float64)
    nx, ny = S.shape
    s = S.tolist()
    D = [[0.0] * ny for _ in range(nx)]
    step = [[2] * ny for _ in range(nx)]
    D[0][0] = s[0][0]
    for j in range(1, ny):
        D[0][j] = D[0][j - 1] + s[0][j]
    for i in range(1, nx):
        Di, Dp, si, ci = D[i], D[i - 1], s[i], step[i]
        Di[0] = Dp[0] + si[0]
        ci[0] = 1
        for j in range(1, ny):
            m, code = Dp[j - 1], 0
            if Dp[j] < m:
                m, code = Dp[j], 1
            if Di[j - 1] < m:
                m, code = Di[j - 1], 2
            Di[j] = m + si[j]
            ci[j] = code
    xi, yi = nx - 1, ny - 1
    path = [(xi, yi)]
    while xi > 0 or yi > 0:
        code = step[xi][yi]
        if code != 2:
            xi -= 1
        if code != 1:
            yi -= 1
        path.append((xi, yi))
    path.reverse()
    return np.array(D), path, get_warping_function(path)


def get_warping_function(coordinates):
    """dtw.py get_warping_function: per row of the grid the LAST column the path has in it."""
    n_rows = int(coordinates[-1][0]) + 1
    warping_function = [0] * n_rows
    for i, j in coordinates:      # the path rises in both indices: the last entry of a row is its largest column
        warping_function[int(i)] = int(j)
    return warping_function


def warp_motion(frames, warp_function):
    """dtw.py warp_motion: the frames at the warping function's indices."""
    return [frames[idx] for idx in warp_function]


def get_average_time_line(motions):
    """MotionModelConstructor.get_average_time_line: the key of the motion whose length is closest to the mean length
    (the first one on ties)."""
    mean = np.mean([len(m) for m in motions.values()])
    best_key, least_distance = None, np.inf
    for k, m in motions.items():
        d = abs(len(m) - mean)
        if d < least_distance:
            best_key, least_distance = k, d
    return best_key


# ---- the device ------------------------------------------------------------------------------------------------------------
def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def _check_limits(n_ref_frames, lengths, n_joints=1):
    longest = max([int(n_ref_frames)] + [int(f) for f in lengths])
    if longest > MAX_FRAMES or n_joints > MAX_JOINTS:
        raise ValueError("DTW: %d frames (at most %d), %d joints (at most %d)" % (longest, MAX_FRAMES, n_joints, MAX_JOINTS))
    if n_ref_frames < 1 or any(f < 1 for f in lengths):
        raise ValueError("DTW: a motion without frames")


def _paths_on_device(ctx, bufs, grids_dev, n_ref_frames, offsets, accumulated):
    """mg_dtw_paths and the download of its results; returns (per-motion dicts, the warping functions' device buffer)."""
    n, fr, total = len(offsets) - 1, int(n_ref_frames), int(offsets[-1])
    n_pairs = total + n * (fr - 1)
    d_dev = bufs.malloc(8 * fr * total) if accumulated else None
    t_dev, p_dev, l_dev, w_dev = bufs.malloc(8 * n), bufs.malloc(8 * n_pairs), bufs.malloc(4 * n), bufs.malloc(4 * n * fr)
    _capi.dtw_paths(ctx, grids_dev, fr, offsets, d_dev, t_dev, p_dev, l_dev, w_dev)
    totals = ctx.download(t_dev, (n,), np.float64)
    pairs = ctx.download(p_dev, (n_pairs, 2), np.int32)
    lengths = ctx.download(l_dev, (n,), np.int32)
    warps = ctx.download(w_dev, (n, fr), np.int32)
    D = ctx.download(d_dev, (fr * total,), np.float64) if accumulated else None
    out = []
    for m in range(n):
        b0, f = int(offsets[m]), int(offsets[m + 1] - offsets[m])
        p0 = b0 + m * (fr - 1)
        out.append({"total": float(totals[m]), "path": pairs[p0:p0 + int(lengths[m])].copy(), "warping_function": warps[m].copy(),
                    "D": D[fr * b0:fr * (b0 + f)].reshape(fr, f).copy() if accumulated else None})
    return out, w_dev


def distance_grids(ref_cloud, clouds, weights=None, ctx=None):
    """mg_dtw_distance_grids: the grids S[n] (Fr, F_n) of the clouds `clouds` (a list of (F_n, J, 3) arrays) against
    ref_cloud (Fr, J, 3)."""
    ctx = _capi.default_context(ctx)
    ref = np.ascontiguousarray(ref_cloud, dtype=np.float64)
    clouds = [np.asarray(c, dtype=np.float64).reshape(-1, ref.shape[1], 3) for c in clouds]
    if not clouds:
        return []
    _check_limits(len(ref), [len(c) for c in clouds], ref.shape[1])
    off = _offsets([len(c) for c in clouds])
    with ctx.buffers() as bufs:
        a_dev, b_dev, s_dev = bufs.upload(ref), bufs.upload(np.concatenate(clouds)), bufs.malloc(8 * len(ref) * int(off[-1]))
        _capi.dtw_distance_grids(ctx, a_dev, len(ref), b_dev, off, ref.shape[1], weights, s_dev)
        S = ctx.download(s_dev, (len(ref) * int(off[-1]),), np.float64)
    return [S[len(ref) * int(off[m]):len(ref) * int(off[m + 1])].reshape(len(ref), -1).copy() for m in range(len(clouds))]


def paths_from_grids(grids, accumulated=True, ctx=None):
    """mg_dtw_paths on given grids (a list of (Fr, F_n) arrays with one Fr): per grid {"D" (None without accumulated),
    "total", "path" (L, 2) int32, "warping_function" (Fr,) int32}."""
    ctx = _capi.default_context(ctx)
    grids = [np.ascontiguousarray(g, dtype=np.float64) for g in grids]
    if not grids:
        return []
    fr = grids[0].shape[0]
    if any(g.ndim != 2 or g.shape[0] != fr for g in grids):
        raise ValueError("the grids of one call have the reference motion's frames as their rows")
    _check_limits(fr, [g.shape[1] for g in grids])
    off = _offsets([g.shape[1] for g in grids])
    with ctx.buffers() as bufs:
        s_dev = bufs.upload(np.concatenate([g.reshape(-1) for g in grids]))
        return _paths_on_device(ctx, bufs, s_dev, fr, off, accumulated)[0]


def dtw_batch(ref_cloud, clouds, weights=None, accumulated=False, ctx=None):
    """Grids and paths of N clouds against ref_cloud without leaving the device in between; per motion the dict of
    paths_from_grids."""
    ctx = _capi.default_context(ctx)
    ref = np.ascontiguousarray(ref_cloud, dtype=np.float64)
    clouds = [np.asarray(c, dtype=np.float64).reshape(-1, ref.shape[1], 3) for c in clouds]
    if not clouds:
        return []
    _check_limits(len(ref), [len(c) for c in clouds], ref.shape[1])
    off = _offsets([len(c) for c in clouds])
    with ctx.buffers() as bufs:
        a_dev, b_dev, s_dev = bufs.upload(ref), bufs.upload(np.concatenate(clouds)), bufs.malloc(8 * len(ref) * int(off[-1]))
        _capi.dtw_distance_grids(ctx, a_dev, len(ref), b_dev, off, ref.shape[1], weights, s_dev)
        return _paths_on_device(ctx, bufs, s_dev, len(ref), off, accumulated)[0]


def _reference_indices(references, n):
    if references is None:
        return None
    refs = [int(r) for r in references]
    if any(r < 0 or r >= n for r in refs):
        raise ValueError("a reference index outside the %d motions: %r" % (n, refs))
    return np.asarray(refs, dtype=np.int64)


def all_pairs_costs(clouds, weights=None, references=None, ctx=None):
    """mg_dtw_pair_costs: the (R, N) float64 matrix of total DTW costs, entry (r, n) = dtw_batch(clouds[references[r]],
    clouds)[n]["total"] bit for bit; clouds: a list of (F_n, J, 3) arrays; references: a list of indices into it (None: all,
    R = N).  No grid, accumulated cost or path is formed in memory."""
    ctx = _capi.default_context(ctx)
    clouds = [np.asarray(c, dtype=np.float64) for c in clouds]
    if not clouds:
        return np.zeros((0, 0))
    n_joints = clouds[0].shape[1]
    clouds = [c.reshape(-1, n_joints, 3) for c in clouds]
    refs = _reference_indices(references, len(clouds))
    n_refs = len(clouds) if refs is None else len(refs)
    if n_refs == 0:
        return np.zeros((0, len(clouds)))
    _check_limits(1, [len(c) for c in clouds], n_joints)
    off = _offsets([len(c) for c in clouds])
    with ctx.buffers() as bufs:
        c_dev, o_dev = bufs.upload(np.concatenate(clouds)), bufs.malloc(8 * n_refs * len(clouds))
        _capi.dtw_pair_costs(ctx, c_dev, off, n_joints, weights, refs, o_dev)
        return ctx.download(o_dev, (n_refs, len(clouds)), np.float64)


def all_pairs_costs_host(clouds, weights=None, references=None):
    """all_pairs_costs from distance_grid_host and dtw_paths_host."""
    clouds = [np.asarray(c, dtype=np.float64) for c in clouds]
    refs = _reference_indices(references, len(clouds))
    refs = range(len(clouds)) if refs is None else refs
    out = np.zeros((len(refs), len(clouds)))
    for r, m in enumerate(refs):
        for n, c in enumerate(clouds):
            out[r, n] = dtw_paths_host(distance_grid_host(clouds[int(m)], c, weights))[0][-1, -1]
    return out


def reference_from_costs(costs, keys):
    """The selection the reference's find_optimal_dtw means (dtw.py:133-146): row r of `costs` (R, N) holds the path costs of the
    N motions against candidate keys[r]; its mean is the entries added in column order, then divided by N
    (avg_distances[i] += path_cost; avg_distances[i] /= n); the FIRST least mean wins (strict <).  Returns (key, the R means)."""
    costs = np.asarray(costs, dtype=np.float64)
    keys = list(keys)
    if costs.ndim != 2 or costs.shape[0] != len(keys) or len(keys) == 0 or costs.shape[1] == 0:
        raise ValueError("costs %r for %d candidate keys" % (costs.shape, len(keys)))
    if not np.all(np.isfinite(costs)):
        raise ValueError("the costs hold non-finite values")
    n = costs.shape[1]
    means = np.zeros(len(keys))
    best_key, best_d = None, np.inf
    for r, row in enumerate(costs.tolist()):
        total = 0.0
        for v in row:
            total += v
        means[r] = total / n
        if means[r] < best_d:
            best_key, best_d = keys[r], means[r]
    return best_key, means


def select_reference_motion(skeleton, joints, motions, candidates=None, ctx=None):
    """The motion the others are best warped against: (key, OrderedDict candidate key -> mean cost), the key with the FIRST
    least mean DTW cost of all motions against it.  One forward-kinematics call for all motions (the clouds stay on the
    device), one mg_dtw_pair_costs call; candidates: the keys to choose among (None: all, in the motions' order)."""
    ctx = _capi.default_context(ctx)
    keys = list(motions.keys())
    candidates = keys if candidates is None else list(candidates)
    missing = [k for k in candidates if k not in motions]
    if missing or not candidates:
        raise KeyError("the candidates %r are not among the motions" % (missing,))
    frames = [np.asarray(motions[k], dtype=np.float64) for k in keys]
    n_dim = frames[0].shape[1]
    if any(f.ndim != 2 or f.shape[1] != n_dim for f in frames):
        raise ValueError("the motions of one call have the same channels")
    idx = skeleton.indices(joints)
    _check_limits(1, [len(f) for f in frames], len(idx))
    off = _offsets([len(f) for f in frames])
    total, nj = int(off[-1]), len(idx)
    refs = None if candidates == keys else np.asarray([keys.index(k) for k in candidates], dtype=np.int64)
    with ctx.buffers() as bufs:
        f_dev, c_dev = bufs.upload(np.concatenate(frames)), bufs.malloc(8 * total * nj * 3)
        ctx.joint_positions_dev(skeleton, idx, f_dev, total, n_dim, c_dev)
        o_dev = bufs.malloc(8 * len(candidates) * len(keys))
        _capi.dtw_pair_costs(ctx, c_dev, off, nj, None, refs, o_dev)
        costs = ctx.download(o_dev, (len(candidates), len(keys)), np.float64)
    key, means = reference_from_costs(costs, candidates)
    return key, collections.OrderedDict((k, float(v)) for k, v in zip(candidates, means))


def _as_path(pairs):
    return [(int(i), int(j)) for i, j in pairs]


def run_dtw(x, y, ctx=None):
    """dtw.py run_dtw: (path, D) of the clouds x (Nx, J, 3) and y (Ny, J, 3)."""
    r = dtw_batch(x, [y], accumulated=True, ctx=ctx)[0]
    return _as_path(r["path"]), r["D"]


def find_optimal_dtw(point_clouds, mean_key, weights=None, ctx=None):
    """The find_optimal_dtw_async leg with a reference motion: {key: path} of every motion's clouds against
    point_clouds[mean_key], in one batched call."""
    if mean_key not in point_clouds:
        raise KeyError("find_optimal_dtw needs the key of the reference motion (the all-pairs search is not reproduced): %r" % (mean_key,))
    keys = list(point_clouds.keys())
    results = dtw_batch(point_clouds[mean_key], [point_clouds[k] for k in keys], weights=weights, ctx=ctx)
    return {k: _as_path(r["path"]) for k, r in zip(keys, results)}


def _align_section_dev(ctx, bufs, skeleton, idx, f_dev, off, n_dim, ref_index):
    """The device-input form of _align_section: f_dev the ragged table (off[-1], n_dim) of the motions' frames, ref_index the
    reference motion's position (None: the FIRST least mean cost of mg_dtw_pair_costs over the same clouds).  Forward
    kinematics, grids, paths and the warp without leaving the device; returns (the warped frames (n, fr, n_dim), a device
    buffer of the scope `bufs`, the warping functions (n, fr) int32 on the host, ref_index)."""
    total, n, nj = int(off[-1]), len(off) - 1, len(idx)
    with ctx.buffers() as tmp:
        c_dev = tmp.malloc(8 * total * nj * 3)
        ctx.joint_positions_dev(skeleton, idx, f_dev, total, n_dim, c_dev)
        if ref_index is None:
            p_dev = tmp.malloc(8 * n * n)
            _capi.dtw_pair_costs(ctx, c_dev, off, nj, None, None, p_dev)
            ref_index = reference_from_costs(ctx.download(p_dev, (n, n), np.float64), range(n))[0]
        fr = int(off[ref_index + 1] - off[ref_index])
        ref_dev = c_dev.address + 8 * int(off[ref_index]) * nj * 3      # the reference motion's clouds, where they lie
        s_dev = tmp.malloc(8 * fr * total)
        _capi.dtw_distance_grids(ctx, ref_dev, fr, c_dev, off, nj, None, s_dev)
        _, w_dev = _paths_on_device(ctx, tmp, s_dev, fr, off, False)
        o_dev = bufs.malloc(8 * n * fr * n_dim)
        _capi.warp_motions(ctx, f_dev, off, n_dim, w_dev, fr, o_dev)
        warps = ctx.download(w_dev, (n, fr), np.int32)
    return o_dev, warps, ref_index


def _align_section(ctx, skeleton, joints, motions, mean_key):
    keys = list(motions.keys())
    frames = [np.asarray(motions[k], dtype=np.float64) for k in keys]
    n_dim = frames[0].shape[1]
    if any(f.ndim != 2 or f.shape[1] != n_dim for f in frames):
        raise ValueError("the motions of one call have the same channels")
    idx = skeleton.indices(joints)
    fr = len(motions[mean_key])
    _check_limits(fr, [len(f) for f in frames], len(idx))
    off = _offsets([len(f) for f in frames])
    with ctx.buffers() as bufs:
        o_dev, warps, _ = _align_section_dev(ctx, bufs, skeleton, idx, bufs.upload(np.concatenate(frames)), off, n_dim, keys.index(mean_key))
        warped = ctx.download(o_dev, (len(keys), fr, n_dim), np.float64)
    return (collections.OrderedDict((k, warped[m]) for m, k in enumerate(keys)),
            collections.OrderedDict((k, [int(v) for v in warps[m]]) for m, k in enumerate(keys)))


REFERENCE_SELECTIONS = ("average_time_line", "least_mean_cost")


def align_frames_temporally(skeleton, joints, motions, mean_key=None, sections=None, ctx=None, reference_selection="average_time_line"):
    """MotionModelConstructor._align_frames_temporally / _align_frames_temporally_split on the device: `motions` {key: (F_k, D)
    quaternion frames} -> (warped_frames {key: (Fr, D) array}, warping_functions {key: list of Fr frame indices}), two
    OrderedDicts in the input's key order.  skeleton: a _capi.Skeleton; joints: the joints (names or indices) whose global
    positions make a frame's point cloud (mg_joint_positions).  mean_key: the reference motion; None: reference_selection
    decides, "average_time_line" (get_average_time_line, the length closest to the mean length) or "least_mean_cost"
    (select_reference_motion over the WHOLE motions, once, also with sections: the reference passes one mean_key to every
    section).  sections: {key: [{"start_idx", "end_idx"}, ...]}: every motion is cut into its sections on the
    host, the sections are aligned one batched call each, and the results are concatenated."""
    ctx = _capi.default_context(ctx)
    if reference_selection not in REFERENCE_SELECTIONS:
        raise ValueError("reference_selection %r (one of %r)" % (reference_selection, REFERENCE_SELECTIONS))
    if mean_key is None:
        mean_key = get_average_time_line(motions) if reference_selection == "average_time_line" else select_reference_motion(
            skeleton, joints, motions, ctx=ctx)[0]
    if mean_key not in motions:
        raise KeyError("the reference motion %r is not among the motions" % (mean_key,))
    if sections is None:
        return _align_section(ctx, skeleton, joints, motions, mean_key)
    n_sections = len(sections[list(motions.keys())[0]])
    results = []
    for s in range(n_sections):
        part = collections.OrderedDict((k, np.asarray(m)[sections[k][s]["start_idx"]:sections[k][s]["end_idx"]]) for k, m in motions.items())
        results.append(_align_section(ctx, skeleton, joints, part, mean_key))
    warped_frames, warping_functions = collections.OrderedDict(), collections.OrderedDict()
    for k in motions.keys():
        warped_frames[k] = np.concatenate([r[0][k] for r in results])
        warping_functions[k] = [v for r in results for v in r[1][k]]
    return warped_frames, warping_functions
