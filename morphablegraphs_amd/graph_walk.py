"""A graph walk and its motion as one array of frames (reference morphablegraphs/motion_generator/graph_walk.py).

GraphWalk.convert_graph_walk_to_quaternion_frames (:154-176) back-projects every step, aligns it to the last frame so far
(MotionVector.append_frames; smoothing is off during synthesis, :102) and appends it.  Here the walk's frames are assembled on
the device by mg_walk_frames (csrc/mg_walk.hip): a chain kernel forms every step's transform, a frames kernel writes every row
once where it ends up -- for one walk (HipGraphWalk) or a population of walks over the same nodes (assemble_walks).

assemble_walk_host is the NumPy statement of the same arithmetic on the frames side; it needs no library.

Out of scope (anim_utils code with no statement here): transition smoothing of the exported motion, foot_joint-based
alignment, IK constraint creation, get_average_keyframe_constraint_error, plotting and export.
"""
import ctypes as C

import numpy as np

from . import _capi
from .candidate_scoring import alignment_from_start_pose

MG_WALK_MAX_STEPS = _capi.MG_WALK_MAX_STEPS


# ---- the arithmetic on the host ------------------------------------------------------------------------------------
def _basis_rows(knots, times):
    """First tap i0 and the four weights of a clamped cubic B-spline at every time, de Boor's recurrence on the span
    FITPACK's splev picks (ext = 0: times outside the knots use the end spans)."""
    t = np.asarray(knots, dtype=np.float64)
    n = len(t)
    i0 = np.empty(len(times), dtype=np.int64)
    w = np.empty((len(times), 4))
    for f, x in enumerate(np.asarray(times, dtype=np.float64)):
        l = 3
        while not (x < t[l + 1] or l == n - 5):
            l += 1
        h = [1.0, 0.0, 0.0, 0.0]
        for j in range(1, 4):
            hh = h[:j]
            h[0] = 0.0
            for i in range(1, j + 1):
                li, lj = l + i, l + i - j
                if t[li] == t[lj]:
                    h[i] = 0.0
                    continue
                fac = hh[i - 1] / (t[li] - t[lj])
                h[i - 1] = h[i - 1] + fac * (t[li] - x)
                h[i] = fac * (x - t[lj])
        i0[f], w[f] = l - 3, h
    return i0, w


def _untimed_grid(n_canonical_frames, speed=1.0):
    """The time function of a step without a time model (motion_primitive.py:233): linspace(0, F, int(F * (1 / speed)))."""
    count = int(n_canonical_frames * (1.0 / float(speed)))
    if count < 1:
        raise ValueError("a step of %d canonical frames has no sample at speed %g" % (n_canonical_frames, speed))
    return np.linspace(0, n_canonical_frames, count)


class _HostModel(object):
    """The spatial model of a primitive as NumPy arrays, from the reference's JSON dict or a HipMotionPrimitive."""

    def __init__(self, src):
        if isinstance(src, dict):
            eig = np.asarray(src["eigen_vectors_spatial"], dtype=np.float64).T     # (NB * D, L)
            mean = np.asarray(src["mean_spatial_vector"], dtype=np.float64)
            self.n_basis, self.n_dim = int(src["n_basis_spatial"]), int(src["n_dim_spatial"])
            self.knots = np.asarray(src["b_spline_knots_spatial"], dtype=np.float64)
            self.n_canonical_frames = int(src["n_canonical_frames"])
            tm = np.asarray(src.get("translation_maxima", (1.0, 1.0, 1.0)), dtype=np.float64)
        else:
            src = getattr(src, "motion_primitive", src)
            eig, mean = np.asarray(src.s_pca["eigen_vectors"], dtype=np.float64), np.asarray(src.s_pca["mean_vector"], dtype=np.float64)
            self.n_basis, self.n_dim = int(src.s_pca["n_basis"]), int(src.s_pca["n_dim"])
            self.knots = np.asarray(src.s_pca["knots"], dtype=np.float64)
            self.n_canonical_frames = int(src.n_canonical_frames)
            tm = np.asarray(src.translation_maxima, dtype=np.float64)
        scale = np.ones(self.n_dim)
        scale[:3] = tm
        scale = np.tile(scale, self.n_basis)
        self.eigen, self.mean = eig * scale[:, None], mean * scale       # scaled once, as the library holds them
        self.n_components = self.eigen.shape[1]

    def frames(self, alpha, times=None, speed=1.0):
        """(control points (NB, D), frames (T, D)) of one latent vector at `times` (None: the canonical grid at `speed`)."""
        cp = (self.mean + self.eigen @ np.asarray(alpha, dtype=np.float64)).reshape(self.n_basis, self.n_dim)
        if times is None:
            times = _untimed_grid(self.n_canonical_frames, speed)
        i0, w = _basis_rows(self.knots, times)
        out = w[:, 0:1] * cp[i0]
        for j in range(1, 4):
            out = out + w[:, j:j + 1] * cp[i0 + j]
        return cp, out


def _aligning_links(alignment, skeleton):
    """(quaternion channels along the aligning node's chain, ref_dir) of a first-step record: the record's node for a
    previous-frame record, else the root and (0, 0, 1)."""
    joint, ref_dir = 0, (0.0, 0.0, 1.0)
    if alignment is not None and alignment.get("joint", 0) != _capi.MG_ALIGN_START_POSE:
        joint, ref_dir = alignment.get("joint", 0), tuple(alignment.get("ref_dir", ref_dir))
    if skeleton is None:
        if joint != 0:
            raise ValueError("aligning joint %r is not the root: a skeleton is needed" % (joint,))
        return [3], ref_dir
    return [int(skeleton.quat_channel[j]) for j in skeleton.chain(joint) if skeleton.quat_channel[j] >= 0], ref_dir


def _heading(pose, links, ref_dir):
    """Unit (x, z) of the chain's orientation in `pose` applied to ref_dir (Skeleton.heading on channel lists)."""
    q = np.array([1.0, 0.0, 0.0, 0.0])
    for ch in links:
        qj = pose[ch:ch + 4]
        q = _capi._quat_mul(q, qj / np.linalg.norm(qj))
    v, u = np.asarray(ref_dir, dtype=np.float64), q[1:]
    p = v + 2.0 * (q[0] * np.cross(u, v) + np.cross(u, np.cross(u, v)))
    d = np.array([p[0], p[2]])
    return d / np.linalg.norm(d)


def _transform_frames(frames, c, s, tx, tz, ty=0.0):
    """mg_align_frames' map on (T, D) frames: positions (c x + s z + tx, y + ty, -s x + c z + tz), root quaternion turned."""
    out = np.array(frames, dtype=np.float64)
    x, z = frames[:, 0], frames[:, 2]
    out[:, 0], out[:, 1], out[:, 2] = c * x + s * z + tx, frames[:, 1] + ty, c * z - s * x + tz
    phi = np.arctan2(s, c)
    aw, ay = np.cos(0.5 * phi), np.sin(0.5 * phi)
    qw, qx, qy, qz = frames[:, 3], frames[:, 4], frames[:, 5], frames[:, 6]
    out[:, 3], out[:, 4], out[:, 5], out[:, 6] = aw * qw - ay * qy, aw * qx + ay * qz, aw * qy + ay * qw, aw * qz - ay * qx
    return out


def _step_transform(first_pose, target, links, ref_dir):
    """(c, s, tx, tz, ty) that puts a step whose first control point is `first_pose` onto target = (heading, (x, z)) or, for a
    start pose, ((cos, sin), (x, z), height)."""
    p0x, p0z = first_pose[0], first_pose[2]
    if len(target) == 3:
        (c, s), (px, pz), ty = target
    else:
        (hx, hz), (px, pz) = target
        bx, bz = _heading(first_pose, links, ref_dir)
        c, s, ty = hx * bx + hz * bz, hx * bz - hz * bx, 0.0
    return c, s, px - (c * p0x + s * p0z), pz - (c * p0z - s * p0x), ty


def _first_target(alignment):
    if alignment is None:
        return None
    h = np.asarray(alignment["heading"], dtype=np.float64)
    h = h / np.linalg.norm(h)
    pos = alignment["position"]
    if alignment.get("joint", 0) == _capi.MG_ALIGN_START_POSE:
        return (h[0], h[1]), (float(pos[0]), float(pos[2])), float(pos[1])
    return (h[0], h[1]), (float(pos[0]), float(pos[2]))


def _latent_offsets(models, latent_offset):
    if latent_offset is not None:
        return [int(v) for v in latent_offset]
    return [int(v) for v in np.concatenate(([0], np.cumsum([m.n_components for m in models])[:-1]))]


def assemble_walk_host(models, S, latent_offset=None, times=None, alignment=None, skeleton=None, speed=1.0):
    """The frames of walks over `models` (one per step: JSON dicts or primitives), NumPy only -- the statement of
    mg_walk_frames' arithmetic.  S (n_walks, ld); step i reads columns latent_offset[i] .. (default: back to back);
    times: None (canonical grids) or times[w][i] = the step's time row, None for a step without a time model: its canonical
    grid at `speed`, linspace(0, F, int(F * (1 / speed))), as back_project takes it (motion_primitive.py:233); alignment: None, a previous-frame record
    (Skeleton.alignment_to) or a start-pose record (alignment_from_start_pose), for the FIRST step; every later step is aligned
    to the aligned last sample of the step before it.  Returns (frames (n_walks, T, D) padded with NaN, offsets
    (n_walks, n_steps + 1), transforms (n_walks, n_steps, 4) = (c, s, tx, tz))."""
    models = [m if isinstance(m, _HostModel) else _HostModel(m) for m in models]
    S = np.atleast_2d(np.asarray(S, dtype=np.float64))
    offs = _latent_offsets(models, latent_offset)
    links, ref_dir = _aligning_links(alignment, skeleton)
    n, m = len(S), len(models)
    walks, offsets, transforms = [], np.zeros((n, m + 1), dtype=np.int64), np.zeros((n, m, 4))
    for w in range(n):
        target, parts = _first_target(alignment), []
        for i, model in enumerate(models):
            cp, fr = model.frames(S[w, offs[i]:offs[i] + model.n_components], None if times is None else times[w][i], speed)
            if target is None:
                transforms[w, i] = (1.0, 0.0, 0.0, 0.0)
            else:
                c, s, tx, tz, ty = _step_transform(cp[0], target, links, ref_dir)
                fr = _transform_frames(fr, c, s, tx, tz, ty)
                transforms[w, i] = (c, s, tx, tz)
            target = (tuple(_heading(fr[-1], links, ref_dir)), (fr[-1, 0], fr[-1, 2]))
            parts.append(fr)
            offsets[w, i + 1] = offsets[w, i] + len(fr)
        walks.append(np.concatenate(parts))
    T = int(offsets[:, -1].max()) if n else 0
    frames = np.full((n, T, models[0].n_dim if m else 0), np.nan)
    for w, fr in enumerate(walks):
        frames[w, :len(fr)] = fr
    return frames, offsets, transforms


def align_frames_host(frames, alignment, skeleton=None):
    """(T, D) frames of one step put onto a first-step record the way mg_align_frames does, with the step's heading read from
    its first FRAME (what MotionVector.append_frames has: frames, not control points)."""
    frames = np.asarray(frames, dtype=np.float64)
    target = _first_target(alignment)
    if target is None:
        return frames.copy()
    links, ref_dir = _aligning_links(alignment, skeleton)
    c, s, tx, tz, ty = _step_transform(frames[0], target, links, ref_dir)
    return _transform_frames(frames, c, s, tx, tz, ty)


# ---- the device --------------------------------------------------------------------------------------------------
def _primitive_of(node):
    return getattr(node, "motion_primitive", node)


def _address(buf):
    return buf.address if isinstance(buf, _capi.DeviceBuffer) else int(buf)


def _record_node(alignment):
    """(joint, ref_dir) later steps are aligned through: a previous-frame record's, else the root and (0, 0, 1)."""
    if alignment is None or alignment.get("joint", 0) == _capi.MG_ALIGN_START_POSE:
        return 0, (0.0, 0.0, 1.0)
    return alignment.get("joint", 0), tuple(alignment.get("ref_dir", (0.0, 0.0, 1.0)))


def walk_frames_dev(prims, latent_offset, d_S, dtype, n_walks, ld, d_frames, walk_stride, d_times=None, lengths=None, t_cap=0,
                    frame_offset=None, alignment=None, skeleton=None, d_transforms=None):
    """mg_walk_frames on device buffers.  prims: _capi.Primitive per step; lengths / frame_offset: host arrays (n_walks, n_steps)."""
    m = len(prims)
    lib = prims[0].lib
    handles = (C.c_void_p * m)(*[p.handle.value for p in prims])
    lo = np.ascontiguousarray(latent_offset, dtype=np.int64)
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    fo = None if frame_offset is None else np.ascontiguousarray(frame_offset, dtype=np.int64)
    al = _capi.ConstraintSet._marshal_alignment(alignment, skeleton) if alignment is not None else None
    sk = skeleton.desc() if skeleton is not None else None
    code = _capi.MG_F64 if np.dtype(dtype) == np.float64 else _capi.MG_F32
    _capi._check(lib.mg_walk_frames(m, handles, _capi._host_ptr(lo), _capi._dev_ptr(d_S), code, int(n_walks), int(ld),
                                    _capi._dev_ptr(d_times) if d_times is not None else None, _capi._host_ptr(ln), int(t_cap), _capi._host_ptr(fo),
                                    C.byref(al) if al is not None else None, C.byref(sk) if sk is not None else None, _capi._dev_ptr(d_frames),
                                    int(walk_stride), _capi._dev_ptr(d_transforms) if d_transforms is not None else None))


def _sample_times(ctx, bufs, mps, d_G, G, goffs, speed):
    """The time rows of every (walk, step) on the device: d_times (n_walks, n_steps, t_cap), lengths (n_walks, n_steps) on the host.
    One mg_time_function_sample_rows per step with a time model, its rows n_steps * t_cap doubles apart so that they land in place
    (a row that needs more than t_cap samples is not written and reports how many: the table is laid out again); the lengths of all
    steps come back in one download; steps without a time model get their canonical grid at `speed`.  With smooth_time_parameters
    the rows pass through the host -- or, for a primitive with smooth_on_device, come smoothed from
    mg_time_function_sample_smoothed_rows and stay where they are (ValueError naming the (walk, step) whose row has fewer than
    15 samples, as scipy would, once the lengths are known)."""
    from .time_smoothing import require_smoothing_window
    n, m = G.shape[0], len(mps)
    has_time = [mp.has_time_parameters and mp.get_n_time_components() > 0 for mp in mps]
    timed = [i for i, ht in enumerate(has_time) if ht]
    grids = [None if ht else _untimed_grid(mp.n_canonical_frames, speed) for mp, ht in zip(mps, has_time)]
    t_cap = max([int(4 * mp.n_canonical_frames / min(float(speed), 1.0)) + 8 if ht else len(g) for mp, ht, g in zip(mps, has_time, grids)])
    on_device = [ht and mp.smooth_time_parameters and getattr(mp, "smooth_on_device", False) for mp, ht in zip(mps, has_time)]
    smooth = any(ht and mp.smooth_time_parameters and not dev for mp, ht, dev in zip(mps, has_time, on_device))
    item = G.dtype.itemsize
    while True:
        lengths = np.zeros((n, m), dtype=np.int32)
        if len(timed) < m:
            host = np.zeros((n, m, t_cap))
            for i, g in enumerate(grids):
                if g is not None:
                    host[:, i, :len(g)], lengths[:, i] = g, len(g)
            d_t = bufs.upload(host)
        else:
            d_t = bufs.malloc(8 * n * m * t_cap)
        d_l = bufs.malloc(4 * n * max(len(timed), 1))
        for j, i in enumerate(timed):
            prim = mps[i]._prim
            sample_rows = prim.lib.mg_time_function_sample_smoothed_rows if on_device[i] else prim.lib.mg_time_function_sample_rows
            _capi._check(sample_rows(prim.handle, C.c_void_p(d_G.address + int(goffs[i]) * item), _capi._dtype_code(G), n, G.shape[1], float(speed),
                                     C.c_void_p(d_t.address + 8 * i * t_cap), C.c_void_p(d_l.address + 4 * j * n), t_cap, m * t_cap, None))
        if timed:
            ln = ctx.download(d_l, (len(timed), n), np.int32)
            if (ln == 0).any():
                raise ValueError("a time function is not finite")
            lengths[:, timed] = np.abs(ln).T            # (negative: the samples the row would need)
        if lengths.max() <= t_cap:
            break
        t_cap = int(lengths.max()) + 8
    if any(on_device):
        require_smoothing_window(np.where(np.array(on_device)[None, :], lengths, 0), "walk %d, step %d")
    if smooth:
        times = ctx.download(d_t, (n, m, t_cap), np.float64)
        for i, (mp, ht) in enumerate(zip(mps, has_time)):
            if ht and mp.smooth_time_parameters and not on_device[i]:
                for w in range(n):
                    times[w, i, :lengths[w, i]] = mp._smooth_time_function(times[w, i, :lengths[w, i]])
        d_t = bufs.upload(times)
    return d_t, lengths, t_cap


def _piece_times(ctx, bufs, mps, n, G=None, goffs=None, speed=1.0):
    """(d_times, lengths int32, t_cap, rows the longest walk needs) of one piece: what _assemble_piece takes as `timing`, known
    before the frame rows are sized.  G None: the canonical grids, (None, None, 0, their sum)."""
    if G is None:
        return None, None, 0, sum(mp.n_canonical_frames for mp in mps)
    d_t, ln, t_cap = _sample_times(ctx, bufs, mps, bufs.upload(G), G, goffs, speed)
    return d_t, ln, t_cap, int(ln.astype(np.int64).sum(axis=1).max()) if n else 0


def _assemble_piece(ctx, bufs, mps, S, offs, d_frames, row0, walk_stride, alignment, skeleton, timing, d_transforms=None):
    """One mg_walk_frames call for at most MG_WALK_MAX_STEPS steps: the frames land in d_frames from row `row0` of every walk on.
    timing: the piece's _piece_times.  Returns the offsets (n_walks, n_steps + 1) relative to row0."""
    n, m = S.shape[0], len(mps)
    d_S = bufs.upload(S)
    prims = [mp._prim for mp in mps]
    d_t, ln, t_cap, _ = timing
    if ln is None:
        lengths = np.tile(np.array([mp.n_canonical_frames for mp in mps], dtype=np.int64), (n, 1))
    else:
        lengths = ln.astype(np.int64)
    offsets = np.zeros((n, m + 1), dtype=np.int64)
    offsets[:, 1:] = np.cumsum(lengths, axis=1)
    if n and offsets[:, -1].max() > walk_stride - row0:
        raise ValueError("the walk needs %d rows, %d are left" % (int(offsets[:, -1].max()), walk_stride - row0))
    D = prims[0].n_dim
    walk_frames_dev(prims, offs, d_S, S.dtype, n, S.shape[1], _address(d_frames) + 8 * row0 * D, walk_stride, d_t, ln, t_cap,
                    offsets[:, :-1] if ln is not None else None, alignment, skeleton, d_transforms)
    return offsets


def _walk_rows(mps, time_parameters, speed):
    """The rows a walk usually stays within, before its lengths are known (a step without a time model has int(F / speed) <=
    4 F / min(speed, 1) + 8 of them; a time function may ask for more: the rows then follow the lengths)."""
    if time_parameters is None:
        return sum(mp.n_canonical_frames for mp in mps)
    return sum(int(4 * mp.n_canonical_frames / min(float(speed), 1.0)) + 8 for mp in mps)


def assemble_walks(graph, node_keys, S, time_parameters=None, alignment=None, skeleton=None, speed=1.0, with_transforms=False, ctx=None):
    """The frames of a population of walks over the nodes `node_keys` of `graph` (a HipMotionStateGraph or HipPrimitiveSet):
    S (n_walks, sum of the steps' spatial latents), float32 or float64 -- the batch the global objectives score;
    time_parameters: None (canonical grids) or (n_walks, sum of the steps' time latents) for the time-warped motion.
    Returns (frames (n_walks, T, D) float64 with NaN behind a walk's end, offsets (n_walks, n_steps + 1)[, transforms])."""
    mps = [_primitive_of(graph.nodes[k]) for k in node_keys]
    S = _capi._latents(S)
    G = None if time_parameters is None else _capi._latents(time_parameters)
    n, m = S.shape[0], len(mps)
    offs = np.concatenate(([0], np.cumsum([mp.get_n_spatial_components() for mp in mps]))).astype(np.int64)
    goffs = np.concatenate(([0], np.cumsum([mp.get_n_time_components() for mp in mps]))).astype(np.int64)
    if S.shape[1] < offs[-1] or (G is not None and G.shape[1] < goffs[-1]):
        raise ValueError("latent rows are shorter than the walk's steps need")
    ctx = ctx or mps[0]._prim.ctx
    D = mps[0]._prim.n_dim
    pieces = [(a, min(a + MG_WALK_MAX_STEPS, m)) for a in range(0, m, MG_WALK_MAX_STEPS)]
    with ctx.buffers() as bufs:
        # the time functions first: the frame rows are sized by the lengths they give (beyond MG_WALK_MAX_STEPS steps the time tables
        # of all n_walks x pieces stay on the device until the call ends: n_walks x n_steps x t_cap doubles, a fraction of the frames)
        if m <= MG_WALK_MAX_STEPS:
            timing = _piece_times(ctx, bufs, mps, n, G, goffs[:-1], speed)
            rows = max(timing[3], 1)
        else:
            timing = [[_piece_times(ctx, bufs, mps[a:b], 1, None if G is None else G[w:w + 1], goffs[a:b], speed) for a, b in pieces] for w in range(n)]
            rows = max([sum(t[3] for t in tw) for tw in timing] + [1])
        d_f = bufs.malloc(8 * max(n, 1) * rows * D)
        d_x = bufs.malloc(8 * max(n, 1) * m * 4) if with_transforms else None
        if m <= MG_WALK_MAX_STEPS:
            offsets = _assemble_piece(ctx, bufs, mps, S, offs[:-1], d_f, 0, rows, alignment, skeleton, timing, d_x)
        else:
            # a longer walk in pieces: the last frame of one piece gives the previous-frame record of the next, walk by walk
            joint, ref_dir = _record_node(alignment)
            sk = skeleton if skeleton is not None else _ROOT_ONLY
            offsets = np.zeros((n, m + 1), dtype=np.int64)
            for w in range(n):
                al, row0 = alignment, 0
                for (a, b), tm in zip(pieces, timing[w]):
                    d_w = d_f.address + 8 * w * rows * D
                    d_xw = d_x.address + 8 * (w * m + a) * 4 if d_x is not None else None
                    po = _assemble_piece(ctx, bufs, mps[a:b], S[w:w + 1], offs[a:b], d_w, row0, rows, al, skeleton if (al is alignment or joint != 0) else None,
                                         tm, d_xw)
                    offsets[w, a + 1:b + 1] = row0 + po[0, 1:]
                    row0 = int(offsets[w, b])
                    last = ctx.download(d_f.address + 8 * ((w * rows + row0 - 1) * D), (D,), np.float64)
                    al = sk.alignment_to(last, joint, ref_dir)
        # only the rows the walks own come back; NaN behind a walk's end
        T = int(offsets[:, -1].max()) if n else 0
        if T == rows:
            frames = ctx.download(d_f, (n, T, D), np.float64)
        else:
            frames = np.empty((n, T, D))
            for w in range(n):
                frames[w] = ctx.download(d_f.address + 8 * w * rows * D, (T, D), np.float64)
        for w in range(n):
            frames[w, int(offsets[w, -1]):] = np.nan
        if with_transforms:
            return frames, offsets, ctx.download(d_x, (n, m, 4), np.float64)
        return frames, offsets


def walk_step_lengths(mps, S, offsets=None, method="arc_length"):
    """Step lengths of a population of walks over the primitives `mps` (one per step; a primitive may repeat) in ONE
    mg_step_lengths call: (n_walks, n_steps) float64.  S (n_walks, ld) float32 or float64; step i reads its spatial latents from
    column offsets[i] on (default: back to back).  One item per step over the shared matrix; a step's length does not depend on
    its alignment (a rotation about y and a translation keep ground-plane lengths), so the unaligned control points are scored."""
    mps = [_primitive_of(mp) for mp in mps]
    S = _capi._latents(S)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum([mp.get_n_spatial_components() for mp in mps])[:-1]))
    out = _capi.step_lengths([(mp._prim, S, int(off)) for mp, off in zip(mps, offsets)], method)
    return np.stack(out, axis=1) if out else np.zeros((S.shape[0], 0))


_ROOT_ONLY = _capi.Skeleton([("root", None, (0.0, 0.0, 0.0))], ["root"])


# ---- the reference's classes -----------------------------------------------------------------------------------------
class HipGraphWalkStep(object):
    """GraphWalkEntry (graph_walk.py:44-69)."""

    def __init__(self, node_key, parameters, n_spatial_components, n_time_components, start_frame=0, end_frame=0, motion_primitive_constraints=None,
                 arc_length=0.0):
        self.node_key = tuple(node_key)
        self.parameters = np.array(parameters, dtype=np.float64)
        self.n_spatial_components = int(n_spatial_components)
        self.n_time_components = int(n_time_components)
        self.start_frame = start_frame
        self.end_frame = end_frame
        self.motion_primitive_constraints = motion_primitive_constraints
        self.arc_length = arc_length

    @staticmethod
    def from_graph(motion_state_graph, node_key, parameters, start_frame=0, end_frame=0, motion_primitive_constraints=None, arc_length=0.0):
        node = motion_state_graph.nodes[node_key]
        return HipGraphWalkStep(node_key, parameters, node.get_n_spatial_components(), node.get_n_time_components(), start_frame, end_frame,
                                motion_primitive_constraints, arc_length)

    @staticmethod
    def from_json(motion_state_graph, data):
        return HipGraphWalkStep.from_graph(motion_state_graph, tuple(data["node_key"]), np.array(data["parameters"]), data["start_frame"], data["end_frame"],
                                           arc_length=data.get("arc_length", 0.0))

    def to_json(self):
        return {"node_key": self.node_key, "parameters": self.parameters.tolist(), "arc_length": self.arc_length,
                "start_frame": self.start_frame, "end_frame": self.end_frame}


class _DeviceRows(object):
    """A walk's frames in one device buffer that grows; rows [0, n) are the walk."""

    def __init__(self, ctx):
        self.ctx, self.buf, self.capacity, self.n_dim = ctx, None, 0, None

    def reserve(self, rows, n_dim, keep):
        self.n_dim = n_dim
        if rows <= self.capacity:
            return
        kept = self.read(keep) if keep else None
        if self.buf is not None:
            self.buf.free()
        self.capacity = max(int(rows), 2 * self.capacity)
        self.buf = self.ctx.malloc(8 * self.capacity * n_dim)
        if keep:
            self.write(0, kept)

    def address(self, row=0):
        return self.buf.address + 8 * row * self.n_dim

    def read(self, n, row0=0):
        return self.ctx.download(self.address(row0), (n, self.n_dim), np.float64)

    def write(self, row0, frames):
        self.ctx.upload_into(self.address(row0), np.ascontiguousarray(frames, dtype=np.float64))

    def free(self):
        if self.buf is not None:
            self.buf.free()
        self.buf, self.capacity = None, 0


class _HostRows(object):
    """The same rows in a NumPy array (HipGraphWalk(host=True): the arithmetic's statement, no device)."""

    def __init__(self):
        self.rows, self.n_dim = None, None

    def reserve(self, rows, n_dim, keep):
        self.n_dim = n_dim
        if self.rows is None or rows > len(self.rows):
            new = np.full((int(rows), n_dim), np.nan)
            if keep:
                new[:keep] = self.rows[:keep]
            self.rows = new

    def read(self, n, row0=0):
        return self.rows[row0:row0 + n].copy()

    def write(self, row0, frames):
        self.rows[row0:row0 + len(frames)] = frames

    def free(self):
        self.rows = None


class HipGraphWalk(object):
    """GraphWalk's method table over a HipMotionStateGraph or HipPrimitiveSet; the walk's frames live on the device.

    skeleton: a _capi.Skeleton, needed when the aligning node is not the root (default: the graph's hip_skeleton); the aligning
    node and reference direction come from the graph's reference skeleton (aligning_root_node, aligning_root_dir) where it has
    one, else the root and (0, 0, 1).  host=True keeps the frames in NumPy and assembles them with assemble_walk_host: the
    statement of the arithmetic, for graphs whose nodes carry no device primitive."""

    def __init__(self, motion_state_graph, start_pose=None, use_time_parameters=False, skeleton=None, ctx=None, host=False):
        self.motion_state_graph = motion_state_graph
        self.steps = []
        self.start_pose = start_pose
        self.use_time_parameters = use_time_parameters
        self.skeleton = skeleton if skeleton is not None else getattr(motion_state_graph, "hip_skeleton", None)
        ref_sk = getattr(motion_state_graph, "skeleton", None)
        node = getattr(ref_sk, "aligning_root_node", None)
        if node is not None and self.skeleton is None and node != getattr(ref_sk, "root", node):
            raise ValueError("aligning node %r is not the root joint: pass a _capi.Skeleton" % (node,))
        self._joint = 0 if node is None or self.skeleton is None else self.skeleton.index(node)
        self._ref_dir = tuple(float(v) for v in getattr(ref_sk, "aligning_root_dir", (0.0, 0.0, 1.0)))
        self._ctx, self._is_host = ctx, bool(host)
        self._rows, self._n_frames = None, 0
        self._cache = None               # the downloaded copy, until the next change

    def _store(self):
        if self._rows is None:
            if self._is_host:
                self._rows = _HostRows()
            else:
                if self._ctx is None:
                    self._ctx = _primitive_of(next(iter(self.motion_state_graph.nodes.values())))._prim.ctx
                self._rows = _DeviceRows(self._ctx)
        return self._rows

    def _alignment_at(self, n_kept):
        """The record a step is aligned to when `n_kept` rows precede it."""
        if n_kept > 0:
            return (self.skeleton or _ROOT_ONLY).alignment_to(self._store().read(1, n_kept - 1)[0], self._joint, self._ref_dir)
        return alignment_from_start_pose(self.start_pose) if self.start_pose is not None else None

    def _record_skeleton(self, alignment):
        return self.skeleton if _record_node(alignment)[0] != 0 else None

    # ---- graph_walk.py:154-176 -----------------------------------------------------------------------
    def convert_graph_walk_to_quaternion_frames(self, start_step=0, use_time_parameters=False, step_size=1.0):
        """The frames before steps[start_step].start_frame are kept, the rest is rebuilt from the last kept frame; every rebuilt
        step gets its start_frame and end_frame."""
        start_frame = 0 if start_step == 0 else int(self.steps[start_step].start_frame)
        steps = self.steps[start_step:]
        self._cache = None
        if not steps:
            self._n_frames = start_frame
            return
        mps = [_primitive_of(self.motion_state_graph.nodes[st.node_key]) for st in steps]
        warped = bool(use_time_parameters) and any(mp.has_time_parameters and mp.get_n_time_components() > 0 for mp in mps)
        if not warped and float(step_size) != 1.0:
            raise NotImplementedError("a step size other than 1 on the canonical grid")
        store = self._store()
        D = int(mps[0].s_pca["n_dim"])
        store.reserve(start_frame + _walk_rows(mps, True if warped else None, step_size), D, start_frame)
        n_s = [st.n_spatial_components for st in steps]
        n_t = [st.n_time_components for st in steps]
        S = np.concatenate([st.parameters[:k] for st, k in zip(steps, n_s)])[None, :]
        G = np.concatenate([st.parameters[k:k + t] for st, k, t in zip(steps, n_s, n_t)])[None, :] if warped else None
        offs, goffs = np.concatenate(([0], np.cumsum(n_s))), np.concatenate(([0], np.cumsum(n_t)))
        row0 = start_frame
        for a in range(0, len(steps), MG_WALK_MAX_STEPS):     # a long walk in pieces: one piece's last frame is the next one's previous frame
            b = min(a + MG_WALK_MAX_STEPS, len(steps))
            al = self._alignment_at(row0)
            if self._is_host:
                times = None
                if warped:
                    times = [[mp.back_project_time_function(G[0, goffs[a + i]:goffs[a + i + 1]], step_size)
                              if mp.has_time_parameters and mp.get_n_time_components() > 0 else None for i, mp in enumerate(mps[a:b])]]
                fr, po, _ = assemble_walk_host(mps[a:b], S, offs[a:b], times, al, self._record_skeleton(al), step_size if warped else 1.0)
                store.reserve(row0 + fr.shape[1], D, row0)       # (a time function may ask for more rows than _walk_rows assumed)
                store.write(row0, fr[0])
            else:
                with self._ctx.buffers() as bufs:
                    timing = _piece_times(self._ctx, bufs, mps[a:b], 1, G, goffs[a:b], step_size)
                    store.reserve(row0 + timing[3], D, row0)     # (a time function may ask for more rows than _walk_rows assumed)
                    po = _assemble_piece(self._ctx, bufs, mps[a:b], S, offs[a:b], store.address(), row0, store.capacity, al, self._record_skeleton(al), timing)
                    self._ctx.synchronize()
            for st, lo, hi in zip(steps[a:b], po[0, :-1], po[0, 1:]):
                st.start_frame, st.end_frame = int(row0 + lo), int(row0 + hi - 1)
            row0 += int(po[0, -1])
        self._n_frames = row0

    # ---- the reference's method table ---------------------------------------------------------------
    def append_quat_frames(self, new_frames):
        """MotionVector.append_frames: the frames aligned to the last frame so far (or the start pose) and appended."""
        new_frames = np.asarray(new_frames, dtype=np.float64)
        store = self._store()
        store.n_dim = new_frames.shape[1]
        al = self._alignment_at(self._n_frames)
        aligned = align_frames_host(new_frames, al, self._record_skeleton(al))
        store.reserve(self._n_frames + len(aligned), new_frames.shape[1], self._n_frames)
        store.write(self._n_frames, aligned)
        self._n_frames += len(aligned)
        self._cache = None

    def get_quat_frames(self):
        """The walk's frames (n_frames, n_dim): downloaded once, the copy kept until the next change."""
        if self._cache is None:
            if self._n_frames == 0:
                return None
            self._cache = self._store().read(self._n_frames)
        return self._cache

    def get_num_of_frames(self):
        return self._n_frames

    def update_arc_lengths(self):
        """Sets every step's arc_length to the length travelled up to and including it (GraphWalkEntry.arc_length, which the
        reference fills from get_step_length_for_sample step by step) from one mg_step_lengths call; returns the per-step lengths."""
        if not self.steps:
            return np.zeros(0)
        mps = [_primitive_of(self.motion_state_graph.nodes[st.node_key]) for st in self.steps]
        n_s = [st.n_spatial_components for st in self.steps]
        S = np.concatenate([st.parameters[:k] for st, k in zip(self.steps, n_s)])[None, :]
        lengths = walk_step_lengths(mps, S, np.concatenate(([0], np.cumsum(n_s)[:-1])))[0]
        for st, travelled in zip(self.steps, np.cumsum(lengths)):
            st.arc_length = float(travelled)
        return lengths

    def advance_along_trajectory(self, trajectory, travelled, look_ahead):
        """GraphWalkPlanner._update_path's rule (graph_walk_planner.py:269-273) for this walk: the arc length of `trajectory` (a
        _capi.Trajectory) travelled once the walk's last frame is taken into account, from the arc length travelled before it.
        The last frame's root position is read where the frames are -- on the device no frame is downloaded
        (trajectory_queries.advance_along_trajectory)."""
        from .trajectory_queries import advance_along_trajectory
        if self._n_frames == 0:
            return float(travelled)
        store = self._store()
        if self._is_host:
            return float(advance_along_trajectory(trajectory, store.read(1, self._n_frames - 1)[:, :3], travelled, look_ahead)[0])
        return float(advance_along_trajectory(trajectory, store.address(self._n_frames - 1), travelled, look_ahead, n=1)[0])

    def get_global_spatial_parameter_vector(self, start_step=0):
        out = []
        for step in self.steps[start_step:]:
            out += step.parameters[:step.n_spatial_components].tolist()
        return out

    def get_global_time_parameter_vector(self, start_step=0):
        out = []
        for step in self.steps[start_step:]:
            out += step.parameters[step.n_spatial_components:].tolist()
        return out

    def update_spatial_parameters(self, parameter_vector, start_step=0):
        offset = 0
        for step in self.steps[start_step:]:
            step.parameters[:step.n_spatial_components] = parameter_vector[offset:offset + step.n_spatial_components]
            offset += step.n_spatial_components

    def update_time_parameters(self, parameter_vector, start_step, end_step):
        offset = 0
        for step in self.steps[start_step:end_step]:
            step.parameters[step.n_spatial_components:] = parameter_vector[offset:offset + step.n_time_components]
            offset += step.n_time_components

    def get_step_from_keyframe(self, keyframe):
        found = -1
        for index, step in enumerate(self.steps):      # the reference's loop does not stop at the first match
            if step.start_frame <= keyframe <= step.end_frame:
                found = index
        return found

    def to_json(self):
        return {"start_pose": self.start_pose, "use_time_parameters": self.use_time_parameters, "steps": [s.to_json() for s in self.steps]}

    @staticmethod
    def from_json(graph, data, skeleton=None, ctx=None, host=False):
        walk = HipGraphWalk(graph, data.get("start_pose"), data.get("use_time_parameters", False), skeleton, ctx, host)
        walk.steps = [HipGraphWalkStep.from_json(graph, s) for s in data["steps"]]
        return walk

    def close(self):
        if self._rows is not None:
            self._rows.free()
        self._rows, self._n_frames, self._cache = None, 0, None
