"""Spatial alignment of motions on the device, and the per-frame preparation in front of the fPCA: the reference's
MotionModelConstructor._align_frames_spatially (construction/motion_model_constructor.py:244-263) and the first two statements
of run_spatial_dimension_reduction (:359-360: normalize_root_translation, align_quaternion_frames).

align_motions_spatially turns every motion about y so that its frame `frame_idx` faces `ref_orientation` (the reference: frame
0 and [0, -1]) and moves it so that this frame's root position is the origin, height included (mg_align_motions_spatially, one
upload, one launch for all motions).  The contract of a motion is the header comment of csrc/mg_spatial_align.hip;
align_motions_spatially_host restates it in NumPy, statement for statement, and is the yardstick of the CPU tests.

Where the reference goes through anim_utils (pose_orientation_quat, get_rotation_angle: a heading, an angle in degrees modulo
360) and transformations (quaternion_from_euler, quaternion_matrix, quaternion_from_matrix), the contract goes from the two
unit vectors to (cos, sin) and from there to the rotation of the root position and to the quaternion about y.  The heading is
the project's restatement (Skeleton.heading, mg_candidate_alignment): PARITY UNPINNED, as the forward kinematics and the
point-cloud distance.  The sign of a root quaternion is quaternion_from_matrix's: w >= 0.

prepare_aligned_frames is mg_prepare_aligned_frames for equally long motions; its host form is fpca.normalize_root_translation
and fpca.align_quaternion_frames composed.  The device functions have no CPU fallback.
"""
import collections

import numpy as np

from . import _capi
from .fpca import align_quaternion_frames, normalize_root_translation

MAX_JOINTS = _capi.MG_SPATIAL_ALIGN_MAX_JOINTS
REF_ORIENTATION = (0.0, -1.0)      # MotionModelConstructor.ref_orientation: look into -z


# ---- host restatements ---------------------------------------------------------------------------------------------------
def _unit_reference(ref_orientation):
    r0, r1 = (float(v) for v in ref_orientation)
    rn = np.sqrt(r0 * r0 + r1 * r1)
    if not (np.isfinite(rn) and rn > 0.0):
        raise ValueError("ref_orientation = (%g, %g)" % (r0, r1))
    return r0 / rn, r1 / rn


def motion_transform_host(frame, ref_orientation=REF_ORIENTATION):
    """(cos, sin, dx, dy, dz) of the motion whose frame `frame_idx` is `frame`, or None if the root turns z onto the y axis
    (sa_motion_transform of csrc/mg_spatial_align.hip)."""
    rx, rz = _unit_reference(ref_orientation)
    f = np.asarray(frame, dtype=np.float64)
    aw, ax, ay, az = f[3], f[4], f[5], f[6]
    with np.errstate(all="ignore"):
        n = 1.0 / np.sqrt(((aw * aw + ax * ax) + ay * ay) + az * az)
        aw, ax, ay, az = aw * n, ax * n, ay * n, az * n
        vx, vy, vz = 0.0, 0.0, 1.0
        cx, cy, cz = ay * vz - az * vy, az * vx - ax * vz, ax * vy - ay * vx
        dx, dz = ay * cz - az * cy, ax * cy - ay * cx
        bx, bz = vx + 2.0 * (aw * cx + dx), vz + 2.0 * (aw * cz + dz)
        l = bx * bx + bz * bz
        if not (np.isfinite(l) and l > 0.0):
            return None
        m = 1.0 / np.sqrt(l)
    hx, hz = bx * m, bz * m
    c = hx * rx + hz * rz
    s = hx * rz - hz * rx
    return np.array([c, s, c * f[0] - s * f[2], f[1], s * f[0] + c * f[2]])


def _half_angle(c, s):
    """(ch, sh): the rotation about y as a quaternion is (ch, 0, -sh, 0)."""
    if c >= 0.0:
        ch = np.sqrt((1.0 + c) / 2.0)
        sh = s / (2.0 * ch)
    else:
        sh = np.copysign(np.sqrt((1.0 - c) / 2.0), s)
        ch = s / (2.0 * sh)
    return ch, sh


def align_motion_host(frames, transform):
    """One motion under its transform (cos, sin, dx, dy, dz): the frames loop of sa_align_kernel, all frames at once."""
    f = np.array(frames, dtype=np.float64)
    c, s, dx, dy, dz = (np.float64(v) for v in transform)
    ch, sh = _half_angle(c, s)
    out = f.copy()
    out[:, 0] = (c * f[:, 0] - s * f[:, 2]) - dx
    out[:, 1] = f[:, 1] - dy
    out[:, 2] = (s * f[:, 0] + c * f[:, 2]) - dz
    w, x, y, z = f[:, 3], f[:, 4], f[:, 5], f[:, 6]
    n = 1.0 / np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w * n, x * n, y * n, z * n
    p = np.stack([ch * w + sh * y, ch * x - sh * z, ch * y - sh * w, ch * z + sh * x], axis=1)
    p[p[:, 0] < 0.0] *= -1.0
    out[:, 3:7] = p
    return out


def _checked(motions):
    out = collections.OrderedDict()
    n_dim = None
    for key, m in motions.items():
        a = np.asarray(m, dtype=np.float64)
        n_dim = a.shape[1] if n_dim is None and a.ndim == 2 else n_dim
        if a.ndim != 2 or a.shape[1] != n_dim or len(a) < 1:
            raise ValueError("the motions of one call are (F_k >= 1, D) arrays with one D")
        out[key] = a
    if n_dim is not None and (n_dim < 7 or (n_dim - 3) % 4 or (n_dim - 3) // 4 > MAX_JOINTS):
        raise ValueError("%d channels (3 + 4 J with 1 <= J <= %d)" % (n_dim, MAX_JOINTS))
    return out, n_dim


def _check_frame_idx(motions, frame_idx):
    for key, m in motions.items():
        if not 0 <= int(frame_idx) < len(m):
            raise ValueError("frame_idx = %d, motion %r has %d frames" % (frame_idx, key, len(m)))


def align_motions_spatially_host(motions, frame_idx=0, ref_orientation=REF_ORIENTATION, return_transforms=False):
    """mg_align_motions_spatially in NumPy: {key: (F_k, D)} -> OrderedDict {key: (F_k, D)}; return_transforms: also the (N, 5)
    array of (cos, sin, dx, dy, dz).  ValueError for what the device refuses."""
    motions, _ = _checked(motions)
    _check_frame_idx(motions, frame_idx)
    out, transforms = collections.OrderedDict(), []
    for key, m in motions.items():
        if not np.all(np.isfinite(m)):
            raise ValueError("the frames hold non-finite values")
        n2 = ((m[:, 3] * m[:, 3] + m[:, 4] * m[:, 4]) + m[:, 5] * m[:, 5]) + m[:, 6] * m[:, 6]
        if not np.all(np.isfinite(n2) & (n2 > 0.0)):
            raise ValueError("a root quaternion is zero (or its norm overflows)")
        t = motion_transform_host(m[int(frame_idx)], ref_orientation)
        if t is None:
            raise ValueError("motion %r: the root of frame %d turns z onto the y axis (no heading)" % (key, frame_idx))
        transforms.append(t)
        out[key] = align_motion_host(m, t)
    return (out, np.array(transforms).reshape(-1, 5)) if return_transforms else out


def prepare_aligned_frames_host(motions, n_joints=None):
    """(fpca.align_quaternion_frames(J, scaled), scale_vec) with scaled, scale_vec = fpca.normalize_root_translation(motions);
    n_joints None: all (D - 3) / 4."""
    motions = collections.OrderedDict((k, np.asarray(v, dtype=np.float64)) for k, v in motions.items())
    if n_joints is None:
        n_joints = (next(iter(motions.values())).shape[1] - 3) // 4
    scaled, scale_vec = normalize_root_translation(motions)
    return align_quaternion_frames(int(n_joints), scaled), np.asarray(scale_vec, dtype=np.float64)


# ---- the device ------------------------------------------------------------------------------------------------------------
def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def upload_and_align(ctx, bufs, motions, frame_idx=0, ref_orientation=REF_ORIENTATION, transforms=False):
    """The captures go up once; returns (aligned device table of the scope `bufs`, offsets, D, transforms or None).  The input
    table is freed on the way out."""
    motions, n_dim = _checked(motions)
    _check_frame_idx(motions, frame_idx)
    off = _offsets([len(m) for m in motions.values()])
    out_dev = bufs.malloc(8 * int(off[-1]) * n_dim)
    with ctx.buffers() as inputs:
        f_dev = inputs.upload(np.concatenate(list(motions.values())))
        t_dev = inputs.malloc(8 * 5 * len(motions)) if transforms else None
        _capi.align_motions_spatially(ctx, f_dev, off, n_dim, frame_idx, ref_orientation, out_dev, t_dev)
        t = ctx.download(t_dev, (len(motions), 5), np.float64) if transforms else None
    return out_dev, off, n_dim, t


def align_motions_spatially(motions, frame_idx=0, ref_orientation=REF_ORIENTATION, ctx=None, return_transforms=False):
    """MotionModelConstructor._align_frames_spatially on the device: `motions` {key: (F_k, D) quaternion frames} -> OrderedDict
    {key: (F_k, D)} in the input's key order; return_transforms: also the (N, 5) array of (cos, sin, dx, dy, dz)."""
    ctx = _capi.default_context(ctx)
    keys = list(motions.keys())
    if not keys:
        return (collections.OrderedDict(), np.zeros((0, 5))) if return_transforms else collections.OrderedDict()
    with ctx.buffers() as bufs:
        out_dev, off, n_dim, t = upload_and_align(ctx, bufs, motions, frame_idx, ref_orientation, return_transforms)
        table = ctx.download(out_dev, (int(off[-1]), n_dim), np.float64)
    out = collections.OrderedDict((k, table[int(off[i]):int(off[i + 1])].copy()) for i, k in enumerate(keys))
    return (out, t) if return_transforms else out


def prepare_aligned_frames(motions, n_joints=None, ctx=None):
    """mg_prepare_aligned_frames: equally long `motions` {key: (F, D)} -> (OrderedDict {key: (F, D)}, scale_vec (3,))."""
    ctx = _capi.default_context(ctx)
    keys = list(motions.keys())
    table = np.ascontiguousarray([np.asarray(motions[k], dtype=np.float64) for k in keys])
    if table.ndim != 3:
        raise ValueError("prepare_aligned_frames takes motions of one length")
    n, n_frames, n_dim = table.shape
    if n_joints is None:
        n_joints = (n_dim - 3) // 4
    with ctx.buffers() as bufs:
        f_dev, o_dev = bufs.upload(table), bufs.malloc(table.nbytes)
        scale_vec = _capi.prepare_aligned_frames(ctx, f_dev, n, n_frames, n_dim, n_joints, o_dev)
        out = ctx.download(o_dev, table.shape, np.float64)
    return collections.OrderedDict((k, out[i]) for i, k in enumerate(keys)), scale_vec
