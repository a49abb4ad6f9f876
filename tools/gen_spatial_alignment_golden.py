"""Writes tests/golden/spatial_alignment.npz: what the reference's MotionModelConstructor._align_frames_spatially
(construction/motion_model_constructor.py:244-263) and construction/utils.py's normalize_root_translation and
align_quaternion_frames do on small synthetic motions.

    python tools/gen_spatial_alignment_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/spatial_alignment.npz]

_align_frames_spatially is compiled from its own lines of motion_model_constructor.py (the module around it imports anim_utils
throughout); construction/utils.py is imported unmodified (rotate_frames, normalize_root_translation,
align_quaternion_frames).  Prints are discarded.  What is absent on this side is stubbed, each stub a restatement written
here -- PARITY UNPINNED, all five:
  pose_orientation_quat(frame)      anim_utils.animation_data.utils: the x and z of quaternion_matrix(frame[3:7]) applied to
                                    (0, 0, 1), divided by their length;
  get_rotation_angle(p1, p2)        anim_utils.animation_data.utils: atan2(p2[1], p2[0]) - atan2(p1[1], p1[0]) in degrees,
                                    brought into [-180, 180];
  quaternion_from_euler(ai, aj, ak) transformations, axes 'sxyz': the product of the three half-angle rotations;
  quaternion_matrix(q)              transformations: the homogeneous matrix of q scaled by sqrt(2 / (q . q));
  quaternion_from_matrix(M)         transformations, isprecise=False: the eigenvector of the largest eigenvalue of the
                                    symmetric 4 x 4 matrix K(M) (numpy.linalg.eigh), negated when its w < 0.

Contents:
  a<s>_*   alignment sets: name, ref_orientation (2), n motions m<k>: in (F, D), out (F, D), heading_len (the x-z length of the
           heading of frame 0 before normalising), min_w (the least |w| of the output's root quaternions).  The sets cover the
           reference's own [0, -1], where every aligned root quaternion lies near the w = 0 sign boundary, two other
           orientations, J = 1, 2 and 19, motions of 1 and 2 frames and root quaternions that are not normalised.
  q<s>_*   preparation sets: n_joints, in (N, F, D), out (N, F, D), scale (3), min_dot (the least |dot| of a joint quaternion with
           the first frame's).  One set has a root channel that is 0 everywhere (nothing is scaled, the scale is ones), one has
           its largest magnitude with a negative sign in the last frame of the last motion.
A draw is kept only if heading_len >= 1e-3, min_w >= 1e-3 (the sign of a root quaternion is decided by its w) and min_dot >= 1e-6;
otherwise it is drawn again with the next seed, and the redraws are counted.  More than one draw in four redrawn fails the
tool.  The archive is written with fixed timestamps: running the tool again gives the identical file.
"""
import argparse
import ast
import collections
import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile
from copy import copy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADING_LEN, MIN_W, MIN_DOT = 1e-3, 1e-3, 1e-6


# ---- the stubs -----------------------------------------------------------------------------------------------------------------
def quaternion_matrix(quaternion):
    q = np.array(quaternion, dtype=np.float64, copy=True)
    n = np.dot(q, q)
    if n < np.finfo(float).eps * 4.0:
        return np.identity(4)
    q *= np.sqrt(2.0 / n)
    q = np.outer(q, q)
    return np.array([[1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0], 0.0],
                     [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0], 0.0],
                     [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2], 0.0],
                     [0.0, 0.0, 0.0, 1.0]])


def quaternion_from_matrix(matrix):
    M = np.asarray(matrix, dtype=np.float64)[:4, :4]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = M[0, 0], M[0, 1], M[0, 2], M[1, 0], M[1, 1], M[1, 2], M[2, 0], M[2, 1], M[2, 2]
    K = np.array([[m00 - m11 - m22, 0.0, 0.0, 0.0],
                  [m01 + m10, m11 - m00 - m22, 0.0, 0.0],
                  [m02 + m20, m12 + m21, m22 - m00 - m11, 0.0],
                  [m21 - m12, m02 - m20, m10 - m01, m00 + m11 + m22]])
    K /= 3.0
    w, V = np.linalg.eigh(K)
    q = V[[3, 0, 1, 2], np.argmax(w)]
    if q[0] < 0.0:
        np.negative(q, q)
    return q


def quaternion_from_euler(ai, aj, ak):
    ai, aj, ak = ai / 2.0, aj / 2.0, ak / 2.0
    ci, si, cj, sj, ck, sk = np.cos(ai), np.sin(ai), np.cos(aj), np.sin(aj), np.cos(ak), np.sin(ak)
    cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
    return np.array([cj * cc + sj * ss, cj * sc - sj * cs, cj * ss + sj * cc, cj * cs - sj * sc])


def pose_orientation_quat(quaternion_frame):
    rotated = np.dot(quaternion_matrix(copy(quaternion_frame[3:7])), np.array([0.0, 0.0, 1.0, 1.0]))
    dir_vec = np.array([rotated[0], rotated[2]])
    STATE["heading_len"] = float(np.linalg.norm(dir_vec))
    return dir_vec / np.linalg.norm(dir_vec)


def get_rotation_angle(point1, point2):
    theta1 = np.rad2deg(np.arctan2(point1[1], point1[0]))
    theta2 = np.rad2deg(np.arctan2(point2[1], point2[0]))
    delta = theta2 - theta1
    if delta < -180.0:
        delta += 360.0
    elif delta > 180.0:
        delta -= 360.0
    return delta


STATE = {"heading_len": None}


def load_reference(reference):
    for name in ("transformations", "anim_utils", "anim_utils.animation_data", "anim_utils.animation_data.motion_distance"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["transformations"].quaternion_matrix = quaternion_matrix
    sys.modules["transformations"].quaternion_from_matrix = quaternion_from_matrix
    sys.modules["anim_utils.animation_data.motion_distance"].convert_quat_frame_to_point_cloud = None
    base = os.path.join(reference, "morphablegraphs", "construction")
    spec = importlib.util.spec_from_file_location("mgref_construction_utils", os.path.join(base, "utils.py"))
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)
    tree = ast.parse(open(os.path.join(base, "motion_model_constructor.py")).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "_align_frames_spatially")
    ns = {"np": np, "copy": copy, "collections": collections, "pose_orientation_quat": pose_orientation_quat, "get_rotation_angle": get_rotation_angle,
          "quaternion_from_euler": quaternion_from_euler, "rotate_frames": utils.rotate_frames}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "motion_model_constructor.py", "exec"), ns)
    return utils, ns["_align_frames_spatially"]


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


# ---- synthetic motions ---------------------------------------------------------------------------------------------------------
def quat_about(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2.0)], np.sin(angle / 2.0) * axis])


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def capture(rng, n_frames, n_joints, towards_boundary):
    """A walk with a slowly turning, tilted root.  towards_boundary: the set is aligned to [0, -1], half a turn away from the
    direction the heading is measured against, so every aligned root quaternion has a small w; the turn then goes the way the
    tilt leans, which keeps w on one side of 0."""
    t = np.linspace(0.0, 1.0, n_frames) if n_frames > 1 else np.zeros(1)
    tilt_axis = rng.standard_normal(3)
    tilt_axis /= np.linalg.norm(tilt_axis)
    if abs(tilt_axis[1]) < 0.3:
        tilt_axis[1] = np.copysign(0.3, tilt_axis[1])
    tilt0, yaw0, drift = rng.uniform(0.25, 1.0), rng.uniform(-np.pi, np.pi), rng.uniform(0.1, 0.8)
    if towards_boundary:
        drift = np.copysign(drift, tilt_axis[1])
    else:
        drift *= rng.choice([-1.0, 1.0])
    frames = np.zeros((n_frames, 3 + 4 * n_joints))
    frames[:, 0] = rng.uniform(-3, 3) + 0.5 * np.sin(2.0 * t) + 0.02 * rng.standard_normal(n_frames)
    frames[:, 1] = 0.9 + 0.05 * np.sin(6.0 * t + rng.uniform(0, 6))
    frames[:, 2] = rng.uniform(-3, 3) + 1.8 * t + 0.02 * rng.standard_normal(n_frames)
    scale = rng.choice([1.0, 3.0, rng.uniform(0.5, 2.0)])
    for i in range(n_frames):
        q = quat_mul(quat_about((0, 1, 0), yaw0 + drift * t[i]), quat_about(tilt_axis, tilt0 + 0.1 * np.sin(3.0 * t[i])))
        frames[i, 3:7] = scale * q
    other = rng.standard_normal((n_frames, n_joints - 1, 4))
    other /= np.linalg.norm(other, axis=2, keepdims=True)
    frames[:, 7:] = other.reshape(n_frames, -1)
    return frames


ALIGN_SETS = [
    {"name": "reference_orientation_j2", "ref": [0, -1], "n_joints": 2, "lengths": [11, 1, 2, 7]},
    {"name": "reference_orientation_j19", "ref": [0, -1], "n_joints": 19, "lengths": [33, 5]},
    {"name": "plus_z_j1", "ref": [0, 1], "n_joints": 1, "lengths": [9, 4, 1]},
    {"name": "oblique_j2", "ref": [1.0, 0.5], "n_joints": 2, "lengths": [6, 13]},
]

PREPARE_SETS = [
    {"name": "one_frame", "shape": (1, 1, 7), "zero": None, "negative_max": False},
    {"name": "j19", "shape": (3, 17, 79), "zero": None, "negative_max": True},
    {"name": "flat_ground", "shape": (2, 9, 11), "zero": 1, "negative_max": False},
]


class _Skeleton(object):
    def __init__(self, n_joints):
        self.animated_joints = ["joint_%d" % j for j in range(n_joints)]


def prepare_input(rng, shape, zero, negative_max):
    n, f, d = shape
    x = np.zeros(shape)
    x[:, :, :3] = rng.uniform(-2.0, 2.0, (n, f, 3))
    q = rng.standard_normal((n, f, (d - 3) // 4, 4))
    q /= np.linalg.norm(q, axis=3, keepdims=True)
    x[:, :, 3:] = q.reshape(n, f, -1)
    if zero is not None:
        x[:, :, zero] = 0.0
    if negative_max:
        x[-1, -1, 0] = -7.5
    return x


def _write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "spatial_alignment.npz"))
    args = ap.parse_args()
    utils, align_frames_spatially = load_reference(args.reference)
    out = {"a_n_sets": np.int64(len(ALIGN_SETS)), "q_n_sets": np.int64(len(PREPARE_SETS))}
    draws = redraws_total = 0
    for s, st in enumerate(ALIGN_SETS):
        p = "a%d_" % s
        constructor = types.SimpleNamespace(ref_orientation=list(st["ref"]))
        out.update({p + "name": np.array(st["name"]), p + "ref_orientation": np.array(st["ref"], dtype=np.float64), p + "n": np.int64(len(st["lengths"]))})
        for k, length in enumerate(st["lengths"]):
            for seed in range(10):
                draws += 1
                rng = np.random.default_rng(7000 + 100 * s + 10 * k + seed)
                frames = capture(rng, length, st["n_joints"], st["ref"] == [0, -1])
                with quiet():
                    aligned = align_frames_spatially(constructor, collections.OrderedDict([("m", frames.copy())]))["m"]
                heading_len, min_w = STATE["heading_len"], float(np.min(np.abs(aligned[:, 3])))
                if heading_len >= HEADING_LEN and min_w >= MIN_W:
                    break
                print("%s motion %d: seed %d: heading %.3g, min |w| %.3g; next seed" % (st["name"], k, seed, heading_len, min_w))
                redraws_total += 1
            else:
                raise RuntimeError("set %d motion %d: no seed passes the conditions" % (s, k))
            q = p + "m%d_" % k
            out.update({q + "in": frames, q + "out": np.asarray(aligned, dtype=np.float64), q + "heading_len": np.float64(heading_len),
                        q + "min_w": np.float64(min_w), q + "seed": np.int64(seed)})
            print("%-28s motion %d: %2d x %2d  heading %.3f  min |w| %.3g" % (st["name"], k, frames.shape[0], frames.shape[1], heading_len, min_w))
    for s, st in enumerate(PREPARE_SETS):
        p = "q%d_" % s
        n_joints = (st["shape"][2] - 3) // 4
        for seed in range(10):
            draws += 1
            x = prepare_input(np.random.default_rng(7900 + 10 * s + seed), st["shape"], st["zero"], st["negative_max"])
            dots = np.einsum("nfjc,jc->nfj", x[:, :, 3:].reshape(x.shape[0], x.shape[1], n_joints, 4), x[0, 0, 3:].reshape(n_joints, 4))
            min_dot = float(np.min(np.abs(dots)))
            if min_dot >= MIN_DOT:
                break
            print("%s: seed %d: min |dot| %.3g; next seed" % (st["name"], seed, min_dot))
            redraws_total += 1
        else:
            raise RuntimeError("preparation set %d: no seed passes the condition" % s)
        motions = collections.OrderedDict(("m%d" % i, x[i].copy()) for i in range(len(x)))
        with quiet():
            scaled, scale = utils.normalize_root_translation(motions)
            smoothed = utils.align_quaternion_frames(_Skeleton(n_joints), scaled)
        result = np.array([smoothed[k] for k in motions.keys()], dtype=np.float64)
        out.update({p + "name": np.array(st["name"]), p + "n_joints": np.int64(n_joints), p + "in": x, p + "out": result,
                    p + "scale": np.asarray(scale, dtype=np.float64), p + "min_dot": np.float64(min_dot), p + "seed": np.int64(seed)})
        print("%-28s %s  scale %s  flipped %d  min |dot| %.3g" % (st["name"], x.shape, np.asarray(scale), int(np.sum(dots < 0)), min_dot))
    if 4 * redraws_total > draws:
        raise RuntimeError("%d of %d draws redrawn: more than a quarter" % (redraws_total, draws))
    out.update({"draws": np.int64(draws), "redraws": np.int64(redraws_total)})
    _write_npz(args.out, out)
    print("draws %d, redraws %d" % (draws, redraws_total))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
