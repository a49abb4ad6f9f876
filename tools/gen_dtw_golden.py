"""Writes tests/golden/dtw.npz: what the reference's exact dynamic time warping (construction/dtw.py: get_distgrid, find_path,
run_dtw, get_warping_function, warp_motion) and MotionModelConstructor.get_average_time_line do on small synthetic inputs.

    python tools/gen_dtw_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/dtw.npz]

construction/dtw.py is imported unmodified.  `anim_utils`, `anim_utils.animation_data`, `anim_utils.animation_data.
motion_distance` and `fastdtw` are stubs, and ONE shim is set in this process: scipy.zeros_like = numpy.zeros_like (dtw.py:44
calls sp.zeros_like, which current scipy no longer has).  Prints are discarded.  get_average_time_line is compiled from its
own lines of construction/motion_model_constructor.py (the module around it imports anim_utils throughout).

The cell distance is the one piece with no source under the reference (anim_utils' _transform_invariant_point_cloud_distance).
The stub that run_dtw picks up as its default distance calls the project's restatement, imported from oracle.mg_oracle:
align_point_clouds_2d, transform_point_cloud, then the mean point distance as in pose_constraint_error (PARITY UNPINNED).  Every
value it returns is recorded in call order: that is S.  For the grid-only cases the stub returns the entries of a given grid.

Contents:
  p<s>_*   point-cloud sets: ref (Fr, J, 3), weights (J), n motions m<k>: cloud, S, D, path, warp, spread (the largest change
           of S over 3 reruns of the restatement with the joints permuted), gap (the smallest gap, relative to D[-1,-1],
           between the chosen predecessor and the runner-up over the path's back-steps), redraws.  Set 0: Fr < F, Fr > F,
           Fr = F, a motion of one frame, the reference motion itself; set 1: non-uniform weights.
  g<i>_*   grid-only cases: S, D, path, warp -- integer grids full of exact ties, a grid whose optimum runs along the first
           row and down the last column, a 1 x F and an F x 1 grid.
  e_*      end to end: a skeleton (names, parents, offsets, animated joints), quaternion motions of different lengths, the
           reference motion's key by get_average_time_line, per motion S-free results: path, warp and warp_motion's frames.
A motion drawn from point clouds is kept only if gap >= 1e-6 (the device's S differs from this host's in the last bits; only
gaps on the path decide the path); otherwise it is drawn again with the next seed, and the redraws are counted.  More than one
draw in four redrawn fails the tool.  The archive is written with fixed timestamps: running the tool again gives the
identical file.
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import mg_oracle  # noqa: E402

GAP = 1e-6
STATE = {"weights": None, "grid": None, "record": []}


def cell_distance(a, b):
    if STATE["grid"] is not None:
        return STATE["grid"][a, b]
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = np.ones(len(a)) if STATE["weights"] is None else STATE["weights"]
    theta, ox, oz = mg_oracle.align_point_clouds_2d(a, b, w)
    fitted = mg_oracle.transform_point_cloud(b, theta, ox, oz)
    d = float(np.linalg.norm(a - fitted, axis=1).sum() / len(b))
    STATE["record"].append(d)
    return d


def load_reference(reference):
    import scipy
    scipy.zeros_like = np.zeros_like
    for name in ("anim_utils", "anim_utils.animation_data", "anim_utils.animation_data.motion_distance", "fastdtw"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["anim_utils.animation_data.motion_distance"]._transform_invariant_point_cloud_distance = cell_distance
    sys.modules["fastdtw"].fastdtw = None
    base = os.path.join(reference, "morphablegraphs", "construction")
    spec = importlib.util.spec_from_file_location("mgref_dtw", os.path.join(base, "dtw.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tree = ast.parse(open(os.path.join(base, "motion_model_constructor.py")).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "get_average_time_line")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "motion_model_constructor.py", "exec"), ns)
    return mod, ns["get_average_time_line"]


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def reference_dtw(mod, x, y, weights=None, grid=None):
    """run_dtw as it stands; returns S (as the distance was called), D, path, warping function."""
    STATE.update({"weights": weights, "grid": grid, "record": []})
    with quiet():
        path, D = mod.run_dtw(x, y)
        warp = mod.get_warping_function(path)
    S = np.array(grid, dtype=np.float64) if grid is not None else np.array(STATE["record"]).reshape(len(x), len(y))
    return S, np.asarray(D, dtype=np.float64), np.asarray(path, dtype=np.int32).reshape(-1, 2), np.asarray(warp, dtype=np.int32)


def path_gap(D, path):
    """The smallest gap between the chosen predecessor and the runner-up over the path's back-steps, relative to D[-1,-1]
    (inf when the path never had a choice)."""
    gap = np.inf
    for i, j in path:
        if i > 0 and j > 0:
            c = np.sort([D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]])
            gap = min(gap, (c[1] - c[0]) / abs(D[-1, -1]) if D[-1, -1] != 0 else np.inf)
    return float(gap)


def spread_of_S(a, b, weights, S, rng):
    worst = 0.0
    for _ in range(3):
        perm = rng.permutation(a.shape[1])
        STATE.update({"weights": None if weights is None else weights[perm], "grid": None, "record": []})
        again = np.array([[cell_distance(x[perm], y[perm]) for y in b] for x in a])
        worst = max(worst, float(np.max(np.abs(again - S))))
    return worst


# ---- synthetic walking-like clouds --------------------------------------------------------------------------------------------
def time_warp(rng, n_frames):
    if n_frames == 1:
        return np.array([rng.uniform(0.2, 0.8)])
    steps = np.exp(0.5 * np.cumsum(rng.standard_normal(n_frames - 1)) * 0.25 + 0.15 * rng.standard_normal(n_frames - 1))
    t = np.concatenate([[0.0], np.cumsum(steps)])
    return t / t[-1]


def gait(n_joints, seed):
    rng = np.random.default_rng(seed)
    return {"rest": rng.uniform(-0.5, 0.5, (n_joints, 3)) * np.array([0.6, 1.8, 0.4]) + np.array([0.0, 0.9, 0.0]),
            "amp": rng.uniform(0.05, 0.35, (n_joints, 3)), "phase": rng.uniform(0, 2 * np.pi, (n_joints, 3))}


def walking_clouds(rng, g, t, noise=0.004):
    """A gait cycle and a half along +z at the (warped) times t in [0, 1], turned and moved as a whole."""
    ph = 2 * np.pi * 1.5 * t[:, None, None] + g["phase"][None]
    pos = g["rest"][None] + g["amp"][None] * np.sin(ph)
    pos[:, :, 2] += 2.4 * t[:, None]
    pos[:, :, 0] += 0.3 * np.sin(np.pi * t)[:, None]
    ang, shift = rng.uniform(-np.pi, np.pi), rng.uniform(-2.0, 2.0, 2)
    c, s = np.cos(ang), np.sin(ang)
    out = pos.copy()
    out[:, :, 0] = pos[:, :, 0] * c + pos[:, :, 2] * s + shift[0]
    out[:, :, 2] = -pos[:, :, 0] * s + pos[:, :, 2] * c + shift[1]
    return out + noise * rng.standard_normal(out.shape)


POINT_SETS = [
    {"name": "walk_j12_fr48", "n_joints": 12, "n_ref": 48, "lengths": [57, 41, 48, 1, "self"], "weights": False},
    {"name": "walk_j9_fr45_weights", "n_joints": 9, "n_ref": 45, "lengths": [52, 38], "weights": True},
]


def tie_grid(rng, shape, high):
    return rng.integers(0, high, shape).astype(np.float64)


def grid_cases():
    rng = np.random.default_rng(4100)
    corner = 5.0 + tie_grid(rng, (12, 15), 4)
    corner[0, :] = 0.25
    corner[:, -1] = 0.25
    return [("ties_20x23", tie_grid(rng, (20, 23), 3)), ("all_ones_17x17", np.ones((17, 17))), ("ties_31x9", tie_grid(rng, (31, 9), 2)),
            ("first_row_last_column_12x15", corner), ("one_row_1x9", tie_grid(rng, (1, 9), 3) + 0.5), ("one_column_11x1", tie_grid(rng, (11, 1), 3) + 0.5)]


# ---- the end-to-end case -----------------------------------------------------------------------------------------------------
SKELETON = [("Hips", None, (0.0, 0.0, 0.0)), ("Spine", "Hips", (0.0, 0.25, 0.02)), ("Head", "Spine", (0.0, 0.45, 0.03)),
            ("LeftHand", "Spine", (0.35, 0.2, 0.1)), ("RightHand", "Spine", (-0.35, 0.2, 0.1)), ("LeftFoot", "Hips", (0.12, -0.85, 0.05)),
            ("RightFoot", "Hips", (-0.12, -0.85, 0.05))]
ANIMATED = ["Hips", "Spine"]


def quaternion_motion(rng, canon, t):
    """Frames (F, 11) at the warped times t of a canonical motion: root path and two joints' rotations, smooth in time."""
    n = len(t)
    frames = np.zeros((n, 3 + 4 * len(ANIMATED)))
    frames[:, 0] = 0.4 * np.sin(np.pi * t) + canon["root"][0]
    frames[:, 1] = 0.9 + 0.04 * np.sin(4 * np.pi * t)
    frames[:, 2] = 2.0 * t + canon["root"][1]
    for j in range(len(ANIMATED)):
        axis_angle = canon["amp"][j][None, :] * np.sin(2 * np.pi * canon["freq"][j][None, :] * t[:, None] + canon["phase"][j][None, :])
        ang = np.linalg.norm(axis_angle, axis=1)
        q = np.concatenate([np.cos(ang / 2)[:, None], axis_angle / np.maximum(ang, 1e-12)[:, None] * np.sin(ang / 2)[:, None]], axis=1)
        frames[:, 3 + 4 * j:7 + 4 * j] = q
    frames[:, 3:] += 0.002 * rng.standard_normal((n, 4 * len(ANIMATED)))
    for j in range(len(ANIMATED)):
        frames[:, 3 + 4 * j:7 + 4 * j] /= np.linalg.norm(frames[:, 3 + 4 * j:7 + 4 * j], axis=1, keepdims=True)
    return frames


def clouds_of(frames):
    return np.array([[mg_oracle.joint_global_position(f, SKELETON, ANIMATED, j[0]) for j in SKELETON] for f in frames])


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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dtw.npz"))
    args = ap.parse_args()
    mod, average_time_line = load_reference(args.reference)
    out = {}
    draws = redraws_total = 0
    for s, ps in enumerate(POINT_SETS):
        p = "p%d_" % s
        g = gait(ps["n_joints"], 5000 + s)
        rng = np.random.default_rng(5100 + s)
        ref = walking_clouds(rng, g, np.linspace(0.0, 1.0, ps["n_ref"]))
        weights = rng.uniform(0.2, 2.0, ps["n_joints"]) if ps["weights"] else None
        out.update({p + "name": np.array(ps["name"]), p + "ref": ref, p + "weights": np.ones(ps["n_joints"]) if weights is None else weights,
                    p + "n": np.int64(len(ps["lengths"]))})
        for k, length in enumerate(ps["lengths"]):
            redraws = 0
            for seed in range(10):
                draws += 1
                mrng = np.random.default_rng(5200 + 100 * s + 10 * k + seed)
                cloud = ref.copy() if length == "self" else walking_clouds(mrng, g, time_warp(mrng, length))
                S, D, path, warp = reference_dtw(mod, ref, cloud, weights)
                gap = path_gap(D, path)
                if gap >= GAP:
                    break
                print("%s motion %d: seed %d: gap %.3g; next seed" % (ps["name"], k, seed, gap))
                redraws += 1
                redraws_total += 1
            else:
                raise RuntimeError("set %d motion %d: no seed passes the gap condition" % (s, k))
            spread = spread_of_S(ref, cloud, weights, S, np.random.default_rng(5900 + 10 * s + k))
            q = p + "m%d_" % k
            out.update({q + "cloud": cloud, q + "S": S, q + "D": D, q + "path": path, q + "warp": warp, q + "spread": np.float64(spread),
                        q + "gap": np.float64(gap), q + "redraws": np.int64(redraws), q + "seed": np.int64(seed)})
            print("%-22s motion %d: %2d x %2d  path %3d  total %.6g  gap %.3g  spread %.3g  redraws %d" % (
                ps["name"], k, S.shape[0], S.shape[1], len(path), D[-1, -1], gap, spread, redraws))
    cases = grid_cases()
    out["n_grids"] = np.int64(len(cases))
    for i, (name, S) in enumerate(cases):
        S2, D, path, warp = reference_dtw(mod, list(range(S.shape[0])), list(range(S.shape[1])), grid=S)
        q = "g%d_" % i
        out.update({q + "name": np.array(name), q + "S": S2, q + "D": D, q + "path": path, q + "warp": warp})
        print("%-28s %2d x %2d  path %3d  total %.6g" % (name, S.shape[0], S.shape[1], len(path), D[-1, -1]))
    # end to end
    lengths = [34, 41, 30, 38, 44, 36]
    for seed in range(10):
        draws += 1
        rng = np.random.default_rng(6000 + seed)
        canon = {"root": rng.uniform(-0.5, 0.5, 2), "amp": rng.uniform(0.2, 0.7, (len(ANIMATED), 3)), "freq": rng.uniform(0.6, 1.6, (len(ANIMATED), 3)),
                 "phase": rng.uniform(0, 2 * np.pi, (len(ANIMATED), 3))}
        keys = ["walk_%02d" % i for i in range(len(lengths))]
        motions = collections.OrderedDict((k, quaternion_motion(rng, canon, time_warp(rng, n))) for k, n in zip(keys, lengths))
        mean_key = average_time_line(None, motions)
        clouds = {k: clouds_of(m) for k, m in motions.items()}
        results, worst = {}, np.inf
        for k in keys:
            S, D, path, warp = reference_dtw(mod, clouds[mean_key], clouds[k])
            with quiet():
                warped = np.array(mod.warp_motion(motions[k], warp.tolist()))
            results[k] = (path, warp, warped, D[-1, -1])
            worst = min(worst, path_gap(D, path))
        if worst >= GAP:
            break
        print("end to end: seed %d: gap %.3g; next seed" % (seed, worst))
        redraws_total += 1
    else:
        raise RuntimeError("end to end: no seed passes the gap condition")
    out.update({"e_keys": np.array(keys), "e_mean_key": np.array(mean_key), "e_gap": np.float64(worst), "e_seed": np.int64(seed),
                "e_joint_names": np.array([j[0] for j in SKELETON]), "e_joint_parents": np.array(["" if j[1] is None else j[1] for j in SKELETON]),
                "e_joint_offsets": np.array([j[2] for j in SKELETON], dtype=np.float64), "e_animated_joints": np.array(ANIMATED)})
    for i, k in enumerate(keys):
        path, warp, warped, total = results[k]
        out.update({"e_m%d_frames" % i: motions[k], "e_m%d_path" % i: path, "e_m%d_warp" % i: warp, "e_m%d_warped" % i: warped,
                    "e_m%d_total" % i: np.float64(total)})
    print("end to end: reference %s (%d frames), gap %.3g" % (mean_key, len(motions[mean_key]), worst))
    if 4 * redraws_total > draws:
        raise RuntimeError("%d of %d draws redrawn: more than a quarter" % (redraws_total, draws))
    out.update({"n_point_sets": np.int64(len(POINT_SETS)), "draws": np.int64(draws), "redraws": np.int64(redraws_total)})
    _write_npz(args.out, out)
    print("draws %d, redraws %d" % (draws, redraws_total))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
