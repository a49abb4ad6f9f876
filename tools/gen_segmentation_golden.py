"""Writes tests/golden/segmentation.npz: what the reference's keyframe search (construction/keyframe_detection.py: argmin,
argmin_multi, KeyframeDetector.find_instance / find_instances) and segmentation (construction/segmentation.py: Segmentation.
extract_single_segments, extract_segments) do on small synthetic captures.

    python tools/gen_segmentation_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/segmentation.npz]

keyframe_detection.py, segmentation.py and the construction/utils.py they import are loaded unmodified, as the submodules of an
empty stand-in package (segmentation.py imports its neighbours relatively).  `anim_utils`, `anim_utils.animation_data`,
`anim_utils.animation_data.motion_distance` and `transformations` are stubs.  Prints are discarded.  No scipy shim was needed:
scipy.ndimage.filters / morphology still import (the tool installs stand-in modules only if that import fails).

The distance is the one piece with no source under the reference (anim_utils' _transform_invariant_point_cloud_distance).  The
stub that KeyframeDetector picks up as its default distance calls the project's restatement, imported from oracle.mg_oracle:
align_point_clouds_2d, transform_point_cloud, then the mean point distance as in pose_constraint_error (PARITY UNPINNED).  Every
value it returns is recorded in call order: extract_single_segments calls it for every frame against the start keyframe, then
for every frame against the end keyframe, and those two runs are the recorded distances.  For the distance-only cases the stub
returns the entries of given arrays.  convert_quat_frame_to_point_cloud is the identity for these two kinds of cases and the
oracle's forward kinematics for the end-to-end case.

The reference stacks all motions' clouds with np.array, which raises for motions of different lengths under current NumPy, so
it is called once per capture, with a list of that one capture; its flat list of slices is then in motion order and start
order.  A capture is handed over as a sequence that answers m[start:end] with (start, end), so that empty slices keep their
indices too.

Contents:
  p<s>_*   point-cloud sets: weights (J), start, end (the keyframes, (J, 3)), n captures c<k>: cloud (F, J, 3), S, E (the
           distances of every frame to the start and the end keyframe), spread (the largest change of S and E over 3 reruns of
           the restatement with the joints permuted), single (2), per setting t<j> (threshold, min_segment_size): multi
           (n, 2), margin, redraws, seed.  Set 0: uniform weights, captures of fewer and more than 1024 frames, one of 3000;
           set 1: non-uniform weights.  The clouds are rounded to multiples of 2^-16 (they compress; they are float64 inputs
           like any other).
  g<i>_*   distance-only cases: S, E, single, per setting t<j>: threshold, min, multi -- integer arrays full of exact ties,
           instances on adjacent frames so that every window is dropped, a motion without a kept segment, a one-frame motion,
           threshold 0, min_segment_size 0.
  e_*      end to end: the skeleton of tests/golden/dtw.npz (names, parents, offsets, animated joints), quaternion captures,
           the two keyframe poses, threshold, min_segment_size, the (motion, start, end) triples of extract_segments and of
           extract_single_segments, the concatenated slices, margin.
A capture drawn from point clouds (or the end-to-end set) is kept only if every decision the reference made on it has a margin
of at least 1e-6, relative to the largest distance: each `v <= m + threshold` test, and each arg-min against its runner-up (the
device's distances differ from this host's in the last bits); otherwise it is drawn again with the next seed, and the redraws
are counted.  More than one draw in four redrawn fails the tool.  The archive is written with fixed timestamps: running the
tool again gives the identical file.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import mg_oracle  # noqa: E402
from gen_dtw_golden import ANIMATED, SKELETON, _write_npz  # noqa: E402

MARGIN = 1e-6
STATE = {"weights": None, "dist": None, "record": [], "fk": False}
START_TAG, END_TAG = [0], [1]      # the "keyframes" of the distance-only cases


def cell_distance(a, b):
    if STATE["dist"] is not None:
        return STATE["dist"][b[0]][int(a[0])]
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = np.ones(len(a)) if STATE["weights"] is None else STATE["weights"]
    theta, ox, oz = mg_oracle.align_point_clouds_2d(a, b, w)
    fitted = mg_oracle.transform_point_cloud(b, theta, ox, oz)
    d = float(np.linalg.norm(a - fitted, axis=1).sum() / len(b))
    STATE["record"].append(d)
    return d


def to_point_cloud(skeleton, frame):
    if not STATE["fk"]:
        return frame
    return np.array([mg_oracle.joint_global_position(frame, SKELETON, ANIMATED, j[0]) for j in SKELETON])


def load_reference(reference):
    try:
        import scipy.ndimage.filters  # noqa: F401
        import scipy.ndimage.morphology  # noqa: F401
    except ImportError:
        import scipy.ndimage
        for name in ("filters", "morphology"):
            sys.modules["scipy.ndimage." + name] = scipy.ndimage
    for name in ("anim_utils", "anim_utils.animation_data", "anim_utils.animation_data.motion_distance", "transformations"):
        sys.modules.setdefault(name, types.ModuleType(name))
    md = sys.modules["anim_utils.animation_data.motion_distance"]
    md._transform_invariant_point_cloud_distance = cell_distance
    md._point_cloud_distance = None
    md.convert_quat_frame_to_point_cloud = to_point_cloud
    sys.modules["transformations"].quaternion_matrix = sys.modules["transformations"].quaternion_from_matrix = None
    base = os.path.join(reference, "morphablegraphs", "construction")
    pkg = types.ModuleType("mgref_construction")
    pkg.__path__ = []
    sys.modules["mgref_construction"] = pkg
    mods = {}
    for name in ("keyframe_detection", "utils", "segmentation"):
        spec = importlib.util.spec_from_file_location("mgref_construction." + name, os.path.join(base, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        with warnings_off():
            spec.loader.exec_module(mods[name])
    return mods["segmentation"], mods["keyframe_detection"]


@contextlib.contextmanager
def warnings_off():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


class Capture(object):
    """A motion as the reference reads it (len, iteration over the frames) that answers a slice with its indices."""

    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    def __iter__(self):
        return iter(self.frames)

    def __getitem__(self, key):
        return (key.start, key.stop)


def reference_segments(seg_mod, frames, start_keyframe, end_keyframe, settings, weights=None, dist=None, fk=False):
    """The reference on one capture: (S, E, single pair, [pairs per setting]); S and E as its distance was called."""
    STATE.update({"weights": weights, "dist": dist, "record": [], "fk": fk})
    with quiet():
        single = seg_mod.Segmentation(None, 10).extract_single_segments([Capture(frames)], start_keyframe, end_keyframe)
    if dist is None:
        assert len(STATE["record"]) == 2 * len(frames)
        S, E = np.array(STATE["record"][:len(frames)]), np.array(STATE["record"][len(frames):])
    else:
        S, E = np.array(dist[0], dtype=np.float64), np.array(dist[1], dtype=np.float64)
    multi = []
    for threshold, min_size in settings:
        with quiet():
            pairs = seg_mod.Segmentation(None, min_size).extract_segments([Capture(frames)], start_keyframe, end_keyframe, threshold)
        multi.append(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    assert len(single) == 1
    return S, E, np.asarray(single[0], dtype=np.int32), multi


def runner_up_gap(values):
    v = np.sort(np.asarray(values))
    return float(v[1] - v[0]) if len(v) > 1 else np.inf


def decision_margin(kd_mod, S, E, settings):
    """The least margin, relative to the largest distance, of every decision the reference made: both whole-capture arg-mins,
    and per setting each threshold test and the arg-min of each searched window."""
    scale = max(float(np.max(S)), float(np.max(E)))
    margin = min(runner_up_gap(S), runner_up_gap(E))
    for threshold, min_size in settings:
        limit = float(np.min(S)) + threshold
        margin = min(margin, float(np.min(np.abs(S - limit))))
        instances = kd_mod.argmin_multi(S.tolist(), threshold)
        for i, start in enumerate(instances):
            window_end = len(S) - 1 if i + 1 == len(instances) else instances[i + 1]
            if window_end - start >= min_size:
                margin = min(margin, runner_up_gap(E[start:window_end]))
    return margin / scale


def spread_of(frames, keyframes, weights, golden, rng):
    worst = 0.0
    for _ in range(3):
        perm = rng.permutation(frames.shape[1])
        STATE.update({"weights": None if weights is None else weights[perm], "dist": None, "record": [], "fk": False})
        again = np.array([[cell_distance(f[perm], k[perm]) for f in frames] for k in keyframes])
        worst = max(worst, float(np.max(np.abs(again - golden))))
    return worst


# ---- synthetic captures: a cyclic pose sequence, walked forward, turned and moved frame by frame ------------------------------
def cycle(n_joints, seed):
    rng = np.random.default_rng(seed)
    return {"rest": rng.uniform(-0.5, 0.5, (n_joints, 3)) * np.array([0.6, 1.8, 0.4]) + np.array([0.0, 0.9, 0.0]),
            "amp": rng.uniform(0.05, 0.35, (n_joints, 3)), "phase": rng.uniform(0, 2 * np.pi, (n_joints, 3)),
            "harmonic": rng.integers(1, 3, (n_joints, 3)).astype(np.float64)}


def pose(c, t):
    return c["rest"][None] + c["amp"][None] * np.sin(2 * np.pi * t[:, None, None] * c["harmonic"][None] + c["phase"][None])


def rounded(x):
    return np.round(x * 65536.0) / 65536.0


def capture_clouds(rng, c, n_frames, period, noise=0.004):
    t = np.arange(n_frames) / period + rng.uniform(0.0, 1.0)
    t = t + 0.02 * np.sin(2 * np.pi * rng.uniform(0.1, 0.3) * t + rng.uniform(0, 2 * np.pi))      # the tempo drifts
    pos = pose(c, t)
    pos[:, :, 2] += 1.2 * t[:, None]
    ang = rng.uniform(-np.pi, np.pi) + 0.6 * np.sin(0.37 * t + rng.uniform(0, 2 * np.pi))
    cs, sn = np.cos(ang)[:, None], np.sin(ang)[:, None]
    shift = rng.uniform(-2.0, 2.0, 2)
    out = pos.copy()
    out[:, :, 0] = pos[:, :, 0] * cs + pos[:, :, 2] * sn + shift[0]
    out[:, :, 2] = -pos[:, :, 0] * sn + pos[:, :, 2] * cs + shift[1]
    return rounded(out + noise * rng.standard_normal(out.shape))


POINT_SETS = [
    {"name": "cycle_j6", "n_joints": 6, "captures": [(300, 97.0), (1400, 410.0), (3000, 640.0)], "weights": False},
    {"name": "cycle_j5_weights", "n_joints": 5, "captures": [(640, 171.0), (1100, 236.0)], "weights": True},
]
POINT_SETTINGS = [(0.01, 10), (0.03, 60)]
KEY_PHASES = (0.15, 0.70)


def distance_cases():
    rng = np.random.default_rng(7100)
    ties = rng.integers(0, 3, 200).astype(np.float64), rng.integers(0, 4, 200).astype(np.float64)
    adjacent = np.ones(120), rng.integers(0, 3, 120).astype(np.float64)
    adjacent[0][108:120] = 0.0
    nothing_kept = 2.0 + rng.uniform(0.0, 1.0, 90), 2.0 + rng.uniform(0.0, 1.0, 90)
    nothing_kept[0][[10, 50]] = 0.5
    nothing_kept[1][[10, 50]] = 0.25         # the end keyframe is closest where each window starts
    smooth = np.abs(np.sin(np.arange(260) * 0.061)) + 0.01 * rng.uniform(0.0, 1.0, 260), np.abs(np.cos(np.arange(260) * 0.061)) + 0.01 * rng.uniform(0.0, 1.0, 260)
    exact = smooth[0].copy(), smooth[1].copy()
    exact[0][[31, 140, 141, 222]] = 0.0
    return [("integer_ties", ties, [(0.0, 3), (1.0, 2), (1.0, 0), (2.0, 10)]),
            ("adjacent_instances_every_window_dropped", adjacent, [(0.5, 15), (0.0, 12)]),
            ("no_kept_segment", nothing_kept, [(0.1, 10), (0.1, 0)]),
            ("one_frame", (np.array([0.75]), np.array([0.5])), [(1.0, 10), (1.0, 0), (0.0, 0)]),
            ("threshold_0", exact, [(0.0, 10), (0.0, 0)]),
            ("min_segment_size_0", smooth, [(0.05, 0), (0.3, 0), (0.3, 1)])]


# ---- the end-to-end case -----------------------------------------------------------------------------------------------------
def quaternion_capture(rng, canon, t):
    """Frames (F, 11) of a cyclic motion at the times t (one cycle per unit): root path and two joints' rotations."""
    n = len(t)
    frames = np.zeros((n, 3 + 4 * len(ANIMATED)))
    frames[:, 0] = 0.3 * t + canon["root"][0]
    frames[:, 1] = 0.9 + 0.04 * np.sin(4 * np.pi * t)
    frames[:, 2] = 1.1 * t + canon["root"][1]
    for j in range(len(ANIMATED)):
        axis_angle = canon["amp"][j][None, :] * np.sin(2 * np.pi * canon["freq"][j][None, :] * t[:, None] + canon["phase"][j][None, :])
        ang = np.linalg.norm(axis_angle, axis=1)
        q = np.concatenate([np.cos(ang / 2)[:, None], axis_angle / np.maximum(ang, 1e-12)[:, None] * np.sin(ang / 2)[:, None]], axis=1)
        frames[:, 3 + 4 * j:7 + 4 * j] = q
    frames[:, 3:] += 0.002 * rng.standard_normal((n, 4 * len(ANIMATED)))
    for j in range(len(ANIMATED)):
        frames[:, 3 + 4 * j:7 + 4 * j] /= np.linalg.norm(frames[:, 3 + 4 * j:7 + 4 * j], axis=1, keepdims=True)
    return frames


E_LENGTHS, E_PERIODS, E_SETTING = [150, 230, 96], [47.0, 52.0, 41.0], (0.004, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "segmentation.npz"))
    args = ap.parse_args()
    seg_mod, kd_mod = load_reference(args.reference)
    out = {}
    draws = redraws_total = 0
    for s, ps in enumerate(POINT_SETS):
        p = "p%d_" % s
        c = cycle(ps["n_joints"], 7000 + s)
        rng = np.random.default_rng(7010 + s)
        weights = rng.uniform(0.2, 2.0, ps["n_joints"]) if ps["weights"] else None
        keys = rounded(pose(c, np.array(KEY_PHASES)))
        out.update({p + "name": np.array(ps["name"]), p + "weights": np.ones(ps["n_joints"]) if weights is None else weights, p + "start": keys[0],
                    p + "end": keys[1], p + "n": np.int64(len(ps["captures"]))})
        for k, (length, period) in enumerate(ps["captures"]):
            redraws = 0
            for seed in range(10):
                draws += 1
                cloud = capture_clouds(np.random.default_rng(7200 + 100 * s + 10 * k + seed), c, length, period)
                S, E, single, multi = reference_segments(seg_mod, cloud, keys[0], keys[1], POINT_SETTINGS, weights)
                margin = decision_margin(kd_mod, S, E, POINT_SETTINGS)
                if margin >= MARGIN:
                    break
                print("%s capture %d: seed %d: margin %.3g; next seed" % (ps["name"], k, seed, margin))
                redraws += 1
                redraws_total += 1
            else:
                raise RuntimeError("set %d capture %d: no seed passes the margin condition" % (s, k))
            spread = spread_of(cloud, keys, weights, np.array([S, E]), np.random.default_rng(7900 + 10 * s + k))
            q = p + "c%d_" % k
            out.update({q + "cloud": cloud, q + "S": S, q + "E": E, q + "spread": np.float64(spread), q + "single": single, q + "margin": np.float64(margin),
                        q + "redraws": np.int64(redraws), q + "seed": np.int64(seed)})
            for j, pairs in enumerate(multi):
                out[q + "t%d_multi" % j] = pairs
            print("%-18s capture %d: %4d frames  single %s  segments %s  margin %.3g  spread %.3g  max distance %.3g  redraws %d" % (
                ps["name"], k, length, single.tolist(), [len(m) for m in multi], margin, spread, max(S.max(), E.max()), redraws))
    out["p_settings"] = np.array(POINT_SETTINGS, dtype=np.float64)
    cases = distance_cases()
    out["n_distance_cases"] = np.int64(len(cases))
    for i, (name, (S, E), settings) in enumerate(cases):
        S2, E2, single, multi = reference_segments(seg_mod, [[f] for f in range(len(S))], START_TAG, END_TAG, settings, dist=(S, E))
        q = "g%d_" % i
        out.update({q + "name": np.array(name), q + "S": S2, q + "E": E2, q + "single": single, q + "settings": np.array(settings, dtype=np.float64)})
        for j, pairs in enumerate(multi):
            out[q + "t%d_multi" % j] = pairs
        print("%-42s %3d frames  single %s  segments %s" % (name, len(S), single.tolist(), [m.tolist() if len(m) < 4 else len(m) for m in multi]))
    # end to end
    for seed in range(10):
        draws += 1
        rng = np.random.default_rng(7500 + seed)
        canon = {"root": rng.uniform(-0.5, 0.5, 2), "amp": rng.uniform(0.2, 0.7, (len(ANIMATED), 3)),
                 "freq": rng.integers(1, 3, (len(ANIMATED), 3)).astype(np.float64), "phase": rng.uniform(0, 2 * np.pi, (len(ANIMATED), 3))}
        motions = [quaternion_capture(rng, canon, np.arange(n) / period + rng.uniform(0.0, 1.0)) for n, period in zip(E_LENGTHS, E_PERIODS)]
        key_poses = quaternion_capture(rng, canon, np.array(KEY_PHASES))
        triples, singles, worst = [], [], np.inf
        for m, frames in enumerate(motions):
            S, E, single, multi = reference_segments(seg_mod, frames, key_poses[0], key_poses[1], [E_SETTING], fk=True)
            worst = min(worst, decision_margin(kd_mod, S, E, [E_SETTING]))
            triples += [(m, int(a), int(b)) for a, b in multi[0]]
            singles.append((m, int(single[0]), int(single[1])))
        if worst >= MARGIN:
            break
        print("end to end: seed %d: margin %.3g; next seed" % (seed, worst))
        redraws_total += 1
    else:
        raise RuntimeError("end to end: no seed passes the margin condition")
    out.update({"e_n": np.int64(len(motions)), "e_start": key_poses[0], "e_end": key_poses[1], "e_threshold": np.float64(E_SETTING[0]),
                "e_min_segment_size": np.int64(E_SETTING[1]), "e_segments": np.array(triples, dtype=np.int32).reshape(-1, 3),
                "e_single": np.array(singles, dtype=np.int32), "e_slices": np.concatenate([motions[m][a:b] for m, a, b in triples]),
                "e_margin": np.float64(worst), "e_seed": np.int64(seed),
                "e_joint_names": np.array([j[0] for j in SKELETON]), "e_joint_parents": np.array(["" if j[1] is None else j[1] for j in SKELETON]),
                "e_joint_offsets": np.array([j[2] for j in SKELETON], dtype=np.float64), "e_animated_joints": np.array(ANIMATED)})
    for m, frames in enumerate(motions):
        out["e_m%d_frames" % m] = frames
    print("end to end: %d captures, segments %s, single %s, margin %.3g" % (len(motions), triples, singles, worst))
    if 4 * redraws_total > draws:
        raise RuntimeError("%d of %d draws redrawn: more than a quarter" % (redraws_total, draws))
    out.update({"n_point_sets": np.int64(len(POINT_SETS)), "draws": np.int64(draws), "redraws": np.int64(redraws_total)})
    _write_npz(args.out, out)
    print("draws %d, redraws %d" % (draws, redraws_total))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
