"""Writes tests/golden/feature_points_warped.npz: what the reference's FeaturePointModel (construction/feature_point_model.py)
records in create_feature_points and create_root_pos_ori / convert_ori_to_angle_deg on two small synthetic models WITH a time
model -- the reference's default route, back_project(s, use_time_parameters=True): the frames are those of the time-warped motion.

    python tools/gen_feature_point_warped_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/feature_points_warped.npz]

The reference's feature_point_model.py and motion_primitive.py run unmodified, loaded as tools/gen_feature_point_golden.py loads
them and with the same anim_utils stand-ins (see that file's header: pose_orientation_quat, get_rotation_angle and
get_cartesian_coordinates_from_quaternion are restated, PARITY UNPINNED).

The sample count.  _invert_canonical_to_sample_time_function (motion_primitive.py:313-314) hands np.linspace the FLOAT
round(t(F - 2)) * (1 / speed); every NumPy from 1.18 on raises TypeError there.  For the duration of the reference's
calls np.linspace is given int(num) -- the value NumPy < 1.18 made of that float -- as oracle/gen_golden.py does; nothing else
of NumPy or the reference is touched.  The time functions are read where the reference returns them (a recording subclass of
its MotionPrimitive: back_project_time_function's result is kept, then handed on unchanged).

Contents, per model m<k>_: the arrays of tools/gen_feature_point_golden.py's fixture (low_dimension_vectors and root_latents are
full rows here: spatial then time latents), the time model (model_eigen_vectors_time, model_mean_time_vector,
model_b_spline_knots_time, model_n_basis_time), and of every recorded motion the canonical time of frame frame_idx (time_mid) and
its length (n_frames; root_n_frames for create_root_pos_ori's motions).  Asserted of the inputs, so no case is left out: every
heading length is above 0.1; every candidate's round(t(F - 2)) is at least 1e-6 from a tie (tests/timewarp_cases.count_margins);
frame_idx is a frame of every candidate's motion.  The archive is written with fixed timestamps.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_feature_point_golden as base  # noqa: E402
import timewarp_cases  # noqa: E402
from morphablegraphs_amd import synthetic  # noqa: E402

MARGIN = 1.0e-6


def cases():
    root_only = ([("Hips", None, (0.0, 0.0, 0.0)), ("Hips_EndSite", "Hips", (0.0, 9.0, 2.0))], ["Hips"])
    humanoid = synthetic.make_skeleton(5)       # Hips, Spine, Spine1, Neck, Head animated: 23 channels; arms and legs rigid
    return [
        {"data": synthetic.make_primitive(seed=221, n_components=3, n_frames=12, n_basis=7, n_dim=7, n_gmm=2, name="walk_tiny_timed",
                                          n_time_components=1, n_basis_time=4),
         "skeleton": root_only, "joints": ["Hips", "Hips_EndSite"], "frame_idx": 5, "n": 12, "seed": 4201},
        {"data": synthetic.make_primitive(seed=222, n_components=6, n_frames=30, n_basis=9, n_dim=23, n_gmm=3, name="carry_small_timed",
                                          translation_maxima=(1.5, 2.0, 0.5), n_time_components=3, n_basis_time=6),
         "skeleton": humanoid, "joints": ["Head_EndSite", "LeftHand", "Hips", "RightToeBase"], "frame_idx": 21, "n": 10, "seed": 4202},
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "feature_points_warped.npz"))
    args = ap.parse_args()
    fpm, Model = base.load_reference(args.reference)

    class Timed(Model):
        time_functions = None

        def back_project_time_function(self, gamma, speed=1.0):
            time_function = Model.back_project_time_function(self, gamma, speed)
            self.time_functions.append(np.array(time_function, dtype=np.float64))
            return time_function

    out = {"n_models": np.int64(len(cases()))}
    real_linspace = np.linspace
    np.linspace = lambda start, stop, num=50, **kw: real_linspace(start, stop, int(num), **kw)
    try:
        for k, case in enumerate(cases()):
            p = "m%d_" % k
            data, (joints, animated) = case["data"], case["skeleton"]
            model = base.make_model(fpm, Timed, data, base._Skeleton(joints, animated))
            mp = model.motion_primitive_model
            assert mp.has_time_parameters and not mp.smooth_time_parameters
            del base.HEADING_LENGTHS[:]
            np.random.seed(case["seed"])
            mp.time_functions = []
            model.create_feature_points(list(case["joints"]), case["n"], case["frame_idx"])
            point_times = mp.time_functions
            mp.draws, mp.time_functions = [], []
            model.create_root_pos_ori(case["n"])
            root_latents, root_times = np.array(mp.draws), mp.time_functions
            model.convert_ori_to_angle_deg()
            lengths = np.array(base.HEADING_LENGTHS)
            assert len(lengths) == 2 * case["n"] and lengths.min() > base.MIN_HEADING_LEN, "a heading of length %.3g: choose another model" % lengths.min()
            assert len(point_times) == len(root_times) == case["n"]
            latents = np.array(model.low_dimension_vectors, dtype=np.float64)
            L = len(data["eigen_vectors_spatial"])
            for rows in (latents, root_latents):
                for row in rows:
                    half, _ = timewarp_cases.count_margins(timewarp_cases.canonical_time_function(data, row[L:]), 1.0)
                    assert half >= MARGIN, "round(t(F - 2)) is %.3g from a tie: choose another seed" % half
            assert min(len(t) for t in point_times) > case["frame_idx"], "frame_idx beyond a candidate's motion"
            for key in ("eigen_vectors_spatial", "mean_spatial_vector", "b_spline_knots_spatial", "gmm_weights", "gmm_means", "gmm_covars", "translation_maxima",
                        "eigen_vectors_time", "mean_time_vector", "b_spline_knots_time"):
                out[p + "model_" + key] = np.asarray(data[key], dtype=np.float64)
            names = [j[0] for j in joints]
            out.update({p + "model_n_basis": np.int64(data["n_basis_spatial"]), p + "model_n_dim": np.int64(data["n_dim_spatial"]),
                        p + "model_n_basis_time": np.int64(data["n_basis_time"]),
                        p + "model_name": np.array(data["name"]), p + "n_canonical_frames": np.int64(data["n_canonical_frames"]),
                        p + "joint_names": np.array(names), p + "joint_parents": np.array([-1 if j[1] is None else names.index(j[1]) for j in joints], dtype=np.int64),
                        p + "joint_offsets": np.array([j[2] for j in joints], dtype=np.float64), p + "animated_joints": np.array(animated),
                        p + "feature_joints": np.array(case["joints"]), p + "frame_idx": np.int64(case["frame_idx"]), p + "seed": np.int64(case["seed"]),
                        p + "low_dimension_vectors": latents,
                        p + "feature_points": np.array(model.feature_points, dtype=np.float64),
                        p + "orientations": np.array(model.orientations, dtype=np.float64),
                        p + "time_mid": np.array([t[case["frame_idx"]] for t in point_times]),
                        p + "n_frames": np.array([len(t) for t in point_times], dtype=np.int64),
                        p + "root_latents": root_latents, p + "root_pos": np.array(model.root_pos, dtype=np.float64),
                        p + "root_orientation": np.array(model.root_orientation, dtype=np.float64),
                        p + "root_rot_angles": np.array(model.root_rot_angles, dtype=np.float64),
                        p + "root_n_frames": np.array([len(t) for t in root_times], dtype=np.int64), p + "heading_len": lengths})
            print("%-18s L %d + %d F %d D %d  joints %s at frame %d of %d .. %d: %d + %d samples, heading length %.3f .. %.3f" % (
                data["name"], L, len(data["eigen_vectors_time"][0]), data["n_canonical_frames"], data["n_dim_spatial"], case["joints"], case["frame_idx"],
                min(len(t) for t in point_times), max(len(t) for t in point_times), len(model.feature_points), len(model.root_pos), lengths.min(), lengths.max()))
    finally:
        np.linspace = real_linspace
    base._write_npz(args.out, out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
