"""ctypes binding of libmg_hip.so (include/mg_hip.h) -- the only way host code reaches
the HIP kernels.  There is no CPU fallback: if the library or a gfx950 device is missing
every compute call raises.

The thin object layer here (Context / Primitive / TimeGrid / ConstraintSet / DeviceBuffer)
only owns handles and converts NumPy arrays; the reference-shaped classes live in
motion_primitive.py / motion_spline.py / gaussian_mixture.py.
"""
import ctypes as C
import functools
import itertools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libmg_hip.so")   # the product library; tools pass another build to load_library(path)

MG_OK = 0
MG_ERR_INVALID_ARGUMENT = -1     # enum mg_status (include/mg_hip.h)
MG_ERR_UNSUPPORTED = -4         # enum mg_status (include/mg_hip.h): a shape the kernels do not take
MG_F32, MG_F64 = 0, 1
MG_PATH_AUTO, MG_PATH_MFMA, MG_PATH_DIRECT = 0, 1, 2
MG_ALIGN_START_POSE = -1   # mg_alignment_desc.joint: the start-pose branch of the reference's alignment
MG_OPT_FORCE_VALU_SCORE, MG_OPT_FORCE_VALU_SAMPLE, MG_OPT_RING_SLOTS, MG_OPT_CHUNK_WINDOW, MG_OPT_CHUNK_SAMPLES = 0, 1, 2, 3, 4
MG_OPT_FRAMES_KERNEL = 5   # 0 = by batch size, 1 = tile-major, 2 = chunk-stationary
MG_OPT_PLACED_FAST_PCT = 6   # mg_device_malloc_placed's acceptance ratio in percent (tests)
MG_OPT_OPTIONS_STEP = 7      # mg_options_step: 0 = one launch per step where possible, 1 = a chain of launches per option
MG_OPT_PLAIN_MALLOC = 8      # 1 = mg_device_malloc is one hipMalloc whatever the size (no placed output regions)
MG_OPT_GMM_KERNEL = 9        # mg_gmm_log_prob: 0 = by batch size, 1 = one tile per workgroup, 2 = fragments resident in LDS
MG_OPT_SCORE_KERNEL = 10     # mg_score_constraints: 0 = by batch size, 1 = a wave per 16 candidates, 2 = a wave per 64 candidates
MG_OPT_ROOT_MODE = 11        # root channels of the float32 frames kernels: 0, 1 = float64 pipeline (default), 2 = mean/delta split, 3 = split where the gate allows
MG_OPT_PLACED_HOLD = 12      # n > 0: the placement scan holds at most n candidates at once (tests)
MG_OPT_TRAJECTORY_LANES = 13  # closest-point walks: 1 = one lane per candidate whatever the batch, 8 = eight lanes up to 65536 candidates (default: eight while <= 28672 candidates are in flight, four up to 40960)
MG_OPT_TRAJECTORY_SEARCH = 14  # closest-point search of the trajectory constraints: 0 = the reference's (scipy L-BFGS-B restated for one variable), 1 = the monotone walk of rounds 2-4
MG_OPT_COUNT = 15
MG_CONSTRAINT_POSITION, MG_CONSTRAINT_DIRECTION_2D, MG_CONSTRAINT_JOINT_POSITION = 0, 1, 2
MG_CONSTRAINT_JOINT_MIDPOINT, MG_CONSTRAINT_JOINT_ORIENTATION, MG_CONSTRAINT_LOOK_AT, MG_CONSTRAINT_POSE = 3, 4, 5, 6
MG_CONSTRAINT_VALUE_POSITION, MG_CONSTRAINT_VALUE_HEADING = 7, 8   # values of the aligned motion, not errors (chained graph-walk steps)
PROFILE_SLOTS = {"frames": 0, "gmm_log_prob": 1, "score_constraints": 2, "argmin": 3,
                 "gmm_sample": 4, "spline_evaluate": 5, "step": 6, "options_step": 7, "joint_tracks": 8, "frame_constraints": 9, "trajectory": 10,
                 "cluster_tree_search": 11, "walk_frames": 12, "walk_time": 13, "step_lengths": 14, "feature_points": 15,
                 "feature_points_warped": 16, "mixture_scores": 17, "point_clouds": 18, "feature_points_warped_smoothed": 19}
DEVICE_TABLES = {"fused": 0, "tree": 1, "walk": 2, "walk_score": 3, "walk_time": 4, "step_length": 5, "feature_points": 6,
                 "feature_points_warped": 7, "mixture_scores": 8, "point_clouds": 9, "walks_mixed": 10, "walks_sample": 11,
                 "walks_warped": 12, "walks_time": 13, "savgol": 14, "walks_time_smoothed": 15,
                 "feature_points_smoothed": 16}    # MG_TABLE_* (include/mg_hip.h)
MG_TREE_MAX_DEPTH, MG_TREE_MAX_CHILDREN, MG_TREE_MAX_CANDIDATES = 64, 256, 64    # include/mg_hip.h
MG_TREE_TIE, MG_TREE_NO_RESULT, MG_TREE_OVERFLOW, MG_TREE_NO_MEAN = 1, 2, 4, 8
MG_TREE_MAX_TRAJECTORIES = 4    # root trajectory constraints of one search (mg_cluster_tree_search_trajectories)
MG_KD_MAX_DEPTH = 64
# struct mg_tree_search_record
TREE_SEARCH_RECORD = np.dtype([("row", "<i8"), ("leaf", "<i4"), ("flags", "<i4"), ("evaluations", "<i8"), ("value", "<f8")])
MG_WALK_MAX_STEPS = 64           # steps of one mg_walk_frames call (include/mg_hip.h)
MG_WALK_TILE = 32                # frames per workgroup of mg_walk_frames_kernel (csrc/mg_walk.hip)
MG_FUSED_MAX_OPTIONS = 24        # options of one mg_options_step_device_counts launch (csrc/mg_options.hip)
MG_STEP_LENGTH_MAX_ITEMS = 256   # non-empty items of one mg_step_lengths launch (include/mg_hip.h); a call with more goes in slices
MG_SLEN_TILE = 16                # candidates per workgroup of mg_step_length_kernel (csrc/mg_step_length_layout.h)
MG_SLEN_LDS_MAX = 150 * 1024     # bytes of LDS past which mg_step_lengths refuses an item (csrc/mg_step_length_layout.h)
MG_FEATURE_POINTS_MAX_ITEMS = 256   # non-empty items of one mg_feature_points launch (include/mg_hip.h); a call with more goes in slices
MG_FEATURE_POINTS_MAX_JOINTS = 32   # listed joints of one item
MG_FEATURE_POINTS_TILE = 16         # candidates per workgroup of mg_feature_points_kernel (csrc/mg_feature_points.hip)
MG_FEATURE_POINTS_WARPED_MAX_F = 256   # canonical frames mg_feature_points_warped inverts in LDS (include/mg_hip.h)
MG_FEATURE_MIXTURE_MAX_DIM, MG_FEATURE_MIXTURE_MAX_COMPONENTS = 96, 64   # caps of mg_feature_mixture_create (include/mg_hip.h)
MG_MIXTURE_SCORES_MAX_ITEMS = 256   # non-empty items of one mg_mixture_scores launch (include/mg_hip.h); a call with more goes in slices
MG_MIXTURE_SCORES_TILE = 64         # targets per workgroup of mg_mixture_scores_kernel (csrc/mg_mixture_image.h)


def mixture_lds_bytes(n_components, dim):
    """Dynamic LDS of a workgroup of mg_mixture_scores_kernel (mg_mix_lds_of, csrc/mg_mixture_image.h): up to 8 dimensions the
    mixture's image, above the tile's targets [dim][65] and its weighted log-probabilities [K][64]; past 64 KB the kernel takes
    the large-LDS opt-in."""
    if dim <= 8:
        return n_components * (dim * (dim + 1) // 2 + dim + 1) * 8
    return (dim * 65 + n_components * MG_MIXTURE_SCORES_TILE) * 8


@functools.lru_cache(maxsize=None)
def _option_record(stride):
    return np.dtype([("index", "<i8"), ("error", "<f8"), ("latent", "<f8", ((stride - 16) // 8,))])


def option_records(raw, m, stride):
    """The result records of the planner steps (mg_options_step & co., include/mg_hip.h): m records {int64 index, float64 error,
    float64 latent[(stride - 16) / 8]} side by side every `stride` bytes from the start of the uint8 array `raw`, copied out as a
    structured array with the fields index, error and latent (an option's winner: the first n_gmm_dims of its latent)."""
    return raw[:m * stride].copy().view(_option_record(stride))


# every symbol include/mg_hip.h declares (tests check the built library exports them all)
EXPORTED_SYMBOLS = [
    "mg_version", "mg_last_error", "mg_status_string",
    "mg_context_create", "mg_context_destroy", "mg_context_set_stream", "mg_context_set_reserved_cus", "mg_context_set_option", "mg_context_arena_begin", "mg_context_arena_end", "mg_context_arena_bytes", "mg_context_synchronize",
    "mg_dist_unique_id", "mg_dist_init", "mg_dist_all_gather", "mg_dist_finalize", "mg_dist_preflight", "mg_dist_info",
    "mg_context_device_info", "mg_device_malloc", "mg_device_malloc_chunked", "mg_device_malloc_placed", "mg_device_probe_placement", "mg_device_placement_info", "mg_device_free", "mg_context_trim_outputs", "mg_context_output_bytes", "mg_memcpy_h2d", "mg_memcpy_d2h", "mg_memcpy_d2d_rows",
    "mg_memset", "mg_profile_enable", "mg_profile_reset", "mg_profile_get", "mg_profile_get_samples",
    "mg_primitive_create", "mg_primitive_destroy", "mg_primitive_info", "mg_primitive_info2", "mg_primitive_root_mode", "mg_primitive_get_precisions_cholesky",
    "mg_time_function_canonical", "mg_time_function_canonical_host", "mg_time_function_sample", "mg_time_function_sample_rows",
    "mg_time_function_sample_smoothed", "mg_time_function_sample_smoothed_rows", "mg_back_project_frames_at",
    "mg_trajectory_create", "mg_trajectory_create_typed", "mg_trajectory_spline_type", "mg_trajectory_tables", "mg_trajectory_destroy", "mg_score_trajectory", "mg_score_trajectory_chained", "mg_score_trajectories", "mg_score_trajectory_points", "mg_trajectory_closest_points", "mg_trajectory_plan", "mg_joint_positions",
    "mg_trajectory_sample_parameters", "mg_trajectory_points_by_arc_length", "mg_trajectory_arc_length_of_points", "mg_trajectory_points_at_parameters",
    "mg_time_grid_create", "mg_time_grid_destroy", "mg_primitive_canonical_grid", "mg_time_grid_size",
    "mg_time_grid_get_tables",
    "mg_back_project_frames", "mg_back_project_frames_f64", "mg_back_project_coeffs", "mg_spline_evaluate",
    "mg_gmm_log_prob", "mg_gmm_sample", "mg_constraint_set_create", "mg_constraint_set_destroy",
    "mg_score_constraints", "mg_argmin_first", "mg_argmin_first_dev", "mg_step_frames_and_logp", "mg_step_plan", "mg_step_plan_for", "mg_step_plan_dtype",
    "mg_back_project_frames_host", "mg_back_project_frames_f64_host", "mg_back_project_coeffs_host",
    "mg_spline_evaluate_host", "mg_gmm_log_prob_host", "mg_gmm_sample_host", "mg_score_constraints_host",
    "mg_score_constraint_residuals", "mg_objective_error_and_naturalness", "mg_gmm_log_prob_jac", "mg_score_constraint_residuals_host",
    "mg_gmm_log_prob_jac_host", "mg_constraint_set_create_fk", "mg_constraint_set_create_aligned", "mg_constraint_set_create_full", "mg_constraint_set_update", "mg_best_candidate", "mg_best_candidate_host",
    "mg_align_frames", "mg_frame_constraint_width", "mg_score_frame_constraint", "mg_score_frame_constraints", "mg_options_frame_lists", "mg_track_plan_create", "mg_track_plan_destroy", "mg_joint_tracks",
    "mg_score_constraint_residuals_chained", "mg_score_plan", "mg_option_step", "mg_options_step", "mg_options_step_device_counts", "mg_option_step_rows", "mg_options_step_rows", "mg_gmm_sample_rows", "mg_dist_broadcast",
    "mg_cluster_tree_create", "mg_cluster_tree_destroy", "mg_cluster_tree_search", "mg_cluster_tree_search_host",
    "mg_cluster_tree_search_trajectories", "mg_cluster_tree_search_trajectories_host", "mg_cluster_tree_search_plan",
    "mg_cluster_tree_search_frames", "mg_cluster_tree_search_frames_host", "mg_cluster_tree_search_frames_plan",
    "mg_cluster_tree_create_kd", "mg_kmeans_segments", "mg_gmm_em_fit",
    "mg_spline_fit_batch", "mg_pca_fit", "mg_pca_project", "mg_pca_backproject",
    "mg_dtw_distance_grids", "mg_dtw_paths", "mg_warp_motions", "mg_dtw_pair_costs",
    "mg_keyframe_distances", "mg_segment_search",
    "mg_align_motions_spatially", "mg_prepare_aligned_frames",
    "mg_walk_frames", "mg_walk_frames_host",
    "mg_walks_sample_latents", "mg_walks_sample_latents_host", "mg_walks_frames", "mg_walks_frames_host",
    "mg_walks_time_functions", "mg_walks_time_functions_host", "mg_walks_time_functions_smoothed", "mg_walks_time_functions_smoothed_host", "mg_walks_frames_at", "mg_walks_frames_at_host",
    "mg_score_walk_residuals", "mg_score_walk_residuals_host", "mg_score_walk_residuals_steps", "mg_score_walk_residuals_steps_host",
    "mg_score_walk_time", "mg_score_walk_time_host", "mg_walk_time_table_uploads", "mg_context_table_uploads",
    "mg_step_lengths", "mg_step_lengths_host",
    "mg_feature_points", "mg_feature_points_host", "mg_feature_points_warped", "mg_feature_points_warped_host",
    "mg_feature_points_warped_smoothed", "mg_feature_points_warped_smoothed_host",
    "mg_feature_mixture_create", "mg_feature_mixture_destroy", "mg_feature_mixture_info", "mg_feature_mixture_get_image",
    "mg_mixture_scores", "mg_mixture_scores_host",
    "mg_point_cloud_features", "mg_pca_fit_leading",
    "mg_sfpca_create", "mg_sfpca_errors", "mg_sfpca_projector", "mg_sfpca_destroy",
]


class MGError(RuntimeError):
    def __init__(self, status, message):
        RuntimeError.__init__(self, "libmg_hip status %d: %s" % (status, message))
        self.status = status


class PrimitiveDesc(C.Structure):
    _fields_ = [("n_basis", C.c_int32), ("n_dim", C.c_int32), ("n_components", C.c_int32),
                ("n_canonical_frames", C.c_int32), ("n_gmm", C.c_int32), ("eigen_is_transposed", C.c_int32),
                ("eigen_vectors", C.c_void_p), ("mean_vector", C.c_void_p), ("translation_maxima", C.c_void_p),
                ("knots", C.c_void_p), ("gmm_weights", C.c_void_p), ("gmm_means", C.c_void_p),
                ("gmm_covars", C.c_void_p), ("n_gmm_dims", C.c_int32), ("n_time_components", C.c_int32),
                ("n_basis_time", C.c_int32), ("reserved", C.c_int32), ("eigen_vectors_time", C.c_void_p),
                ("mean_time_vector", C.c_void_p), ("knots_time", C.c_void_p)]


class KeyframeConstraint(C.Structure):
    _fields_ = [("type", C.c_int32), ("joint", C.c_int32), ("canonical_keyframe", C.c_double),
                ("weight_factor", C.c_double), ("target", C.c_double * 3), ("ref_dir", C.c_double * 3),
                ("joint2", C.c_int32), ("reserved", C.c_int32)]


class PoseConstraintDesc(C.Structure):   # struct mg_pose_constraint
    _fields_ = [("n_points", C.c_int32), ("has_velocity", C.c_int32), ("joints", C.c_void_p), ("points", C.c_void_p),
                ("weights", C.c_void_p), ("velocity", C.c_double * 3)]


class SkeletonDesc(C.Structure):   # struct mg_skeleton_desc
    _fields_ = [("n_joints", C.c_int32), ("reserved", C.c_int32), ("parents", C.c_void_p), ("offsets", C.c_void_p),
                ("quat_channel", C.c_void_p)]


class AlignmentDesc(C.Structure):   # struct mg_alignment_desc
    _fields_ = [("joint", C.c_int32), ("reserved", C.c_int32), ("position", C.c_double * 3), ("heading", C.c_double * 2),
                ("ref_dir", C.c_double * 3)]


MG_FRAME_CA_POSITION, MG_FRAME_DISCRETE_TRAJECTORY, MG_FRAME_LOCAL_TRAJECTORY, MG_FRAME_TRAJECTORY_SET, MG_FRAME_JOINT_ROTATION = 1, 2, 3, 4, 5
MG_FRAME_JOINT_TRAJECTORY = 6      # a TrajectoryConstraint on any joint as a member of a constraint list (start_arc = its min_u)
MG_FRAME_MAX_JOINTS = 8
MG_TRACK_MAX_REQUESTS = 4
MG_FRAME_LIST_MAX = 4        # per-frame constraints of one option in mg_options_frame_lists


class FrameConstraintDesc(C.Structure):   # struct mg_frame_constraint_desc
    _fields_ = [("type", C.c_int32), ("n_frames", C.c_int32), ("n_points", C.c_int32), ("n_joints", C.c_int32), ("weight", C.c_double),
                ("target", C.c_double * 3), ("axis_on", C.c_int32 * 3), ("quat_channel", C.c_int32), ("points_dev", C.c_void_p),
                ("start_arc", C.c_double), ("trajectories", C.c_void_p * MG_FRAME_MAX_JOINTS), ("arc0", C.c_double * MG_FRAME_MAX_JOINTS),
                ("range_start", C.c_double * MG_FRAME_MAX_JOINTS), ("range_end", C.c_double * MG_FRAME_MAX_JOINTS),
                ("has_range", C.c_int32 * MG_FRAME_MAX_JOINTS), ("quaternion", C.c_double * 4)]


MG_SPLINE_CATMULL_ROM, MG_SPLINE_BSPLINE, MG_SPLINE_FITTED_BSPLINE = 0, 1, 2    # mg_trajectory_create_typed: the reference's SPLINE_TYPE_*


class TrajectoryPlanInfo(C.Structure):   # struct mg_trajectory_plan_info
    _fields_ = [("kernel", C.c_int32), ("lanes", C.c_int32), ("poly_lds", C.c_int32), ("needs_paths", C.c_int32), ("together", C.c_int32),
                ("candidates_per_workgroup", C.c_int32), ("lds_bytes", C.c_int64)]


class ScorePlanInfo(C.Structure):   # struct mg_score_plan_info
    _fields_ = [("kernel", C.c_int32), ("lds_opt_in", C.c_int32), ("rows", C.c_int32), ("row_tiles", C.c_int32), ("lds_bytes", C.c_int64),
                ("workgroups", C.c_int64)]


class TreeSearchPlanInfo(C.Structure):   # struct mg_tree_search_plan_info
    _fields_ = [("lds_bytes", C.c_int64), ("w_rows", C.c_int32), ("root_rows", C.c_int32), ("poly_doubles", C.c_int32),
                ("trajectory_slots", C.c_int32), ("lds_opt_in", C.c_int32), ("refused", C.c_int32)]


class TreeFrameLists(C.Structure):   # struct mg_tree_frame_lists
    _fields_ = [("plans", C.c_void_p), ("grids", C.c_void_p), ("n_constraints", C.c_void_p), ("constraints", C.c_void_p), ("request_of", C.c_void_p),
                ("rotation_grids", C.c_void_p)]


class TreeFramesPlanInfo(C.Structure):   # struct mg_tree_frames_plan_info
    _fields_ = [("lds_bytes", C.c_int64), ("w_rows", C.c_int32), ("root_rows", C.c_int32), ("poly_doubles", C.c_int32),
                ("trajectory_slots", C.c_int32), ("lds_opt_in", C.c_int32), ("refused", C.c_int32), ("track_group", C.c_int32),
                ("control_points", C.c_int32), ("tables_lds", C.c_int32), ("pad", C.c_int32), ("table_bytes", C.c_int64), ("scratch_bytes", C.c_int64)]


MG_TREE_TRACK_GROUP = 4      # children whose control points a frames search keeps in LDS side by side (csrc/mg_tree_plan.h)
MG_SCORE_KERNELS = ("valu", "tile", "wide")   # MG_SCORE_KERNEL_*
MG_TRAJ_KERNELS = ("staged_lds", "staged_global", "stream", "coop8", "coop4", "stream_multi", "coop8_multi", "coop4_multi")   # MG_TRAJ_KERNEL_*


def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def rotate_by_quaternion(q, v):
    """v rotated by the (w, x, y, z) quaternion q (normalised first)."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q)
    v = np.asarray(v, dtype=np.float64)
    u = q[1:]
    return v + 2.0 * (q[0] * np.cross(u, v) + np.cross(u, np.cross(u, v)))


class Skeleton(object):
    """The part of an anim_utils Skeleton forward kinematics needs: joints = [(name, parent name or None,
    (ox, oy, oz)), ...] with parents before children and the root first; animated_joints = names in pose-vector
    order (root translation at [0:3], then one (w,x,y,z) quaternion per animated joint)."""

    _serials = itertools.count(1)

    def __init__(self, joints, animated_joints):
        self.serial = next(Skeleton._serials)   # a stable identity for caches (id() of a collected object can be reused)
        self.names = [j[0] for j in joints]
        index = {n: i for i, n in enumerate(self.names)}
        if len(index) != len(self.names):
            raise ValueError("duplicate joint names")
        self.parents = np.array([-1 if j[1] is None else index[j[1]] for j in joints], dtype=np.int32)
        self.offsets = np.ascontiguousarray([j[2] for j in joints], dtype=np.float64).reshape(len(joints), 3)
        self.animated_joints = list(animated_joints)
        chan = {n: 3 + 4 * i for i, n in enumerate(self.animated_joints)}
        self.quat_channel = np.array([chan.get(n, -1) for n in self.names], dtype=np.int32)
        if self.parents[0] != -1 or np.any(self.parents[1:] >= np.arange(1, len(joints))) or np.any(self.parents[1:] < 0):
            raise ValueError("joint 0 must be the root and parents must precede their children")

    def index(self, joint):
        return int(joint) if isinstance(joint, (int, np.integer)) else self.names.index(joint)

    def indices(self, joints):
        """The joints (names or indices) as the int32 vector mg_joint_positions reads."""
        return np.ascontiguousarray([self.index(j) for j in joints], dtype=np.int32)

    def chain(self, joint):
        out, j = [], self.index(joint)
        while j >= 0:
            out.insert(0, j)
            j = int(self.parents[j])
        return out

    def heading(self, frame, joint=0, ref_dir=(0.0, 0.0, 1.0)):
        """Unit (x, z) of the joint's global orientation in `frame` applied to ref_dir: what anim_utils'
        get_global_node_orientation_vector returns for one pose vector (host side, once per step: the previous
        motion's last frame; the candidates' own headings are computed on the device)."""
        frame = np.asarray(frame, dtype=np.float64)
        q = np.array([1.0, 0.0, 0.0, 0.0])
        for j in self.chain(joint):
            ch = int(self.quat_channel[j])
            if ch >= 0:
                qj = frame[ch:ch + 4]
                nq = np.linalg.norm(qj)
                if not (np.isfinite(nq) and nq > 0.0):
                    raise ValueError("quaternion of joint %r in the previous frame is zero or not finite" % (self.names[j],))
                q = _quat_mul(q, qj / nq)
        v = np.asarray(ref_dir, dtype=np.float64)
        u = q[1:]
        p = v + 2.0 * (q[0] * np.cross(u, v) + np.cross(u, np.cross(u, v)))
        d = np.array([p[0], p[2]])
        return d / np.linalg.norm(d)

    def alignment_to(self, prev_frame, joint=0, ref_dir=(0.0, 0.0, 1.0)):
        """The alignment record (ConstraintSet `alignment`) that attaches a candidate to a previous motion ending
        in `prev_frame` (= prev_frames[-1] of motion_primitive_constraints.py:110-114)."""
        prev_frame = np.asarray(prev_frame, dtype=np.float64)
        return {"joint": self.index(joint), "position": [float(v) for v in prev_frame[:3]],
                "heading": [float(v) for v in self.heading(prev_frame, joint, ref_dir)], "ref_dir": [float(v) for v in ref_dir]}

    def desc(self):
        return SkeletonDesc(len(self.names), 0, self.parents.ctypes.data, self.offsets.ctypes.data, self.quat_channel.ctypes.data)


_lib = None


def load_library(path=None):
    """dlopen libmg_hip.so; raises OSError with a build hint if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError("libmg_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C morphablegraphs_amd/csrc` (there is no CPU fallback)" % p)
    # Kernel arguments in device memory instead of host memory the GPU reads over PCIe: the persistent kernels fetch their
    # argument block once per workgroup before anything else can start (0.3-0.5 us of a ~78 us frames launch, tools/ab.py).
    # A setting of the HIP runtime, read when it initialises: it takes effect when this library is the first user of HIP in the
    # process; a value the caller has set is left alone.
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    lib = C.CDLL(p)
    lib.mg_version.restype = C.c_char_p
    lib.mg_last_error.restype = C.c_char_p
    lib.mg_status_string.restype = C.c_char_p
    lib.mg_status_string.argtypes = [C.c_int]
    lib.mg_primitive_canonical_grid.restype = C.c_void_p
    lib.mg_primitive_canonical_grid.argtypes = [C.c_void_p]
    lib.mg_time_grid_size.argtypes = [C.c_void_p]
    for name in ("mg_context_destroy", "mg_primitive_destroy", "mg_time_grid_destroy", "mg_constraint_set_destroy", "mg_trajectory_destroy", "mg_track_plan_destroy",
                 "mg_cluster_tree_destroy", "mg_feature_mixture_destroy", "mg_sfpca_destroy"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [C.c_void_p]
    vp, i32, i64, u64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double
    sigs = {
        "mg_context_create": [i32, vp, C.POINTER(vp)],
        "mg_context_set_stream": [vp, vp],
        "mg_context_set_reserved_cus": [vp, i32],
        "mg_context_set_option": [vp, i32, i32],
        "mg_device_malloc_placed": [vp, i64, i32, C.POINTER(vp), C.POINTER(dbl)],
        "mg_device_probe_placement": [vp, vp, i64, C.POINTER(dbl)],
        "mg_device_placement_info": [vp, vp, C.POINTER(dbl), C.POINTER(dbl)],
        "mg_device_malloc_chunked": [vp, i64, i64, C.POINTER(vp)],
        "mg_context_arena_begin": [vp, i64],
        "mg_context_arena_end": [vp],
        "mg_context_arena_bytes": [vp, C.POINTER(i64), C.POINTER(i64)],
        "mg_dist_unique_id": [vp],
        "mg_dist_init": [vp, i32, i32, vp],
        "mg_dist_all_gather": [vp, vp, vp, i64, i32],
        "mg_dist_finalize": [vp],
        "mg_dist_preflight": [vp],
        "mg_dist_info": [vp, C.POINTER(C.c_int32)],
        "mg_context_synchronize": [vp],
        "mg_context_device_info": [vp, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(i64)],
        "mg_device_malloc": [vp, i64, C.POINTER(vp)],
        "mg_context_trim_outputs": [vp],
        "mg_context_output_bytes": [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)],
        "mg_device_free": [vp, vp],
        "mg_memcpy_h2d": [vp, vp, vp, i64],
        "mg_memcpy_d2h": [vp, vp, vp, i64],
        "mg_memcpy_d2d_rows": [vp, vp, i64, vp, i64, i64, i64],
        "mg_memset": [vp, vp, i32, i64],
        "mg_profile_enable": [vp, i32],
        "mg_profile_reset": [vp],
        "mg_profile_get": [vp, i32, C.POINTER(dbl), C.POINTER(i64)],
        "mg_profile_get_samples": [vp, i32, vp, i64, C.POINTER(i64)],
        "mg_primitive_create": [vp, C.POINTER(PrimitiveDesc), C.POINTER(vp)],
        "mg_primitive_info": [vp, C.POINTER(C.c_int32)],
        "mg_primitive_info2": [vp, C.POINTER(C.c_int32)],
        "mg_primitive_root_mode": [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double)],
        "mg_time_function_canonical": [vp, vp, i32, i64, i64, vp],
        "mg_trajectory_create": [vp, vp, i32, i32, C.POINTER(vp)],
        "mg_trajectory_create_typed": [vp, vp, i32, i32, i32, C.POINTER(vp)],
        "mg_trajectory_spline_type": [vp],
        "mg_trajectory_tables": [vp, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(dbl)],
        "mg_joint_positions": [vp, vp, vp, i32, vp, i64, i32, vp],
        "mg_score_trajectory": [vp, vp, vp, vp, i32, i64, i64, dbl, dbl, vp, vp, i32, vp],
        "mg_score_trajectory_chained": [vp, vp, vp, vp, i32, i64, i64, dbl, dbl, vp, vp, vp, i32, vp],
        "mg_score_trajectories": [i32, vp, vp, vp, i32, i64, vp, vp, vp, vp, vp, i32],
        "mg_score_trajectory_points": [vp, vp, vp, i64, i32, dbl, dbl, vp, i32, vp],
        "mg_trajectory_closest_points": [vp, vp, vp, i64, i32, dbl, vp, vp, vp],
        "mg_trajectory_plan": [vp, i32, i32, i32, i64, i64, i32, vp],
        "mg_trajectory_sample_parameters": [vp, vp, C.POINTER(C.c_int32)],
        "mg_trajectory_points_by_arc_length": [vp, vp, vp, i64, dbl, vp, vp, vp, vp],
        "mg_trajectory_arc_length_of_points": [vp, vp, vp, vp, i64, vp, vp, vp],
        "mg_trajectory_points_at_parameters": [vp, vp, vp, vp, i64, vp],
        "mg_align_frames": [vp, vp, i64, i32, vp, i32, C.POINTER(AlignmentDesc)],
        "mg_frame_constraint_width": [C.POINTER(FrameConstraintDesc), i32],
        "mg_score_frame_constraint": [vp, C.POINTER(FrameConstraintDesc), vp, i64, i32, i32, vp, i32, vp],
        "mg_time_function_canonical_host": [vp, vp, i32, i64, i64, vp],
        "mg_primitive_get_precisions_cholesky": [vp, vp],
        "mg_time_grid_create": [vp, vp, C.c_int32, C.POINTER(vp)],
        "mg_time_grid_get_tables": [vp, vp, vp, vp],
        "mg_back_project_frames": [vp, vp, vp, i32, i64, i64, vp, i32],
        "mg_back_project_frames_f64": [vp, vp, vp, i32, i64, i64, vp],
        "mg_back_project_coeffs": [vp, vp, i32, i64, i64, vp, i32],
        "mg_spline_evaluate": [vp, vp, vp, i64, vp],
        "mg_gmm_log_prob": [vp, vp, i32, i64, i64, vp, i32],
        "mg_gmm_sample": [vp, i64, vp, u64, vp, i32, i64, vp],
        "mg_constraint_set_create": [vp, vp, C.c_int32, C.POINTER(vp)],
        "mg_score_constraints": [vp, vp, vp, i32, i64, i64, vp, i32],
        "mg_argmin_first": [vp, vp, i32, i64, C.POINTER(i64), C.POINTER(dbl)],
        "mg_argmin_first_dev": [vp, vp, i32, i64, vp],
        "mg_step_frames_and_logp": [vp, vp, i32, i64, i64, vp, vp],
        "mg_step_plan": [vp, i64, C.POINTER(C.c_int32)],
        "mg_step_plan_for": [vp, i64, vp, C.POINTER(C.c_int32)],
        "mg_step_plan_dtype": [vp, i64, vp, i32, C.POINTER(C.c_int32)],
        "mg_back_project_frames_host": [vp, vp, vp, i32, i64, i64, vp, i32],
        "mg_back_project_frames_f64_host": [vp, vp, vp, i32, i64, i64, vp],
        "mg_back_project_coeffs_host": [vp, vp, i32, i64, i64, vp, i32],
        "mg_spline_evaluate_host": [vp, vp, vp, i64, vp],
        "mg_gmm_log_prob_host": [vp, vp, i32, i64, i64, vp, i32],
        "mg_gmm_sample_host": [vp, i64, vp, u64, vp, i32, i64, vp],
        "mg_score_constraints_host": [vp, vp, vp, i32, i64, i64, vp, i32],
        "mg_score_constraint_residuals": [vp, vp, vp, i32, i64, i64, vp],
        "mg_constraint_set_create_fk": [vp, vp, vp, i32, vp],
        "mg_constraint_set_create_aligned": [vp, vp, vp, i32, vp, vp],
        "mg_constraint_set_update": [vp, vp, i32, vp],
        "mg_constraint_set_create_full": [vp, vp, vp, i32, vp, i32, vp, vp],
        "mg_best_candidate": [vp, vp, vp, i32, i64, i64, C.POINTER(i64), C.POINTER(dbl)],
        "mg_best_candidate_host": [vp, vp, vp, i32, i64, i64, C.POINTER(i64), C.POINTER(dbl)],
        "mg_score_constraint_residuals_chained": [vp, vp, vp, i32, i64, i64, vp, vp],
        "mg_score_plan": [vp, vp, i64, vp],
        "mg_option_step": [vp, vp, i64, vp, u64, vp, i32, i64, vp, vp],
        "mg_option_step_rows": [vp, vp, i64, vp, u64, i64, i64, vp, i32, i64, vp, vp],
        "mg_options_step_rows": [i32, vp, vp, i64, vp, vp, i64, i64, vp, i32, vp, vp, vp, i64, vp],
        "mg_gmm_sample_rows": [vp, i64, vp, u64, i64, i64, vp, i32, i64, vp],
        "mg_dist_broadcast": [vp, vp, i64, i32],
        "mg_objective_error_and_naturalness": [vp, vp, vp, i32, i64, i64, dbl, dbl, vp, vp, vp],
        "mg_time_function_sample": [vp, vp, i32, i64, i64, dbl, vp, vp, i32, vp],
        "mg_time_function_sample_rows": [vp, vp, i32, i64, i64, dbl, vp, vp, i32, i64, vp],
        "mg_time_function_sample_smoothed": [vp, vp, i32, i64, i64, dbl, vp, vp, i32, vp],
        "mg_time_function_sample_smoothed_rows": [vp, vp, i32, i64, i64, dbl, vp, vp, i32, i64, vp],
        "mg_back_project_frames_at": [vp, vp, i32, i64, i64, vp, vp, i32, vp, i32],
        "mg_track_plan_create": [vp, vp, i32, vp, vp, i32, C.POINTER(vp)],
        "mg_joint_tracks": [vp, vp, i32, i64, i64, vp, vp, vp],
        "mg_score_frame_constraints": [vp, i32, vp, vp, vp, vp, i64, vp, i32, vp],
        "mg_options_frame_lists": [i32, vp, vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp],
        "mg_options_step": [i32, vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, i64, vp],
        "mg_options_step_device_counts": [i32, vp, vp, i64, vp, vp, i32, vp, vp, vp, i64, vp, vp],
        "mg_gmm_log_prob_jac": [vp, vp, i32, i64, i64, vp],
        "mg_score_constraint_residuals_host": [vp, vp, vp, i32, i64, i64, vp],
        "mg_gmm_log_prob_jac_host": [vp, vp, i32, i64, i64, vp],
        "mg_cluster_tree_create": [vp, i32, i32, vp, vp, vp, vp, i64, C.POINTER(vp)],
        "mg_cluster_tree_create_kd": [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp)],
        "mg_cluster_tree_search": [i32, vp, vp, vp, i32, vp],
        "mg_cluster_tree_search_host": [i32, vp, vp, vp, i32, vp],
        "mg_cluster_tree_search_trajectories": [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp],
        "mg_cluster_tree_search_trajectories_host": [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp],
        "mg_cluster_tree_search_plan": [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp],
        "mg_cluster_tree_search_frames": [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp],
        "mg_cluster_tree_search_frames_host": [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp],
        "mg_cluster_tree_search_frames_plan": [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp],
        "mg_kmeans_segments": [vp, vp, i64, i32, i32, vp, vp, i32, i32, vp, vp, u64, i32, dbl, vp, vp, vp, vp],
        "mg_gmm_em_fit": [vp, vp, i64, i32, i32, vp, vp, dbl, dbl, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "mg_spline_fit_batch": [vp, vp, i64, i32, i32, vp, i32, vp],
        "mg_pca_fit": [vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp],
        "mg_pca_project": [vp, vp, vp, i64, i64, i64, vp],
        "mg_pca_backproject": [vp, vp, vp, vp, i64, i64, i64, vp],
        "mg_dtw_distance_grids": [vp, vp, i32, vp, vp, i64, i32, vp, vp],
        "mg_dtw_paths": [vp, vp, i32, vp, i64, vp, vp, vp, vp, vp],
        "mg_warp_motions": [vp, vp, vp, i64, i32, vp, i32, vp],
        "mg_dtw_pair_costs": [vp, vp, vp, i64, i32, vp, vp, i64, vp],
        "mg_keyframe_distances": [vp, vp, vp, i64, i32, vp, i32, vp, vp],
        "mg_segment_search": [vp, vp, vp, vp, i64, i32, dbl, i32, vp, vp, vp],
        "mg_align_motions_spatially": [vp, vp, vp, i64, i32, i64, vp, vp, vp],
        "mg_prepare_aligned_frames": [vp, vp, i64, i32, i32, i32, vp, vp],
        "mg_walk_frames": [i32, vp, vp, vp, i32, i64, i64, vp, vp, i32, vp, vp, vp, vp, i64, vp],
        "mg_walk_frames_host": [i32, vp, vp, vp, i32, i64, i64, vp, vp, i32, vp, vp, vp, vp, i64, vp],
        "mg_walks_sample_latents": [i32, vp, vp, vp, i64, i32, u64, vp, i32, i64, vp],
        "mg_walks_sample_latents_host": [i32, vp, vp, vp, i64, i32, u64, vp, i32, i64, vp],
        "mg_walks_frames": [i32, vp, vp, vp, vp, i32, i64, i32, i64, vp, vp, vp, vp, i64, vp],
        "mg_walks_frames_host": [i32, vp, vp, vp, vp, i32, i64, i32, i64, vp, vp, vp, vp, i64, vp],
        "mg_walks_time_functions": [i32, vp, vp, vp, vp, i32, i64, i32, i64, dbl, vp, vp, i32],
        "mg_walks_time_functions_host": [i32, vp, vp, vp, vp, i32, i64, i32, i64, dbl, vp, vp, i32],
        "mg_walks_time_functions_smoothed": [i32, vp, vp, vp, vp, vp, i32, i64, i32, i64, dbl, vp, vp, i32],
        "mg_walks_time_functions_smoothed_host": [i32, vp, vp, vp, vp, vp, i32, i64, i32, i64, dbl, vp, vp, i32],
        "mg_walks_frames_at": [i32, vp, vp, vp, vp, i32, i64, i32, i64, vp, vp, i32, vp, vp, vp, vp, i64, vp],
        "mg_walks_frames_at_host": [i32, vp, vp, vp, vp, i32, i64, i32, i64, vp, vp, i32, vp, vp, vp, vp, i64, vp],
        "mg_score_walk_residuals": [i32, vp, vp, i32, i64, i64, vp, i64, vp, vp],
        "mg_score_walk_residuals_host": [i32, vp, vp, i32, i64, i64, vp, i64, vp, vp],
        "mg_score_walk_residuals_steps": [i32, vp, vp, i32, i64, i64, vp, i64, vp, vp, vp],
        "mg_score_walk_residuals_steps_host": [i32, vp, vp, i32, i64, i64, vp, i64, vp, vp, vp],
        "mg_score_walk_time": [i32, vp, vp, i32, i64, i64, i32, vp, dbl, dbl, dbl, dbl, vp, vp, vp],
        "mg_score_walk_time_host": [i32, vp, vp, i32, i64, i64, i32, vp, dbl, dbl, dbl, dbl, vp, vp, vp],
        "mg_walk_time_table_uploads": [vp, C.POINTER(i64)],
        "mg_context_table_uploads": [vp, C.c_int, C.POINTER(i64)],
        "mg_step_lengths": [i32, vp, i32],
        "mg_step_lengths_host": [i32, vp, i32],
        "mg_feature_points": [i32, vp, i32],
        "mg_feature_points_host": [i32, vp, i32],
        "mg_feature_points_warped": [i32, vp, i32],
        "mg_feature_points_warped_host": [i32, vp, i32],
        "mg_feature_points_warped_smoothed": [i32, vp, vp, i32],
        "mg_feature_points_warped_smoothed_host": [i32, vp, vp, i32],
        "mg_feature_mixture_create": [vp, i32, i32, vp, vp, vp, dbl, C.POINTER(vp)],
        "mg_feature_mixture_info": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(dbl)],
        "mg_feature_mixture_get_image": [vp, vp, vp, vp],
        "mg_mixture_scores": [vp, i32, vp],
        "mg_mixture_scores_host": [vp, i32, vp],
        "mg_point_cloud_features": [vp, vp, vp, vp, i32, i32, vp, i32, i64, i64, vp],
        "mg_pca_fit_leading": [vp, vp, i64, i64, dbl, dbl, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp],
        "mg_sfpca_create": [vp, vp, i32, i32, i32, vp, vp, i32, vp, i32, C.POINTER(vp)],
        "mg_sfpca_errors": [vp, vp, i32, i32, i32, vp, vp],
        "mg_sfpca_projector": [vp, vp, i32, i32, vp, vp],
    }
    for name, argtypes in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    if path is None or _lib is None:   # an explicit path given before first use (a tool's A/B build) becomes the library
        _lib = lib
    return lib


def _check(status):
    if status != MG_OK:
        raise MGError(status, load_library().mg_last_error().decode("utf-8", "replace"))


def _dtype_code(arr):
    if arr.dtype == np.float32:
        return MG_F32
    if arr.dtype == np.float64:
        return MG_F64
    raise TypeError("expected float32 or float64 array, got %s" % arr.dtype)


def _latents(a):
    """2-D C-contiguous float32/float64 view of a latent batch."""
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2:
        raise ValueError("latents must be (n_samples, n_components)")
    return np.ascontiguousarray(a)


class Context(object):
    """One per (process, device).  stream: raw hipStream_t (int) or None."""

    def __init__(self, device=0, stream=None, lib=None):
        self.lib = lib if lib is not None else load_library()   # lib: another build loaded with load_library(path) (tools)
        h = C.c_void_p()
        _check(self.lib.mg_context_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self.handle = h
        self.device = int(device)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mg_context_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_reserved_cus(self, n):
        """Leave n CUs free of the persistent frames kernel (for RCCL kernels running beside it)."""
        _check(self.lib.mg_context_set_reserved_cus(self.handle, int(n)))

    def set_option(self, option, value):
        """Test / tuning switches (MG_OPT_*): explicit calls, the library reads no environment variable."""
        _check(self.lib.mg_context_set_option(self.handle, int(option), int(value)))

    def arena_begin(self, block_bytes=0):
        """Until arena_end(), device constants of new primitives come out of shared blocks (one graph, one arena)."""
        _check(self.lib.mg_context_arena_begin(self.handle, int(block_bytes)))

    def arena_end(self):
        _check(self.lib.mg_context_arena_end(self.handle))

    def arena_bytes(self):
        r, u = C.c_int64(0), C.c_int64(0)
        _check(self.lib.mg_context_arena_bytes(self.handle, C.byref(r), C.byref(u)))
        return int(r.value), int(u.value)

    def trajectory_plan(self, n_components, rows, n_seg, n, total=None, points=False):
        """mg_trajectory_plan: the kernel the trajectory scorers launch for n candidates per scorer (`total` in flight) of a primitive
        with n_components latents and rows = 3 n_basis + 4 root rows against a spline of n_seg segments, under this context's options;
        launches nothing.  MGError (MG_ERR_UNSUPPORTED) where mg_score_trajectory raises it."""
        info = TrajectoryPlanInfo()
        _check(self.lib.mg_trajectory_plan(self.handle, int(n_components), int(rows), int(n_seg), int(n), int(n if total is None else total),
                                           1 if points else 0, C.byref(info)))
        return {"kernel": MG_TRAJ_KERNELS[info.kernel], "lanes": int(info.lanes), "poly_lds": bool(info.poly_lds),
                "needs_paths": bool(info.needs_paths), "together": bool(info.together),
                "candidates_per_workgroup": int(info.candidates_per_workgroup), "lds_bytes": int(info.lds_bytes)}

    def synchronize(self):
        _check(self.lib.mg_context_synchronize(self.handle))

    def table_uploads(self, name):
        """How often the per-call device table `name` (a key of DEVICE_TABLES) of this context has been (re)written."""
        n = C.c_int64()
        _check(self.lib.mg_context_table_uploads(self.handle, DEVICE_TABLES[name], C.byref(n)))
        return int(n.value)

    # ---- multi-GPU (RCCL loaded on first use; one process per GPU) ----------------------------------
    def dist_unique_id(self):
        """128 opaque bytes made on rank 0 and carried to the other ranks out of band."""
        buf = C.create_string_buffer(128)
        _check(self.lib.mg_dist_unique_id(buf))
        return buf.raw

    def dist_init(self, rank, n_ranks, unique_id):
        _check(self.lib.mg_dist_init(self.handle, int(rank), int(n_ranks), C.c_char_p(bytes(unique_id))))

    def dist_all_gather(self, local_dev, gathered_dev, count, dtype=np.float32):
        """gathered[r * count + i] = rank r's local[i], on the context's stream."""
        code = MG_F64 if np.dtype(dtype) == np.float64 else MG_F32
        _check(self.lib.mg_dist_all_gather(self.handle, _dev_ptr(local_dev), _dev_ptr(gathered_dev), int(count), code))

    def dist_broadcast(self, buf_dev, nbytes, root=0):
        """nbytes bytes of buf_dev from rank `root` to every rank, on the context's stream."""
        _check(self.lib.mg_dist_broadcast(self.handle, _dev_ptr(buf_dev), int(nbytes), int(root)))

    def upload_into(self, buf, arr):
        arr = np.ascontiguousarray(arr)
        _check(self.lib.mg_memcpy_h2d(self.handle, _dev_ptr(buf), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def copy_rows_dev(self, dst_dev, dst_pitch, src_dev, src_pitch, row_bytes, rows):
        """mg_memcpy_d2d_rows: `rows` rows of row_bytes bytes between device matrices of their own pitches (bytes), asynchronous on
        the context's stream."""
        _check(self.lib.mg_memcpy_d2d_rows(self.handle, _dev_ptr(dst_dev), int(dst_pitch), _dev_ptr(src_dev), int(src_pitch), int(row_bytes), int(rows)))

    def dist_finalize(self):
        _check(self.lib.mg_dist_finalize(self.handle))

    def dist_preflight(self):
        """librccl loads and the context's device answers (mg_dist_preflight): exchanged between the ranks before mg_dist_init."""
        _check(self.lib.mg_dist_preflight(self.handle))

    def dist_info(self):
        """{'rank', 'ranks', 'device'} of the communicator as RCCL reports them (mg_dist_info); ranks 0 without one."""
        out = (C.c_int32 * 3)()
        _check(self.lib.mg_dist_info(self.handle, out))
        return {"rank": int(out[0]), "ranks": int(out[1]), "device": int(out[2])}

    def set_stream(self, stream):
        _check(self.lib.mg_context_set_stream(self.handle, C.c_void_p(stream) if stream else None))

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu, mem = C.c_int32(), C.c_int64()
        _check(self.lib.mg_context_device_info(self.handle, name, C.byref(ncu), C.byref(mem)))
        return {"name": name.value.decode(), "n_cu": ncu.value, "total_mem": mem.value}

    def malloc(self, nbytes, chunk_bytes=0):
        return DeviceBuffer(self, nbytes, chunk_bytes)

    def malloc_placed(self, nbytes, max_candidates=0):
        """A buffer for a large kernel output in the part of the card's memory where the frames kernel's store stream
        runs at the fill rate (mg_device_malloc_placed).  .placement = {"probed", "ratio", "pattern_us", "fast"}."""
        return DeviceBuffer(self, nbytes, placed=True, max_candidates=max_candidates)

    def trim_outputs(self):
        """Release the placed output regions no piece of which is in use (mg_context_trim_outputs)."""
        _check(self.lib.mg_context_trim_outputs(self.handle))

    def output_bytes(self):
        """(reserved, in_use, regions, fast regions) of the context's placed output regions."""
        r, u, n, f = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        _check(self.lib.mg_context_output_bytes(self.handle, C.byref(r), C.byref(u), C.byref(n), C.byref(f)))
        return r.value, u.value, n.value, f.value

    def probe_placement(self, buf, nbytes=None):
        info = (C.c_double * 4)()
        _check(self.lib.mg_device_probe_placement(self.handle, _dev_ptr(buf), int(nbytes if nbytes is not None else buf.nbytes), info))
        return {"probed": int(info[0]), "ratio": float(info[1]), "pattern_us": float(info[2]), "fast": bool(info[3])}

    def placement_info(self, buf):
        """What the output arena knows about memory it handed out (no probe): 'region' False for memory from elsewhere."""
        info, tbps = (C.c_double * 4)(), C.c_double()
        _check(self.lib.mg_device_placement_info(self.handle, _dev_ptr(buf), info, C.byref(tbps)))
        return {"region": bool(info[0]), "ratio": float(info[1]), "pattern_us": float(info[2]), "fast": bool(info[3]), "pattern_TBps": float(tbps.value)}

    def buffers(self):
        """with ctx.buffers() as bufs: the device buffers of one call (DeviceBuffers), freed on the way out."""
        return DeviceBuffers(self)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(self, arr.nbytes)
        _check(self.lib.mg_memcpy_h2d(self.handle, buf.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return buf

    def download(self, buf, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        ptr = buf.ptr if isinstance(buf, DeviceBuffer) else C.c_void_p(int(buf))
        _check(self.lib.mg_memcpy_d2h(self.handle, out.ctypes.data_as(C.c_void_p), ptr, out.nbytes))
        return out

    def profile_enable(self, on=True):
        """on: False/0 = off, True/1 = bracket every launch, n > 1 = bracket every n-th launch of a slot."""
        _check(self.lib.mg_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        _check(self.lib.mg_profile_reset(self.handle))

    def profile_get(self, slot):
        ms, n = C.c_double(), C.c_int64()
        _check(self.lib.mg_profile_get(self.handle, PROFILE_SLOTS.get(slot, slot), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_samples(self, slot, capacity=65536):
        """The individual event-bracketed durations (ms) of a slot, oldest first."""
        out = np.empty(int(capacity), dtype=np.float32)
        n = C.c_int64()
        _check(self.lib.mg_profile_get_samples(self.handle, PROFILE_SLOTS.get(slot, slot), out.ctypes.data_as(C.c_void_p),
                                               int(capacity), C.byref(n)))
        return out[:n.value].copy()

    def joint_positions(self, skeleton, joints, frames):
        """(N, D) float64 frames -> (N, len(joints), 3) global joint positions by forward kinematics (mg_joint_positions);
        joints: names or indices of `skeleton` (a Skeleton)."""
        F = np.ascontiguousarray(frames, dtype=np.float64)
        if F.ndim != 2:
            raise ValueError("frames must be (n_frames, n_dim)")
        idx = skeleton.indices(joints)
        with self.buffers() as bufs:
            d_f, d_o = bufs.upload(F), bufs.malloc(8 * F.shape[0] * len(idx) * 3)
            self.joint_positions_dev(skeleton, idx, d_f, F.shape[0], F.shape[1], d_o)
            return self.download(d_o, (F.shape[0], len(idx), 3), np.float64)

    def joint_positions_dev(self, skeleton, joint_indices, frames_dev, n_frames, n_dim, out_dev):
        """mg_joint_positions on device tables: out_dev (n_frames, len(joint_indices), 3) float64 <- frames_dev (n_frames, n_dim)
        float64; joint_indices: skeleton.indices(joints)."""
        d = skeleton.desc()
        _check(self.lib.mg_joint_positions(self.handle, C.byref(d), _host_ptr(joint_indices), len(joint_indices), _dev_ptr(frames_dev),
                                           int(n_frames), int(n_dim), _dev_ptr(out_dev)))

    def argmin_first(self, values_dev, n, dtype=np.float32):
        idx, val = C.c_int64(), C.c_double()
        ptr = values_dev.ptr if isinstance(values_dev, DeviceBuffer) else C.c_void_p(int(values_dev))
        code = MG_F64 if np.dtype(dtype) == np.float64 else MG_F32
        _check(self.lib.mg_argmin_first(self.handle, ptr, code, int(n), C.byref(idx), C.byref(val)))
        return idx.value, val.value


class DeviceBuffer(object):
    def __init__(self, ctx, nbytes, chunk_bytes=0, placed=False, max_candidates=0):
        """chunk_bytes > 0: assembled from separate physical chunks of that size (mg_device_malloc_chunked);
        placed: probed for the fast placement class (mg_device_malloc_placed)."""
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.placement = None
        p = C.c_void_p()
        if placed:
            info = (C.c_double * 4)()
            _check(ctx.lib.mg_device_malloc_placed(ctx.handle, self.nbytes, int(max_candidates), C.byref(p), info))
            self.placement = {"probed": int(info[0]), "ratio": float(info[1]), "pattern_us": float(info[2]), "fast": bool(info[3])}
        elif chunk_bytes:
            _check(ctx.lib.mg_device_malloc_chunked(ctx.handle, self.nbytes, int(chunk_bytes), C.byref(p)))
        else:
            _check(ctx.lib.mg_device_malloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p

    @property
    def address(self):
        return self.ptr.value

    def free(self):
        if getattr(self, "ptr", None) and self.ctx.handle:
            self.ctx.lib.mg_device_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffers(object):
    """The device buffers of one call (Context.buffers()): leaving the `with` block frees every buffer upload and malloc
    handed out, whether the body returned or raised, except those release() gave to the caller."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def upload(self, arr):
        self.bufs.append(self.ctx.upload(np.ascontiguousarray(arr)))
        return self.bufs[-1]

    def malloc(self, nbytes):
        self.bufs.append(self.ctx.malloc(max(int(nbytes), 8)))     # an empty table still has an address
        return self.bufs[-1]

    def release(self, buf):
        """buf outlives the block: whoever takes it frees it."""
        self.bufs.remove(buf)
        return buf

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def default_context(ctx):
    """ctx, or the process's shared context of device 0 for None."""
    if ctx is not None:
        return ctx
    from .motion_primitive import get_context
    return get_context(0)


def _dev_ptr(x):
    if isinstance(x, DeviceBuffer):
        return x.ptr
    return C.c_void_p(int(x))


def _host_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _offsets_arg(offsets):
    """An offsets table as the contiguous int64 vector the library reads."""
    return np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)


def _weights_arg(weights, n_joints):
    """Joint weights as a contiguous float64 vector of length n_joints, or None (ones)."""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != int(n_joints):
        raise ValueError("%d weights for %d joints" % (len(w), int(n_joints)))
    return w


class TimeGrid(object):
    def __init__(self, prim, times=None, handle=None):
        self.prim = prim
        self.owned = handle is None
        if handle is None:
            t = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float64)
            h = C.c_void_p()
            _check(prim.lib.mg_time_grid_create(prim.handle, t.ctypes.data_as(C.c_void_p), len(t), C.byref(h)))
            handle = h
        self.handle = handle
        self.size = prim.lib.mg_time_grid_size(self.handle)

    def tables(self):
        i0 = np.empty(self.size, dtype=np.int32)
        w = np.empty((self.size, 4))
        t = np.empty(self.size)
        _check(self.prim.lib.mg_time_grid_get_tables(self.handle, i0.ctypes.data_as(C.c_void_p),
                                                     w.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)))
        return i0, w, t

    def close(self):
        if self.owned and getattr(self, "handle", None) and self.prim.handle and self.prim.ctx.handle:
            self.prim.lib.mg_time_grid_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ConstraintSet(object):
    """constraints: list of dicts {"type": "position"|"direction"|"joint_position"|"joint_midpoint"|
    "joint_orientation"|"look_at"|"pose" ({"joints": names, "points": (N, 3), "weights": (N,), "velocity": xyz or None}), "t": float, "weight": float, "target": [x|None, y|None, z|None] | [dx, dz],
    "ref_dir": (rx, ry, rz), "joint": name or index, "joint2": second joint of a midpoint, "orientation": wanted
    global (w,x,y,z) of a joint_orientation (or "target": that orientation applied to ref_dir), "offset": a point in
    the joint's own frame instead of its origin (joint_position), "look_at": {"joint", "target" xyz}}; a `skeleton`
    (Skeleton) is needed for "joint_position", "joint_midpoint" and for orientations of joints other than the root.  `alignment` = {"joint", "position", "heading",
    "ref_dir"} (Skeleton.alignment_to) switches to global coordinates: every candidate is aligned to the previous
    motion before its constraints are evaluated; without a skeleton the aligning node is the root joint."""

    def __init__(self, prim, constraints, skeleton=None, alignment=None):
        self.prim = prim
        self.skeleton = skeleton
        self.alignment = alignment
        n = len(constraints)
        arr = self._marshal(constraints, skeleton)
        h = C.c_void_p()
        poses = [c for c in constraints if c["type"] == "pose"]
        if poses:
            if skeleton is None:
                raise ValueError("pose constraints need a skeleton")
            keep = []                                    # arrays the descriptors point at
            parr = (PoseConstraintDesc * len(poses))()
            for i, c in enumerate(poses):
                joints = np.ascontiguousarray([skeleton.index(j) for j in c["joints"]], dtype=np.int32)
                pts = np.ascontiguousarray(c["points"], dtype=np.float64).reshape(len(joints), 3)
                wts = np.ascontiguousarray(c.get("weights", np.ones(len(joints))), dtype=np.float64).reshape(len(joints))
                keep += [joints, pts, wts]
                parr[i].n_points, parr[i].has_velocity = len(joints), int(c.get("velocity") is not None)
                parr[i].joints, parr[i].points, parr[i].weights = joints.ctypes.data, pts.ctypes.data, wts.ctypes.data
                for a in range(3):
                    parr[i].velocity[a] = float(c["velocity"][a]) if c.get("velocity") is not None else 0.0
            al = self._marshal_alignment(alignment, skeleton) if alignment is not None else None
            d = skeleton.desc()
            _check(prim.lib.mg_constraint_set_create_full(prim.handle, C.byref(d), C.cast(arr, C.c_void_p), n, C.cast(parr, C.c_void_p),
                                                          len(poses), C.byref(al) if al is not None else None, C.byref(h)))
        elif alignment is not None:
            al = self._marshal_alignment(alignment, skeleton)
            d = skeleton.desc() if skeleton is not None else None
            _check(prim.lib.mg_constraint_set_create_aligned(prim.handle, C.byref(d) if d is not None else None,
                                                             C.cast(arr, C.c_void_p), n, C.byref(al), C.byref(h)))
        elif skeleton is None:
            _check(prim.lib.mg_constraint_set_create(prim.handle, C.cast(arr, C.c_void_p), n, C.byref(h)))
        else:
            d = skeleton.desc()
            _check(prim.lib.mg_constraint_set_create_fk(prim.handle, C.byref(d), C.cast(arr, C.c_void_p), n, C.byref(h)))
        self.handle = h
        self.n = n

    def update(self, constraints, alignment=None):
        """New targets / weights / previous frame for the same STRUCTURE (types, joints, keyframes, relative points,
        aligning joint): one small stream-ordered launch instead of a new set (mg_constraint_set_update)."""
        arr = self._marshal(constraints, self.skeleton)
        al = self._marshal_alignment(alignment, self.skeleton) if alignment is not None else None
        _check(self.prim.lib.mg_constraint_set_update(self.handle, C.cast(arr, C.c_void_p), len(constraints),
                                                      C.byref(al) if al is not None else None))
        self.alignment = alignment

    @staticmethod
    def _marshal_alignment(alignment, skeleton):
        al = AlignmentDesc()
        j = alignment.get("joint", 0)
        al.joint = int(j) if (skeleton is None or j == MG_ALIGN_START_POSE) else skeleton.index(j)
        for a in range(3):
            al.position[a] = float(alignment["position"][a])
            al.ref_dir[a] = float(alignment.get("ref_dir", (0.0, 0.0, 1.0))[a])
        al.heading[0], al.heading[1] = float(alignment["heading"][0]), float(alignment["heading"][1])
        return al

    @staticmethod
    def _marshal(constraints, skeleton):
        n = len(constraints)
        arr = (KeyframeConstraint * max(n, 1))()
        for i, c in enumerate(constraints):
            k = arr[i]
            k.canonical_keyframe = float(c["t"])
            k.weight_factor = float(c.get("weight", 1.0))
            if c["type"] == "position":
                k.type = MG_CONSTRAINT_POSITION
                for a in range(3):
                    v = c["target"][a]
                    k.target[a] = float("nan") if v is None else float(v)
            elif c["type"] == "joint_position":
                if skeleton is None:
                    raise ValueError("joint_position constraints need a skeleton")
                k.type = MG_CONSTRAINT_JOINT_POSITION
                k.joint = skeleton.index(c["joint"])
                for a in range(3):
                    v = c["target"][a]
                    k.target[a] = float("nan") if v is None else float(v)
                    k.ref_dir[a] = float(c["offset"][a]) if c.get("offset") is not None else 0.0   # point in the joint's frame
            elif c["type"] == "look_at":
                if skeleton is None and c.get("joint", 0) not in (0, None):
                    raise ValueError("look_at on joint %r needs a skeleton (only the root joint, 0, does not)" % (c["joint"],))
                k.type = MG_CONSTRAINT_LOOK_AT
                k.joint = 0 if skeleton is None else skeleton.index(c.get("joint", 0) or 0)
                rd = c.get("ref_dir", (0.0, 0.0, 1.0))
                for a in range(3):
                    k.target[a] = float(c["target"][a])
                    k.ref_dir[a] = float(rd[a])
            elif c["type"] == "joint_midpoint":
                if skeleton is None:
                    raise ValueError("joint_midpoint constraints need a skeleton")
                k.type = MG_CONSTRAINT_JOINT_MIDPOINT
                k.joint, k.joint2 = skeleton.index(c["joint"]), skeleton.index(c["joint2"])
                for a in range(3):
                    v = c["target"][a]
                    k.target[a] = float("nan") if v is None else float(v)
            elif c["type"] == "joint_orientation":
                k.type = MG_CONSTRAINT_JOINT_ORIENTATION
                if skeleton is None and c.get("joint", 0) not in (0, None):
                    raise ValueError("the orientation of joint %r needs a skeleton (only the root joint, 0, does not)" % (c["joint"],))
                k.joint = 0 if skeleton is None else skeleton.index(c.get("joint", 0) or 0)
                rd = c.get("ref_dir", (0.0, 0.0, 1.0))
                tv = rotate_by_quaternion(c["orientation"], rd) if "orientation" in c else c["target"]
                for a in range(3):
                    k.ref_dir[a] = float(rd[a])
                    k.target[a] = float(tv[a])
            elif c["type"] == "pose":
                k.type = MG_CONSTRAINT_POSE
                k.joint = sum(1 for q in constraints[:i] if q["type"] == "pose")   # index into the pose array
            elif c["type"] == "value_position":      # {"type", "t", "axis": 0 | 1 | 2}: the (aligned) root position's component
                k.type = MG_CONSTRAINT_VALUE_POSITION
                k.target[0] = float(int(c["axis"]))
            elif c["type"] == "value_heading":       # {"type", "t", "axis": 0 | 2, "joint", "ref_dir"}: the (aligned) unit heading's component
                k.type = MG_CONSTRAINT_VALUE_HEADING
                if skeleton is None and c.get("joint", 0) not in (0, None):
                    raise ValueError("the heading of joint %r needs a skeleton (only the root joint, 0, does not)" % (c["joint"],))
                k.joint = 0 if skeleton is None else skeleton.index(c.get("joint", 0) or 0)
                k.target[0] = float(int(c["axis"]))
                rd = c.get("ref_dir", (0.0, 0.0, 1.0))
                for a in range(3):
                    k.ref_dir[a] = float(rd[a])
            elif c["type"] == "direction":
                k.type = MG_CONSTRAINT_DIRECTION_2D
                k.target[0], k.target[1], k.target[2] = float(c["target"][0]), float(c["target"][1]), 0.0
                rd = c.get("ref_dir", (0.0, 0.0, 1.0))
                for a in range(3):
                    k.ref_dir[a] = float(rd[a])
            else:
                raise ValueError("unknown constraint type %r" % (c["type"],))
        return arr

    def close(self):
        # the C object points at its primitive and context: never touch it after either of them has been destroyed
        if getattr(self, "handle", None) and self.prim.handle and self.prim.ctx.handle:
            self.prim.lib.mg_constraint_set_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Trajectory(object):
    """A trajectory on the device for mg_score_trajectory: control_points (n, 3), the reference's TrajectoryConstraint spline
    (trajectory_constraint.py:33-38); granularity = the step of the closest-point search.  spline_type: the reference's
    SPLINE_TYPE_* (parameterized_spline.py:36-38): 0 Catmull-Rom (mg_trajectory_create, as ever), 1 B-spline, 2 fitted B-spline
    (mg_trajectory_create_typed)."""

    def __init__(self, prim, control_points, granularity=1000, spline_type=0):
        self.prim = prim
        cp = np.ascontiguousarray(np.asarray(control_points, dtype=np.float64))
        if cp.ndim != 2 or cp.shape[1] != 3:
            raise ValueError("control_points must be (n, 3)")
        h = C.c_void_p()
        if int(spline_type) == MG_SPLINE_CATMULL_ROM:
            _check(prim.lib.mg_trajectory_create(prim.handle, cp.ctypes.data_as(C.c_void_p), cp.shape[0], int(granularity), C.byref(h)))
        else:
            _check(prim.lib.mg_trajectory_create_typed(prim.handle, cp.ctypes.data_as(C.c_void_p), cp.shape[0], int(granularity), int(spline_type),
                                                       C.byref(h)))
        self.handle = h
        self.spline_type = int(spline_type)

    def tables(self):
        """mg_trajectory_tables: (poly (n_seg * 12 + 3,), relative arc lengths (granularity + 1,), full arc length) as the kernels read them"""
        n_seg, G, full = C.c_int32(), C.c_int32(), C.c_double()
        _check(self.prim.lib.mg_trajectory_tables(self.handle, None, None, C.byref(n_seg), C.byref(G), C.byref(full)))
        poly, arc = np.empty(n_seg.value * 12 + 3), np.empty(G.value + 1)
        _check(self.prim.lib.mg_trajectory_tables(self.handle, poly.ctypes.data_as(C.c_void_p), arc.ctypes.data_as(C.c_void_p), None, None, None))
        return poly, arc, full.value

    def sample_parameters(self):
        """mg_trajectory_sample_parameters: the parameters arc_length_of_points scans (u += 1.0 / granularity while u <= 1.0)"""
        n = C.c_int32()
        _check(self.prim.lib.mg_trajectory_sample_parameters(self.handle, None, C.byref(n)))
        us = np.empty(n.value)
        _check(self.prim.lib.mg_trajectory_sample_parameters(self.handle, us.ctypes.data_as(C.c_void_p), None))
        return us

    # ---- the arc-length queries (mg_trajectory_arc.hip); the _dev forms take device pointers and leave the results on the device ----
    def points_by_arc_length_dev(self, arcs_dev, n, points_dev=None, tangents_dev=None, angles_dev=None, reference_dir=None, eval_range=0.5):
        """mg_trajectory_points_by_arc_length on device arrays: arcs_dev (n) -> points_dev (n, 3), tangents_dev (n, 3), angles_dev (n),
        each optional.  Waits for the launch only when tangents or angles are asked for."""
        ref = None if reference_dir is None else (C.c_double * 2)(float(reference_dir[0]), float(reference_dir[1]))
        ptr = lambda b: _dev_ptr(b) if b is not None else None
        _check(self.prim.lib.mg_trajectory_points_by_arc_length(self.prim.handle, self.handle, ptr(arcs_dev), int(n), float(eval_range), ptr(points_dev),
                                                                ptr(tangents_dev), ptr(angles_dev), ref))

    def points_by_arc_length(self, arcs, tangents=False, reference_dir=None, eval_range=0.5):
        """ParameterizedSpline.query_point_by_absolute_arc_length for arcs (n): points (n, 3); tangents=True: (points, unit tangents
        (n, 3)) as get_tangent_at_arc_length gives them; reference_dir (2,): (points, tangents, angles in degrees (n)) as
        get_angle_at_arc_length_2d does."""
        a = np.ascontiguousarray(arcs, dtype=np.float64).reshape(-1)
        n, ctx = len(a), self.prim.ctx
        want_t, want_a = bool(tangents) or reference_dir is not None, reference_dir is not None
        if n == 0:
            out = (np.empty((0, 3)),) + ((np.empty((0, 3)),) if want_t else ()) + ((np.empty(0),) if want_a else ())
            return out if len(out) > 1 else out[0]
        with ctx.buffers() as bufs:
            d_a, d_p = bufs.upload(a), bufs.malloc(n * 24)
            d_t = bufs.malloc(n * 24) if want_t else None
            d_g = bufs.malloc(n * 8) if want_a else None
            self.points_by_arc_length_dev(d_a, n, d_p, d_t, d_g, reference_dir, eval_range)
            out = (ctx.download(d_p, (n, 3), np.float64),)
            if want_t:
                out += (ctx.download(d_t, (n, 3), np.float64),)
            if want_a:
                out += (ctx.download(d_g, (n,), np.float64),)
        return out if len(out) > 1 else out[0]

    def arc_length_of_points_dev(self, points_dev, n, arc_out_dev, min_arc_dev=None, min_point_dev=None, min_index_dev=None):
        """mg_trajectory_arc_length_of_points on device arrays: points_dev (n, 3), min_arc_dev (n) or None -> arc_out_dev (n),
        min_point_dev (n, 3) and min_index_dev (n) int32, both optional.  Asynchronous."""
        ptr = lambda b: _dev_ptr(b) if b is not None else None
        _check(self.prim.lib.mg_trajectory_arc_length_of_points(self.prim.handle, self.handle, ptr(points_dev), ptr(min_arc_dev), int(n), ptr(arc_out_dev),
                                                                ptr(min_point_dev), ptr(min_index_dev)))

    def arc_length_of_points(self, points, min_arc_length=None):
        """ParameterizedSpline.get_absolute_arc_length_of_point for points (n, 3): (arc lengths (n), the curve's points there (n, 3),
        the parameters' indices (n) int32); min_arc_length: None (0), a number or (n).  Where no parameter qualifies the arc length
        and the index are -1 and the point's row is NaN."""
        P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n, ctx = len(P), self.prim.ctx
        if n == 0:
            return np.empty(0), np.empty((0, 3)), np.empty(0, dtype=np.int32)
        with ctx.buffers() as bufs:
            d_p, d_o, d_i = bufs.upload(P), bufs.malloc(n * 8), bufs.malloc(n * 4)
            d_q = bufs.upload(np.full((n, 3), np.nan))
            d_m = None if min_arc_length is None else bufs.upload(np.ascontiguousarray(np.broadcast_to(np.asarray(min_arc_length, dtype=np.float64), (n,))))
            self.arc_length_of_points_dev(d_p, n, d_o, d_m, d_q, d_i)
            return ctx.download(d_o, (n,), np.float64), ctx.download(d_q, (n, 3), np.float64), ctx.download(d_i, (n,), np.int32)

    def points_at_parameters_dev(self, u_dev, n, points_dev, u_max_dev=None):
        """mg_trajectory_points_at_parameters on device arrays: u_dev (n), each no further than u_max_dev (n) where given -> points_dev (n, 3)"""
        _check(self.prim.lib.mg_trajectory_points_at_parameters(self.prim.handle, self.handle, _dev_ptr(u_dev), _dev_ptr(u_max_dev) if u_max_dev is not None else None,
                                                                int(n), _dev_ptr(points_dev)))

    def close(self):
        if getattr(self, "handle", None) and self.prim.handle and self.prim.ctx.handle:
            self.prim.lib.mg_trajectory_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WalkScoreStep(C.Structure):   # struct mg_walk_score_step
    _fields_ = [("prim", C.c_void_p), ("scored", C.c_void_p), ("exit", C.c_void_p), ("latent_offset", C.c_int64), ("n_own", C.c_int32),
                ("column_offset", C.c_int64)]


class WalkScoreTable(object):
    """The step table of mg_score_walk_residuals: one (primitive, scored set or None, exit set or None, latent offset, own
    columns, column offset) per step.  Holds the primitives and sets, so none of them is collected while the table is in use."""

    def __init__(self, steps):
        if not steps:
            raise ValueError("a walk has at least one step")
        self.steps = list(steps)
        self.n_steps = len(self.steps)
        self.lib, self.ctx = self.steps[0][0].lib, self.steps[0][0].ctx
        self.array = (WalkScoreStep * self.n_steps)()
        for rec, (prim, scored, exit_set, latent_offset, n_own, column_offset) in zip(self.array, self.steps):
            rec.prim = prim.handle.value
            rec.scored = scored.handle.value if scored is not None else None
            rec.exit = exit_set.handle.value if exit_set is not None else None
            rec.latent_offset, rec.n_own, rec.column_offset = int(latent_offset), int(n_own), int(column_offset)

    def sets(self):
        return [cs for st in self.steps for cs in st[1:3] if cs is not None]

    def score_dev(self, lat_dev, lat_dtype, n, ld, residuals_dev=None, ld_res=0, errors_dev=None, exit_state_dev=None, step_exits_dev=None):
        """mg_score_walk_residuals on device buffers: asynchronous on the context's stream.  step_exits_dev: (n, n_steps, 4) float64
        for the exit values of every step (mg_score_walk_residuals_steps)."""
        code = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        ptr = lambda b: _dev_ptr(b) if b is not None else None
        if step_exits_dev is None:
            _check(self.lib.mg_score_walk_residuals(self.n_steps, C.cast(self.array, C.c_void_p), ptr(lat_dev), code, int(n), int(ld), ptr(residuals_dev),
                                                    int(ld_res), ptr(errors_dev), ptr(exit_state_dev)))
        else:
            _check(self.lib.mg_score_walk_residuals_steps(self.n_steps, C.cast(self.array, C.c_void_p), ptr(lat_dev), code, int(n), int(ld),
                                                          ptr(residuals_dev), int(ld_res), ptr(errors_dev), ptr(exit_state_dev), ptr(step_exits_dev)))

    def score(self, S, ld_res, residuals=True, errors=True, exit_state=True, fill=0.0, step_exits=False):
        """(residuals (n, ld_res) or None, errors (n) or None, exit state (n, 4) or None) for host latents S
        (mg_score_walk_residuals_host); columns no step owns hold `fill`.  step_exits=True: a fourth member, the exit values of
        every step (n, n_steps, 4) (mg_score_walk_residuals_steps_host)."""
        S = _latents(S)
        n = S.shape[0]
        res = np.full((n, int(ld_res)), fill, dtype=np.float64) if residuals else None
        err = np.empty(n, dtype=np.float64) if errors else None
        ex = np.empty((n, 4), dtype=np.float64) if exit_state else None
        if not step_exits:
            _check(self.lib.mg_score_walk_residuals_host(self.n_steps, C.cast(self.array, C.c_void_p), S.ctypes.data_as(C.c_void_p), _dtype_code(S), n,
                                                         S.shape[1], _host_ptr(res), int(ld_res), _host_ptr(err), _host_ptr(ex)))
            return res, err, ex
        st = np.empty((n, self.n_steps, 4), dtype=np.float64)
        _check(self.lib.mg_score_walk_residuals_steps_host(self.n_steps, C.cast(self.array, C.c_void_p), S.ctypes.data_as(C.c_void_p), _dtype_code(S), n,
                                                           S.shape[1], _host_ptr(res), int(ld_res), _host_ptr(err), _host_ptr(ex), _host_ptr(st)))
        return res, err, ex, st


class WalkTimeStep(C.Structure):   # struct mg_walk_time_step
    _fields_ = [("prim", C.c_void_p), ("latent_offset", C.c_int64), ("spatial", C.c_void_p)]


class WalkTimeConstraint(C.Structure):   # struct mg_walk_time_constraint
    _fields_ = [("step_index", C.c_int32), ("keyframe_index", C.c_int32), ("desired_time", C.c_double)]


class WalkTimeTable(object):
    """The tables of mg_score_walk_time: per step (primitive, first column of its time latents, its n_components fixed spatial
    latents), and the constraints (step counted from the window's first step, canonical keyframe, desired time) in list order.
    The spatial latents go to the device once, in one buffer of the table's own (close() frees it); the table holds the
    primitives, so none of them is collected while it is in use."""

    def __init__(self, steps, constraints, start_keyframe, frame_time):
        if not steps:
            raise ValueError("a window has at least one step")
        self.steps = [(prim, int(off), np.ascontiguousarray(sp, dtype=np.float64)) for prim, off, sp in steps]
        self.n_steps = len(self.steps)
        self.lib, self.ctx = self.steps[0][0].lib, self.steps[0][0].ctx
        self.start_keyframe, self.frame_time = float(start_keyframe), float(frame_time)
        for prim, _, sp in self.steps:
            if sp.shape != (prim.n_components,):
                raise ValueError("a step's spatial latents must be (n_components,) = (%d,), got %r" % (prim.n_components, sp.shape))
        self.n_latents = max(off + prim.n_time_components for prim, off, _ in self.steps)
        self._spatial = self.ctx.upload(np.concatenate([sp for _, _, sp in self.steps]))
        self.array = (WalkTimeStep * self.n_steps)()
        self.host_array = (WalkTimeStep * self.n_steps)()
        at = 0
        for rec, hrec, (prim, off, sp) in zip(self.array, self.host_array, self.steps):
            rec.prim = hrec.prim = prim.handle.value
            rec.latent_offset = hrec.latent_offset = off
            rec.spatial = self._spatial.address + 8 * at
            hrec.spatial = sp.ctypes.data
            at += len(sp)
        self.constraints = [(int(s), int(k), float(t)) for s, k, t in constraints]
        self.n_constraints = len(self.constraints)
        self.carray = (WalkTimeConstraint * max(self.n_constraints, 1))()
        for rec, (s, k, t) in zip(self.carray, self.constraints):
            rec.step_index, rec.keyframe_index, rec.desired_time = s, k, t

    def close(self):
        if getattr(self, "_spatial", None) is not None:
            self._spatial.free()
        self._spatial = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def table_uploads(self):
        """How often this context's device table of steps and constraints has been (re)written."""
        n = C.c_int64()
        _check(self.lib.mg_walk_time_table_uploads(self.ctx.handle, C.byref(n)))
        return int(n.value)

    def score_dev(self, lat_dev, lat_dtype, n, ld, error_scale, quality_scale, objective_dev, error_dev=None, loglik_dev=None):
        """mg_score_walk_time on device buffers: asynchronous on the context's stream."""
        if self._spatial is None:
            raise ValueError("the table is closed")
        code = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        ptr = lambda b: _dev_ptr(b) if b is not None else None
        _check(self.lib.mg_score_walk_time(self.n_steps, C.cast(self.array, C.c_void_p), ptr(lat_dev), code, int(n), int(ld), self.n_constraints,
                                           C.cast(self.carray, C.c_void_p), self.start_keyframe, self.frame_time, float(error_scale), float(quality_scale),
                                           ptr(objective_dev), ptr(error_dev), ptr(loglik_dev)))

    def score(self, S, error_scale, quality_scale, parts=True):
        """objective (n), or (objective, error, average log-likelihood), for host latents S (mg_score_walk_time_host)."""
        S = _latents(S)
        n = S.shape[0]
        obj = np.empty(n, dtype=np.float64)
        err = np.empty(n, dtype=np.float64) if parts else None
        ll = np.empty(n, dtype=np.float64) if parts else None
        _check(self.lib.mg_score_walk_time_host(self.n_steps, C.cast(self.host_array, C.c_void_p), S.ctypes.data_as(C.c_void_p), _dtype_code(S), n, S.shape[1],
                                                self.n_constraints, C.cast(self.carray, C.c_void_p), self.start_keyframe, self.frame_time, float(error_scale),
                                                float(quality_scale), _host_ptr(obj), _host_ptr(err), _host_ptr(ll)))
        return (obj, err, ll) if parts else obj


class StepLengthItem(C.Structure):   # struct mg_step_length_item
    _fields_ = [("prim", C.c_void_p), ("latents", C.c_void_p), ("latent_offset", C.c_int64), ("n_samples", C.c_int64), ("ld", C.c_int64),
                ("arc_length", C.c_void_p), ("distance", C.c_void_p)]


def _items_call(lib, name, n_items, table, latent_dtype, host):
    """An item-table entry point on a table of its item structs as it stands: `name`_host (host pointers in the table;
    synchronises) or `name` (device pointers; asynchronous on the context's stream); table None passes NULL."""
    code = MG_F64 if np.dtype(latent_dtype) == np.float64 else MG_F32
    fn = getattr(lib, name + "_host" if host else name)
    _check(fn(int(n_items), C.cast(table, C.c_void_p) if table is not None else None, code))


def step_lengths_table(lib, n_items, table, latent_dtype, host=True):
    """mg_step_lengths_host or mg_step_lengths on a (StepLengthItem * n) table (_items_call)."""
    _items_call(lib, "mg_step_lengths", n_items, table, latent_dtype, host)


def step_lengths(items, method="both"):
    """Step lengths of every candidate of every item in one mg_step_lengths call.  items: (primitive, S) or (primitive, S,
    latent_offset) with S (n, ld) float32 or float64 latents, one dtype for the call; an item reads the n_components columns from
    latent_offset (default 0) on, and items that pass the same array share one copy of it on the device.  Per item (n,) float64:
    the ground-plane arc length of the root path over the canonical frames ("arc_length"), the distance between its first and
    last root position ("distance"), or the pair of them ("both")."""
    if method not in ("arc_length", "distance", "both"):
        raise NotImplementedError("step length method %r" % (method,))
    items = [(it[0], _latents(it[1]), int(it[2]) if len(it) > 2 else 0) for it in items]   # (_latents returns a conforming array itself)
    if not items:
        return []
    dtypes = set(S.dtype for _, S, _ in items)
    if len(dtypes) != 1:
        raise TypeError("the items of one call share a latent dtype, got %s" % sorted(str(d) for d in dtypes))
    table = (StepLengthItem * len(items))()
    out = []
    for rec, (prim, S, off) in zip(table, items):
        arc = np.empty(S.shape[0], dtype=np.float64) if method != "distance" else None
        dist = np.empty(S.shape[0], dtype=np.float64) if method != "arc_length" else None
        rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = prim.handle.value, S.ctypes.data, off, S.shape[0], S.shape[1]
        rec.arc_length = arc.ctypes.data if arc is not None else None
        rec.distance = dist.ctypes.data if dist is not None else None
        out.append((arc, dist) if method == "both" else arc if dist is None else dist)
    step_lengths_table(items[0][0].lib, len(items), table, dtypes.pop())
    return out


class FeaturePointItem(C.Structure):   # struct mg_feature_point_item
    _fields_ = [("prim", C.c_void_p), ("latents", C.c_void_p), ("latent_offset", C.c_int64), ("n_samples", C.c_int64), ("ld", C.c_int64),
                ("skeleton", C.c_void_p), ("joints", C.c_void_p), ("n_joints", C.c_int32), ("frame_idx", C.c_int32),
                ("start_root", C.c_void_p), ("points", C.c_void_p), ("root_end", C.c_void_p), ("heading_end", C.c_void_p),
                ("heading_len", C.c_void_p)]


FEATURE_POINT_OUTPUTS = ("start_root", "points", "root_end", "heading_end", "heading_len")


def feature_points_table(lib, n_items, table, latent_dtype, host=True):
    """mg_feature_points_host or mg_feature_points on a (FeaturePointItem * n) table (_items_call)."""
    _items_call(lib, "mg_feature_points", n_items, table, latent_dtype, host)


def feature_point_widths(n_joints):
    """Doubles per candidate of the five outputs, in FEATURE_POINT_OUTPUTS' order."""
    return {"start_root": 3, "points": 3 * int(n_joints), "root_end": 2, "heading_end": 2, "heading_len": 1}


def _feature_point_table(items, outputs, known, record, fill):
    """What feature_points and feature_points_warped share: the `record` table over the items' latents and joint lists, one array per
    wanted output; fill(rec, it, S, n_joints) sets the members only one of them has and returns its own outputs' {name: (shape,
    dtype)}.  Returns (table, per-item arrays, things to keep alive, latent dtype)."""
    unknown = [o for o in outputs if o not in known]
    if unknown:
        raise ValueError("unknown outputs %r" % (unknown,))
    if not items:
        return None, [], [], None
    prepared = [(it, _latents(it["S"])) for it in items]
    dtypes = set(S.dtype for _, S in prepared)
    if len(dtypes) != 1:
        raise TypeError("the items of one call share a latent dtype, got %s" % sorted(str(d) for d in dtypes))
    table = (record * len(prepared))()
    keep, out = [], []
    for rec, (it, S) in zip(table, prepared):
        sk, joints = it.get("skeleton"), it.get("joints") or []
        idx = sk.indices(joints) if joints else np.zeros(0, dtype=np.int32)
        desc = sk.desc() if sk is not None else None
        keep.append((idx, desc, sk, S))
        rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = it["prim"].handle.value, S.ctypes.data, int(it.get("latent_offset", 0)), S.shape[0], S.shape[1]
        rec.skeleton = C.addressof(desc) if desc is not None else None
        rec.joints, rec.n_joints, rec.frame_idx = (idx.ctypes.data if len(idx) else None), len(idx), int(it.get("frame_idx", 0))
        shapes = {name: ((S.shape[0], width) if name != "heading_len" else (S.shape[0],), np.float64)
                  for name, width in feature_point_widths(len(idx)).items() if width > 0}
        shapes.update(fill(rec, it, S, len(idx)))
        arrays = {}
        for name, (shape, dtype) in shapes.items():
            if name in outputs:
                arrays[name] = np.empty(shape, dtype=dtype)
                setattr(rec, name, arrays[name].ctypes.data)
        out.append(arrays)
    return table, out, keep, dtypes.pop()


def feature_points(items, outputs=FEATURE_POINT_OUTPUTS):
    """The feature points of every candidate of every item in one mg_feature_points call.  items: dicts with prim (a Primitive),
    S (n, ld) float32 or float64 latents (one dtype for the call), and optionally latent_offset (0), skeleton (a Skeleton), joints
    (names or indices, default none) and frame_idx (0).  Items that pass the same array share one copy of it on the device.  Returns
    per item a dict of float64 arrays: start_root (n, 3), points (n, 3 J; only with joints), root_end (n, 2), heading_end (n, 2),
    heading_len (n,), those of `outputs`."""
    table, out, keep, dtype = _feature_point_table(items, outputs, FEATURE_POINT_OUTPUTS, FeaturePointItem, lambda rec, it, S, n_joints: {})
    if items:
        feature_points_table(items[0]["prim"].lib, len(items), table, dtype)
    return out


class WarpedFeaturePointItem(C.Structure):   # struct mg_warped_feature_point_item
    _fields_ = FeaturePointItem._fields_ + [("time_offset", C.c_int64), ("time_mid", C.c_void_p), ("n_frames", C.c_void_p)]


WARPED_FEATURE_POINT_OUTPUTS = FEATURE_POINT_OUTPUTS + ("time_mid", "n_frames")


def feature_points_warped_table(lib, n_items, table, latent_dtype, host=True):
    """mg_feature_points_warped_host or mg_feature_points_warped on a (WarpedFeaturePointItem * n) table (_items_call)."""
    _items_call(lib, "mg_feature_points_warped", n_items, table, latent_dtype, host)


def feature_points_warped_smoothed_table(lib, n_items, table, smooth, latent_dtype, host=True):
    """mg_feature_points_warped_smoothed_host or mg_feature_points_warped_smoothed on a (WarpedFeaturePointItem * n) table; smooth:
    one flag per item (host)."""
    flags = np.ascontiguousarray(np.asarray(smooth).astype(bool), dtype=np.uint8)
    if len(flags) != int(n_items):
        raise ValueError("%d smoothing flags for %d items" % (len(flags), n_items))
    code = MG_F64 if np.dtype(latent_dtype) == np.float64 else MG_F32
    fn = getattr(lib, "mg_feature_points_warped_smoothed" + ("_host" if host else ""))
    _check(fn(int(n_items), C.cast(table, C.c_void_p) if table is not None else None, _host_ptr(flags), code))


def feature_points_warped(items, outputs=WARPED_FEATURE_POINT_OUTPUTS, smooth=None):
    """The feature points of the TIME-WARPED motion of every candidate of every item in one mg_feature_points_warped call: items as
    for feature_points, on primitives with a time model; a row of S holds the spatial latents from latent_offset on and the time
    latents from time_offset on (default: right behind the spatial ones), frame_idx counts the warped motion's frames.  Returns per
    item what feature_points returns, and time_mid (n,) float64 -- the canonical time of frame frame_idx, NaN where the candidate's
    motion is shorter -- and n_frames (n,) int32, the warped length (0: no time function).  smooth: None, or one flag per item --
    ONE mg_feature_points_warped_smoothed call instead: a flagged item's three times are those of the smoothed time function, and a
    candidate of fewer than 15 frames is NaN in every output but n_frames."""
    def fill(rec, it, S, n_joints):
        off = it.get("time_offset")
        rec.time_offset = int(off) if off is not None else int(it.get("latent_offset", 0)) + it["prim"].n_components
        return {"time_mid": ((S.shape[0],), np.float64), "n_frames": ((S.shape[0],), np.int32)}

    table, out, keep, dtype = _feature_point_table(items, outputs, WARPED_FEATURE_POINT_OUTPUTS, WarpedFeaturePointItem, fill)
    if items and smooth is not None:
        feature_points_warped_smoothed_table(items[0]["prim"].lib, len(items), table, smooth, dtype)
    elif items:
        feature_points_warped_table(items[0]["prim"].lib, len(items), table, dtype)
    return out


class FeatureMixture(object):
    """A reachability mixture as the scoring kernel reads it (mg_feature_mixture): weights (K,), means (K, dim), full covariances
    (K, dim, dim) and the log-likelihood threshold; the image -- precision Cholesky factors, mu . P, the constants -- is formed once
    on the host in float64 and, with a context, copied to its device.  ctx None and host=True: no device copy (and no device
    needed): such a mixture is scored by mixture_scores_host alone.  ctx None and host=False: the process's shared context."""

    def __init__(self, ctx, weights, means, covars, threshold=-np.inf, host=False):
        self.ctx = None if host else default_context(ctx)
        self.lib = self.ctx.lib if self.ctx is not None else load_library()
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        mu = np.ascontiguousarray(np.atleast_2d(np.asarray(means, dtype=np.float64)))
        if len(mu) != len(w):
            raise ValueError("%d weights, %d means" % (len(w), len(mu)))
        cov = np.ascontiguousarray(np.asarray(covars, dtype=np.float64).reshape(len(w), mu.shape[1], mu.shape[1]))
        self.handle = None
        h = C.c_void_p()
        _check(self.lib.mg_feature_mixture_create(self.ctx.handle if self.ctx is not None else None, len(w), mu.shape[1], _host_ptr(w), _host_ptr(mu),
                                                  _host_ptr(cov), float(threshold), C.byref(h)))
        self.handle = h
        self.n_components, self.dim, self.threshold = len(w), mu.shape[1], float(threshold)

    def image(self):
        """(prec_chol (K, dim, dim) upper triangular, mu . P (K, dim), c (K,)) as the library formed them."""
        P, m, c = np.empty((self.n_components, self.dim, self.dim)), np.empty((self.n_components, self.dim)), np.empty(self.n_components)
        _check(self.lib.mg_feature_mixture_get_image(self.handle, _host_ptr(P), _host_ptr(m), _host_ptr(c)))
        return P, m, c

    def close(self):
        if getattr(self, "handle", None) and (self.ctx is None or self.ctx.handle):
            self.lib.mg_feature_mixture_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MixtureScoreItem(C.Structure):   # struct mg_mixture_score_item
    _fields_ = [("mixture", C.c_void_p), ("targets", C.c_void_p), ("target_offset", C.c_int64), ("n_targets", C.c_int64), ("ld", C.c_int64),
                ("logp", C.c_void_p), ("wlp", C.c_void_p), ("reachable", C.c_void_p)]


MIXTURE_SCORE_OUTPUTS = ("logp", "wlp", "reachable")


def mixture_scores_table(ctx, n_items, table, host=False, lib=None):
    """mg_mixture_scores (device pointers in the table; asynchronous on the context's stream) or mg_mixture_scores_host (host
    pointers; runs on the host, ctx may be None) on a (MixtureScoreItem * n) table as it stands; table None passes NULL."""
    lib = lib or (ctx.lib if ctx is not None else load_library())
    fn = lib.mg_mixture_scores_host if host else lib.mg_mixture_scores
    _check(fn(ctx.handle if ctx is not None else None, int(n_items), C.cast(table, C.c_void_p) if table is not None else None))


def _mixture_items(items, outputs):
    """[(mixture, X (n, ld) float64 contiguous, offset)] and the per-item output arrays of a mixture_scores call."""
    unknown = [o for o in outputs if o not in MIXTURE_SCORE_OUTPUTS]
    if unknown or not outputs:
        raise ValueError("outputs %r: some of %r" % (tuple(outputs), MIXTURE_SCORE_OUTPUTS))
    prepared, out = [], []
    for it in items:
        mix, X = it[0], np.asarray(it[1], dtype=np.float64)
        X = X if X.ndim == 2 and X.flags.c_contiguous else np.ascontiguousarray(X.reshape(-1, mix.dim) if X.ndim != 2 else X)
        prepared.append((mix, X, int(it[2]) if len(it) > 2 else 0))
        shapes = {"logp": ((len(X),), np.float64), "wlp": ((len(X), mix.n_components), np.float64), "reachable": ((len(X),), np.int32)}
        out.append({name: np.empty(*shapes[name]) for name in outputs})
    return prepared, out


def _same_array(a, b):
    return a is b or (a.ctypes.data == b.ctypes.data and a.shape == b.shape and a.strides == b.strides)


def mixture_scores(items, outputs=("logp",), ctx=None):
    """Every target of every item against its mixture in ONE mg_mixture_scores launch.  items: (FeatureMixture, X) or (FeatureMixture,
    X, target_offset) with X (n, ld) float64 targets; an item reads the mixture's dim columns from target_offset (default 0) on, and
    items that pass the same array share ONE copy of it on the device.  Returns per item a dict of those of `outputs`: logp (n,)
    float64, wlp (n, K) float64 weighted log-probabilities, reachable (n,) bool: not (logp < threshold)."""
    prepared, out = _mixture_items(items, outputs)
    if not prepared:
        return out
    ctx = ctx if ctx is not None else prepared[0][0].ctx
    table = (MixtureScoreItem * len(prepared))()
    with ctx.buffers() as bufs:
        shared, devs = [], []
        for rec, (mix, X, off), arrays in zip(table, prepared, out):
            d_x = next((d for Y, d in shared if _same_array(X, Y)), None)
            if d_x is None and X.size:
                d_x = bufs.upload(X)
                shared.append((X, d_x))
            rec.mixture, rec.targets, rec.target_offset, rec.n_targets, rec.ld = mix.handle.value, (d_x.address if d_x is not None else None), off, X.shape[0], X.shape[1]
            devs.append({name: bufs.malloc(a.nbytes) for name, a in arrays.items()})
            for name, d in devs[-1].items():
                setattr(rec, name, d.address)
        mixture_scores_table(ctx, len(prepared), table)
        for arrays, dev in zip(out, devs):
            for name in arrays:
                if arrays[name].size:
                    arrays[name] = ctx.download(dev[name], arrays[name].shape, arrays[name].dtype)
    return [_mixture_outputs(arrays) for arrays in out]


def _mixture_outputs(arrays):
    if "reachable" in arrays:
        arrays["reachable"] = arrays["reachable"].astype(bool)
    return arrays


def mixture_scores_host(items, outputs=("logp",)):
    """mixture_scores by mg_mixture_scores_host: the same statements on the host, no device (the mixtures may be host-only)."""
    prepared, out = _mixture_items(items, outputs)
    if not prepared:
        return out
    table = (MixtureScoreItem * len(prepared))()
    for rec, (mix, X, off), arrays in zip(table, prepared, out):
        rec.mixture, rec.targets, rec.target_offset, rec.n_targets, rec.ld = mix.handle.value, (X.ctypes.data if X.size else None), off, X.shape[0], X.shape[1]
        for name, a in arrays.items():
            setattr(rec, name, a.ctypes.data)
    mixture_scores_table(None, len(prepared), table, host=True, lib=prepared[0][0].lib)
    return [_mixture_outputs(arrays) for arrays in out]


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


class ClusterTree(object):
    """A flattened FeatureClusterTree on the device (mg_cluster_tree_create): node 0 the root, means (n_nodes, dim), the
    children in CSR form (child_begin (n_nodes + 1), children), first_index = indices[0] per node (-1: none), n_rows rows of
    data.  It lives in the primitive's context and serves every primitive of that context whose n_components <= dim."""

    def __init__(self, prim, means, child_begin, children, first_index, n_rows):
        fi = np.ascontiguousarray(np.asarray(first_index, dtype=np.int64))
        means, n_nodes, cb, ch = self._nodes(prim, means, 0, child_begin, children)
        if n_nodes < 1 or cb.shape != (n_nodes + 1,) or fi.shape != (n_nodes,):
            raise ValueError("means (n_nodes, dim), child_begin (n_nodes + 1), first_index (n_nodes)")
        self._create("mg_cluster_tree_create", prim, n_nodes, means.shape[1], means, cb, ch, fi, int(n_rows))

    def _nodes(self, prim, rows, n_kd, child_begin, children):
        """The arrays both kinds have: the float64 table (its last rows the cluster nodes') and the children's CSR pair."""
        self.ctx, self.lib = prim.ctx, prim.lib
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64))
        self.dim = rows.shape[1] if rows.ndim == 2 else 0
        return rows, (rows.shape[0] - n_kd if rows.ndim == 2 else 0), _i32(child_begin), _i32(children)

    def _create(self, entry, prim, n_nodes, *args):
        """entry(prim, n_nodes, args..., &handle): arrays go as pointers (an empty one as NULL)."""
        h = C.c_void_p()
        args = [(a.ctypes.data_as(C.c_void_p) if a.size else None) if isinstance(a, np.ndarray) else a for a in args]
        _check(getattr(self.lib, entry)(prim.handle, n_nodes, *(args + [C.byref(h)])))
        self.handle, self.n_nodes = h, n_nodes

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.lib.mg_cluster_tree_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KdClusterTree(ClusterTree):
    """A flattened k-means / KD ClusterTree on the device (mg_cluster_tree_create_kd): points (n_kd + n_nodes, dim), the KD
    points then the cluster nodes' means; the cluster nodes' children (child_begin, children), leaf flags and KD roots
    (kd_begin, kd_roots); the KD nodes' kd_left, kd_right, kd_inner.  Searched by search_cluster_trees like ClusterTree."""

    def __init__(self, prim, points, n_kd, child_begin, children, leaf, kd_begin, kd_roots, kd_left, kd_right, kd_inner):
        n_kd = int(n_kd)
        points, n_nodes, cb, ch = self._nodes(prim, points, n_kd, child_begin, children)
        lf, kb, kr, kl, krt, ki = [_i32(a) for a in (leaf, kd_begin, kd_roots, kd_left, kd_right, kd_inner)]
        if n_nodes < 1 or cb.shape != (n_nodes + 1,) or lf.shape != (n_nodes,) or kb.shape != (n_nodes + 1,) or \
                any(a.shape != (n_kd,) for a in (kl, krt, ki)) or ch.shape != (n_nodes - 1,) or kr.shape != (int(kb[-1]),):
            raise ValueError("points (n_kd + n_nodes, dim), child_begin / kd_begin (n_nodes + 1), children (n_nodes - 1), leaf (n_nodes), "
                             "kd_roots (kd_begin[-1]), kd_left / kd_right / kd_inner (n_kd)")
        self._create("mg_cluster_tree_create_kd", prim, n_nodes, n_kd, points.shape[1], points, cb, ch, lf, kb, kr, kl, krt, ki)
        self.n_kd = n_kd


def _tree_search_handles(prims, trees, csets):
    """The handle arrays of len(prims) (Primitive, ClusterTree, ConstraintSet) triples."""
    m = len(prims)
    if not (len(trees) == m and len(csets) == m):
        raise ValueError("prims, trees and csets must have one entry per search")
    vp = C.c_void_p
    hp = (vp * max(m, 1))(*[p.handle.value for p in prims])
    ht = (vp * max(m, 1))(*[t.handle.value if t.handle else None for t in trees])
    hc = (vp * max(m, 1))(*[c.handle.value if c.handle else None for c in csets])
    return m, hp, ht, hc


def _tree_search_trajectories(m, trajectories, alignments):
    """The flat trajectory arrays of mg_cluster_tree_search_trajectories: (counts, handles, min_u, weights, alignment pointers, the
    alignment records they point to -- keep them until the call has returned)."""
    vp = C.c_void_p
    if len(trajectories) != m or (alignments is not None and len(alignments) != m):
        raise ValueError("trajectories and alignments must have one entry per search")
    flat = [t for per in trajectories for t in per]
    counts = (C.c_int32 * max(m, 1))(*[len(per) for per in trajectories])
    n = max(len(flat), 1)
    th = (vp * n)(*[t[0].handle.value if t[0] is not None and t[0].handle else None for t in flat])
    mu = (C.c_double * n)(*[float(t[1]) for t in flat])
    wt = (C.c_double * n)(*[float(t[2]) for t in flat])
    descs = [ConstraintSet._marshal_alignment(a, None) if a is not None else None for a in (alignments or [None] * m)]
    al = (vp * max(m, 1))(*[C.addressof(d) if d is not None else None for d in descs])
    return counts, th, mu, wt, al, descs


def search_cluster_trees(prims, trees, csets, n_candidates, records_dev=None, trajectories=None, alignments=None):
    """mg_cluster_tree_search for len(prims) (Primitive, ClusterTree, ConstraintSet) triples of one context: ONE launch.
    Returns the records (TREE_SEARCH_RECORD array), read back in one copy; with records_dev (a DeviceBuffer of
    len(prims) * 32 bytes) the records stay there and nothing is returned.
    trajectories: per search a list of (Trajectory | None, min_u, weight), the root trajectory constraints scored behind the
    set in list order (mg_cluster_tree_search_trajectories, the same one launch); alignments: per search the alignment dict
    the trajectories are scored under (None: local coordinates), as score_trajectory_dev takes it."""
    m, hp, ht, hc = _tree_search_handles(prims, trees, csets)
    vp = C.c_void_p
    lib = prims[0].lib if m else load_library()
    if trajectories is not None:
        counts, th, mu, wt, al, descs = _tree_search_trajectories(m, trajectories, alignments)
        if records_dev is not None:
            _check(lib.mg_cluster_tree_search_trajectories(m, hp, ht, hc, counts, th, mu, wt, al, int(n_candidates), _dev_ptr(records_dev)))
            return None
        out = np.zeros(m, dtype=TREE_SEARCH_RECORD)
        _check(lib.mg_cluster_tree_search_trajectories_host(m, hp, ht, hc, counts, th, mu, wt, al, int(n_candidates), out.ctypes.data_as(vp)))
        return out
    if records_dev is not None:
        _check(lib.mg_cluster_tree_search(m, hp, ht, hc, int(n_candidates), _dev_ptr(records_dev)))
        return None
    out = np.zeros(m, dtype=TREE_SEARCH_RECORD)
    _check(lib.mg_cluster_tree_search_host(m, hp, ht, hc, int(n_candidates), out.ctypes.data_as(vp)))
    return out


def cluster_tree_search_plan(prims, trees, csets, n_candidates, trajectories=None, alignments=None):
    """mg_cluster_tree_search_plan: what search_cluster_trees with these arguments would stage in its workgroups' LDS -- dict(lds_bytes,
    w_rows, root_rows, poly_doubles, trajectory_slots, lds_opt_in, refused).  Launches nothing."""
    m, hp, ht, hc = _tree_search_handles(prims, trees, csets)
    lib = prims[0].lib if m else load_library()
    info = TreeSearchPlanInfo()
    if trajectories is not None:
        counts, th, mu, wt, al, descs = _tree_search_trajectories(m, trajectories, alignments)
        _check(lib.mg_cluster_tree_search_plan(m, hp, ht, hc, counts, th, mu, wt, al, int(n_candidates), C.byref(info)))
    else:
        _check(lib.mg_cluster_tree_search_plan(m, hp, ht, hc, None, None, None, None, None, int(n_candidates), C.byref(info)))
    return dict(lds_bytes=int(info.lds_bytes), w_rows=int(info.w_rows), root_rows=int(info.root_rows), poly_doubles=int(info.poly_doubles),
                trajectory_slots=int(info.trajectory_slots), lds_opt_in=bool(info.lds_opt_in), refused=bool(info.refused))


def _tree_frame_lists(m, frame_lists):
    """struct mg_tree_frame_lists for m searches: frame_lists[s] is None or an object with .plan (TrackPlan), .grids (one TimeGrid or
    None per request), .descs (FrameConstraintDesc array), .req_of and .rotation_grids (one TimeGrid or None per constraint).  Returns
    (the struct, what it points to -- keep both until the call has returned)."""
    vp, R, K = C.c_void_p, MG_TRACK_MAX_REQUESTS, MG_FRAME_LIST_MAX
    if len(frame_lists) != m:
        raise ValueError("frame_lists must have one entry per search")
    plans, grids, counts = (vp * max(m, 1))(), (vp * max(m * R, 1))(), (C.c_int32 * max(m, 1))()
    cons, req, rot = (vp * max(m * K, 1))(), (C.c_int32 * max(m * K, 1))(), (vp * max(m * K, 1))()
    for s, fl in enumerate(frame_lists):
        if fl is None:
            continue
        n = len(fl.descs)
        if n > K or len(fl.grids) > R:
            raise ValueError("a search takes at most %d per-frame constraints over %d requests" % (K, R))
        plans[s], counts[s] = fl.plan.handle.value, n
        for q, g in enumerate(fl.grids):
            grids[s * R + q] = g.handle.value if g is not None else None
        for i in range(n):
            cons[s * K + i] = C.addressof(fl.descs[i])
            req[s * K + i] = int(fl.req_of[i])
            g = fl.rotation_grids[i]
            rot[s * K + i] = g.handle.value if g is not None else None
    lists = TreeFrameLists()
    keep = (plans, grids, counts, cons, req, rot)
    lists.plans, lists.grids, lists.n_constraints, lists.constraints, lists.request_of, lists.rotation_grids = [C.addressof(a) for a in keep]
    return lists, keep


def _tree_frames_arguments(prims, trees, csets, trajectories, alignments, frame_lists):
    m, hp, ht, hc = _tree_search_handles(prims, trees, csets)
    counts, th, mu, wt, al, descs = _tree_search_trajectories(m, trajectories if trajectories is not None else [[]] * m, None)
    # the alignment records: marshalled with the list's skeleton where the search has a list (its aligning joint may carry a name)
    for s, a in enumerate(alignments or [None] * m):
        if a is not None:
            fl = frame_lists[s]
            descs[s] = ConstraintSet._marshal_alignment(a, fl.skeleton if fl is not None else None)
            al[s] = C.addressof(descs[s])
    lists, keep = _tree_frame_lists(m, frame_lists)
    return m, (hp, ht, hc, counts, th, mu, wt, al, C.byref(lists)), (descs, lists, keep)


def cluster_tree_frames_plan(prims, trees, csets, n_candidates, trajectories, alignments, frame_lists):
    """mg_cluster_tree_search_frames_plan: what search_cluster_trees_frames with these arguments would stage -- the fields of
    cluster_tree_search_plan, then track_group, control_points, tables_lds, table_bytes and scratch_bytes.  Launches nothing."""
    m, args, keep = _tree_frames_arguments(prims, trees, csets, trajectories, alignments, frame_lists)
    lib = prims[0].lib if m else load_library()
    info = TreeFramesPlanInfo()
    _check(lib.mg_cluster_tree_search_frames_plan(m, *args, int(n_candidates), C.byref(info)))
    return dict(lds_bytes=int(info.lds_bytes), w_rows=int(info.w_rows), root_rows=int(info.root_rows), poly_doubles=int(info.poly_doubles),
                trajectory_slots=int(info.trajectory_slots), lds_opt_in=bool(info.lds_opt_in), refused=bool(info.refused),
                track_group=int(info.track_group), control_points=int(info.control_points), tables_lds=bool(info.tables_lds),
                table_bytes=int(info.table_bytes), scratch_bytes=int(info.scratch_bytes))


def search_cluster_trees_frames(prims, trees, csets, n_candidates, trajectories, alignments, frame_lists, scratch_dev=None):
    """mg_cluster_tree_search_frames_host: search_cluster_trees with per-frame constraint lists in the objective, ONE launch and one
    read-back.  frame_lists: per search None or its list (frame_constraints.TreeFrameList).  scratch_dev: a DeviceBuffer of at least
    cluster_tree_frames_plan(...)["scratch_bytes"]; None: sized by the plan query, allocated and freed here."""
    m, args, keep = _tree_frames_arguments(prims, trees, csets, trajectories, alignments, frame_lists)
    lib = prims[0].lib if m else load_library()
    out = np.zeros(m, dtype=TREE_SEARCH_RECORD)
    if m == 0:
        return out
    own = None
    if scratch_dev is None:
        info = TreeFramesPlanInfo()
        _check(lib.mg_cluster_tree_search_frames_plan(m, *args, int(n_candidates), C.byref(info)))
        own = scratch_dev = prims[0].ctx.malloc(max(int(info.scratch_bytes), 256))
    try:
        _check(lib.mg_cluster_tree_search_frames_host(m, *args, int(n_candidates), _dev_ptr(scratch_dev), int(scratch_dev.nbytes),
                                                      out.ctypes.data_as(C.c_void_p)))
    finally:
        if own is not None:
            own.free()
    return out


MG_KMEANS_MAX_DIM, MG_KMEANS_MAX_K, MG_KMEANS_MAX_N_INIT = 128, 64, 16   # mg_kmeans_segments (include/mg_hip.h)


def kmeans_segments(ctx, points_dev, n_rows, dim, seg_begin, rows, k, n_init=1, init=None, node_ids=None, seed=0, max_iter=300, tol=1e-4):
    """mg_kmeans_segments: k-means of every segment rows[seg_begin[s]:seg_begin[s + 1]] of the device table points_dev (n_rows, dim)
    float64.  Returns (labels per position of rows (int32), centres (n_segments, k, dim), inertia (n_segments), n_iter (n_segments))."""
    sb = np.ascontiguousarray(seg_begin, dtype=np.int64)
    r = np.ascontiguousarray(rows, dtype=np.int64)
    S = len(sb) - 1
    if S < 0 or (S > 0 and len(r) != sb[-1]):
        raise ValueError("seg_begin (n_segments + 1) must end at len(rows)")
    labels = np.zeros(max(len(r), 1), dtype=np.int32)
    centres = np.zeros((max(S, 1), int(k), int(dim)), dtype=np.float64)
    inertia = np.zeros(max(S, 1), dtype=np.float64)
    n_iter = np.zeros(max(S, 1), dtype=np.int32)
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
    if ini is not None and ini.shape != (S, int(k), int(dim)):
        raise ValueError("init must be (n_segments, k, dim)")
    ids = None if node_ids is None else np.ascontiguousarray(node_ids, dtype=np.uint64)
    if ids is not None and ids.shape != (S,):
        raise ValueError("node_ids must have one entry per segment")
    _check(ctx.lib.mg_kmeans_segments(ctx.handle, _dev_ptr(points_dev), int(n_rows), int(dim), int(max(S, 0)), _host_ptr(sb), _host_ptr(r), int(k),
                                      int(n_init), _host_ptr(ini), _host_ptr(ids), int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_iter), float(tol),
                                      _host_ptr(labels), _host_ptr(centres), _host_ptr(inertia), _host_ptr(n_iter)))
    return labels[:len(r)], centres[:S], inertia[:S], n_iter[:S]


MG_GMM_EM_MAX_DIM, MG_GMM_EM_MAX_K = 64, 64        # mg_gmm_em_fit (include/mg_hip.h)
MG_GMM_EM_CONVERGED, MG_GMM_EM_MAX_ITER, MG_GMM_EM_ILL_DEFINED = 1, 2, 3


def gmm_em_fit(ctx, points_dev, n, dim, n_comp, labels, tol=1e-3, reg_covar=1e-6, max_iter=100):
    """mg_gmm_em_fit: EM of len(n_comp) full-covariance mixtures over the device table points_dev (n, dim) float64, fit f
    from the labels labels[f] (n,).  Returns one dict per fit: weights, means, covariances, precisions_cholesky,
    lower_bounds (n_iter entries), n_iter, status, score, labels."""
    K = np.ascontiguousarray(n_comp, dtype=np.int32).reshape(-1)
    F, NC, n, dim = len(K), int(K.sum()), int(n), int(dim)
    lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(F, n) if F else np.zeros((0, n), dtype=np.int32)
    w = np.zeros(max(NC, 1))
    mu = np.zeros((max(NC, 1), dim))
    cov = np.zeros((max(NC, 1), dim, dim))
    prec = np.zeros((max(NC, 1), dim, dim))
    lbs = np.zeros((max(F, 1), int(max_iter)))
    n_iter = np.zeros(max(F, 1), dtype=np.int32)
    status = np.zeros(max(F, 1), dtype=np.int32)
    score = np.zeros(max(F, 1))
    lout = np.zeros((max(F, 1), n), dtype=np.int32)
    _check(ctx.lib.mg_gmm_em_fit(ctx.handle, _dev_ptr(points_dev), n, dim, F, _host_ptr(K) if F else None, _host_ptr(lab) if F else None, float(tol),
                                 float(reg_covar), int(max_iter), _host_ptr(w), _host_ptr(mu), _host_ptr(cov), _host_ptr(prec), _host_ptr(lbs),
                                 _host_ptr(n_iter), _host_ptr(status), _host_ptr(score), _host_ptr(lout)))
    out, c0 = [], 0
    for f in range(F):
        k = int(K[f])
        out.append({"weights": w[c0:c0 + k].copy(), "means": mu[c0:c0 + k].copy(), "covariances": cov[c0:c0 + k].copy(),
                    "precisions_cholesky": prec[c0:c0 + k].copy(), "lower_bounds": lbs[f, :n_iter[f]].copy(), "n_iter": int(n_iter[f]),
                    "status": int(status[f]), "score": float(score[f]), "labels": lout[f].copy()})
        c0 += k
    return out


MG_FPCA_MAX_BASIS, MG_FPCA_MAX_FRAMES, MG_PCA_MAX_SHORT, MG_PCA_MAX_LONG, MG_PCA_MAX_SWEEPS = 64, 1024, 4096, 1 << 20, 30   # mg_fpca.hip (include/mg_hip.h)
MG_PCA_CONVERGED, MG_PCA_SWEEP_CAP = 1, 2
MG_PCA_PROJECT_MAX_SIDE = (1 << 24) - 1


def spline_fit_batch(ctx, motions_dev, n_motions, n_frames, n_dims, operator_dev, n_basis, coeffs_dev):
    """mg_spline_fit_batch: coeffs_dev (n_motions, n_basis, n_dims) = operator (n_basis, n_frames) . motion, per motion."""
    _check(ctx.lib.mg_spline_fit_batch(ctx.handle, _dev_ptr(motions_dev), int(n_motions), int(n_frames), int(n_dims), _dev_ptr(operator_dev),
                                       int(n_basis), _dev_ptr(coeffs_dev)))


def pca_fit(ctx, a_dev, n, p, centred_dev, centre=True):
    """mg_pca_fit of the device matrix a_dev (n, p) float64; centred_dev receives a - mean (a itself with centre=False).  Returns {"mean" (p,),
    "singular_values" (min,), "vt" (min, p), "n_sweeps", "status"}."""
    n, p = int(n), int(p)
    m = max(min(n, p), 1)
    mean, sv, vt = np.zeros(max(p, 1)), np.zeros(m), np.zeros((m, max(p, 1)))
    sweeps, status = C.c_int32(0), C.c_int32(0)
    _check(ctx.lib.mg_pca_fit(ctx.handle, _dev_ptr(a_dev), n, p, 1 if centre else 0, _dev_ptr(centred_dev), _host_ptr(mean), _host_ptr(sv), _host_ptr(vt),
                              C.byref(sweeps), C.byref(status)))
    return {"mean": mean, "singular_values": sv, "vt": vt, "n_sweeps": int(sweeps.value), "status": int(status.value)}


def pca_project(ctx, x_dev, vt_dev, n, p, l, low_dev):
    """mg_pca_project: low_dev (n, l) = x_dev (n, p) . vt_dev (l, p)^T."""
    _check(ctx.lib.mg_pca_project(ctx.handle, _dev_ptr(x_dev), _dev_ptr(vt_dev), int(n), int(p), int(l), _dev_ptr(low_dev)))


def pca_backproject(ctx, low_dev, vt_dev, mean_dev, n, p, l, high_dev):
    """mg_pca_backproject: high_dev (n, p) = low_dev (n, l) . vt_dev (l, p) + mean_dev (p) (None: no mean)."""
    _check(ctx.lib.mg_pca_backproject(ctx.handle, _dev_ptr(low_dev), _dev_ptr(vt_dev), None if mean_dev is None else _dev_ptr(mean_dev),
                                      int(n), int(p), int(l), _dev_ptr(high_dev)))


MG_SFPCA_MAX_SAMPLES, MG_SFPCA_MAX_BASIS, MG_SFPCA_MAX_JOINTS = 1024, 64, 64   # mg_sfpca.hip (include/mg_hip.h)


class ScaledFPCA(object):
    """mg_sfpca_create on the device coefficients coeffs_dev (n, n_basis, n_dims) float64: the handle that scores weight vectors
    (errors) and returns the leading eigenvectors of one (projector).  skeleton: a Skeleton; joints: the int32 indices of the
    joints whose positions are compared; design: the (n_sampled_frames, n_basis) B-spline design rows at the sampled frames."""

    def __init__(self, ctx, coeffs_dev, n, n_basis, n_dims, skeleton, joints, design):
        self.ctx, self.n, self.n_weights = ctx, int(n), 3 + (int(n_dims) - 3) // 4
        design = np.ascontiguousarray(design, dtype=np.float64)
        if design.ndim != 2 or design.shape[1] != int(n_basis):
            raise ValueError("design must be (n_sampled_frames, n_basis = %d), got %s" % (n_basis, design.shape))
        joints = np.ascontiguousarray(joints, dtype=np.int32).reshape(-1)
        d = skeleton.desc()
        h = C.c_void_p()
        self.handle = None
        _check(ctx.lib.mg_sfpca_create(ctx.handle, _dev_ptr(coeffs_dev), int(n), int(n_basis), int(n_dims), C.byref(d), _host_ptr(joints), len(joints),
                                       _host_ptr(design), len(design), C.byref(h)))
        self.handle = h

    def errors(self, weights, npc):
        """mg_sfpca_errors: (errors (m,), statuses (m,)) of the weight vectors weights (m, 3 + J)."""
        w = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, dtype=np.float64)))
        errors, statuses = np.zeros(len(w)), np.zeros(len(w), dtype=np.int32)
        _check(self.ctx.lib.mg_sfpca_errors(self.handle, _host_ptr(w), len(w), w.shape[1], int(npc), _host_ptr(errors), _host_ptr(statuses)))
        return errors, statuses

    def projector(self, weights, npc):
        """mg_sfpca_projector: (u_k (n, npc), status) of one weight vector."""
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        u = np.zeros((self.n, max(int(npc), 1)))
        status = C.c_int32(0)
        _check(self.ctx.lib.mg_sfpca_projector(self.handle, _host_ptr(w), len(w), int(npc), _host_ptr(u), C.byref(status)))
        return u, int(status.value)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.mg_sfpca_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pca_fit_leading(ctx, a_dev, n, p, centred_dev, fraction, tol=0.0, max_iterations=0, k_cap=64):
    """mg_pca_fit_leading of the device matrix a_dev (n, p) float64: the leading principal components that sklearn's PCA(n_components=fraction)
    keeps, by blocked subspace iteration; centred_dev receives a - mean.  tol, max_iterations: 0 = the library's.  Returns {"mean" (p,), "k",
    "singular_values" (k,), "vt" (k, p), "ratios" (k,), "iterations", "status"}.  k_cap: room for the components at the first try; a call
    that keeps more is repeated with the count it reported."""
    n, p = int(n), int(p)
    for _ in range(2):
        k_cap = max(int(k_cap), 1)
        mean, sv, vt, ratios = np.zeros(max(p, 1)), np.zeros(k_cap), np.zeros((k_cap, max(p, 1))), np.zeros(k_cap)
        k, iters, status = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        rc = ctx.lib.mg_pca_fit_leading(ctx.handle, _dev_ptr(a_dev), n, p, float(fraction), float(tol), int(max_iterations), _dev_ptr(centred_dev),
                                        _host_ptr(mean), k_cap, C.byref(k), _host_ptr(sv), _host_ptr(vt), _host_ptr(ratios), C.byref(iters), C.byref(status))
        if rc == MG_ERR_INVALID_ARGUMENT and k.value > k_cap:
            k_cap = k.value
            continue
        _check(rc)
        kk = int(k.value)
        return {"mean": mean, "k": kk, "singular_values": sv[:kk].copy(), "vt": vt[:kk].copy(), "ratios": ratios[:kk].copy(),
                "iterations": int(iters.value), "status": int(status.value)}
    _check(rc)


def point_cloud_features_dev(prim, grid, skeleton, joint_indices, step, latents_dev, latent_dtype, n, ld, out_dev):
    """mg_point_cloud_features: out_dev (n, F, len(joint_indices), 3) float64 <- n latent rows (ld elements each, float32 or float64) of
    `prim` (a Primitive) on the device, at the F times of `grid` (a TimeGrid; None: the canonical grid); joint_indices:
    skeleton.indices(joints), or None for a NULL list.  Asynchronous on the context's stream."""
    d = skeleton.desc() if skeleton is not None else None
    code = MG_F64 if np.dtype(latent_dtype) == np.float64 else MG_F32
    _check(prim.lib.mg_point_cloud_features(prim.handle, prim._grid_handle(grid), C.byref(d) if d is not None else None, None if joint_indices is None else _host_ptr(joint_indices),
                                            0 if joint_indices is None else len(joint_indices), int(step), None if latents_dev is None else _dev_ptr(latents_dev),
                                            code, int(n), int(ld), None if out_dev is None else _dev_ptr(out_dev)))


MG_DTW_MAX_FRAMES, MG_DTW_MAX_JOINTS = 1024, 64   # mg_dtw.hip (include/mg_hip.h)


def dtw_distance_grids(ctx, ref_cloud_dev, n_ref_frames, clouds_dev, offsets, n_joints, weights, grids_dev):
    """mg_dtw_distance_grids: grids_dev <- S[n] (n_ref_frames, F_n) of every motion of the ragged cloud table clouds_dev
    (offsets[-1], n_joints, 3); offsets: (n_motions + 1) host integers; weights: (n_joints) or None (ones)."""
    off, w = _offsets_arg(offsets), _weights_arg(weights, n_joints)
    _check(ctx.lib.mg_dtw_distance_grids(ctx.handle, _dev_ptr(ref_cloud_dev), int(n_ref_frames), _dev_ptr(clouds_dev), _host_ptr(off), len(off) - 1,
                                         int(n_joints), _host_ptr(w), _dev_ptr(grids_dev)))


def dtw_paths(ctx, grids_dev, n_ref_frames, offsets, accumulated_dev, totals_dev, paths_dev, path_lengths_dev, warping_dev):
    """mg_dtw_paths: accumulated cost (accumulated_dev None: not stored), totals, paths, path lengths and warping functions
    of the grids in grids_dev; every output on the device, laid out as include/mg_hip.h says."""
    off = _offsets_arg(offsets)
    _check(ctx.lib.mg_dtw_paths(ctx.handle, _dev_ptr(grids_dev), int(n_ref_frames), _host_ptr(off), len(off) - 1,
                                None if accumulated_dev is None else _dev_ptr(accumulated_dev), _dev_ptr(totals_dev), _dev_ptr(paths_dev),
                                _dev_ptr(path_lengths_dev), _dev_ptr(warping_dev)))


def warp_motions(ctx, frames_dev, offsets, n_dim, warping_dev, n_ref_frames, warped_dev):
    """mg_warp_motions: warped_dev (n_motions, n_ref_frames, n_dim) <- rows warping_dev[n][i] of motion n's frames."""
    off = _offsets_arg(offsets)
    _check(ctx.lib.mg_warp_motions(ctx.handle, _dev_ptr(frames_dev), _host_ptr(off), len(off) - 1, int(n_dim), _dev_ptr(warping_dev), int(n_ref_frames),
                                   _dev_ptr(warped_dev)))


def dtw_pair_costs(ctx, clouds_dev, offsets, n_joints, weights, ref_indices, costs_dev):
    """mg_dtw_pair_costs: costs_dev (n_refs, n_motions) <- the total DTW cost of every motion of the ragged cloud table clouds_dev
    (offsets[-1], n_joints, 3) against the reference motions ref_indices (host integers; None: all motions in order); offsets:
    (n_motions + 1) host integers; weights: (n_joints) or None (ones).  Returns n_refs."""
    off, w = _offsets_arg(offsets), _weights_arg(weights, n_joints)
    refs = None if ref_indices is None else np.ascontiguousarray(ref_indices, dtype=np.int64).reshape(-1)
    n_refs = len(off) - 1 if refs is None else len(refs)
    _check(ctx.lib.mg_dtw_pair_costs(ctx.handle, _dev_ptr(clouds_dev), _host_ptr(off), len(off) - 1, int(n_joints), _host_ptr(w), _host_ptr(refs), n_refs,
                                     _dev_ptr(costs_dev)))
    return n_refs


MG_SEGMENT_SINGLE, MG_SEGMENT_MULTI = 0, 1             # enum mg_segment_mode (include/mg_hip.h)
MG_SEGMENT_MAX_KEYFRAMES, MG_SEGMENT_MAX_JOINTS = 8, 64   # mg_segment.hip (include/mg_hip.h)


def keyframe_distances(ctx, clouds_dev, offsets, n_joints, keyframes_dev, n_keyframes, weights, dist_dev):
    """mg_keyframe_distances: dist_dev (n_keyframes, offsets[-1]) <- the distance of every frame of the ragged cloud table
    clouds_dev (offsets[-1], n_joints, 3) to every keyframe of keyframes_dev (n_keyframes, n_joints, 3); offsets: (n_motions + 1)
    host integers; weights: (n_joints) or None (ones)."""
    off, w = _offsets_arg(offsets), _weights_arg(weights, n_joints)
    _check(ctx.lib.mg_keyframe_distances(ctx.handle, _dev_ptr(clouds_dev), _host_ptr(off), len(off) - 1, int(n_joints), _dev_ptr(keyframes_dev),
                                         int(n_keyframes), _host_ptr(w), _dev_ptr(dist_dev)))


def segment_search(ctx, start_dist_dev, end_dist_dev, offsets, mode, threshold, min_segment_size, segment_offsets, segments_dev, counts_dev):
    """mg_segment_search: the kept (start, end) int32 pairs of every motion into segments_dev (motion n's at pair
    segment_offsets[n]) and their numbers into counts_dev; offsets, segment_offsets: (n_motions + 1) host integers."""
    off, seg_off = _offsets_arg(offsets), _offsets_arg(segment_offsets)
    if len(seg_off) != len(off):
        raise ValueError("%d segment offsets for %d offsets" % (len(seg_off), len(off)))
    _check(ctx.lib.mg_segment_search(ctx.handle, _dev_ptr(start_dist_dev), _dev_ptr(end_dist_dev), _host_ptr(off), len(off) - 1, int(mode),
                                     float(threshold), int(min_segment_size), _host_ptr(seg_off), _dev_ptr(segments_dev), _dev_ptr(counts_dev)))


MG_SPATIAL_ALIGN_MAX_JOINTS, MG_SPATIAL_ALIGN_FRAMES_PER_WORKGROUP = 64, 32   # mg_spatial_align.hip


def align_motions_spatially(ctx, frames_dev, offsets, n_dim, frame_idx, ref_orientation, out_dev, transforms_dev=None):
    """mg_align_motions_spatially: out_dev (offsets[-1], n_dim) <- every motion of the ragged table frames_dev turned about y and
    moved so that its frame frame_idx faces ref_orientation (two host numbers) at the origin; transforms_dev: None, or
    (n_motions, 5) for each motion's (cos, sin, dx, dy, dz)."""
    off = _offsets_arg(offsets)
    r = np.ascontiguousarray(ref_orientation, dtype=np.float64).reshape(-1)
    if len(r) != 2:
        raise ValueError("ref_orientation has two entries (x, z)")
    _check(ctx.lib.mg_align_motions_spatially(ctx.handle, _dev_ptr(frames_dev), _host_ptr(off), len(off) - 1, int(n_dim), int(frame_idx), _host_ptr(r),
                                              _dev_ptr(out_dev), None if transforms_dev is None else _dev_ptr(transforms_dev)))


def prepare_aligned_frames(ctx, frames_dev, n_motions, n_frames, n_dim, n_joints, out_dev):
    """mg_prepare_aligned_frames: out_dev (n_motions, n_frames, n_dim) <- frames_dev with the root positions divided by their largest
    magnitudes and the first n_joints quaternions flipped into the hemisphere of frame 0 of motion 0.  Returns scale_vec (3,)."""
    scale = np.ones(3)
    _check(ctx.lib.mg_prepare_aligned_frames(ctx.handle, _dev_ptr(frames_dev), int(n_motions), int(n_frames), int(n_dim), int(n_joints), _dev_ptr(out_dev),
                                             _host_ptr(scale)))
    return scale


class TrackPlan(object):
    """What mg_joint_tracks needs that does not change between calls (mg_track_plan_create): per request its joints' chains; the
    channels to keep; the aligning node's chain.  requests: [[joint, ...], ...] (indices or names of `skeleton`), at most 4."""

    def __init__(self, prim, skeleton, requests, align_joint=0):
        self.prim, self.skeleton = prim, skeleton
        self.requests = [[skeleton.index(j) for j in r] for r in requests]
        nj = np.ascontiguousarray([len(r) for r in self.requests], dtype=np.int32)
        flat = np.ascontiguousarray([j for r in self.requests for j in r], dtype=np.int32)
        d = skeleton.desc()
        h = C.c_void_p()
        _check(prim.lib.mg_track_plan_create(prim.handle, C.byref(d), len(self.requests), nj.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p),
                                             int(align_joint), C.byref(h)))
        self.handle = h

    def tracks_dev(self, lat_dev, lat_dtype, n, ld, grids, out_devs, alignment=None):
        """grids: one TimeGrid or None (canonical) per request; out_devs: one device buffer (n, T, joints, 3) float64 per request."""
        m = len(self.requests)
        g = (C.c_void_p * m)(*[(x.handle if x is not None else None) for x in grids])
        o = (C.c_void_p * m)(*[_dev_ptr(x).value for x in out_devs])
        al = ConstraintSet._marshal_alignment(alignment, self.skeleton) if alignment is not None else None
        lc = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        _check(self.prim.lib.mg_joint_tracks(self.handle, _dev_ptr(lat_dev), lc, int(n), int(ld), C.byref(al) if al is not None else None, g, o))

    def close(self):
        if getattr(self, "handle", None) and self.prim.handle and self.prim.ctx.handle:
            self.prim.lib.mg_track_plan_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Primitive(object):
    """Device-resident constants of one motion primitive, built from the reference's JSON dict."""
    _serials = itertools.count(1)

    def __init__(self, ctx, data):
        self.serial = next(Primitive._serials)   # a stable identity for caches (id() and the handle's address can both be reused)
        self.ctx = ctx
        self.lib = ctx.lib
        eig = np.ascontiguousarray(np.asarray(data["eigen_vectors_spatial"], dtype=np.float64))
        mean = np.ascontiguousarray(np.asarray(data["mean_spatial_vector"], dtype=np.float64))
        knots = np.ascontiguousarray(np.asarray(data["b_spline_knots_spatial"], dtype=np.float64))
        tm = np.ascontiguousarray(np.asarray(data.get("translation_maxima", [1.0, 1.0, 1.0]), dtype=np.float64))
        nb, nd = int(data["n_basis_spatial"]), int(data["n_dim_spatial"])
        if eig.ndim != 2 or eig.shape[1] != nb * nd:
            raise ValueError("eigen_vectors_spatial must be (n_components, n_basis*n_dim)")
        if mean.shape != (nb * nd,) or knots.shape != (nb + 4,) or tm.shape != (3,):
            raise ValueError("mean/knots/translation_maxima have the wrong shape")
        d = PrimitiveDesc()
        d.n_basis, d.n_dim, d.n_components = nb, nd, eig.shape[0]
        d.n_canonical_frames = int(data["n_canonical_frames"])
        d.eigen_is_transposed = 0
        d.eigen_vectors = eig.ctypes.data
        d.mean_vector = mean.ctypes.data
        d.translation_maxima = tm.ctypes.data
        d.knots = knots.ctypes.data
        keep = [eig, mean, knots, tm]
        if "gmm_weights" in data and data["gmm_weights"] is not None:
            gw = np.ascontiguousarray(np.asarray(data["gmm_weights"], dtype=np.float64))
            gm = np.ascontiguousarray(np.asarray(data["gmm_means"], dtype=np.float64))
            gc = np.ascontiguousarray(np.asarray(data["gmm_covars"], dtype=np.float64))
            # the reference fits the mixture over the concatenated (spatial, time) latents: Lg >= L columns
            L = eig.shape[0]
            Lg = gm.shape[1] if gm.ndim == 2 else -1
            if gm.ndim != 2 or gm.shape[0] != len(gw) or Lg < L or gc.shape != (len(gw), Lg, Lg):
                raise ValueError("gmm_means/gmm_covars have the wrong shape")
            d.n_gmm = len(gw)
            d.n_gmm_dims = Lg
            d.gmm_weights, d.gmm_means, d.gmm_covars = gw.ctypes.data, gm.ctypes.data, gc.ctypes.data
            keep += [gw, gm, gc]
        else:
            d.n_gmm = 0
        if data.get("eigen_vectors_time") is not None:
            et = np.ascontiguousarray(np.asarray(data["eigen_vectors_time"], dtype=np.float64))
            mt = np.ascontiguousarray(np.asarray(data["mean_time_vector"], dtype=np.float64))
            kt = np.ascontiguousarray(np.asarray(data["b_spline_knots_time"], dtype=np.float64))
            nbt = int(data["n_basis_time"])
            if et.ndim != 2 or et.shape[0] != nbt or mt.shape != (nbt,) or kt.shape != (nbt + 4,):
                raise ValueError("eigen_vectors_time must be (n_basis_time, n_time_components); mean_time_vector (n_basis_time); knots (n_basis_time + 4)")
            d.n_time_components, d.n_basis_time = et.shape[1], nbt
            d.eigen_vectors_time, d.mean_time_vector, d.knots_time = et.ctypes.data, mt.ctypes.data, kt.ctypes.data
            keep += [et, mt, kt]
        h = C.c_void_p()
        _check(self.lib.mg_primitive_create(ctx.handle, C.byref(d), C.byref(h)))
        self.handle = h
        info = (C.c_int32 * 8)()
        _check(self.lib.mg_primitive_info(self.handle, info))
        (self.n_basis, self.n_dim, self.n_components, self.n_canonical_frames, self.n_gmm,
         self.kk, mfma, self.n_chunks) = [int(v) for v in info]
        self.mfma_supported = bool(mfma)
        info2 = (C.c_int32 * 4)()
        _check(self.lib.mg_primitive_info2(self.handle, info2))
        self.n_gmm_dims, self.n_time_components, self.n_basis_time, self.kk_gmm = [int(v) for v in info2]
        est = C.c_double()
        _check(self.lib.mg_primitive_root_mode(self.handle, None, C.byref(est)))
        self.root_split_estimate = float(est.value)   # the mean/delta split's error estimate (mg_primitive_root_mode)
        self.canonical_grid = TimeGrid(self, handle=C.c_void_p(self.lib.mg_primitive_canonical_grid(self.handle)))

    @property
    def root_split(self):
        """True when the float32 frames kernels compute this primitive's root channels by the mean/delta split (MG_OPT_ROOT_MODE
        2, or 3 where the accuracy gate of mg_primitive_root_mode allows it), False for the float64 pipeline (the default)."""
        split = C.c_int32()
        _check(self.lib.mg_primitive_root_mode(self.handle, C.byref(split), None))
        return bool(split.value)

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.lib.mg_primitive_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- queries -----------------------------------------------------------------------
    def precisions_cholesky(self):
        out = np.empty((self.n_gmm, self.n_gmm_dims, self.n_gmm_dims))
        _check(self.lib.mg_primitive_get_precisions_cholesky(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def score_trajectory_dev(self, trajectory, lat_dev, lat_dtype, n, ld, errors_dev, min_u=0.0, weight=1.0, alignment=None,
                             accumulate=False, residuals_dev=None, grid=None):
        """mg_score_trajectory on device buffers: errors_dev (n) float64 written or added to."""
        al = ConstraintSet._marshal_alignment(alignment, None) if alignment is not None else None
        code = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        _check(self.lib.mg_score_trajectory(self.handle, trajectory.handle, self._grid_handle(grid), _dev_ptr(lat_dev), code, int(n), int(ld),
                                            float(min_u), float(weight), C.byref(al) if al is not None else None, _dev_ptr(errors_dev),
                                            1 if accumulate else 0, _dev_ptr(residuals_dev) if residuals_dev is not None else None))

    def score_trajectory_chained_dev(self, trajectory, lat_dev, lat_dtype, n, ld, align_cand_dev, template, errors_dev, min_u=0.0, weight=1.0,
                                     accumulate=False, residuals_dev=None, grid=None):
        """mg_score_trajectory_chained on device buffers: align_cand_dev (n, 4) float64, every candidate's previous unit heading (x, z)
        and root position (x, z); template: the previous-frame record whose node and ref_dir are used."""
        al = ConstraintSet._marshal_alignment(template, None) if template is not None else None
        code = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        _check(self.lib.mg_score_trajectory_chained(self.handle, trajectory.handle, self._grid_handle(grid), _dev_ptr(lat_dev), code, int(n), int(ld),
                                                    float(min_u), float(weight), C.byref(al) if al is not None else None,
                                                    _dev_ptr(align_cand_dev) if align_cand_dev is not None else None, _dev_ptr(errors_dev),
                                                    1 if accumulate else 0, _dev_ptr(residuals_dev) if residuals_dev is not None else None))

    def score_trajectory_chained(self, trajectory, S, align_cand, template, min_u=0.0, weight=1.0, residuals=False, grid=None):
        """score_trajectory with every sample aligned to ITS OWN previous motion: align_cand (n, 4) as in
        score_constraint_residuals_chained."""
        S = _latents(S)
        A = np.ascontiguousarray(align_cand, dtype=np.float64)
        assert A.shape == (S.shape[0], 4)
        n, T = S.shape[0], self._grid_size(grid)
        d_S, d_A, d_e = self.ctx.upload(S), self.ctx.upload(A), self.ctx.malloc(max(n, 1) * 8)
        d_r = self.ctx.malloc(max(n * T, 1) * 8) if residuals else None
        try:
            self.score_trajectory_chained_dev(trajectory, d_S, S.dtype, n, S.shape[1], d_A, template, d_e, min_u, weight, False, d_r, grid)
            err = self.ctx.download(d_e, (n,), np.float64)
            return (err, self.ctx.download(d_r, (n, T), np.float64)) if residuals else err
        finally:
            for b in (d_S, d_A, d_e, d_r):
                if b is not None:
                    b.free()

    @staticmethod
    def score_trajectories_dev(prims, trajectories, lat_devs, lat_dtype, n, lds, err_devs, min_us, weights, alignments=None, accumulate=False):
        """mg_score_trajectories: the k-th primitive's n resident candidates against the k-th trajectory, all in one launch (primitives of
        one context); err_devs[k] (n,) float64 written or added to."""
        m = len(prims)
        vp = C.c_void_p
        keep = [ConstraintSet._marshal_alignment(a, None) if a is not None else None for a in (alignments or [None] * m)]
        al = (vp * m)(*[(C.addressof(a) if a is not None else None) for a in keep]) if alignments is not None else None
        code = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        _check(prims[0].lib.mg_score_trajectories(m, (vp * m)(*[p.handle.value for p in prims]), (vp * m)(*[t.handle.value for t in trajectories]),
                                                  (vp * m)(*[_dev_ptr(x).value for x in lat_devs]), code, int(n), (C.c_int64 * m)(*[int(x) for x in lds]),
                                                  (C.c_double * m)(*[float(x) for x in min_us]), (C.c_double * m)(*[float(x) for x in weights]), al,
                                                  (vp * m)(*[_dev_ptr(x).value for x in err_devs]), 1 if accumulate else 0))

    def score_trajectory(self, trajectory, S, min_u=0.0, weight=1.0, alignment=None, residuals=False, grid=None):
        """(n,) float64 errors = weight * average distance of the root path to the trajectory; with residuals=True also
        the (n, T) per-sample residuals (TrajectoryConstraint.get_residual_vector times the weight)."""
        S = _latents(S)
        n, T = S.shape[0], self._grid_size(grid)
        d_S, d_e = self.ctx.upload(S), self.ctx.malloc(max(n, 1) * 8)
        d_r = self.ctx.malloc(max(n * T, 1) * 8) if residuals else None
        try:
            self.score_trajectory_dev(trajectory, d_S, S.dtype, n, S.shape[1], d_e, min_u, weight, alignment, False, d_r, grid)
            err = self.ctx.download(d_e, (n,), np.float64)
            return (err, self.ctx.download(d_r, (n, T), np.float64)) if residuals else err
        finally:
            for b in (d_S, d_e, d_r):
                if b is not None:
                    b.free()

    def joint_tracks(self, skeleton, joints, S, grid=None):
        """(B, T, len(joints), 3) float64: the global positions of `joints` in every frame of every sample's motion -- float64
        back projection (mg_back_project_frames_f64) and forward kinematics (mg_joint_positions) on the device, only the
        tracks come back.  What the per-frame constraints of the reference walk a motion for (trajectory constraints on other
        joints than the root, collision avoidance, local and discrete trajectories)."""
        S = _latents(S)
        n, T = S.shape[0], self._grid_size(grid)
        idx = np.ascontiguousarray([skeleton.index(j) for j in joints], dtype=np.int32)
        ctx = self.ctx
        d_S = ctx.upload(S)
        d_f = ctx.malloc(max(n * T * self.n_dim, 1) * 8)
        d_o = ctx.malloc(max(n * T * len(idx) * 3, 1) * 8)
        try:
            _check(self.lib.mg_back_project_frames_f64(self.handle, self._grid_handle(grid), d_S.ptr, _dtype_code(S), n, S.shape[1], d_f.ptr))
            d = skeleton.desc()
            _check(self.lib.mg_joint_positions(ctx.handle, C.byref(d), idx.ctypes.data_as(C.c_void_p), len(idx), d_f.ptr, n * T, self.n_dim, d_o.ptr))
            return ctx.download(d_o, (n, T, len(idx), 3), np.float64)
        finally:
            for b in (d_S, d_f, d_o):
                b.free()

    def trajectory_closest_points(self, trajectory, points, min_u=0.0, evaluations=False):
        """mg_trajectory_closest_points: points (n, T, 3) float64 -> (parameters (n, T), distances (n, T)): the reference's
        find_closest_point_fast chained frame to frame (trajectory_constraint.py:103-113) for every row; evaluations: also the
        (f, g) evaluations every search took (n, T) int32."""
        P = np.ascontiguousarray(points, dtype=np.float64)
        n, T = P.shape[0], P.shape[1]
        ctx = self.ctx
        d_p, d_u, d_d = ctx.upload(P), ctx.malloc(max(n * T, 1) * 8), ctx.malloc(max(n * T, 1) * 8)
        d_n = ctx.malloc(max(n * T, 1) * 4) if evaluations else None
        try:
            if d_n is not None:
                _check(self.lib.mg_memset(ctx.handle, d_n.ptr, 0, max(n * T, 1) * 4))
            _check(self.lib.mg_trajectory_closest_points(self.handle, trajectory.handle, d_p.ptr, n, T, float(min_u), d_u.ptr, d_d.ptr,
                                                         d_n.ptr if d_n is not None else None))
            out = (ctx.download(d_u, (n, T), np.float64), ctx.download(d_d, (n, T), np.float64))
            return out + (ctx.download(d_n, (n, T), np.int32),) if evaluations else out
        finally:
            for b in (d_p, d_u, d_d, d_n):
                if b is not None:
                    b.free()

    def score_trajectory_points(self, trajectory, points, min_u=0.0, weight=1.0, residuals=False):
        """mg_score_trajectory_points: points (n, T, 3) float64 followed along the trajectory instead of the root path."""
        P = np.ascontiguousarray(points, dtype=np.float64)
        n, T = P.shape[0], P.shape[1]
        ctx = self.ctx
        d_p, d_e = ctx.upload(P), ctx.malloc(max(n, 1) * 8)
        d_r = ctx.malloc(max(n * T, 1) * 8) if residuals else None
        try:
            _check(self.lib.mg_score_trajectory_points(self.handle, trajectory.handle, d_p.ptr, n, T, float(min_u), float(weight), d_e.ptr, 0,
                                                       d_r.ptr if d_r is not None else None))
            err = ctx.download(d_e, (n,), np.float64)
            return (err, ctx.download(d_r, (n, T), np.float64)) if residuals else err
        finally:
            for b in (d_p, d_e, d_r):
                if b is not None:
                    b.free()

    def time_function_canonical(self, gamma):
        """(B, n_time_components) time latents -> (B, n_canonical_frames) float64: the reference's
        _back_transform_gamma_to_canonical_time_function (motion_primitive.py:289-302) for every row."""
        G = _latents(gamma)
        out = np.empty((G.shape[0], self.n_canonical_frames), dtype=np.float64)
        _check(self.lib.mg_time_function_canonical_host(self.handle, G.ctypes.data_as(C.c_void_p), _dtype_code(G), G.shape[0], G.shape[1],
                                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def time_function_sample(self, gamma, speed=1.0, t_cap=None, with_canonical=False, smoothed=False):
        """(B, n_time_components) time latents -> (times (B, t_cap) float64 padded with NaN, lengths (B)): the spline's time function
        t'(t) of every row (mg_time_function_sample: back_project_time_function, motion_primitive.py:268-319, for the batch).
        smoothed: mg_time_function_sample_smoothed, the rows after the Savitzky-Golay pass (a row of 0 < T < 15 samples reports T
        and stays NaN)."""
        sample = self.lib.mg_time_function_sample_smoothed if smoothed else self.lib.mg_time_function_sample
        G = _latents(gamma)
        B, F = G.shape[0], self.n_canonical_frames
        ctx = self.ctx
        cap = int(t_cap) if t_cap is not None else int(4 * F / min(float(speed), 1.0)) + 8
        while True:
            d_g, d_t, d_l = ctx.upload(G), ctx.malloc(max(B, 1) * cap * 8), ctx.malloc(max(B, 1) * 4)
            d_c = ctx.malloc(max(B, 1) * F * 8) if with_canonical else None
            try:
                _check(self.lib.mg_memset(ctx.handle, d_t.ptr, 0xff, max(B, 1) * cap * 8))      # NaN padding
                _check(sample(self.handle, d_g.ptr, _dtype_code(G), B, G.shape[1], float(speed), d_t.ptr, d_l.ptr, cap, d_c.ptr if d_c is not None else None))
                lens = ctx.download(d_l, (B,), np.int32)
                if B and lens.min() < 0 and t_cap is None:      # a row needs more samples than assumed: once more with room for it
                    cap = int(-lens.min()) + 8
                    continue
                times = ctx.download(d_t, (B, cap), np.float64)
                canonical = ctx.download(d_c, (B, F), np.float64) if d_c is not None else None
            finally:
                for b in (d_g, d_t, d_l, d_c):
                    if b is not None:
                        b.free()
            return (times, lens, canonical) if with_canonical else (times, lens)

    def back_project_warped_smoothed(self, S, n_spatial, speed=1.0, dtype=np.float64):
        """(B, n_spatial + n_time) latents -> (frames (B, t_max, D) padded with NaN, lengths (B), times (B, t_max) padded with NaN): the
        SMOOTHED time function of every row (mg_time_function_sample_smoothed on the time columns) and the frames at it
        (mg_back_project_frames_at on the spatial columns), the times never leaving the device in between: the lengths come back
        (the sampling launch runs again only where a row needs more samples than 4 F + 8), a row of fewer than
        15 samples raises ValueError as scipy would, then the frames launch reads the rows where the sampler left them."""
        from .time_smoothing import require_smoothing_window
        S = _latents(S)
        B, F, ctx = S.shape[0], self.n_canonical_frames, self.ctx
        item = np.dtype(dtype).itemsize
        cap = int(4 * F / min(float(speed), 1.0)) + 8
        off = n_spatial * S.dtype.itemsize
        with ctx.buffers() as bufs:
            d_s, d_l = bufs.upload(S), bufs.malloc(max(B, 1) * 4)
            while True:
                d_t = bufs.malloc(max(B, 1) * cap * 8)
                _check(self.lib.mg_memset(ctx.handle, d_t.ptr, 0xff, max(B, 1) * cap * 8))      # NaN padding
                _check(self.lib.mg_time_function_sample_smoothed(self.handle, C.c_void_p(d_s.address + off), _dtype_code(S), B, S.shape[1], float(speed),
                                                                 d_t.ptr, d_l.ptr, cap, None))
                lens = ctx.download(d_l, (B,), np.int32)
                if not B or lens.min() >= 0:
                    break
                cap = int(-lens.min()) + 8                                                      # a row needs more samples than assumed: once more
            require_smoothing_window(lens, "candidate %d")
            d_o = bufs.malloc(max(B, 1) * cap * self.n_dim * item)
            _check(self.lib.mg_memset(ctx.handle, d_o.ptr, 0xff, max(B, 1) * cap * self.n_dim * item))
            _check(self.lib.mg_back_project_frames_at(self.handle, d_s.ptr, _dtype_code(S), B, S.shape[1], d_t.ptr, d_l.ptr, cap, d_o.ptr,
                                                      MG_F64 if np.dtype(dtype) == np.float64 else MG_F32))
            t_top = int(lens.max()) if B else 0
            frames = ctx.download(d_o, (B, cap, self.n_dim), dtype)[:, :t_top]
            times = ctx.download(d_t, (B, cap), np.float64)[:, :t_top]
        return frames, lens, np.ascontiguousarray(times)

    def back_project_frames_at(self, S, times, lengths=None, dtype=np.float64):
        """(B, ld) latents, (B, t_cap) float64 times, (B) lengths -> (B, t_cap, D) frames of every candidate at ITS OWN times
        (mg_back_project_frames_at); samples beyond a row's length are NaN."""
        S = _latents(S)
        times = np.ascontiguousarray(times, dtype=np.float64)
        B, cap = times.shape
        if S.shape[0] != B:
            raise ValueError("one row of times per candidate")
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        item = np.dtype(dtype).itemsize
        ctx = self.ctx
        d_s, d_t, d_o = ctx.upload(S), ctx.upload(np.where(np.isnan(times), 0.0, times)), ctx.malloc(max(B, 1) * cap * self.n_dim * item)
        d_l = ctx.upload(lens) if lens is not None else None
        try:
            _check(self.lib.mg_memset(ctx.handle, d_o.ptr, 0xff, max(B, 1) * cap * self.n_dim * item))
            _check(self.lib.mg_back_project_frames_at(self.handle, d_s.ptr, _dtype_code(S), B, S.shape[1], d_t.ptr, d_l.ptr if d_l is not None else None, cap,
                                                      d_o.ptr, MG_F64 if np.dtype(dtype) == np.float64 else MG_F32))
            return ctx.download(d_o, (B, cap, self.n_dim), dtype)
        finally:
            for b in (d_s, d_t, d_o, d_l):
                if b is not None:
                    b.free()

    def time_grid(self, times):
        return TimeGrid(self, times)

    def _grid_handle(self, grid):
        return None if grid is None else grid.handle

    def _grid_size(self, grid):
        return self.canonical_grid.size if grid is None else grid.size

    # ---- host-array entry points (upload, launch, download) -------------------------------
    def back_project_frames(self, S, grid=None, path=MG_PATH_AUTO):
        S = _latents(S)
        out = np.empty((S.shape[0], self._grid_size(grid), self.n_dim), dtype=np.float32)
        _check(self.lib.mg_back_project_frames_host(self.handle, self._grid_handle(grid), S.ctypes.data_as(C.c_void_p),
                                                    _dtype_code(S), S.shape[0], S.shape[1],
                                                    out.ctypes.data_as(C.c_void_p), path))
        return out

    def back_project_frames_f64(self, S, grid=None):
        S = _latents(S)
        out = np.empty((S.shape[0], self._grid_size(grid), self.n_dim), dtype=np.float64)
        _check(self.lib.mg_back_project_frames_f64_host(self.handle, self._grid_handle(grid), S.ctypes.data_as(C.c_void_p),
                                                        _dtype_code(S), S.shape[0], S.shape[1],
                                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def step_lengths(self, S, method="arc_length"):
        """(n,) float64 step lengths of the rows of S (n, ld >= n_components; the first n_components columns are read) without
        frames in memory (mg_step_lengths): "arc_length", "distance", or "both" = (arc_length, distance)."""
        return step_lengths([(self, S)], method)[0]

    def back_project_coeffs(self, S, dtype=np.float64):
        S = _latents(S)
        out = np.empty((S.shape[0], self.n_basis, self.n_dim), dtype=dtype)
        _check(self.lib.mg_back_project_coeffs_host(self.handle, S.ctypes.data_as(C.c_void_p), _dtype_code(S),
                                                    S.shape[0], S.shape[1], out.ctypes.data_as(C.c_void_p),
                                                    _dtype_code(out)))
        return out

    def spline_evaluate(self, coeffs, grid=None):
        c = np.ascontiguousarray(coeffs, dtype=np.float64)
        if c.ndim == 2:
            c = c.reshape(1, c.shape[0], c.shape[1])
        if c.shape[1:] != (self.n_basis, self.n_dim):
            raise ValueError("coeffs must be (n, %d, %d)" % (self.n_basis, self.n_dim))
        out = np.empty((c.shape[0], self._grid_size(grid), self.n_dim), dtype=np.float64)
        _check(self.lib.mg_spline_evaluate_host(self.handle, self._grid_handle(grid), c.ctypes.data_as(C.c_void_p),
                                                c.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def gmm_log_prob(self, X, dtype=np.float64):
        X = _latents(X)
        out = np.empty(X.shape[0], dtype=dtype)
        _check(self.lib.mg_gmm_log_prob_host(self.handle, X.ctypes.data_as(C.c_void_p), _dtype_code(X), X.shape[0],
                                             X.shape[1], out.ctypes.data_as(C.c_void_p), _dtype_code(out)))
        return out

    def gmm_sample(self, counts, seed, dtype=np.float64):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        n = int(counts.sum())
        X = np.empty((n, self.n_gmm_dims), dtype=dtype)
        comp = np.empty(n, dtype=np.int32)
        _check(self.lib.mg_gmm_sample_host(self.handle, n, counts.ctypes.data_as(C.c_void_p), C.c_uint64(int(seed)),
                                           X.ctypes.data_as(C.c_void_p), _dtype_code(X), self.n_gmm_dims,
                                           comp.ctypes.data_as(C.c_void_p)))
        return X, comp

    def score_constraints(self, cset, S, dtype=np.float64):
        S = _latents(S)
        out = np.empty(S.shape[0], dtype=dtype)
        _check(self.lib.mg_score_constraints_host(self.handle, cset.handle, S.ctypes.data_as(C.c_void_p), _dtype_code(S),
                                                  S.shape[0], S.shape[1], out.ctypes.data_as(C.c_void_p),
                                                  _dtype_code(out)))
        return out

    def best_candidate(self, cset, S):
        """(best_index, min_error) of the reference's candidate loop (first minimum) for host latents S."""
        S = _latents(S)
        idx, val = C.c_int64(), C.c_double()
        _check(self.lib.mg_best_candidate_host(self.handle, cset.handle, S.ctypes.data_as(C.c_void_p), _dtype_code(S),
                                               S.shape[0], S.shape[1], C.byref(idx), C.byref(val)))
        return idx.value, val.value

    def best_candidate_dev(self, cset, lat_dev, lat_dtype, n, ld):
        lc = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        idx, val = C.c_int64(), C.c_double()
        _check(self.lib.mg_best_candidate(self.handle, cset.handle, _dev_ptr(lat_dev), lc, int(n), int(ld),
                                          C.byref(idx), C.byref(val)))
        return idx.value, val.value

    def score_constraint_residuals(self, cset, S):
        """(n_samples, n_constraints) float64: weight_c * error_c per sample (get_residual_vector, batched)."""
        S = _latents(S)
        out = np.empty((S.shape[0], cset.n), dtype=np.float64)
        _check(self.lib.mg_score_constraint_residuals_host(self.handle, cset.handle, S.ctypes.data_as(C.c_void_p),
                                                           _dtype_code(S), S.shape[0], S.shape[1],
                                                           out.ctypes.data_as(C.c_void_p)))
        return out

    def score_constraint_residuals_chained(self, cset, S, align_cand):
        """The same matrix with every sample aligned to ITS OWN previous motion: align_cand (n, 4) = previous unit heading
        (x, z) and previous root position (x, z) per sample (mg_score_constraint_residuals_chained)."""
        S = _latents(S)
        A = np.ascontiguousarray(align_cand, dtype=np.float64)
        assert A.shape == (S.shape[0], 4)
        ctx = self.ctx
        d_S, d_A, d_R = ctx.upload(S), ctx.upload(A), ctx.malloc(max(S.shape[0] * cset.n, 1) * 8)
        try:
            _check(self.lib.mg_score_constraint_residuals_chained(self.handle, cset.handle, d_S.ptr, _dtype_code(S), S.shape[0], S.shape[1],
                                                                  d_A.ptr, d_R.ptr))
            return ctx.download(d_R, (S.shape[0], cset.n), np.float64)
        finally:
            for b in (d_S, d_A, d_R):
                b.free()

    def gmm_log_prob_jac(self, X):
        """(n_samples, n_components) float64: the reference's log_likelihood_jac (= -grad log p) per row."""
        X = _latents(X)
        out = np.empty((X.shape[0], self.n_gmm_dims), dtype=np.float64)
        _check(self.lib.mg_gmm_log_prob_jac_host(self.handle, X.ctypes.data_as(C.c_void_p), _dtype_code(X), X.shape[0],
                                                 X.shape[1], out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- device-pointer entry points (no copies, asynchronous on the context stream) ----------
    def back_project_frames_dev(self, lat_dev, lat_dtype, n, ld, frames_dev, grid=None, path=MG_PATH_AUTO):
        code = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        _check(self.lib.mg_back_project_frames(self.handle, self._grid_handle(grid), _dev_ptr(lat_dev), code,
                                               int(n), int(ld), _dev_ptr(frames_dev), path))

    def gmm_log_prob_dev(self, x_dev, x_dtype, n, ld, out_dev, out_dtype=np.float32):
        xc = MG_F64 if np.dtype(x_dtype) == np.float64 else MG_F32
        oc = MG_F64 if np.dtype(out_dtype) == np.float64 else MG_F32
        _check(self.lib.mg_gmm_log_prob(self.handle, _dev_ptr(x_dev), xc, int(n), int(ld), _dev_ptr(out_dev), oc))

    def gmm_sample_dev(self, counts, seed, x_dev, x_dtype, ld, component_dev=None, rows=None):
        """Device Philox sampler into device memory: rows grouped by component like sklearn's sample().
        rows = (begin, count): only those rows of the draw (mg_gmm_sample_rows), x_dev (count, ld)."""
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        xc = MG_F64 if np.dtype(x_dtype) == np.float64 else MG_F32
        comp = _dev_ptr(component_dev) if component_dev is not None else C.c_void_p(0)
        n = int(counts.sum())
        begin, count = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        _check(self.lib.mg_gmm_sample_rows(self.handle, n, counts.ctypes.data_as(C.c_void_p), C.c_uint64(int(seed)), begin, count,
                                           _dev_ptr(x_dev), xc, int(ld), comp))

    def objective_dev(self, cset, lat_dev, lat_dtype, n, ld, error_scale, quality_scale, obj_dev=None, err_dev=None, logp_dev=None):
        """error_scale * constraint error + quality_scale * (-log p) of n device-resident candidates in one launch
        (mg_objective_error_and_naturalness); outputs float64 device buffers, any of them None."""
        lc = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        ptr = lambda b: _dev_ptr(b) if b is not None else None
        _check(self.lib.mg_objective_error_and_naturalness(self.handle, cset.handle, _dev_ptr(lat_dev), lc, int(n), int(ld), float(error_scale),
                                                           float(quality_scale), ptr(logp_dev), ptr(err_dev), ptr(obj_dev)))

    def objective(self, cset, S, error_scale, quality_scale):
        """(objective, errors, log p) for host latents S (n, >= n_gmm_dims); raises MGError(-4) where the one-launch kernel does
        not carry the set."""
        S = _latents(S)
        n = S.shape[0]
        ctx = self.ctx
        d_S, bufs = ctx.upload(S), [ctx.malloc(max(n, 1) * 8) for _ in range(3)]
        try:
            self.objective_dev(cset, d_S, S.dtype, n, S.shape[1], error_scale, quality_scale, bufs[0], bufs[1], bufs[2])
            return tuple(ctx.download(b, (n,), np.float64) for b in bufs)
        finally:
            for b in [d_S] + bufs:
                b.free()

    def score_plan(self, cset, n):
        """mg_score_plan: what the keyframe scorers launch for n candidates against cset under the context's options -- dict(kernel
        "valu" | "tile" | "wide", lds_bytes, lds_opt_in, workgroups, rows, row_tiles); launches nothing.  MGError (MG_ERR_UNSUPPORTED)
        where mg_score_constraints raises it."""
        info = ScorePlanInfo()
        _check(self.lib.mg_score_plan(self.handle, cset.handle, int(n), C.byref(info)))
        return {"kernel": MG_SCORE_KERNELS[info.kernel], "lds_bytes": int(info.lds_bytes), "lds_opt_in": bool(info.lds_opt_in),
                "workgroups": int(info.workgroups), "rows": int(info.rows), "row_tiles": int(info.row_tiles)}

    def score_constraint_residuals_dev(self, cset, lat_dev, lat_dtype, n, ld, res_dev, align_cand_dev=None):
        """mg_score_constraint_residuals on device pointers: res_dev (n, cset.n) float64; align_cand_dev (n, 4) float64: the chained
        form (mg_score_constraint_residuals_chained)."""
        lc = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        if align_cand_dev is None:
            _check(self.lib.mg_score_constraint_residuals(self.handle, cset.handle, _dev_ptr(lat_dev), lc, int(n), int(ld), _dev_ptr(res_dev)))
        else:
            _check(self.lib.mg_score_constraint_residuals_chained(self.handle, cset.handle, _dev_ptr(lat_dev), lc, int(n), int(ld),
                                                                  _dev_ptr(align_cand_dev), _dev_ptr(res_dev)))

    def score_constraints_dev(self, cset, lat_dev, lat_dtype, n, ld, out_dev, out_dtype=np.float64):
        lc = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        oc = MG_F64 if np.dtype(out_dtype) == np.float64 else MG_F32
        _check(self.lib.mg_score_constraints(self.handle, cset.handle, _dev_ptr(lat_dev), lc, int(n), int(ld),
                                             _dev_ptr(out_dev), oc))

    FRAMES_KERNEL_NAMES = ("mg_frames_direct_kernel", "mg_frames_ws_kernel", "mg_frames_cs_kernel")

    def step_plan(self, n, frames_dev=None, dtype=np.float32):
        """What step_frames_and_logp_dev launches for n candidates of latent dtype `dtype` (into frames_dev, when given: slow-class
        pieces of the output arena get the tile-major kernel): dict(kernel, fused, workgroups, lds_bytes)."""
        plan = (C.c_int32 * 4)()
        code = MG_F64 if np.dtype(dtype) == np.float64 else MG_F32
        _check(self.lib.mg_step_plan_dtype(self.handle, int(n), _dev_ptr(frames_dev) if frames_dev is not None else None, code, plan))
        return dict(kernel=self.FRAMES_KERNEL_NAMES[plan[0]], fused=bool(plan[1]), workgroups=int(plan[2]), lds_bytes=int(plan[3]))

    def step_frames_and_logp_dev(self, lat_dev, lat_dtype, n, ld, frames_dev, logp_dev):
        code = MG_F64 if np.dtype(lat_dtype) == np.float64 else MG_F32
        _check(self.lib.mg_step_frames_and_logp(self.handle, _dev_ptr(lat_dev), code, int(n), int(ld),
                                                _dev_ptr(frames_dev), _dev_ptr(logp_dev)))
