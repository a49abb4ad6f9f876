/* mg_hip.h -- C ABI of the MI355X (gfx950) motion-primitive back-projection /
 * GMM-scoring library (libmg_hip.so).
 *
 * The reference (dfki-asr/morphablegraphs) is 100 % Python and has no FFI; the
 * seam this library sits behind is the duck-typed attribute
 * MotionPrimitiveModelWrapper.motion_primitive
 * (reference morphablegraphs/motion_model/motion_primitive_wrapper.py:49-53,61-85)
 * and the batched scoring seam MotionPrimitiveGenerator.evaluate_samples_using_constraints
 * (reference morphablegraphs/motion_generator/motion_primitive_generator.py:230-261).
 * Each entry point below names the reference function it replaces.  The ctypes
 * stub a maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Conventions: extern "C", opaque handles, plain pointers and sizes, int status
 * return (0 = MG_OK, negative = error; text via mg_last_error()), no exceptions
 * cross the boundary, caller-owned buffers.  One context per (process, device);
 * one handle <-> one host thread.  Pointers named *_dev are device pointers on
 * the context's device, everything else is host memory.  All device work is
 * enqueued on the context's stream; *_host convenience entry points synchronise.
 *
 * Index layout is the reference's and is exact: frames[b][f][d] row-major with
 * d < 3 root translation and 3+4j..3+4j+3 the (w,x,y,z) quaternion of joint j;
 * coefficient flat index = coeff_idx * n_dim + d.
 */
#ifndef MG_HIP_H
#define MG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_context mg_context;
typedef struct mg_primitive mg_primitive;
typedef struct mg_time_grid mg_time_grid;
typedef struct mg_constraint_set mg_constraint_set;

enum {
    MG_OK = 0,
    MG_ERR_INVALID_ARGUMENT = -1,
    MG_ERR_NO_DEVICE = -2,      /* no HIP device / HIP runtime error at init  */
    MG_ERR_HIP = -3,            /* a HIP call failed; see mg_last_error()     */
    MG_ERR_UNSUPPORTED = -4,    /* shape outside what the kernels support     */
    MG_ERR_NOT_POSITIVE_DEFINITE = -5,
    MG_ERR_OUT_OF_MEMORY = -6
};

/* element types of latent inputs / score outputs */
enum { MG_F32 = 0, MG_F64 = 1 };

/* which kernel back_project_frames uses */
enum {
    MG_PATH_AUTO = 0,   /* MFMA tile kernel when it fits, else direct */
    MG_PATH_MFMA = 1,   /* LDS-staged f32 MFMA contraction + spline    */
    MG_PATH_DIRECT = 2  /* one thread per output element               */
};

/* Model arrays exactly as the reference's JSON holds them
 * (reference motion_primitive.py:126-163, _init_gmm_from_json /
 * _init_spatial_parameters_from_json).  All float64, host memory. */
typedef struct mg_primitive_desc {
    int32_t n_basis;             /* n_basis_spatial                                   */
    int32_t n_dim;               /* n_dim_spatial                                     */
    int32_t n_components;        /* L = rows of eigen_vectors_spatial                 */
    int32_t n_canonical_frames;  /* n_canonical_frames                                */
    int32_t n_gmm;               /* K = len(gmm_weights); 0 = no mixture              */
    int32_t eigen_is_transposed; /* 0: JSON layout (L, NB*D); 1: (NB*D, L) as loaded  */
    const double *eigen_vectors; /* eigen_vectors_spatial                             */
    const double *mean_vector;   /* mean_spatial_vector (NB*D)                        */
    const double *translation_maxima; /* 3 values; NULL = [1,1,1] (v3 load path)      */
    const double *knots;         /* b_spline_knots_spatial (NB+4)                     */
    const double *gmm_weights;   /* (K)                                               */
    const double *gmm_means;     /* (K, Lg)                                           */
    const double *gmm_covars;    /* (K, Lg, Lg)                                       */
    /* The reference fits the mixture over the CONCATENATED (spatial, time) latents (reference
     * construction/motion_model_constructor.py:424; motion_primitive.py:229-231 splits s[:n_s] / s[n_s:]):
     * Lg = n_gmm_dims >= n_components, 0 = n_components.  Sampling, log p and its Jacobian work on all Lg columns;
     * back projection and constraint scoring read the first n_components of every row. */
    int32_t n_gmm_dims;
    /* time model (reference motion_primitive.py:164-181, _init_time_parameters_from_json); 0 components = none */
    int32_t n_time_components;   /* columns of eigen_vectors_time                      */
    int32_t n_basis_time;        /* n_basis_time                                      */
    int32_t reserved;
    const double *eigen_vectors_time;  /* (n_basis_time, n_time_components) as the JSON holds it */
    const double *mean_time_vector;    /* (n_basis_time)                               */
    const double *knots_time;          /* b_spline_knots_time (n_basis_time + 4)       */
} mg_primitive_desc;

/* One keyframe constraint, the subset of
 * MotionPrimitiveConstraints.evaluate the fused scorer covers (reference
 * morphablegraphs/constraints/motion_primitive_constraints.py:100-122):
 *  MG_CONSTRAINT_POSITION  -> GlobalTransformConstraint._point_distance
 *      (reference .../keyframe_constraints/global_transform_constraint.py:135-143),
 *      target axes set to NaN are unconstrained (the reference's None);
 *  MG_CONSTRAINT_DIRECTION_2D -> Direction2DConstraint.evaluate_motion_spline
 *      (reference .../keyframe_constraints/direction_2d_constraint.py:42-52), heading =
 *      xz of the root quaternion applied to ref_dir, error in degrees;
 *  MG_CONSTRAINT_JOINT_POSITION -> the same _point_distance for ANY joint of a skeleton (hands, feet: the
 *      keyframe position constraints of reference two_hand_constraint.py:51-93, pose_constraint.py:48-67 go
 *      through Skeleton.nodes[joint].get_global_position): forward kinematics along the joint's chain,
 *      p = t_root + sum_i R(q_j0 q_j1 .. q_j(i-1)) offset(j_i), quaternions (w,x,y,z) normalised like
 *      transformations.quaternion_matrix does; needs a set made by mg_constraint_set_create_fk.
 *      PARITY UNPINNED: the reference's FK lives in anim_utils (absent); pinned by an independent
 *      rotation-matrix oracle and known-answer poses (tests).  A non-zero ref_dir is a point given in the joint's
 *      own frame: p + R_global(joint) ref_dir, RelativeTransformConstraint's `global_matrix . offset`
 *      (reference relative_transform_constraint.py:46-50);
 *  MG_CONSTRAINT_LOOK_AT -> LookAtConstraint.evaluate_frame (reference look_at_constraint.py:55-66): the angle
 *      in RADIANS between the joint's global orientation applied to ref_dir (REFERENCE_VECTOR (0,0,1)) and the
 *      direction from the joint's position to `target`;
 *  MG_CONSTRAINT_JOINT_MIDPOINT -> the first residual of TwoHandConstraint.get_residual_vector_frame
 *      (reference two_hand_constraint.py:66-74): |target - (p(joint) + p(joint2)) / 2|, both by the same FK (the
 *      other two residuals of that constraint are plain MG_CONSTRAINT_JOINT_POSITIONs);
 *  MG_CONSTRAINT_JOINT_ORIENTATION -> GlobalTransformConstraint._quaternion_distance
 *      (reference global_transform_constraint.py:109-121): the angle in RADIANS between the joint's global
 *      orientation (its own quaternion included) applied to ref_dir and `target` = the wanted orientation applied to
 *      ref_dir (the caller rotates; ref_dir = (0,0,1) is the reference's ORIGIN); arccos of the normalised dot
 *      product (transformations.angle_between_vectors), clamped to [-1, 1]. */
enum { MG_CONSTRAINT_POSITION = 0, MG_CONSTRAINT_DIRECTION_2D = 1, MG_CONSTRAINT_JOINT_POSITION = 2,
       MG_CONSTRAINT_JOINT_MIDPOINT = 3, MG_CONSTRAINT_JOINT_ORIENTATION = 4, MG_CONSTRAINT_LOOK_AT = 5,
       MG_CONSTRAINT_POSE = 6 /* mg_keyframe_constraint.joint = index into the mg_pose_constraint array */,
       /* Not errors but VALUES of the (aligned) motion at the keyframe, reported in the residual matrix: what the next step of
        * a graph walk is aligned to (obj_global_*: reference optimization/objective_functions.py:290-380 hands each step the
        * aligned frames of the step before).  weight_factor multiplies the value (use 1).
        *   MG_CONSTRAINT_VALUE_POSITION: component target[0] (0, 1, 2) of the root position;
        *   MG_CONSTRAINT_VALUE_HEADING:  component target[0] (0 = x, 2 = z) of the unit heading = xz of the global orientation
        *                                 of `joint` applied to ref_dir (the aligning node and reference vector of mg_alignment_desc) */
       MG_CONSTRAINT_VALUE_POSITION = 7, MG_CONSTRAINT_VALUE_HEADING = 8 };
#define MG_MAX_CHAIN 32
typedef struct mg_keyframe_constraint {
    int32_t type;
    int32_t joint;              /* MG_CONSTRAINT_JOINT_*: index into the skeleton's joints; else unused */
    double canonical_keyframe;  /* t; may be fractional (graph_walk_planner.py:203) */
    double weight_factor;
    double target[3];           /* position xyz (NaN = free) or direction (x, z, unused) */
    double ref_dir[3];          /* direction / orientation: the vector that is rotated, e.g. (0,0,1) */
    int32_t joint2;             /* MG_CONSTRAINT_JOINT_MIDPOINT: the second joint; else unused */
    int32_t reserved;
} mg_keyframe_constraint;

/* Point-cloud pose constraint, PoseConstraint.evaluate_motion_spline (reference pose_constraint.py:48-67): the global
 * positions of `joints` at the keyframe form a cloud b; it is fitted to the wanted cloud a (`points`) by the optimal
 * weighted 2-D rigid transform (rotation about y, translation in x and z: the closed form of Kovar et al.'s "Motion
 * Graphs", theta = atan2(sum w (ax bz - bx az) - (Sax Sbz - Sbx Saz) / Sw, sum w (ax bx + az bz) - (Sax Sbx + Saz Sbz) / Sw),
 * S* = weighted sums) and the error is the MEAN distance between corresponding points after the fit, plus -- with
 * has_velocity -- |velocity - (p_0(t + 1) - p_0(t))| of the first joint.  PARITY UNPINNED: the fit and the distance are
 * anim_utils' align_point_clouds_2D / calculate_point_cloud_distance (absent); the fit is pinned by its optimality
 * (tests perturb it), the rest by a NumPy oracle. */
typedef struct mg_pose_constraint {
    int32_t n_points;        /* <= MG_MAX_POSE_POINTS */
    int32_t has_velocity;
    const int32_t *joints;   /* (n_points) indices into the skeleton (the reference's node_names) */
    const double *points;    /* (n_points, 3) the wanted cloud */
    const double *weights;   /* (n_points) */
    double velocity[3];
} mg_pose_constraint;
#define MG_MAX_POSE_POINTS 64

/* The part of a skeleton forward kinematics needs (anim_utils Skeleton: nodes with parent / offset, and the
 * pose-vector layout root translation [0:3] + one quaternion per animated joint). */
typedef struct mg_skeleton_desc {
    int32_t n_joints;
    int32_t reserved;
    const int32_t *parents;       /* (n_joints) parent index, -1 for the root (joint 0 must be the root) */
    const double *offsets;        /* (n_joints, 3) offset from the parent in the parent's frame (root: ignored) */
    const int32_t *quat_channel;  /* (n_joints) first pose channel of the joint's (w,x,y,z), -1 = not animated (identity) */
} mg_skeleton_desc;

/* The 2-D alignment MotionPrimitiveConstraints.evaluate applies to every candidate outside local-coordinate mode
 * (reference motion_primitive_constraints.py:110-114, objective_functions.py:35-37 ->
 * anim_utils align_quaternion_frames_automatically): the candidate's control points are rotated about the y axis
 * so that the heading of the aligning node in its FIRST control point equals the heading in the last frame of the
 * previous motion, and translated in x and z so that its first root position lands on that frame's (y untouched);
 * heading = xz of the node's global orientation applied to ref_dir.  Rotation and translation differ per candidate.
 * The scorer never transforms control points: with c = h.b and s = h x b (h = previous heading, b = candidate
 * heading, both unit) a position becomes (c x + s z + tx, y, -s x + c z + tz), a heading (c hx + s hz, -s hx + c hz).
 * PARITY UNPINNED: anim_utils is absent; pinned by a 4x4-matrix oracle that does transform the control points.
 * joint = MG_ALIGN_START_POSE is the other branch of the reference's align_quaternion_frames (objective_functions.py:38-47,
 * taken for the first primitive of a walk, when there are no previous frames but a start pose): every candidate gets the
 * SAME rotation about y, heading = (cos, sin) of the start orientation's y angle; its first root position lands on
 * (position[0], ., position[2]) -- (0, 0) is what the reference's arithmetic produces, see candidate_scoring.py -- and every
 * height is raised by position[1].  Start orientations with x or z angles are not covered. */
#define MG_ALIGN_START_POSE (-1)
typedef struct mg_alignment_desc {
    int32_t joint;        /* skeleton.aligning_root_node as an index into the skeleton (0 = root, no skeleton needed) */
    int32_t reserved;
    double position[3];   /* root position of the previous motion's last frame (x and z are used) */
    double heading[2];    /* (x, z) heading of the aligning node in that frame; normalised by the library */
    double ref_dir[3];    /* skeleton.aligning_root_dir, e.g. (0,0,1) */
} mg_alignment_desc;

/* ---- library / context ------------------------------------------------------ */
const char *mg_version(void);
/* message of the last failed call on this thread */
const char *mg_last_error(void);
const char *mg_status_string(int status);

/* stream: a hipStream_t to enqueue on (e.g. torch's current stream) or NULL for a
 * stream owned by the context. */
int mg_context_create(int device, void *stream, mg_context **out);
void mg_context_destroy(mg_context *ctx);
int mg_context_set_stream(mg_context *ctx, void *stream);
/* The persistent frames kernel normally occupies every CU (one workgroup each, all of its LDS); leave n CUs free
 * so that kernels on other streams -- RCCL's all-gather of the scores -- run beside it instead of behind it. */
int mg_context_set_reserved_cus(mg_context *ctx, int32_t n);
/* Test and tuning switches as explicit calls (the library reads no environment variable): value 0 restores the
 * default.  They select between kernels with identical results or change the launch geometry of grids planned
 * AFTER the call; tests use them to cover the fallback kernels.
 *   MG_OPT_FORCE_VALU_SCORE   1 = constraint scoring on the VALU kernel even where the MFMA kernel applies
 *   MG_OPT_FORCE_VALU_SAMPLE  1 = mixture sampling on the VALU kernel
 *   MG_OPT_RING_SLOTS         2 = two LDS ring slots in the frames kernel even where three fit
 *   MG_OPT_CHUNK_WINDOW       n = at most n basis functions per time-chunk window (4 .. 11)
 *   MG_OPT_CHUNK_SAMPLES      n = at most n time samples per chunk (1 .. 48)
 *   MG_OPT_FRAMES_KERNEL      which LDS-staged frames kernel the MFMA path launches: 0 = by batch size (chunk-stationary
 *                             from two units per workgroup on), 1 = tile-major (units of one tile's consecutive chunks,
 *                             rows shared by neighbouring chunks carried over), 2 = chunk-stationary (a workgroup keeps one
 *                             chunk's eigenvector window in registers; MG_ERR_UNSUPPORTED where the window does not fit)
 *                             -- identical results 
 *   MG_OPT_PLACED_FAST_PCT    mg_device_malloc_placed: pattern / fill ratio (in percent) up to which a candidate counts as
 *                             fast (0 = 115); tests lower it to walk through both recipes
 *   MG_OPT_OPTIONS_STEP       mg_options_step: 0 = one launch for the whole step where every option allows it, 1 = always one
 *                             chain of launches per option (identical results; tests compare the two), 2 = one launch, and
 *                             mg_options_step_device_counts always draws its counts with a kernel in front (never takes the
 *                             counts the step before drew ahead; A/B), 3 = one launch with the release / acquire form of the
 *                             kernel's publication protocol (csrc/mg_options.hip: the fence-free default leans on gfx950's
 *                             write-through behaviour; 3 is the memory model's own protocol -- identical results, a test
 *                             runs both)
 *   MG_OPT_PLAIN_MALLOC       1 = mg_device_malloc is one hipMalloc whatever the size (0: buffers of 64 MiB and more are pieces
 *                             of the context's placed output regions, see mg_device_malloc)
 *   MG_OPT_GMM_KERNEL         mg_gmm_log_prob on the matrix pipe: 0 = by batch size, 1 = one 16-candidate tile per workgroup, fragments
 *                             from L2, 2 = persistent workgroups with the mixture's fragments in LDS (from 20 480 candidates on by
 *                             default; MG_ERR_UNSUPPORTED never: a mixture that does not fit LDS falls back to 1) -- identical results
 *   MG_OPT_SCORE_KERNEL       mg_score_constraints on the matrix pipe: 0 = by batch size, 1 = a wave per 16-candidate tile, (candidate,
 *                             constraint) pairs on the lanes, 2 = a wave per 64 candidates, a lane per candidate (from 49 152
 *                             candidates on by default; sets of at most 16 rows only, every other set keeps 1: mg_score_plan) --
 *                             identical results
 *   MG_OPT_PLACED_HOLD        n > 0: the placement scan holds at most n candidates at once (default: a quarter of the free memory);
 *                             tests use it to make the scan drop candidates while it runs
 *   MG_OPT_TRAJECTORY_LANES   1 = one lane per candidate in the closest-point walks of mg_score_trajectory[_points / ies] whatever the
 *                             batch, 8 / 4 = that many lanes up to 65536 candidates (default: eight lanes while at most 28672
 *                             candidates are in flight, four up to 40960, one beyond -- the same bits in every case); only with
 *                             MG_OPT_TRAJECTORY_SEARCH = 1 (the reference's search is one lane per candidate)
 *   MG_OPT_TRAJECTORY_SEARCH  the closest-point search of the trajectory constraints (mg_score_trajectory[_points / ies], the scorer's
 *                             MG_FRAME_JOINT_TRAJECTORY): 0 = the reference's -- scipy's L-BFGS-B with a forward-difference gradient
 *                             (parameterized_spline.py:303-322) restated for one bounded variable, held to vectors the reference's own
 *                             function produced (tests/golden/trajectory_closest_point.npz) --, 1 = the monotone grid walk + Newton
 *                             refinement of rounds 2-4 (the first local minimum at or after the bound: the same point where the
 *                             distance has one basin ahead of the bound, another one where it has several)
 *   MG_OPT_ROOT_MODE          how the float32 frames kernels compute the root-translation channels (the two forms differ in
 *                             the last bits; see mg_primitive_root_mode): 0, 1 = the float64 pipeline (the default: the faster
 *                             of the two on gfx950), 2 = the mean/delta split, 3 = the split where the primitive's accuracy gate
 *                             allows it */
#define MG_OPT_FORCE_VALU_SCORE 0
#define MG_OPT_FORCE_VALU_SAMPLE 1
#define MG_OPT_RING_SLOTS 2
#define MG_OPT_CHUNK_WINDOW 3
#define MG_OPT_CHUNK_SAMPLES 4
#define MG_OPT_FRAMES_KERNEL 5
#define MG_OPT_PLACED_FAST_PCT 6
#define MG_OPT_OPTIONS_STEP 7
#define MG_OPT_PLAIN_MALLOC 8
#define MG_OPT_GMM_KERNEL 9
#define MG_OPT_SCORE_KERNEL 10
#define MG_OPT_ROOT_MODE 11
#define MG_OPT_PLACED_HOLD 12
#define MG_OPT_TRAJECTORY_LANES 13
#define MG_OPT_TRAJECTORY_SEARCH 14
#define MG_OPT_COUNT 15
int mg_context_set_option(mg_context *ctx, int32_t option, int32_t value);
/* Between _begin and _end every device constant the library uploads for this context (primitives and their
 * canonical grids: a graph's whole set of motion primitives) is bump-allocated from blocks of `block_bytes`
 * (0 = 64 MiB) instead of one hipMalloc each; a block is released when the last array in it has been destroyed
 * (or with the context).  mg_context_arena_bytes reports (reserved, used). */
int mg_context_arena_begin(mg_context *ctx, int64_t block_bytes);
int mg_context_arena_end(mg_context *ctx);
int mg_context_arena_bytes(mg_context *ctx, int64_t *reserved, int64_t *used);
int mg_context_synchronize(mg_context *ctx);
/* name (256 bytes), CU count, total bytes of the context's device */
int mg_context_device_info(mg_context *ctx, char *name, int32_t *n_cu, int64_t *total_mem);

/* Device memory helpers so a host language needs no HIP binding of its own.
 *
 * Where a LARGE KERNEL OUTPUT (the (B, T, D) frames) lands decides between two speed classes of the frames kernel's store
 * stream -- thousands of concurrent ~1 KB-piece streams: 63 vs 80 us for 404 MB stand-alone, 77 vs 97 us for the frames
 * kernel; a plain fill does not see the difference.  The class is a property of the physical memory behind an allocation
 * (the same memory mapped at other virtual addresses keeps it, offsets inside an allocation do not change it, fast memory
 * comes in multi-gigabyte runs), it shows in no translation or L2 counter, and nothing a kernel can choose changes it
 * (DESIGN.md "Placement", profiles/r03_placement/).  So the library PROBES: it times the store pattern and a plain fill on a
 * candidate allocation (~1.5 ms) and keeps the first candidate in the fast class.
 *
 * mg_device_malloc: buffers below 64 MiB are one hipMalloc.  From 64 MiB on the buffer is a piece of one of the context's
 * PLACED REGIONS: the first request of a size runs the scan once, later requests (after mg_device_free, which returns a piece
 * to its region, not to the driver) reuse the region -- an adaptor that allocates its output on every call pays for placement
 * once, and the scratch blocks behind the *_host entry points are placed the same way.  The scan is bounded: at most 32
 * candidates, and never more than a quarter of the free device memory held at once (processes sharing a GPU);
 * mg_context_trim_outputs releases the regions no piece of which is in use, mg_context_output_bytes reports what is held.
 * A caller that brings memory from elsewhere (a framework's tensor) can ask mg_device_probe_placement which class it is in. */
int mg_device_malloc(mg_context *ctx, int64_t bytes, void **out_dev);
int mg_device_free(mg_context *ctx, void *ptr_dev);
int mg_context_trim_outputs(mg_context *ctx);
int mg_context_output_bytes(mg_context *ctx, int64_t *reserved, int64_t *in_use, int32_t *n_regions, int32_t *n_fast);
/* The same buffer assembled from separately created physical chunks (HIP virtual-memory API: one reserved address
 * range, hipMemCreate per chunk_bytes, mapped back to back); one of the scan's two recipes.  Freed with mg_device_free. */
int mg_device_malloc_chunked(mg_context *ctx, int64_t bytes, int64_t chunk_bytes, void **out_dev);
/* mg_device_malloc's placed path with an explicit budget and a report.  max_candidates <= 0: the default scan (16 plain
 * allocations, then -- unless max_candidates == 1 -- twelve assembled from physical chunks of 32 / 8 / 2 MiB, then plain
 * again, 32 in all, at most a quarter of the free memory held -- and, when those were all slow, on with plain allocations up to
 * 400 candidates or six tenths of the free memory held while the scan runs: fast-class memory is sparse, about one 404 MB
 * allocation in thirty, and comes in clusters of the allocation order (on one box the first was the 181st candidate);
 * ~12 ms per candidate, once per region; max_candidates > 0 is an exact budget without that); if nothing is fast the best
 * candidate of all is returned.  info (may be NULL): [0] candidates probed BY
 * THIS CALL (0: the piece came from a region the context already had), [1] pattern time / fill time of the region, [2] its
 * pattern time in us, [3] 1 if it is in the fast class.  The contents are undefined afterwards.  Freed with mg_device_free. */
int mg_device_malloc_placed(mg_context *ctx, int64_t bytes, int32_t max_candidates, void **out_dev, double *info4);
/* the probe alone, on any device buffer of at least 64 MiB: info4 as above ([0] = 1).  It OVERWRITES the buffer (the probe
 * is a store pattern and a fill): call it before the buffer holds anything. */
int mg_device_probe_placement(mg_context *ctx, void *buf_dev, int64_t bytes, double *info4);
/* What the arena already knows about memory it handed out -- no probe, nothing written: info4 = {1 if buf_dev is (inside) a piece
 * of one of the context's placed regions, the region's pattern / fill ratio, its pattern time in us, 1 if the region is in the
 * fast class}; *tbps (may be NULL) = the pattern's rate in TB/s in the scan that classified the region (0: the request was too
 * small to fill the chip).  A region's class is decided ONCE, from its scan (fast from 5.9 TB/s on; the scan stops at the first
 * candidate of 6.0 TB/s and more), and stays: this is what mg_step_plan_for and the kernels' choice go by. */
int mg_device_placement_info(mg_context *ctx, const void *buf_dev, double *info4, double *tbps);
int mg_memcpy_h2d(mg_context *ctx, void *dst_dev, const void *src, int64_t bytes);
int mg_memcpy_d2h(mg_context *ctx, void *dst, const void *src_dev, int64_t bytes);
/* rows x row_bytes from one device matrix into another, each with its own pitch in bytes (a column block of a row-major matrix);
 * asynchronous on the context's stream.  It is the runtime's 2-D copy (hipMemcpy2DAsync), and that copy rejects -- "invalid
 * argument", MG_ERR_HIP, nothing copied -- a source or destination that lies in memory mapped from SEVERAL physical chunks through
 * the virtual-memory API, whatever the pitch (measured on an MI355X: a 986 MB source of 32 MiB or 2 MiB chunks and a 6 MB
 * destination of 2 MiB chunks fail, one 1 GiB chunk and plain allocations pass).  Such memory comes from mg_device_malloc_chunked
 * with a chunk smaller than the buffer and, on devices where the arena's scan settles on that recipe, from any allocation of 64 MiB
 * and more (mg_device_malloc, mg_device_malloc_placed: csrc/mg_placement.hip); MG_OPT_PLAIN_MALLOC keeps mg_device_malloc's
 * buffers out of it.  A caller that must gather from such a buffer uses a kernel or an indexed gather of its own. */
int mg_memcpy_d2d_rows(mg_context *ctx, void *dst_dev, int64_t dst_pitch, const void *src_dev, int64_t src_pitch, int64_t row_bytes, int64_t rows);
int mg_memset(mg_context *ctx, void *dst_dev, int value, int64_t bytes);

/* Kernel timing with HIP events on the context's stream.  enabled = n > 0 brackets every
 * n-th launch of each slot with an event pair (n = 1: every launch; an event pair costs a few
 * microseconds of stream time, so a timed region samples with n ~ 8); totals are resolved on query.
 * slot: 0 = back_project_frames, 1 = gmm_log_prob, 2 = score_constraints, 3 = argmin,
 *       4 = gmm_sample, 5 = spline_evaluate, 6 = fused step, 7 = a planner step in one launch (mg_options_step),
 *       8 = mg_joint_tracks, 9 = mg_score_frame_constraints, 10 = mg_score_trajectory[_points],
 *       11 = mg_cluster_tree_search (both tree kinds: mg_tree_search_kernel or mg_kd_tree_search_kernel),
 *       12 = the frames kernel of mg_walk_frames, 13 = mg_score_walk_time, 14 = mg_step_lengths, 15 = mg_feature_points,
 *       16 = mg_feature_points_warped, 17 = mg_mixture_scores, 18 = mg_point_cloud_features, 19 = mg_feature_points_warped_smoothed. */
int mg_profile_enable(mg_context *ctx, int enabled);
int mg_profile_reset(mg_context *ctx);
int mg_profile_get(mg_context *ctx, int slot, double *total_ms, int64_t *launches);
/* the individual durations (ms) behind mg_profile_get, oldest first, at most `capacity` of them (the library
 * keeps the first 65536 per slot); *n = how many were written */
int mg_profile_get_samples(mg_context *ctx, int slot, float *out_ms, int64_t capacity, int64_t *n);

/* ---- multi-GPU: one process per GPU, one context per process ----------------------------------------
 * The only exchange on the path is the all-gather of per-rank scores.  RCCL is loaded on first use
 * (dlopen of librccl.so.1 -- the copy a host framework already has in the process, if any), so single-GPU users
 * carry no dependency.  mg_dist_unique_id on rank 0, the 128 bytes travel out of band (MPI, a file, a
 * torch.distributed broadcast), then mg_dist_init on every rank; mg_dist_all_gather runs on the context's stream:
 * gathered[r * count + i] = rank r's local[i].  (bench.py keeps torch.distributed's communicator: same library.) */
#define MG_DIST_ID_BYTES 128
int mg_dist_unique_id(void *id_out);
int mg_dist_init(mg_context *ctx, int32_t rank, int32_t n_ranks, const void *id);
int mg_dist_all_gather(mg_context *ctx, const void *local_dev, void *gathered_dev, int64_t count, int dtype);
/* `bytes` bytes of buf_dev from rank `root` to every rank's buf_dev, on the context's stream: how rank 0 -- the one process
 * that runs the reference's control flow -- hands a step's constraint values, seeds and component counts to the workers */
int mg_dist_broadcast(mg_context *ctx, void *buf_dev, int64_t bytes, int32_t root);
int mg_dist_finalize(mg_context *ctx);
/* mg_dist_preflight: everything about the set-up that can fail on one rank alone (librccl and its symbols, the context's device)
 * -- call it on every rank and exchange the outcome BEFORE any rank calls mg_dist_init: ncclCommInitRank is a collective, a rank
 * that enters it alone does not return.  mg_dist_info: the communicator as RCCL reports it, out3 = {rank, ranks, device}
 * (ncclCommUserRank / ncclCommCount / ncclCommCuDevice; -1 where a query is missing), {-1, 0, -1} without a communicator. */
int mg_dist_preflight(mg_context *ctx);
int mg_dist_info(mg_context *ctx, int32_t *out3);

/* ---- primitive -------------------------------------------------------------------
 * Replaces MotionPrimitive._initialize_from_json (reference motion_primitive.py:96-163):
 * transposes/scales/packs the eigenvectors, computes precisions_cholesky_ in float64
 * on the host exactly as sklearn's _compute_precision_cholesky does
 * (reference motion_primitive.py:141-142) and uploads all constants once. */
int mg_primitive_create(mg_context *ctx, const mg_primitive_desc *desc, mg_primitive **out);
void mg_primitive_destroy(mg_primitive *prim);
/* out[8] = {n_basis, n_dim, n_components, n_canonical_frames, n_gmm, kk (MFMA k-steps),
 *           mfma_supported, chunks of the canonical grid}; mg_primitive_info2: out[4] = {n_gmm_dims, n_time_components,
 *           n_basis_time, kk of the mixture} */
int mg_primitive_info(const mg_primitive *prim, int32_t *out8);
int mg_primitive_info2(const mg_primitive *prim, int32_t *out4);
/* How the float32 frames kernels compute the root-translation channels d < 3 of this primitive (the reference computes
 * everything in float64: motion_primitive.py:236-256, motion_spline.py:71-86; the other channels are a float32 pipeline).
 *   split = 0: the float64 pipeline -- control points and spline taps as float64 fma chains, rounded to float32 once;
 *   split = 1: the mean/delta split -- the output is linear in the latent vector, frames[f][d] = M[f][d] + delta[f][d] with
 *              M = the spline of mean' alone, a constant of the time grid evaluated ONCE in float64 on the host and kept as
 *              a float32 pair (Mhi, Mlo), and delta = the spline of E'.s alone, which rides in the ordinary float32 row
 *              tiles; out = Mhi + (Mlo + delta), two float32 additions.
 * The split is an OPTION (MG_OPT_ROOT_MODE 3; it measured 82.8 us against the float64 pipeline's 78.5 us on the fused step,
 * DESIGN.md 6.4, so the default is the float64 pipeline for every primitive); mode 3 takes it when its error estimate -- (L + 8) 2^-24 max_r sqrt(sum_k E'[r][k]^2 m2[k]) over the root rows r, m2[k] the
 * second moment of latent k under the primitive's mixture (1 without a mixture): the float32 rounding a root control point
 * of typical size can collect -- is at most 5e-6, half of the 1e-5 the float32 pose values are held to; *estimate returns
 * it; *split returns what the context's current mode means for this primitive.  MG_OPT_ROOT_MODE 2 forces the split (tests). */
int mg_primitive_root_mode(const mg_primitive *prim, int32_t *split, double *estimate);
/* (K, L, L) float64, upper triangular: sklearn's precisions_cholesky_ */
int mg_primitive_get_precisions_cholesky(const mg_primitive *prim, double *out);

/* MotionPrimitive._back_transform_gamma_to_canonical_time_function for a batch (reference motion_primitive.py:289-302):
 * out[b][i] = sum_{j <= i} exp(mean_t(j) + sum_l phi_l(j) gamma[b][l]) - 1, i = 0 .. n_canonical_frames - 1, with the mean
 * and the harmonics evaluated at the canonical frames by the FITPACK splev recurrence on the time knots (float64, host,
 * once per primitive).  gamma: (B, ld), first n_time_components columns; out: (B, n_canonical_frames) float64.
 * MG_ERR_INVALID_ARGUMENT if the primitive has no time model. */
int mg_time_function_canonical(mg_primitive *prim, const void *gamma_dev, int gamma_dtype, int64_t n_samples, int64_t ld,
                               double *out_dev);
int mg_time_function_canonical_host(mg_primitive *prim, const void *gamma, int gamma_dtype, int64_t n_samples, int64_t ld,
                                    double *out);
/* The TIME-WARPED synthesis of a batch (reference motion_primitive.py:268-319 behind back_project(s, use_time_parameters=True);
 * graph_walk.py:154-176 turns every step of a finished walk into frames this way).
 * mg_time_function_sample: per candidate the spline's time function t'(t) = {0, inverse of the canonical time function t(t') at
 * numpy.linspace(1, t(F-2), num), F - 1}, num = int(round(t(F-2)) * (1 / speed)) -- the reference passes this FLOAT to linspace, a
 * TypeError on NumPy >= 1.18; int() is what older NumPy made of it.  The inverse is the interpolating cubic through (t(i), i),
 * i = 0 .. F-1, that scipy's splrep(k=3, s=0) builds: knots at every data point but the second and the second-to-last, i.e. the
 * not-a-knot cubic, computed here from its second derivatives (the same function; 1e-12 F from FITPACK's B-spline form).
 * times (n, t_cap) float64, lengths (n) int32: samples of row b = lengths[b]; a row that would need more than t_cap samples gets
 * lengths[b] = -needed and is not written.  canonical_out (may be NULL): (n, F) float64, the canonical time functions.
 * mg_back_project_frames_at: frames of every candidate at its own times, (n, t_cap, D) float64 or float32 -- the float64 arithmetic
 * of mg_back_project_frames_f64 (control points as fma chains from the mean, FITPACK basis rows, four taps), one launch for the
 * batch; lengths NULL: every row has t_cap samples.  Device pointers. */
int mg_time_function_sample(mg_primitive *prim, const void *gamma, int dtype, int64_t n, int64_t ld, double speed, double *times, int32_t *lengths,
                            int32_t t_cap, double *canonical_out);
/* The same with the rows of `times` row_pitch >= t_cap doubles apart (mg_time_function_sample: row_pitch = t_cap), so that a batch's
 * rows can land inside a wider table, such as mg_walk_frames' (n_walks, n_steps, t_cap); a row still holds at most t_cap samples. */
int mg_time_function_sample_rows(mg_primitive *prim, const void *gamma, int dtype, int64_t n, int64_t ld, double speed, double *times, int32_t *lengths,
                                 int32_t t_cap, int64_t row_pitch, double *canonical_out);
int mg_back_project_frames_at(mg_primitive *prim, const void *latents, int dtype, int64_t n, int64_t ld, const double *times, const int32_t *lengths,
                              int32_t t_cap, void *out, int out_dtype);
/* The SMOOTHED time function (smooth_time_parameters, reference motion_primitive.py:284-285, 320-331: scipy.signal.savgol_filter(t, 15,
 * 3)) in the same one launch: row b is the Savitzky-Golay pass over mg_time_function_sample's row b, stated as a table -- sample q is a
 * row of the 15 x 15 hat matrix H of the least-squares cubic on 15 points (csrc/mg_savgol_table.h) times 15 unsmoothed samples: row q on
 * the first 15 for q < 7, row 15 - (T - q) on the last 15 for q >= T - 7, row 7 on samples q - 7 .. q + 7 otherwise; acc = H[0] u[0], then
 * acc = acc + H[k] u[k] for k = 1 .. 14, every product and sum rounded on its own (time_smoothing.smooth_time_row_host's bits).  The
 * unsmoothed row is never in memory; the first sample can be negative and the last one is no longer F - 1.  Lengths as above, and a row
 * of 0 < T < 15 samples (scipy raises ValueError there) reports its T and is NOT written.  H travels in a cached table of its own
 * (MG_TABLE_SAVGOL), uploaded once per context. */
int mg_time_function_sample_smoothed(mg_primitive *prim, const void *gamma, int dtype, int64_t n, int64_t ld, double speed, double *times,
                                     int32_t *lengths, int32_t t_cap, double *canonical_out);
int mg_time_function_sample_smoothed_rows(mg_primitive *prim, const void *gamma, int dtype, int64_t n, int64_t ld, double speed, double *times,
                                          int32_t *lengths, int32_t t_cap, int64_t row_pitch, double *canonical_out);

/* ---- time grids ---------------------------------------------------------------------
 * A set of canonical times with its B-spline basis rows (FITPACK splev semantics,
 * ext=0 extrapolation; reference motion_spline.py:86,92) and mean frames, prepared
 * once in float64 on the host.  mg_primitive_canonical_grid = np.linspace(0, F, F)
 * (reference motion_primitive.py:233), owned by the primitive. */
int mg_time_grid_create(mg_primitive *prim, const double *times, int32_t n_times, mg_time_grid **out);
void mg_time_grid_destroy(mg_time_grid *grid);
mg_time_grid *mg_primitive_canonical_grid(mg_primitive *prim);
int mg_time_grid_size(const mg_time_grid *grid);
/* copies the grid's tables: i0 (T) int32, weights (T,4) float64, times (T) float64; any may be NULL */
int mg_time_grid_get_tables(const mg_time_grid *grid, int32_t *i0, double *weights, double *times);

/* Global positions of joints[0 .. n_out) in every row of a (n_frames, n_dim) float64 frame block on the device, by forward
 * kinematics along each joint's chain: out_dev (n_frames, n_out, 3).  What map_motions_to_euclidean_space asks of
 * skeleton.nodes[j].get_global_position(frame) once per sample, frame and joint (reference space_partitioning/features.py:
 * 133-153, under construction/cluster_tree_builder.py:266-301).  PARITY UNPINNED (anim_utils' FK), as for the constraints. */
int mg_joint_positions(mg_context *ctx, const mg_skeleton_desc *skeleton, const int32_t *joints, int32_t n_out,
                       const double *frames_dev, int64_t n_frames, int32_t n_dim, double *out_dev);

/* ---- trajectory constraints -------------------------------------------------------------------------
 * TrajectoryConstraint.evaluate_motion_spline / get_residual_vector for the ROOT joint (reference
 * constraints/spatial_constraints/trajectory_constraint.py:79-121): per time sample of `grid` (NULL = the canonical grid,
 * i.e. get_motion_vector()) the distance from the candidate's root position to the closest point of a Catmull-Rom spline
 * through `control_points` (n_points x 3; reference splines/catmull_rom_spline.py:66-168) whose parameter is at or after
 * the previous sample's, starting at min_u (= min_arc_length / full_arc_length); error = weight * average distance.
 * errors_dev (B) float64: written, or added to with accumulate != 0 (the sum MotionPrimitiveConstraints.evaluate forms);
 * residuals_dev: NULL or (B, T) float64 = weight * distance per sample.  alignment: NULL (local coordinates), the
 * previous-frame record with the ROOT as aligning node, or a start-pose record.
 * The reference searches with scipy's L-BFGS-B from the lower bound (parameterized_spline.py:303-322); so does the device: L-BFGS-B 3.0
 * restated for one bounded variable (csrc/mg_traj_device.h), PINNED by tests/golden/trajectory_closest_point.npz -- 26 chains of 156
 * frames the reference's own function produced --: |u - u_ref| <= 2e-6 of the parameter range and |d - d_ref| <= 1e-6 max(1, d_ref) per
 * frame (measured 1.7e-7 / 2e-9; the forward-difference gradient with h = 1e-8 sets what two correct implementations can agree to).
 * MG_OPT_TRAJECTORY_SEARCH = 1 selects the deterministic walk of rounds 2-4 instead (grid walk u = k / granularity, parabola, Newton
 * steps: the local minimum of the first basin at or after the bound; 25 x faster; the reference's result where the distance has one
 * basin ahead of the bound).  The spline itself is pinned by tests/golden/trajectory_spline.npz. */
typedef struct mg_trajectory mg_trajectory;
int mg_trajectory_create(mg_primitive *prim, const double *control_points, int32_t n_points, int32_t granularity, mg_trajectory **out);
void mg_trajectory_destroy(mg_trajectory *trajectory);
/* The same object for any of the three curves the reference's ParameterizedSpline builds (parameterized_spline.py:36-63; the numbers
 * are the reference's).  Every curve is held as cubic pieces on a uniform parameter grid plus the granularity + 1 arc-length table, so
 * every entry point that takes a mg_trajectory takes all three:
 *   MG_SPLINE_CATMULL_ROM     forwards to mg_trajectory_create: the same tables, the same bits
 *   MG_SPLINE_BSPLINE         the clamped cubic B-spline over n_points - 2 uniform knot values (b_spline.py:70-105), n_points - 3
 *                             pieces; u <= 0 is the first control point, u >= 1 the last
 *   MG_SPLINE_FITTED_BSPLINE  FITPACK's splrep(linspace(0, 1, n_points), values, k = 3) with s = 0 per dimension
 *                             (fitted_b_spline.py:44-47): the interpolating cubic with not-a-knot ends, n_points - 1 pieces
 * Types 1 and 2 need n_points >= 4 (the reference's de Boor indexes out of range below, splrep needs m > k); an unknown type, fewer
 * points, a non-finite coordinate: MG_ERR_INVALID_ARGUMENT, nothing is allocated or launched.  Host statement:
 * morphablegraphs_amd/spline_types.py trajectory_polynomials_host; pinned by tests/golden/trajectory_spline_types.npz. */
#define MG_SPLINE_CATMULL_ROM 0
#define MG_SPLINE_BSPLINE 1
#define MG_SPLINE_FITTED_BSPLINE 2
int mg_trajectory_create_typed(mg_primitive *prim, const double *control_points, int32_t n_points, int32_t granularity, int32_t spline_type,
                               mg_trajectory **out);
/* the type a trajectory was created with (MG_SPLINE_*), -1 for NULL */
int32_t mg_trajectory_spline_type(const mg_trajectory *trajectory);
/* The two tables as the kernels read them, copied to the host (tests and tools): poly_host (n_seg * 12 + 3 doubles: per piece
 * [power 3, 2, 1, 0][x, y, z] of the piece's local parameter, then the last control point) and arc_host (granularity + 1 relative arc
 * lengths) are filled when not NULL; n_seg, granularity and full_arc_length are reported when not NULL. */
int mg_trajectory_tables(const mg_trajectory *trajectory, double *poly_host, double *arc_host, int32_t *n_seg, int32_t *granularity,
                         double *full_arc_length);
int mg_score_trajectory(mg_primitive *prim, const mg_trajectory *trajectory, const mg_time_grid *grid, const void *latents_dev,
                        int latent_dtype, int64_t n_samples, int64_t ld, double min_u, double weight, const mg_alignment_desc *alignment,
                        double *errors_dev, int accumulate, double *residuals_dev);
/* The same scorer with EVERY candidate aligned to its own previous motion -- a step of a graph walk chained on the step before it
 * (obj_global_error_sum and its residual-vector forms with a TrajectoryConstraint in a step's list): align_cand_dev (n_samples, 4)
 * float64, the layout and meaning of mg_score_constraint_residuals_chained's -- per candidate the previous unit heading (x, z) and
 * the previous root position (x, z), used as they are in place of the record's heading and position.  `alignment` is the template:
 * a previous-frame record with the root as aligning node, of which the node and ref_dir are used.  MG_ERR_INVALID_ARGUMENT for a
 * NULL or a start-pose record and for a NULL align_cand_dev with n_samples > 0, MG_ERR_UNSUPPORTED for another aligning joint;
 * nothing is launched then.  n_samples == 0 returns MG_OK.  The plan, the kernel and the launch are those of mg_score_trajectory for
 * the same shape (mg_trajectory_plan), the arithmetic is the same statement for statement: a batch whose candidates all carry the
 * record mg_score_trajectory would normalise to itself gives that call's bits. */
int mg_score_trajectory_chained(mg_primitive *prim, const mg_trajectory *trajectory, const mg_time_grid *grid, const void *latents_dev,
                                int latent_dtype, int64_t n_samples, int64_t ld, double min_u, double weight,
                                const mg_alignment_desc *alignment, const double *align_cand_dev, double *errors_dev, int accumulate,
                                double *residuals_dev);
/* n such scorers of the same batch size in ONE launch -- a planner step scores every option's candidates against the option's own
 * trajectory (reference graph_walk_planner.py:184-226 with a TrajectoryConstraint in every option's constraint list): 4096
 * candidates fill a quarter of the chip, sixteen launches in a row take sixteen times one, side by side they take four.  The
 * primitives must share a context; canonical grids; no residual vectors; alignments: NULL, or n records of which any may be NULL.
 * The same results as n calls of mg_score_trajectory, which this falls back to where the eight-lane walk does not apply. */
int mg_score_trajectories(int32_t n, mg_primitive *const *prims, const mg_trajectory *const *trajectories, const void *const *latents_dev,
                          int latent_dtype, int64_t n_samples, const int64_t *ld, const double *min_u, const double *weight,
                          const mg_alignment_desc *const *alignments, double *const *errors_dev, int accumulate);

/* Which kernel the three entry points above and below launch, stated once (mg_traj_plan in csrc/mg_trajectory.hip) and readable
 * without a launch: for a primitive of n_components latents and `rows` = 3 n_basis + 4 root coefficient rows, a target spline of
 * n_seg = n_points - 1 segments, n_samples candidates per scorer and `total` candidates in flight (n x n_samples for the n scorers of
 * mg_score_trajectories, n_samples otherwise), on the root rows (points = 0) or on given points (points != 0), under the context's
 * MG_OPT_TRAJECTORY_LANES and MG_OPT_TRAJECTORY_SEARCH.  together: the scorer fits the side-by-side launch of mg_score_trajectories
 * (which is taken when EVERY scorer's plan says so; lds_bytes is then the largest of theirs); otherwise the plan is the single
 * launch's.  needs_paths: the kernel writes the candidates' root paths to the context's scratch first (the reference's search in the
 * streaming kernels).  MG_ERR_UNSUPPORTED where mg_score_trajectory reports it.  Launches nothing. */
#define MG_TRAJ_KERNEL_STAGED_LDS 0      /* mg_trajectory_kernel<true>: rows (or nothing, on points) and the polynomials in LDS */
#define MG_TRAJ_KERNEL_STAGED_GLOBAL 1   /* mg_trajectory_kernel<false>: the polynomials stay in global memory */
#define MG_TRAJ_KERNEL_STREAM 2          /* mg_trajectory_stream_kernel */
#define MG_TRAJ_KERNEL_COOP8 3           /* mg_trajectory_coop_kernel<8> */
#define MG_TRAJ_KERNEL_COOP4 4           /* mg_trajectory_coop_kernel<4> */
#define MG_TRAJ_KERNEL_STREAM_MULTI 5    /* mg_trajectory_stream_multi_kernel */
#define MG_TRAJ_KERNEL_COOP8_MULTI 6     /* mg_trajectory_coop_multi_kernel<8> */
#define MG_TRAJ_KERNEL_COOP4_MULTI 7     /* mg_trajectory_coop_multi_kernel<4> */
#define MG_TRAJ_KERNEL_COUNT 8
typedef struct mg_trajectory_plan_info {
    int32_t kernel, lanes, poly_lds, needs_paths, together, candidates_per_workgroup;
    int64_t lds_bytes;
} mg_trajectory_plan_info;
int mg_trajectory_plan(const mg_context *ctx, int32_t n_components, int32_t rows, int32_t n_seg, int64_t n_samples, int64_t total, int32_t points,
                       mg_trajectory_plan_info *out);

/* The same search for positions the caller supplies: points_dev (n_samples, n_times, 3) float64 -- one joint's track from
 * mg_back_project_frames_f64 + mg_joint_positions, aligned by the caller -- for TrajectoryConstraint on joints other than the
 * root (trajectory_constraint.py:95-121 over skeleton.nodes[joint].get_global_position(frame)). */
int mg_score_trajectory_points(mg_primitive *prim, const mg_trajectory *trajectory, const double *points_dev, int64_t n_samples, int32_t n_times,
                               double min_u, double weight, double *errors_dev, int accumulate, double *residuals_dev);

/* ParameterizedSpline.find_closest_point_fast (constraints/spatial_constraints/splines/parameterized_spline.py:303-322) for a batch of
 * point sequences, chained the way TrajectoryConstraint.get_residual_vector chains it (trajectory_constraint.py:103-113: every
 * frame's search is bounded below by, and started at, the parameter the previous frame's search returned; the first by min_u):
 * points_dev (n_samples, n_times, 3) float64 -> params_dev (n_samples, n_times) the spline parameter of every frame's point,
 * distances_dev (n_samples, n_times) its distance to the frame's position, evaluations_dev (n_samples, n_times) int32 the (f, g)
 * evaluations the frame's search took (scipy's nfev / 2; 0 with the monotone walk) -- any may be NULL.  The search is the reference's
 * (MG_OPT_TRAJECTORY_SEARCH 0, the default: scipy's L-BFGS-B restated) or the monotone walk (1).  Pinned by
 * tests/golden/trajectory_closest_point.npz, which the reference's own function produced. */
int mg_trajectory_closest_points(mg_primitive *prim, const mg_trajectory *trajectory, const double *points_dev, int64_t n_samples, int32_t n_times,
                                 double min_u, double *params_dev, double *distances_dev, int32_t *evaluations_dev);

/* ---- arc-length queries on a trajectory (csrc/mg_trajectory_arc.hip) --------------------------------------------------------------
 * What a planner asks of ParameterizedSpline between the scoring launches (constraints/spatial_constraints/splines/
 * parameterized_spline.py), for a batch, on the tables of any of the three spline types.  Every device result has the bits of
 * its NumPy statement in morphablegraphs_amd/spline_types.py (point_by_arc_length_host, tangent_at_arc_length_host,
 * angle_at_arc_length_2d_host, arc_length_of_point_host); the reference's own numbers are in tests/golden/trajectory_arc_queries.npz.
 *
 * The parameters the point look-up scans, as the reference forms them (u = 0; u += 1.0 / granularity while u <= 1.0: granularity or
 * granularity + 1 sums, as they round): built once on the host when the trajectory is created, kept on the device beside its
 * tables.  u_host (NULL, or room for granularity + 1 doubles) receives them, n_samples (NULL or a pointer) their number. */
int mg_trajectory_sample_parameters(const mg_trajectory *trajectory, double *u_host, int32_t *n_samples);

/* query_point_by_absolute_arc_length (:131-155), get_tangent_at_arc_length (:186-207) and the angle of get_angle_at_arc_length_2d
 * (:217-240) for n arc lengths arc_dev (n) float64, one lane per query; any of the outputs may be NULL, not all of them:
 *   points_dev (n, 3)    the point at the arc length; above the full arc length the last control point
 *   tangents_dev (n, 3)  (p(arc + r) - p(arc - r)) / |.| with r = eval_range (the reference's default: 0.5), r += 0.1 while the two
 *                        points coincide, as the reference widens it; the norm is sqrt(x x + y y + z z), summed in that order
 *   angles_dev (n)       degrees between (tangent x, tangent z) and reference_dir (2 doubles on the host, required with angles_dev),
 *                        both normalised: acos of their dot product by the fdlibm statement (the host statement is the same one, so
 *                        the bits agree), times 180 / pi; NaN where rounding takes the dot product outside [-1, 1] (the reference
 *                        raises there)
 * The widening is bounded by MG_ARC_MAX_WIDENINGS rounds: a row that exhausts them (a query more than about a hundred units past the
 * end of the path, or a path of coinciding points) makes the CALL return MG_ERR_UNSUPPORTED, its tangent and angle rows are NaN --
 * never an approximate answer.  Only calls that ask for tangents or angles wait for the launch (they read that flag back).  A
 * non-finite arc length gives NaN rows.  eval_range must be finite and >= 0.  n == 0 returns MG_OK and launches nothing. */
#define MG_ARC_MAX_WIDENINGS 1024
int mg_trajectory_points_by_arc_length(mg_primitive *prim, const mg_trajectory *trajectory, const double *arc_dev, int64_t n, double eval_range,
                                       double *points_dev, double *tangents_dev, double *angles_dev, const double *reference_dir);

/* get_absolute_arc_length_of_point (:242-273) for n points points_dev (n, 3) float64, one wave per point: over the parameters above,
 * among those whose absolute arc length (arc_length_map.py:73-90, restated with its index rounding and its end case) is > the
 * point's min_arc_dev entry (NULL: 0 for every point), the FIRST strict minimum of the distance sqrt(dx dx + dy dy + dz dz) -- products and
 * sums rounded in that order, no contraction; lanes stride over the parameters and reduce on (distance, index), so the smallest
 * index wins among equal distances whatever the order of reduction.  arc_out_dev (n): the arc length at that parameter, -1 where no
 * parameter qualifies (min_arc at or above the full arc length, a point with a non-finite coordinate); min_point_dev (n, 3) or NULL:
 * the curve's point there, the row left UNTOUCHED where the result is -1; min_index_dev (n) int32 or NULL: the parameter's index, -1.
 * The three tables stand in LDS where they fit 64 KiB, else they are read from global memory: the same bits.  Asynchronous on the
 * context's stream.  n == 0 returns MG_OK and launches nothing. */
int mg_trajectory_arc_length_of_points(mg_primitive *prim, const mg_trajectory *trajectory, const double *points_dev, const double *min_arc_dev, int64_t n,
                                       double *arc_out_dev, double *min_point_dev, int32_t *min_index_dev);

/* The curve's points at n parameters u_dev (n), each taken no further than its u_max_dev entry where u_max_dev is not NULL:
 * points_dev (n, 3) -- what stands between mg_trajectory_closest_points (parameters) and mg_trajectory_arc_length_of_points (points)
 * when a walk's travelled arc length is advanced without a download.  One lane per parameter, asynchronous. */
int mg_trajectory_points_at_parameters(mg_primitive *prim, const mg_trajectory *trajectory, const double *u_dev, const double *u_max_dev, int64_t n,
                                       double *points_dev);

/* Constraints that walk a joint through EVERY frame of a candidate (mg_frame_constraints.hip), on float64 frames and joint tracks
 * that are on the device already (mg_back_project_frames_f64, mg_joint_positions):
 *
 * mg_align_frames -- frames_dev (n_samples, n_times, n_dim) float64, in place: every candidate turned about y and moved like
 *   MotionPrimitiveConstraints.evaluate aligns it (reference constraints/motion_primitive_constraints.py:106-116 through
 *   anim_utils' align_quaternion_frames / start-pose transform), the transform derived per candidate from ITS first control point:
 *   vals_dev (n_samples, n_vals) float64 = its root position x, z [and its heading x, z]: the residuals of
 *   MG_CONSTRAINT_VALUE_POSITION (axes 0, 2) [and MG_CONSTRAINT_VALUE_HEADING (axes 0, 2)] constraints at t = 0 with weight 1
 *   (mg_score_constraint_residuals).  alignment: the previous-frame record (n_vals 4) or a start-pose record (n_vals 2).
 *
 * mg_score_frame_constraint -- one constraint for the whole batch, one lane per candidate.  tracks_dev (n_samples, n_times,
 *   n_joints, 3) float64; errors_dev (n_samples) written or, with accumulate != 0, added to; residuals_dev NULL or (n_samples,
 *   mg_frame_constraint_width()) = weight * the constraint's residual vector.  Types (reference classes under
 *   constraints/spatial_constraints/):
 *     MG_FRAME_CA_POSITION          GlobalTransformCAConstraint, keyframe_constraints/global_transform_ca_constraint.py:33-46: the
 *                                   smallest distance of the joint to `target` over the first n_frames frames (axes with axis_on 0 ignored)
 *     MG_FRAME_DISCRETE_TRAJECTORY  DiscreteTrajectoryConstraint, discrete_trajectory_constraint.py:66-90: frame i against points_dev[i]
 *                                   (axes with axis_on 0 zeroed on both sides, frames beyond n_points count 0), averaged over all frames
 *     MG_FRAME_LOCAL_TRAJECTORY     LocalTrajectoryConstraint, keyframe_constraints/local_trajectory_constraint.py:45-78: the target is
 *                                   the point of trajectories[0] at arc length start_arc + the path walked so far; squared xz distances summed
 *     MG_FRAME_TRAJECTORY_SET       TrajectorySetConstraint, trajectory_set_constraint.py:82-104: n_joints joints, one trajectory each,
 *                                   arc0 = joint_arc_lengths, has_range / range_start / range_end = each trajectory's active range
 *     MG_FRAME_JOINT_ROTATION       JointRotationConstraint, keyframe_constraints/joint_rotation_constraint.py:55-72: tracks_dev is the
 *                                   (n_samples, n_times, n_joints = n_dim) FRAME block at the constraint's frame index (n_times 1),
 *                                   quat_channel = 3 + 4 * the joint's index among the animated joints, quaternion = the wanted rotation
 *   A TrajectoryConstraint on any joint is mg_score_trajectory_points.  PARITY UNPINNED (forward kinematics and alignment are
 *   anim_utils'); the arc-length look-up is pinned by tests/golden/trajectory_spline.npz. */
#define MG_FRAME_CA_POSITION 1
#define MG_FRAME_DISCRETE_TRAJECTORY 2
#define MG_FRAME_LOCAL_TRAJECTORY 3
#define MG_FRAME_TRAJECTORY_SET 4
#define MG_FRAME_JOINT_ROTATION 5
#define MG_FRAME_JOINT_TRAJECTORY 6   /* TrajectoryConstraint on any joint, trajectory_constraint.py:79-121: per frame the distance to the closest
                                         point of trajectories[0] at or after the previous frame's parameter (start_arc = the constraint's min_u),
                                         averaged -- mg_score_trajectory_points' arithmetic, as a member of a list (mg_score_frame_constraints) */
#define MG_FRAME_MAX_JOINTS 8
typedef struct mg_frame_constraint_desc {
    int32_t type;
    int32_t n_frames;                 /* frames evaluated, 0 = all n_times (CA_POSITION, LOCAL_TRAJECTORY, TRAJECTORY_SET) */
    int32_t n_points;                 /* DISCRETE_TRAJECTORY */
    int32_t n_joints;                 /* TRAJECTORY_SET; 1 otherwise */
    double weight;
    double target[3];                 /* CA_POSITION */
    int32_t axis_on[3];               /* CA_POSITION: axes of the target that count; DISCRETE_TRAJECTORY: constrained axes */
    int32_t quat_channel;             /* JOINT_ROTATION */
    const double *points_dev;         /* DISCRETE_TRAJECTORY: (n_points, 3) float64 on the device */
    double start_arc;                 /* LOCAL_TRAJECTORY */
    const mg_trajectory *trajectories[MG_FRAME_MAX_JOINTS];
    double arc0[MG_FRAME_MAX_JOINTS], range_start[MG_FRAME_MAX_JOINTS], range_end[MG_FRAME_MAX_JOINTS];
    int32_t has_range[MG_FRAME_MAX_JOINTS];
    double quaternion[4];             /* JOINT_ROTATION: (w, x, y, z) */
} mg_frame_constraint_desc;
int mg_align_frames(mg_primitive *prim, double *frames_dev, int64_t n_samples, int32_t n_times, const double *vals_dev, int32_t n_vals,
                    const mg_alignment_desc *alignment);
int mg_frame_constraint_width(const mg_frame_constraint_desc *constraint, int32_t n_times);
int mg_score_frame_constraint(mg_primitive *prim, const mg_frame_constraint_desc *constraint, const double *tracks_dev, int64_t n_samples,
                              int32_t n_times, int32_t n_joints, double *errors_dev, int accumulate, double *residuals_dev);
/* The per-frame constraints WITHOUT frames in memory (two launches for a whole constraint list) -- what the reference does per candidate in
 * MotionPrimitiveConstraints.evaluate (constraints/motion_primitive_constraints.py:96-118): back-project, align to the previous frames
 * (:106-116), then every constraint's evaluate_motion_spline over skeleton.nodes[joint].get_global_position(frame) of every frame
 * (spatial_constraints/trajectory_constraint.py:79-121, keyframe_constraints/global_transform_ca_constraint.py:33-46, ...):
 * mg_joint_tracks: the tracks (n, T, joints, 3) float64 that mg_back_project_frames_f64 -> mg_align_frames -> mg_joint_positions give
 * through (n, T, n_dim) float64 frames -- ~98 KB of traffic per 'walk' candidate -- from ONE launch that keeps a candidate's control
 * points of the channels the joints' chains read in LDS: the same operations on the same values (bit-identical tracks), 24 bytes per
 * (candidate, time, joint) written.  A plan (mg_track_plan_create) fixes up to 4 requests = (time grid at the call, 1 .. 8 joints);
 * align_joint = the node candidates are aligned through when mg_joint_tracks gets an alignment (0: the root; -1: never aligned).
 * mg_score_frame_constraints: a LIST of constraints over those tracks in one launch per 4 constraints, errors added in list order
 * (what mg_score_frame_constraint gives called once per constraint with accumulate; a joint's trajectory constraint, MG_FRAME_JOINT_TRAJECTORY,
 * below 65 536 candidates as a launch of mg_score_trajectory_points at its place in the order); residuals_dev: NULL, or one pointer (or
 * NULL) per constraint. */
typedef struct mg_track_plan mg_track_plan;
int mg_track_plan_create(mg_primitive *prim, const mg_skeleton_desc *skeleton, int32_t n_requests, const int32_t *n_joints, const int32_t *joints,
                         int32_t align_joint, mg_track_plan **out);
void mg_track_plan_destroy(mg_track_plan *plan);
int mg_joint_tracks(mg_track_plan *plan, const void *latents, int dtype, int64_t n_samples, int64_t ld, const mg_alignment_desc *alignment,
                    const mg_time_grid *const *grids, double *const *tracks_dev);
int mg_score_frame_constraints(mg_primitive *prim, int32_t n_constraints, const mg_frame_constraint_desc *const *constraints, const double *const *tracks_dev,
                               const int32_t *n_times, const int32_t *n_joints, int64_t n_samples, double *errors_dev, int accumulate,
                               double *const *residuals_dev);

/* A planner step's per-frame constraint lists AND the options' first minima, for options whose candidates and errors are on the device
 * already (mg_options_step drew them and scored their keyframe constraints, mg_score_trajectories added their root trajectories) -- the
 * reference scores every option's whole constraint list inside one planner step (motion_generator/graph_walk_planner.py:184-226,
 * constraints/motion_primitive_constraints.py:100-122): TWO launches whatever the number of options (every option's joint tracks;
 * every option's list + its first minimum under mg_argmin_first's rule) and one read-back of the result records.
 *   plans[k]: NULL for an option without a per-frame list (its first minimum is still taken); grids, tracks_dev:
 *   [n_options][MG_TRACK_MAX_REQUESTS] (unused requests NULL; grids NULL = the canonical grid); constraints: [n_options][MG_FRAME_LIST_MAX],
 *   n_constraints[k] <= MG_FRAME_LIST_MAX of them used (no MG_FRAME_JOINT_ROTATION: it reads a frame), request_of[k][i]: the plan's request
 *   whose tracks constraint i reads; errors_dev[k] (n_samples) float64: read, added to, written back; results_dev: record k at
 *   k * result_stride = {int64 index, float64 error, float64 latent[n_gmm_dims]}; results_host: NULL or where the records are copied.
 * The additions are mg_joint_tracks + mg_score_frame_constraints' per option, in list order: the same errors, the same winners. */
#define MG_TRACK_MAX_REQUESTS 4
#define MG_FRAME_LIST_MAX 4
int mg_options_frame_lists(int32_t n_options, mg_primitive *const *prims, mg_track_plan *const *plans, const void *const *latents_dev, int latent_dtype,
                           int64_t n_samples, const int64_t *ld, const mg_alignment_desc *const *alignments, const mg_time_grid *const *grids,
                           double *const *tracks_dev, const int32_t *n_constraints, const mg_frame_constraint_desc *const *constraints,
                           const int32_t *request_of, double *const *errors_dev, void *results_dev, int64_t result_stride, void *results_host);

/* ---- hot path, device pointers ------------------------------------------------------ */

/* MotionPrimitive.back_project(s, False).get_motion_vector() for a batch
 * (reference motion_primitive.py:206-256 + motion_spline.py:71-86), or
 * MotionSpline.evaluate(t) when grid holds arbitrary times (motion_spline.py:89-92).
 * latents: (B, ld) of latent_dtype, first n_components columns used.
 * frames_dev: (B, T, D) float32, written completely.  grid NULL = canonical grid. */
int mg_back_project_frames(mg_primitive *prim, const mg_time_grid *grid,
                           const void *latents_dev, int latent_dtype, int64_t n_samples, int64_t ld,
                           float *frames_dev, int path);

/* Same in float64 throughout (all channels), frames_dev (B, T, D) float64.  Used by the
 * single-sample adaptor calls where the reference's float64 results are expected. */
int mg_back_project_frames_f64(mg_primitive *prim, const mg_time_grid *grid,
                               const void *latents_dev, int latent_dtype, int64_t n_samples, int64_t ld,
                               double *frames_dev);

/* MotionPrimitive.back_project_spatial_coeffs for a batch
 * (reference motion_primitive.py:236-256): coeffs_dev (B, NB, D), float64 when
 * out_dtype == MG_F64 else float32. */
int mg_back_project_coeffs(mg_primitive *prim, const void *latents_dev, int latent_dtype,
                           int64_t n_samples, int64_t ld, void *coeffs_dev, int out_dtype);

/* MotionSpline.get_motion_vector()/evaluate(t) from explicit coefficient arrays
 * (reference motion_spline.py:71-92; callers overwrite spline.coeffs with aligned
 * coefficients, motion_primitive_constraints.py:113): coeffs_dev (n, NB, D) float64 ->
 * frames_dev (n, T, D) float64. */
int mg_spline_evaluate(mg_primitive *prim, const mg_time_grid *grid, const double *coeffs_dev,
                       int64_t n_splines, double *frames_dev);

/* GaussianMixture.score_samples (reference motion_primitive.py:126-144; formula twin
 * extended_mgrd_mixture_model.py:60-108): per-row log p(x), float64 arithmetic.
 * x_dev (B, ld) of x_dtype; logp_dev (B) of out_dtype. */
int mg_gmm_log_prob(mg_primitive *prim, const void *x_dev, int x_dtype, int64_t n_samples, int64_t ld,
                    void *logp_dev, int out_dtype);

/* log_likelihood_jac (reference optimization/objective_functions.py:95-107, inlined again at :190-206):
 * sum_k N_k(x) w_k Sigma_k^-1 (x - mu_k) / p(x) = -grad log p(x), float64; rows where the reference's
 * denominator exp(score(x)) underflows to 0 are all ones, as there.  jac_dev (n_samples, n_components). */
int mg_gmm_log_prob_jac(mg_primitive *prim, const void *x_dev, int x_dtype, int64_t n_samples, int64_t ld,
                        double *jac_dev);

/* GaussianMixture.sample on the device (reference motion_primitive.py:182-189):
 * Philox4x32-10 + Box-Muller + Cholesky; rows grouped by component like sklearn, but NOT
 * bit-compatible with sklearn's Mersenne stream (validated distributionally).  The standard normals
 * carry float32 precision (the uniforms carry 32 bits; Box-Muller on the float32 transcendental units),
 * x = mu + z L^T is float64 arithmetic; same seed, same rows -> same bits on gfx950.
 * counts: host array (K) of rows per component summing to n_samples.
 * x_dev (n, ld) of x_dtype, component_dev (n) int32 or NULL. */
int mg_gmm_sample(mg_primitive *prim, int64_t n_samples, const int64_t *counts, uint64_t seed,
                  void *x_dev, int x_dtype, int64_t ld, int32_t *component_dev);
/* Rows [row_begin, row_begin + row_count) of that same draw of n_samples rows, bit for bit (the generator is counter based: a
 * row's values depend on (seed, row, column group) only): x_dev (row_count, ld), component_dev (row_count).  What a rank of a
 * sharded step draws: the union over the ranks' contiguous blocks IS the single-GPU draw. */
int mg_gmm_sample_rows(mg_primitive *prim, int64_t n_samples, const int64_t *counts, uint64_t seed, int64_t row_begin, int64_t row_count,
                       void *x_dev, int x_dtype, int64_t ld, int32_t *component_dev);

/* ---- fused candidate scoring ------------------------------------------------------------
 * MotionPrimitiveConstraints.evaluate summed over root-joint keyframe constraints
 * (reference motion_primitive_constraints.py:100-122, local-coordinate mode: no
 * alignment), float64 arithmetic, without materialising frames. */
int mg_constraint_set_create(mg_primitive *prim, const mg_keyframe_constraint *cons, int32_t n,
                             mg_constraint_set **out);
/* the same with a skeleton, which MG_CONSTRAINT_JOINT_POSITION constraints need (chains of <= MG_MAX_CHAIN joints) */
int mg_constraint_set_create_fk(mg_primitive *prim, const mg_skeleton_desc *skeleton,
                                const mg_keyframe_constraint *cons, int32_t n, mg_constraint_set **out);
/* global-coordinate mode: every candidate is aligned to the previous motion before its constraints are evaluated
 * (alignment may be NULL = local mode; skeleton may be NULL when no constraint and no alignment needs a chain) */
int mg_constraint_set_create_aligned(mg_primitive *prim, const mg_skeleton_desc *skeleton,
                                     const mg_keyframe_constraint *cons, int32_t n,
                                     const mg_alignment_desc *alignment, mg_constraint_set **out);
/* New targets, weights and reference vectors -- and a new previous frame for the alignment -- for a set whose
 * STRUCTURE stays the same: the same types, joints, keyframes and relative points in the same order, alignment to
 * the same joint (or none).  That is a planner's situation: every step it scores the same kind of constraints with
 * new goals and a new previous motion (graph_walk_planner.py:155-214).  Stream ordered (launches scored before
 * the call see the old values, later ones the new), one small launch, no allocation, no synchronisation;
 * building a new set costs about 200 us, this a few.  MG_ERR_INVALID_ARGUMENT if the structure differs. */
int mg_constraint_set_update(mg_constraint_set *cs, const mg_keyframe_constraint *cons, int32_t n,
                             const mg_alignment_desc *alignment);
/* the general form: MG_CONSTRAINT_POSE entries of `cons` refer to poses[cons[c].joint]; keyframe and weight come
 * from the mg_keyframe_constraint as for every other type.  (mg_constraint_set_update refuses sets with poses.) */
int mg_constraint_set_create_full(mg_primitive *prim, const mg_skeleton_desc *skeleton,
                                  const mg_keyframe_constraint *cons, int32_t n,
                                  const mg_pose_constraint *poses, int32_t n_poses,
                                  const mg_alignment_desc *alignment, mg_constraint_set **out);
void mg_constraint_set_destroy(mg_constraint_set *cs);
int mg_score_constraints(mg_primitive *prim, const mg_constraint_set *cs,
                         const void *latents_dev, int latent_dtype, int64_t n_samples, int64_t ld,
                         void *errors_dev, int out_dtype);

/* The optimiser's objective for a batch in ONE launch: obj[b] = error_scale * err[b] + quality_scale * (-log p(s_b))
 * (reference optimization/objective_functions.py:163-185, obj_spatial_error_sum_and_naturalness; err = what mg_score_constraints
 * returns, log p = what mg_gmm_log_prob returns in float64 -- the same bits: the wave that holds a 16-candidate tile's latents for
 * the mixture scores the constraints on them, and the products and the sum are rounded one by one like NumPy's array arithmetic).
 * logp_out / err_out / obj_out: (n) float64 device pointers, any of them NULL.  Covers sets of root position / 2-D direction
 * constraints (path following), local or aligned through the root joint; MG_ERR_UNSUPPORTED for anything else -- joint
 * constraints, a mixture over time latents, more than 64 dimensions: the kernel runs four waves per SIMD and has no registers for
 * forward-kinematics chains -- then two calls (mg_score_constraints, mg_gmm_log_prob) give the same numbers. */
int mg_objective_error_and_naturalness(mg_primitive *prim, const mg_constraint_set *cs, const void *latents, int dtype, int64_t n, int64_t ld,
                                       double error_scale, double quality_scale, double *logp_out, double *err_out, double *obj_out);

/* MotionPrimitiveConstraints.get_residual_vector (reference motion_primitive_constraints.py:124-144) for the
 * same root-joint keyframe constraints: residuals_dev (n_samples, n_constraints) float64 row-major, entry
 * [b][c] = weight_c * error_c(sample b); feeds the batched forms of obj_spatial_error_residual_vector[_and_
 * naturalness] (reference optimization/objective_functions.py:209-267). */
int mg_score_constraint_residuals(mg_primitive *prim, const mg_constraint_set *cs, const void *latents_dev,
                                  int latent_dtype, int64_t n_samples, int64_t ld, double *residuals_dev);

/* The same matrix with EVERY candidate aligned to ITS OWN previous motion: align_cand_dev (n_samples, 4) float64 = per candidate
 * the previous unit heading (x, z) and the previous root position (x, z), in place of the one record the set was made with (the
 * set must have a previous-frame alignment: its node, chain and reference vector are used).  The steps of a graph walk chained on
 * the device: step i's MG_CONSTRAINT_VALUE_* columns are step i + 1's align_cand (obj_global_error_sum and its residual-vector
 * forms, reference optimization/objective_functions.py:290-380, for a whole batch of concatenated latent vectors). */
int mg_score_constraint_residuals_chained(mg_primitive *prim, const mg_constraint_set *cs, const void *latents_dev, int latent_dtype,
                                          int64_t n_samples, int64_t ld, const double *align_cand_dev, double *residuals_dev);

/* Which kernel mg_score_constraints, mg_score_constraint_residuals[_chained] and mg_best_candidate launch for n_samples >= 1 candidates
 * against this set, stated once (mg_score_route_of in csrc/mg_score_route.h) and readable without a launch, under the context's
 * MG_OPT_SCORE_KERNEL and MG_OPT_FORCE_VALU_SCORE.  rows / row_tiles: the rows of the set's fused keyframe matrices and their 16-row
 * tiles (0 / 0 for a set without the matrix-pipe image: no constraints, or more than 64 components).  The wide kernel holds ONE row
 * tile: only sets of at most 16 rows take it, whatever the option or the batch size; every other set takes the tile kernel.
 * MG_ERR_UNSUPPORTED, with mg_score_constraints' text, where that call reports it.  Launches nothing. */
#define MG_SCORE_KERNEL_VALU 0   /* mg_score_kernel: a lane per candidate, the constraints dealt over four waves */
#define MG_SCORE_KERNEL_TILE 1   /* mg_score_mfma_kernel: a wave per 16 candidates */
#define MG_SCORE_KERNEL_WIDE 2   /* mg_score_mfma64_kernel: a wave per 64 candidates */
typedef struct mg_score_plan_info {
    int32_t kernel, lds_opt_in, rows, row_tiles;
    int64_t lds_bytes, workgroups;
} mg_score_plan_info;
int mg_score_plan(const mg_primitive *prim, const mg_constraint_set *cs, int64_t n_samples, mg_score_plan_info *out);

/* The argmin rule of evaluate_samples_using_constraints
 * (reference motion_primitive_generator.py:251-257): FIRST strict minimum, NaN never
 * wins, (0, +inf) when nothing wins.  values_dev (n) of dtype; result written to host. */
int mg_argmin_first(mg_context *ctx, const void *values_dev, int dtype, int64_t n,
                    int64_t *best_index, double *min_value);
/* device-side result for use inside a stream: out_dev = {int64 index, float64 value} (16 bytes) */
int mg_argmin_first_dev(mg_context *ctx, const void *values_dev, int dtype, int64_t n, void *out_dev);

/* One bench "step": frames (float32, MFMA path) + log p(x) (float32) for the same
 * latent batch, enqueued back to back on the context's stream. */
int mg_step_frames_and_logp(mg_primitive *prim, const void *latents_dev, int latent_dtype,
                            int64_t n_samples, int64_t ld, float *frames_dev, float *logp_dev);

/* What mg_step_frames_and_logp would launch for n_samples FLOAT32 latents, without launching (for profiles and logs):
 * plan[0] = frames kernel (0 = the plain VALU kernel, 1 = tile-major LDS-staged, 2 = chunk-stationary LDS-staged),
 * plan[1] = 1 when log p(x) is scored inside the frames kernel (one launch per step), 0 when it is a second launch,
 * plan[2] = workgroups, plan[3] = LDS bytes per workgroup.  For float64 latents use mg_step_plan_dtype: from 49 latent
 * components on, float64 latents keep the tile-major kernel where float32 ones get the chunk-stationary kernel. */
int mg_step_plan(const mg_primitive *prim, int64_t n_samples, int32_t plan[4]);
/* The same (float32 latents) for a given output buffer: where the frames go can change the kernel -- a piece of a placed region
 * whose scan found only slow-class memory (mg_device_malloc) is written by the tile-major kernel, which is the faster one there
 * (frames_dev NULL: mg_step_plan). */
int mg_step_plan_for(const mg_primitive *prim, int64_t n_samples, const void *frames_dev, int32_t plan[4]);
/* The same for latents of the given dtype (MG_F32: mg_step_plan_for; MG_F64: what a step over float64 latents launches). */
int mg_step_plan_dtype(const mg_primitive *prim, int64_t n_samples, const void *frames_dev, int latent_dtype, int32_t plan[4]);

/* evaluate_samples_using_constraints (reference motion_primitive_generator.py:230-261) in one call: score all
 * candidates against the set, first-minimum argmin, result on the host (no allocation, one synchronisation). */
int mg_best_candidate(mg_primitive *prim, const mg_constraint_set *cs, const void *latents_dev, int latent_dtype,
                      int64_t n_samples, int64_t ld, int64_t *best_index, double *min_error);

/* One outgoing option of a planner step (reference graph_walk_planner.py:184-226), enqueued WITHOUT
 * synchronisation: n candidates from the device sampler (counts per mixture component like mg_gmm_sample) into
 * x_dev (n, ld), their errors into errors_dev (n) float64, and into result_dev the first-minimum
 * {int64 index, float64 error} followed by the winning latent as float64[n_components].  Enqueue all options of a
 * step, synchronise once, read the results. */
int mg_option_step(mg_primitive *prim, const mg_constraint_set *cs, int64_t n_samples, const int64_t *counts,
                   uint64_t seed, void *x_dev, int x_dtype, int64_t ld, double *errors_dev, void *result_dev);

/* ALL outgoing options of a planner step (reference graph_walk_planner.py:184-226: the loop over `options`) in one call:
 * mg_option_step for option k with prims[k], csets[k], counts[k], seeds[k], x_dev[k] (n, ld[k]), errors_dev[k]; result
 * record k at results_dev + k * result_stride bytes (result_stride >= 16 + 8 * n_gmm_dims of every option, a multiple
 * of 8).  All primitives must live in one context.  results_host != NULL: the n_options * result_stride bytes are
 * copied back and the stream is synchronised once -- one round trip for the whole step. */
int mg_options_step(int32_t n_options, mg_primitive *const *prims, const mg_constraint_set *const *csets, int64_t n_samples,
                    const int64_t *const *counts, const uint64_t *seeds, void *const *x_dev, int x_dtype, const int64_t *ld,
                    double *const *errors_dev, void *results_dev, int64_t result_stride, void *results_host);

/* mg_options_step with the COMPONENT COUNTS DRAWN ON THE DEVICE: what GaussianMixture.sample draws with
 * numpy.random.multinomial(n, weights) (reference motion_primitive.py:182-189; 4 us of host time per option) becomes the histogram
 * of n categorical draws per option, keyed by the option's seed:
 *     u_i = (Philox4x32-10(counter = (i >> 2, 0, 0, 0x636e7473), key = seed)[i & 3] + 0.5) / 2^32,   i = 0 .. n_samples - 1
 *     counts[c] = #{i : cum[c-1] <= u_i < cum[c]}, cum = cumulative normalised weights (float64), the last component takes the rest.
 * Distributed like NumPy's counts, NOT NumPy's stream (the status of the device sampler itself); given the counts the step is the one
 * mg_options_step makes, bit for bit.  Two launches per step -- ONE when the step before, run with every seed one less, drew this step's
 * counts ahead (its kernel always draws for seed + 1: a planner counts its steps) -- and no host work per option; the kernels leave
 * the result records (and the counts) in pinned host memory themselves, so results_host / counts_host cost one synchronisation and no copy.
 * counts_host (may be NULL): [n_options][16] int64.  At most 24 options; MG_ERR_UNSUPPORTED where an option does not run on the
 * one-launch kernel (more than 16 components, more than 64 mixture dimensions, a VALU kernel forced): draw on the host then. */
int mg_options_step_device_counts(int32_t n_options, mg_primitive *const *prims, const mg_constraint_set *const *csets, int64_t n_samples,
                                  const uint64_t *seeds, void *const *x_dev, int x_dtype, const int64_t *ld,
                                  double *const *errors_dev, void *results_dev, int64_t result_stride, void *results_host, int64_t *counts_host);

/* One rank's share of a step sharded over GPUs (contiguous candidate blocks, constants replicated): the same
 * calls restricted to the global rows [row_begin, row_begin + row_count) of every option's draw of n_samples candidates.
 * x_dev (row_count, ld) and errors_dev (row_count) hold the block; the index in a result record is the GLOBAL row, so the
 * records of all ranks combine by (smaller error, then smaller index) into exactly the single-GPU result. */
int mg_option_step_rows(mg_primitive *prim, const mg_constraint_set *cs, int64_t n_samples, const int64_t *counts, uint64_t seed,
                        int64_t row_begin, int64_t row_count, void *x_dev, int x_dtype, int64_t ld, double *errors_dev, void *result_dev);
int mg_options_step_rows(int32_t n_options, mg_primitive *const *prims, const mg_constraint_set *const *csets, int64_t n_samples,
                         const int64_t *const *counts, const uint64_t *seeds, int64_t row_begin, int64_t row_count,
                         void *const *x_dev, int x_dtype, const int64_t *ld, double *const *errors_dev, void *results_dev,
                         int64_t result_stride, void *results_host);

/* ---- cluster-tree search (reference space_partitioning/feature_cluster_tree.py:129-187) --------
 * A FeatureClusterTree flattened on the host: node 0 is the root; means (n_nodes, dim) float64, row i the mean of node
 * i (its first n_components entries are what the objective scores); the children of node i are
 * children[child_begin[i] .. child_begin[i + 1]) in the reference's order (CSR, child_begin has n_nodes + 1 entries,
 * child_begin[n_nodes] = n_nodes - 1); first_index[i] = indices[0] of node i, the row of the tree's data a leaf
 * stands for (-1: the node has no indices -- allowed for the root and inner nodes only).  Validated: every node
 * but the root has exactly one parent and is reachable from it (no cycles), depth <= MG_TREE_MAX_DEPTH, at most
 * MG_TREE_MAX_CHILDREN children per node, leaf rows in [0, n_rows), dim >= n_components.  Uploaded once. */
typedef struct mg_cluster_tree mg_cluster_tree;
#define MG_TREE_MAX_DEPTH 64
#define MG_TREE_MAX_CHILDREN 256
#define MG_TREE_MAX_CANDIDATES 64
/* flags of a search record */
#define MG_TREE_TIE 1          /* two equal values met in a heap comparison: the reference raises TypeError there */
#define MG_TREE_NO_RESULT 2    /* no leaf reached (the reference's "failed to find a result"): value +inf, the root's row */
#define MG_TREE_OVERFLOW 4     /* a heap outgrew its bound (cannot happen for a validated tree; the record is not to be used) */
#define MG_TREE_NO_MEAN 8      /* KD trees: the search expanded a non-leaf node whose children are KD trees; the reference raises
                                  AttributeError ('KDTreeWrapper' object has no attribute 'mean') there.  Row and leaf are -1. */
typedef struct mg_tree_search_record {
    int64_t row;               /* first_index of the winning leaf: the data row the search returns (-1: none) */
    int32_t leaf;              /* the winning leaf node */
    int32_t flags;             /* MG_TREE_* */
    int64_t evaluations;       /* objective evaluations: the children scored over the whole descent */
    double value;              /* the winning leaf's value: the objective of its mean (+inf for a root that is a leaf) */
} mg_tree_search_record;
int mg_cluster_tree_create(mg_primitive *prim, int32_t n_nodes, int32_t dim, const double *means, const int32_t *child_begin,
                           const int32_t *children, const int64_t *first_index, int64_t n_rows, mg_cluster_tree **tree);
void mg_cluster_tree_destroy(mg_cluster_tree *tree);
/* find_best_example_excluding_search_candidates(obj, args, n_candidates) for n_searches (prim, tree, constraint set)
 * triples in ONE launch, a workgroup per search: per level every frontier node's children are scored against the set
 * (bit for bit what mg_score_constraints gives for the child's mean), pushed onto a heap per node whose list's first
 * n_candidates entries go onto the level's heap, whose list's first n_candidates entries are the next frontier; leaves
 * go onto the results heap, whose root is the answer.  All primitives and trees in one context; 1 <= n_candidates <=
 * MG_TREE_MAX_CANDIDATES.  records_dev: n_searches records (device memory). */
int mg_cluster_tree_search(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                           const mg_constraint_set *const *csets, int32_t n_candidates, mg_tree_search_record *records_dev);
/* The same launch with root trajectory constraints in the objective (what MotionPrimitiveConstraintsBuilder appends to every
 * primitive's list for path following): search s scores, behind its keyframe set, the trajectory_counts[s] trajectories
 * trajectories[off .. off + count) of the flat arrays (off = the counts before s added up) with their min_u and weights, in list
 * order, aligned by alignments[s]: NULL, a previous-frame record whose joint is the root (0), or a start-pose record -- what
 * mg_score_trajectory accepts.  A row's value has the bits of mg_score_constraints followed by mg_score_trajectory(...,
 * accumulate = 1) per trajectory on the canonical grid, with the context's MG_OPT_TRAJECTORY_SEARCH.  trajectory_counts NULL:
 * no search has any; alignments NULL: none is aligned; a search without trajectories ignores its alignment entry.  Zero
 * trajectories everywhere is mg_cluster_tree_search, byte for byte.  0 <= count <= MG_TREE_MAX_TRAJECTORIES, every trajectory
 * made for its search's primitive; otherwise MG_ERR_INVALID_ARGUMENT, as for a mix of tree kinds; another aligning joint:
 * MG_ERR_UNSUPPORTED.  Nothing is launched on an error.  The launch is timed on profile slot 11. */
#define MG_TREE_MAX_TRAJECTORIES 4
int mg_cluster_tree_search_trajectories(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                        const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                        const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                        const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_search_record *records_dev);

/* What that launch would stage in LDS, readable without a launch: the same validation and the same maxima over the call's searches
 * (latents, constraints, rows of W, root rows 3 NB + 4, polynomial doubles 12 n_seg + 3, trajectory slots, the trees' widths and
 * depths), then the ladder a plan beyond the workgroup's LDS is retried by (W read from memory, then the polynomials, then the
 * root rows).  lds_bytes: the plan's dynamic LDS; w_rows / root_rows / poly_doubles: what is staged (0: read from memory, or
 * nothing to stage); trajectory_slots: the longest trajectory list; lds_opt_in: the plan needs more than 64 KiB; refused: no rung
 * fits and the search returns MG_ERR_UNSUPPORTED (the query itself returns MG_OK and the bare plan's size).  The arguments of
 * mg_cluster_tree_search_trajectories without the records; errors as there.  Launches nothing, uploads nothing. */
typedef struct mg_tree_search_plan_info {
    int64_t lds_bytes;
    int32_t w_rows, root_rows, poly_doubles, trajectory_slots, lds_opt_in, refused;
} mg_tree_search_plan_info;
int mg_cluster_tree_search_plan(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_search_plan_info *out);

/* The same launch with PER-FRAME constraints in the objective (the lists of the pick / carry actions and of the collision-avoidance
 * pass: a collision-avoidance position, a discrete trajectory, a local trajectory or trajectory set looked up by walked arc length, a
 * joint rotation, a joint's trajectory constraint): search s scores, behind its keyframe set and its root trajectories, the
 * n_constraints[s] <= MG_FRAME_LIST_MAX descriptors constraints[s][.] in list order -- the additions of
 * candidate_scoring.errors_of_samples (mg_score_constraints, mg_score_trajectory per trajectory, then mg_joint_tracks +
 * mg_score_frame_constraints, a joint rotation at its place in the list), with the same statements (csrc/mg_frame_device.h).
 * Everything mg_cluster_tree_search_trajectories takes, both tree kinds, several searches per launch, and per search:
 *   plans[s]           the track plan of the search's primitive (mg_track_plan_create: the requests' joints, the aligning joint); NULL
 *                      with n_constraints[s] = 0: the search has no list (it is scored as mg_cluster_tree_search_trajectories scores it)
 *   grids[s][q]        request q's time grid (NULL: the canonical grid), q < MG_TRACK_MAX_REQUESTS
 *   constraints[s][i]  the descriptors, as mg_score_frame_constraints / mg_options_frame_lists take them; request_of[s][i]: the plan's
 *                      request whose tracks constraint i reads (ignored for MG_FRAME_JOINT_ROTATION)
 *   rotation_grids[s][i]  MG_FRAME_JOINT_ROTATION only: a one-sample grid of the primitive at the constraint's frame index
 * alignments[s] aligns the search's trajectories AND its tracks (a previous-frame record's joint is the plan's aligning joint; with
 * trajectories that is the root).  Per chunk of 64 children the workgroup forms the children's joint tracks -- the control points of
 * the channels the joints' chains read, MG_TREE_TRACK_GROUP children at a time in LDS, four taps per channel and frame, the candidate's
 * aligning transform, the chain -- into the search's slab of scratch_dev, and behind a barrier a lane per child runs the chain scorers.
 * scratch_dev: device memory of at least mg_cluster_tree_search_frames_plan's scratch_bytes, 16-byte aligned, owned by the caller and
 * free again when the launch has finished.  The lists' trajectory tables stand in LDS where they fit on the rung the plan took
 * (further rungs of the ladder: after W, the polynomials and the root rows, the lists' tables are read from memory, then the track
 * group is halved down to one child).  No rung fits, or the slabs exceed 256 MiB: MG_ERR_UNSUPPORTED, nothing launched.  No search with
 * a list: mg_cluster_tree_search_trajectories, byte for byte.  The launch is timed on profile slot 11. */
typedef struct mg_tree_frame_lists {
    mg_track_plan *const *plans;                          /* [n_searches] */
    const mg_time_grid *const *grids;                     /* [n_searches][MG_TRACK_MAX_REQUESTS] */
    const int32_t *n_constraints;                         /* [n_searches] */
    const mg_frame_constraint_desc *const *constraints;   /* [n_searches][MG_FRAME_LIST_MAX] */
    const int32_t *request_of;                            /* [n_searches][MG_FRAME_LIST_MAX] */
    const mg_time_grid *const *rotation_grids;            /* [n_searches][MG_FRAME_LIST_MAX], NULL where there are no joint rotations */
} mg_tree_frame_lists;
int mg_cluster_tree_search_frames(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                  const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                  const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                  const mg_alignment_desc *const *alignments, const mg_tree_frame_lists *lists, int32_t n_candidates,
                                  void *scratch_dev, int64_t scratch_bytes, mg_tree_search_record *records_dev);
/* What that launch would stage, readable without a launch: mg_tree_search_plan_info's fields (lds_bytes: the whole dynamic LDS, the
 * lists' regions included), then track_group (children whose control points stand in LDS side by side; 0: no search has a list),
 * control_points (NB x kept channels of the widest list), tables_lds / table_bytes (the lists' tables staged, and their bytes) and
 * scratch_bytes (what scratch_dev must hold).  Launches nothing, uploads nothing. */
typedef struct mg_tree_frames_plan_info {
    int64_t lds_bytes;
    int32_t w_rows, root_rows, poly_doubles, trajectory_slots, lds_opt_in, refused;
    int32_t track_group, control_points, tables_lds, pad;
    int64_t table_bytes, scratch_bytes;
} mg_tree_frames_plan_info;
int mg_cluster_tree_search_frames_plan(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                       const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                       const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                       const mg_alignment_desc *const *alignments, const mg_tree_frame_lists *lists, int32_t n_candidates,
                                       mg_tree_frames_plan_info *out);

/* ---- k-means / KD cluster tree (reference space_partitioning/cluster_tree.py:117-149, cluster_tree_node.py:63-138,
 * kdtree.py:132-164,233-250) ----
 * The ClusterTree of a pickled model, flattened on the host.  Cluster nodes breadth first (node 0 the root): their
 * k-means children in CSR form as for mg_cluster_tree_create (child_begin (n_nodes + 1), children (n_nodes - 1)); leaf[i]
 * the node's `leaf` flag; its KDTreeWrapper children as the KD roots kd_roots[kd_begin[i] .. kd_begin[i + 1]).  KD node
 * k: its point is row k of `points`, its children kd_left[k] / kd_right[k] (-1: none), kd_inner[k] its type == "inner".
 * points: (n_kd + n_nodes, dim) float64, the n_kd KD points followed by every cluster node's mean (row n_kd + i is node
 * i's mean).  Validated: the checks of mg_cluster_tree_create on the cluster nodes; a node has cluster children or KD
 * children, not both; a leaf has no cluster children; every KD node has one parent (a KD root is its cluster node's
 * child) and is reachable; KD depth <= MG_KD_MAX_DEPTH.  A non-leaf node with KD children is allowed: the search flags
 * MG_TREE_NO_MEAN when it expands one.  Destroyed with mg_cluster_tree_destroy.
 *
 * mg_cluster_tree_search takes these trees as well, one kind per call (a mix: MG_ERR_INVALID_ARGUMENT).  Per level the
 * frontier's inner nodes' children are scored and kept as for the other kind, with the reference's (value, idx, node)
 * tuples; every frontier leaf runs its KD descents in the same launch (root point, then at each inner node the right and
 * the left child's points, left only if strictly better), keeps (cost, depth) per descent, (value, point) per leaf and
 * (value, c_idx, point) over the search, comparing points lexicographically on equal values; a leaf without KD trees
 * scores its mean.  Every value has the bits mg_score_constraints gives for that points row.  The record: row = the
 * winning points row (>= n_kd: a leaf's mean), leaf = its cluster node, evaluations = every objective scored;
 * MG_TREE_NO_RESULT: row = n_kd (the root's mean). */
#define MG_KD_MAX_DEPTH 64
int mg_cluster_tree_create_kd(mg_primitive *prim, int32_t n_nodes, int32_t n_kd, int32_t dim, const double *points, const int32_t *child_begin,
                              const int32_t *children, const int32_t *leaf, const int32_t *kd_begin, const int32_t *kd_roots,
                              const int32_t *kd_left, const int32_t *kd_right, const int32_t *kd_inner, mg_cluster_tree **tree);

/* ---- batched k-means for building cluster trees (reference space_partitioning/cluster_tree_node_builder.py:83-100,
 * clustering.py:69-129: sklearn's KMeans(n_clusters=k).fit_predict, once per tree node) ----
 * Every segment s is the rows rows[seg_begin[s] .. seg_begin[s + 1]) of the device table points_dev (n_rows, dim) float64,
 * and all n_segments segments are clustered in one call, with sklearn's KMeans(algorithm="lloyd") semantics per segment:
 * greedy k-means++ (2 + int(ln k) candidates per centre; uniforms from Philox keyed by (seed, node_ids[s], run), node_ids
 * NULL = the segment index) or the caller's initial centres init (n_segments, k, dim; then n_init must be 1); Lloyd
 * iterations with float64 squared distances, ties to the lowest centre, an empty cluster taking the member farthest from
 * its centre (several: descending distance, first position on ties); stop on unchanged labels, on a summed squared centre
 * shift <= tol * mean(var(X, axis=0)) of the segment, or after max_iter iterations, then (not strictly converged) one
 * assignment-only pass.  Of n_init runs the one of least inertia is kept (the first on ties).  Bit-reproducible: no float
 * atomics, every sum in a fixed order.  Host arrays: seg_begin (n_segments + 1, seg_begin[0] = 0, every segment >= k rows),
 * rows (seg_begin[n_segments] entries in [0, n_rows)), outputs labels (one per position of rows), centres (n_segments, k,
 * dim), inertia and n_iter (n_segments).  Synchronises.  MG_ERR_UNSUPPORTED outside 1 <= dim <= 128, 2 <= k <= 64,
 * 1 <= n_init <= 16. */
int mg_kmeans_segments(mg_context *ctx, const double *points_dev, int64_t n_rows, int32_t dim, int32_t n_segments, const int64_t *seg_begin,
                       const int64_t *rows, int32_t k, int32_t n_init, const double *init, const uint64_t *node_ids, uint64_t seed,
                       int32_t max_iter, double tol, int32_t *labels, double *centres, double *inertia, int32_t *n_iter);

/* Batched EM of full-covariance Gaussian mixtures (GMMTrainer's AIC sweep: sklearn GaussianMixture(covariance_type='full',
 * init_params='kmeans', n_init=1) per fit, float64) over one device points table points_dev (n, dim).  Fit f has
 * n_comp[f] components and starts from the one-hot responsibilities of its labels labels_in[f * n .. f * n + n); the
 * M-step computes the covariances in two passes (means first) and adds reg_covar on the diagonal; the loop stops when the
 * lower bound changes by less than tol or after max_iter iterations; a final E-step gives the score (mean log p) and the
 * labels.  Every sum runs in an order fixed by (n, dim, K) alone: a fit gives the same bits alone or in any batch.
 * Outputs (host, components of all fits concatenated): weights (sum K), means (sum K, dim), covariances and
 * precisions_chol (sum K, dim, dim), lower_bounds (n_fits, max_iter; the first n_iter[f] entries set), n_iter, status
 * (1 converged, 2 stopped at max_iter, 3 ill-defined covariance: a non-positive or non-finite Cholesky pivot, which ends
 * that fit only), score (n_fits), labels_out (n_fits, n).  Synchronises.  MG_ERR_UNSUPPORTED outside 1 <= dim <= 64 and
 * 1 <= n_comp[f] <= 64. */
int mg_gmm_em_fit(mg_context *ctx, const double *points_dev, int64_t n, int32_t dim, int32_t n_fits, const int32_t *n_comp,
                  const int32_t *labels_in, double tol, double reg_covar, int32_t max_iter, double *weights, double *means,
                  double *covariances, double *precisions_chol, double *lower_bounds, int32_t *n_iter, int32_t *status,
                  double *score, int32_t *labels_out);

/* ---- functional PCA of aligned motions (reference construction/fpca), float64, synchronising, bit-reproducible ---- */
/* Least-squares cubic B-spline coefficients of a batch of motions: coeffs_dev (n_motions, n_basis, n_dims) =
 * operator . motions_dev[n] per motion, motions_dev (n_motions, n_frames, n_dims) and operator_dev (n_basis, n_frames) --
 * the least-squares operator of the (n_frames, n_basis) design matrix, factored once by the host -- on the device.  A
 * motion gives the same bits alone or in any batch.  MG_ERR_UNSUPPORTED outside n_basis <= 64 and n_frames <= 1024. */
int mg_spline_fit_batch(mg_context *ctx, const double *motions_dev, int64_t n_motions, int32_t n_frames, int32_t n_dims,
                        const double *operator_dev, int32_t n_basis, double *coeffs_dev);

/* PCA of the device matrix a_dev (n, p): mean (host, p) = column means (rows added in row order; zeros when centre is 0:
 * the matrix is taken as it is, as the reference's run_pca takes it), centred_dev (device, n, p) = a - mean, and the singular values (host, min(n, p), descending) and right singular vectors vt (host,
 * (min(n, p), p), rows) of the centred matrix by one-sided Jacobi on the short side, sweeps of round-robin pairs until a
 * whole sweep rotates no pair with |w_i . w_j| > eps sqrt(max(n, p)) |w_i| |w_j|.  n_sweeps: sweeps run; status: 1
 * converged, 2 stopped at the cap of 30 sweeps.  Sign rule: each row's entry of largest magnitude is positive (the first
 * one on ties).  A row whose singular value is at most eps max(n, p) times the largest has no direction of its own and is
 * completed orthonormally to the others.  MG_ERR_UNSUPPORTED outside min(n, p) <= 4096 and max(n, p) <= 2^20;
 * MG_ERR_INVALID_ARGUMENT for a matrix with non-finite values. */
int mg_pca_fit(mg_context *ctx, const double *a_dev, int64_t n, int64_t p, int32_t centre, double *centred_dev, double *mean,
               double *singular_values, double *vt, int32_t *n_sweeps, int32_t *status);

/* low_dev (n, l) = x_dev (n, p) . vt_dev (l, p)^T, and high_dev (n, p) = low_dev (n, l) . vt_dev (l, p) + mean_dev (p; may
 * be NULL); all on the device.  MG_ERR_UNSUPPORTED from n or p of 2^24 on. */
int mg_pca_project(mg_context *ctx, const double *x_dev, const double *vt_dev, int64_t n, int64_t p, int64_t l, double *low_dev);
int mg_pca_backproject(mg_context *ctx, const double *low_dev, const double *vt_dev, const double *mean_dev, int64_t n, int64_t p,
                       int64_t l, double *high_dev);

/* The LEADING principal components of the device matrix a_dev (n, p), for shapes beyond mg_pca_fit's short-side limit: as many as
 * sklearn's PCA(n_components = fraction) keeps, searchsorted(cumsum(ratio), fraction, side = "right") + 1 with ratio = s^2 / |a - mean|_F^2.
 * Blocked subspace iteration on (a - mean)^T (a - mean): Y = Xc Q^T and Z = Y^T Xc on the float64 MFMA GEMMs, the block re-orthonormalised
 * and ordered by mg_pca_fit(Z, centre = 0), until every kept component's residual |Xc^T Xc v - s^2 v| is at most tol s_1^2 or
 * max_iterations rounds have run (tol <= 0: 64 eps sqrt(max(n, p)); max_iterations <= 0: 100).  The block starts at 12 rows and doubles
 * until it captures more than `fraction` with four rows to spare.  mean (host, p): the column means as mg_pca_fit adds them; centred_dev
 * (device, n, p) = a - mean; *k: the components kept; singular_values, ratios (host, k_cap), vt (host, (k_cap, p)): their first *k
 * entries / rows, descending, each row's entry of largest magnitude positive; iterations: rounds run; status: 1 converged, 2 stopped at
 * the cap (the values are then the last round's).  Every sum runs in an order fixed by the shape: two calls give the same bits.
 * Synchronises.  MG_ERR_INVALID_ARGUMENT: NULL, n < 2, fraction outside (0, 1), non-finite values, a matrix without variance, or
 * *k > k_cap (*k then holds the count to ask again with).  MG_ERR_UNSUPPORTED only where an index would overflow -- n >= 2^24, p > 2^20,
 * 2^31 or more 16 x 16 tiles -- or where more than 4096 components (mg_pca_fit's limit for the block) would have to be kept. */
int mg_pca_fit_leading(mg_context *ctx, const double *a_dev, int64_t n, int64_t p, double fraction, double tol, int32_t max_iterations,
                       double *centred_dev, double *mean, int32_t k_cap, int32_t *k, double *singular_values, double *vt, double *ratios,
                       int32_t *iterations, int32_t *status);

/* ---- scaled functional PCA (reference construction/fpca/scaled_fpca.py, sfpca_objective_func): the joint-space error of the rank-npc
 * PCA reconstruction of feature-weighted spline coefficients, for a batch of weight vectors; float64, synchronising, bit-reproducible.
 * A weight vector has 3 + J entries, J = (n_dims - 3) / 4: one per root channel, one per joint (its four quaternion channels share it).
 * The weights enter only through the projector U_k U_k^T on the sample axis, U the eigenvectors of sum_g w_g^2 G_g with G_g the (n, n)
 * Gram matrix of group g's centred columns: mg_sfpca_create forms the G_g, the mean's and the centred samples' frames and
 * the originals' joint positions once; a call combines the G_g, finds the leading eigenvectors by one-sided Jacobi (mg_pca_fit's schedule,
 * stopping rule, cap of 30 sweeps and sign rule; the kept vectors' means taken out -- ones is the centring's null vector -- and one
 * Newton-Schulz step on them), and reconstructs, walks the chains and reduces in one fused kernel.
 *
 * mg_sfpca_create: coeffs_dev (n, n_basis, n_dims) float64 on the device, as mg_spline_fit_batch leaves it (read during the call only);
 * joints (n_joints_out) of `skeleton`: the joints whose global positions are compared; design (host, (n_sampled_frames, n_basis)): the
 * B-spline design rows at the sampled canonical frames.  MG_ERR_UNSUPPORTED, before anything is launched, outside 2 <= n <= 1024,
 * n_basis <= 64, J <= 64, n_sampled_frames <= 1024, n_joints_out <= 256, or for a chain of more than MG_MAX_CHAIN links;
 * MG_ERR_INVALID_ARGUMENT for NULL, n_dims not 3 + 4 J, a joint outside the skeleton, non-finite coefficients or design values.
 *
 * mg_sfpca_errors: weights (host, (m, n_weights)), n_weights == 3 + J, every entry > 0 and finite; 1 <= npc <= n - 1.  errors (host, m):
 * the mean over samples, sampled frames and listed joints of the squared distance between the joint's position in the reconstructed and in
 * the original motion, both evaluated from their control points through `design` and through mg_joint_positions' statements.  statuses
 * (host, m): 1 converged, 2 stopped at the sweep cap.  A weight vector gives the same bits alone or in any batch.
 *
 * mg_sfpca_projector: u_k (host, (n, npc)): the leading eigenvectors as columns, each column's entry of largest magnitude positive (the
 * first one on ties); a column whose eigenvalue is at most eps n times the largest is zero (it carries none of the data).  status as above. */
typedef struct mg_sfpca mg_sfpca;
int mg_sfpca_create(mg_context *ctx, const double *coeffs_dev, int32_t n, int32_t n_basis, int32_t n_dims, const mg_skeleton_desc *skeleton,
                    const int32_t *joints, int32_t n_joints_out, const double *design, int32_t n_sampled_frames, mg_sfpca **handle);
int mg_sfpca_errors(mg_sfpca *handle, const double *weights, int32_t m, int32_t n_weights, int32_t npc, double *errors, int32_t *statuses);
int mg_sfpca_projector(mg_sfpca *handle, const double *weights, int32_t n_weights, int32_t npc, double *u_k, int32_t *status);
void mg_sfpca_destroy(mg_sfpca *handle);

/* ---- temporal alignment: exact dynamic time warping of motions against one reference motion (reference construction/dtw.py),
 * float64, synchronising, bit-reproducible.  Motions are ragged: motion n has F_n = offsets[n + 1] - offsets[n] frames and its rows
 * start at row offsets[n] of a table; offsets is a HOST array of n_motions + 1 entries, offsets[0] = 0, rising.
 * MG_ERR_UNSUPPORTED outside n_ref_frames, F_n <= 1024 and n_joints <= 64; MG_ERR_INVALID_ARGUMENT for offsets that do not start at
 * 0 or do not rise, and for non-finite clouds or grids (found by a check kernel; the DTW kernels are then not launched).
 * n_motions = 0 is MG_OK and does nothing. ---- */
/* The distance grids S[n] (n_ref_frames, F_n), row-major, S[n] at grids_dev + n_ref_frames * offsets[n]: cell (i, j) = the MEAN over
 * the joints of the distance between the reference motion's cloud ref_cloud_dev[i] (n_joints, 3) and clouds_dev[offsets[n] + j]
 * after the weighted closed-form 2-D rigid fit (rotation about y, translation in x and z) of the latter onto the former; weights:
 * HOST array (n_joints), NULL = ones.  Formula and order of every sum: csrc/mg_dtw.hip.  PARITY UNPINNED (the reference's distance
 * is anim_utils' _transform_invariant_point_cloud_distance); the restatement is oracle/mg_oracle.py align_point_clouds_2d. */
int mg_dtw_distance_grids(mg_context *ctx, const double *ref_cloud_dev, int32_t n_ref_frames, const double *clouds_dev, const int64_t *offsets,
                          int64_t n_motions, int32_t n_joints, const double *weights, double *grids_dev);

/* Accumulated cost, optimal path and warping function per grid (get_distgrid's second half, find_path, get_warping_function):
 * D[0,0] = S[0,0], first column and row the running sums, D[i,j] = min(D[i-1,j-1], D[i-1,j], D[i,j-1]) + S[i,j]; back-steps to the
 * first minimum of (diagonal, (i-1, j), (i, j-1)).  Device outputs: accumulated_dev (laid out as the grids; NULL: not stored),
 * totals_dev (n_motions) = D[-1,-1], paths_dev: (i, j) int32 pairs front to back, motion n's at pair offsets[n] + n * (n_ref_frames
 * - 1) with room for n_ref_frames + F_n - 1, path_lengths_dev (n_motions) int32, warping_dev (n_motions, n_ref_frames) int32 = the
 * last j the path has in row i.  D, paths and totals are the reference's bit for bit for the same grids. */
int mg_dtw_paths(mg_context *ctx, const double *grids_dev, int32_t n_ref_frames, const int64_t *offsets, int64_t n_motions,
                 double *accumulated_dev, double *totals_dev, int32_t *paths_dev, int32_t *path_lengths_dev, int32_t *warping_dev);

/* warp_motion for a batch: warped_dev (n_motions, n_ref_frames, n_dim) row i of motion n = row warping_dev[n][i] of motion n's
 * frames in frames_dev (offsets[n_motions], n_dim).  MG_ERR_INVALID_ARGUMENT if an index lies outside its motion (nothing is read
 * for it). */
int mg_warp_motions(mg_context *ctx, const double *frames_dev, const int64_t *offsets, int64_t n_motions, int32_t n_dim,
                    const int32_t *warping_dev, int32_t n_ref_frames, double *warped_dev);

/* All-pairs costs (what the reference's find_optimal_dtw averages per candidate reference motion, construction/dtw.py:125-146):
 * costs_dev (n_refs, n_motions), row-major: costs[r][n] = D[-1,-1] of the DTW of reference motion ref_indices[r] and motion n, both
 * from the one ragged table clouds_dev (offsets[n_motions], n_joints, 3): bit for bit the totals value mg_dtw_paths returns for the
 * grid mg_dtw_distance_grids computes for that pair.  No grid, accumulated cost or path is stored; the call's device block holds the
 * offsets, the weights and the reference indices only.  ref_indices: HOST array (n_refs) of motion indices; NULL = all motions in
 * order, and then n_refs must equal n_motions.  The matrix is not symmetric (the fit of B onto A is not bitwise that of A onto B).
 * weights: HOST array (n_joints), NULL = ones.  MG_ERR_UNSUPPORTED for n_joints > 64 or a motion of more than 1024 frames;
 * MG_ERR_INVALID_ARGUMENT for a NULL argument, offsets that do not start at 0 or do not rise, a reference index outside
 * [0, n_motions), n_refs < 0, and non-finite clouds: those are found by the check kernel that runs in front of the pairs and are
 * answered when the call's one synchronisation returns; costs_dev is then without meaning.  Everything else is answered before any
 * launch.  n_motions = 0 or n_refs = 0 is MG_OK and writes nothing.  A pair gives the same bits alone or in any batch. */
int mg_dtw_pair_costs(mg_context *ctx, const double *clouds_dev, const int64_t *offsets, int64_t n_motions, int32_t n_joints,
                      const double *weights, const int64_t *ref_indices, int64_t n_refs, double *costs_dev);

/* ---- spatial alignment and the per-frame preparation in front of the fPCA (reference construction/motion_model_constructor.py
 * _align_frames_spatially, :244-263, and :359-360; construction/utils.py rotate_frames, normalize_root_translation,
 * align_quaternion_frames), float64, synchronising, bit-reproducible.  A frame is (x, y, z) of the root, then J quaternions
 * (w, x, y, z), the root's first.  Statement for statement: csrc/mg_spatial_align.hip. ---- */
/* out_dev (offsets[n_motions], n_dim) = every motion of frames_dev (ragged as above, no 1024-frame limit) turned about y so that the
 * heading of its frame frame_idx -- x and z of its normalised root quaternion applied to (0, 0, 1), normalised -- is
 * ref_orientation[2] (HOST, normalised by the call), and moved so that the turned root position of that frame is (0, 0, 0),
 * height included.  The rotation is (cos, sin) = (h . r, h x r) of the two unit vectors, never an angle: (x, z) -> (cos x - sin z,
 * sin x + cos z).  Root quaternions come back normalised with w >= 0; every other channel is copied.  transforms_dev: NULL, or
 * (n_motions, 5) for each motion's (cos, sin, dx, dy, dz), d the turned root position of frame frame_idx.  out_dev must not be
 * frames_dev.  MG_ERR_UNSUPPORTED unless n_dim = 3 + 4 J with 1 <= J <= 64, answered before anything else;
 * MG_ERR_INVALID_ARGUMENT for offsets that do not start at 0 or do not rise, a frame_idx outside any motion, a ref_orientation
 * of length 0, and -- found by check kernels, before the kernel proper is launched, so that nothing is written -- non-finite
 * frames, a zero root quaternion, and a frame frame_idx whose root turns z onto the y axis (no heading; the text names the first
 * such motion).  n_motions = 0 is MG_OK and does nothing.  PARITY UNPINNED for the heading and the angle between headings (the
 * reference's pose_orientation_quat and get_rotation_angle are anim_utils'). */
int mg_align_motions_spatially(mg_context *ctx, const double *frames_dev, const int64_t *offsets, int64_t n_motions, int32_t n_dim,
                               int64_t frame_idx, const double *ref_orientation, double *out_dev, double *transforms_dev);

/* out_dev (n_motions, n_frames, n_dim) = frames_dev with the root positions divided by scale_vec[3] (HOST, out) = the largest |x|,
 * |y|, |z| over all frames -- unless one of the three is 0: then nothing is scaled and scale_vec is ones
 * (normalize_root_translation) -- and every quaternion of the first n_joints joints whose dot product with the same joint's
 * quaternion in frame 0 of motion 0 (w, x, y, z added in that order) is < 0 negated (align_quaternion_frames).  Channels from
 * 3 + 4 n_joints on are copied.  Bit for bit the two reference functions wherever no dot product lies within rounding of 0.
 * out_dev must not be frames_dev.  MG_ERR_INVALID_ARGUMENT for 3 + 4 n_joints > n_dim, n_frames < 1 and non-finite frames
 * (check kernel; nothing is written); n_motions = 0 is MG_OK with scale_vec = ones. */
int mg_prepare_aligned_frames(mg_context *ctx, const double *frames_dev, int64_t n_motions, int32_t n_frames, int32_t n_dim,
                              int32_t n_joints, double *out_dev, double *scale_vec);

/* ---- segmentation: cutting clips out of captures at keyframe poses (reference construction/keyframe_detection.py:79-135 argmin,
 * argmin_multi, KeyframeDetector.find_instance / find_instances / calculate_distances; construction/segmentation.py:34-81
 * Segmentation.extract_single_segments / extract_segments), float64, synchronising, bit-reproducible.  Captures are ragged like the
 * motions above: capture n has F_n = offsets[n + 1] - offsets[n] >= 1 frames, offsets a HOST array of n_motions + 1 entries,
 * offsets[0] = 0, rising; there is no 1024-frame limit here.  n_motions = 0 is MG_OK and does nothing.  Non-finite inputs are
 * found by a check kernel and refused with MG_ERR_INVALID_ARGUMENT before the kernel proper is launched (the reference's
 * `v < min_v` silently skips a NaN: a documented difference). ---- */
/* dist_dev (n_keyframes, offsets[n_motions]), row-major: dist[k][f] = the cell of mg_dtw_distance_grids with A = frame f of
 * clouds_dev (offsets[n_motions], n_joints, 3) and B = keyframe k of keyframes_dev (n_keyframes, n_joints, 3): the keyframe is
 * fitted onto the frame (the reference calls distance_measure(frame, keyframe)).  Bit for bit what mg_dtw_distance_grids gives at
 * cell (f, 0) for (reference motion = the capture, one motion = the one-frame keyframe); each frame is read once for all
 * keyframes.  weights: HOST array (n_joints), NULL = ones.  MG_ERR_INVALID_ARGUMENT outside 1 <= n_joints <= 64 and
 * 1 <= n_keyframes <= 8, for a capture without frames and for weights that are negative, non-finite or all 0.  PARITY UNPINNED, as
 * for mg_dtw_distance_grids (formula and order of every sum: csrc/mg_dtw.hip). */
int mg_keyframe_distances(mg_context *ctx, const double *clouds_dev, const int64_t *offsets, int64_t n_motions, int32_t n_joints,
                          const double *keyframes_dev, int32_t n_keyframes, const double *weights, double *dist_dev);

enum mg_segment_mode {
    MG_SEGMENT_SINGLE = 0, /* extract_single_segments: one (argmin start distance, argmin end distance) pair per capture */
    MG_SEGMENT_MULTI = 1   /* extract_segments: every instance of the start keyframe opens a search window */
};

/* The search over given distances start_dist_dev, end_dist_dev (offsets[n_motions] each, capture n's at offsets[n]).  Every
 * arg-min is the FIRST index of the least value (argmin's strict `<`).
 * MG_SEGMENT_SINGLE: start = argmin of the start distances, end = argmin of the end distances; always one pair, which may have
 * end <= start (the reference's empty slice); threshold and min_segment_size are not used.
 * MG_SEGMENT_MULTI (segmentation.py:61-80): m = min of the start distances; the instances are the frames with v <= m + threshold
 * (that one addition, rounded as the host rounds it), in frame order; instance i's window ends at instance i + 1, the last one's
 * at F_n - 1; a window with end - start < min_segment_size is dropped; otherwise e = start + (first index of the minimum of the
 * end distances over [start, window end), 0 for a window without frames), and the segment is kept if e - start >
 * min_segment_size (>= 0).
 * Outputs, on the device: capture n's kept (start, end) int32 pairs, in order of start, at segments_dev + 2 * segment_offsets[n];
 * counts_dev[n] their number.  segment_offsets: HOST array of n_motions + 1 entries; capture n needs room for 1 pair
 * (MG_SEGMENT_SINGLE) or F_n / (min_segment_size + 1) + 1 pairs (the segments are disjoint and longer than min_segment_size),
 * MG_ERR_INVALID_ARGUMENT with less.  MG_ERR_UNSUPPORTED from F_n or n_motions of 2^31 on.  The results are the reference's for
 * the same distances, do not depend on the batch, and two calls give identical bytes. */
int mg_segment_search(mg_context *ctx, const double *start_dist_dev, const double *end_dist_dev, const int64_t *offsets,
                      int64_t n_motions, int32_t mode, double threshold, int32_t min_segment_size, const int64_t *segment_offsets,
                      int32_t *segments_dev, int32_t *counts_dev);

/* ---- a graph walk's motion -------------------------------------------------------------------------------
 * GraphWalk.convert_graph_walk_to_quaternion_frames for a population of walks (reference motion_generator/graph_walk.py:154-176: per
 * step back_project(parameters).get_motion_vector(), then MotionVector.append_frames, which aligns the step to the last frame so far
 * and appends it; smoothing is off during synthesis, :102): the frames of n_walks walks over the SAME node sequence, written once where
 * they end up, in two launches (csrc/mg_walk.hip).
 *   prims[n_steps]           one primitive per step, all of one context and one n_dim (a primitive may repeat)
 *   latents_dev              (n_walks, ld) float32 / float64; step i reads columns latent_offset[i] .. + its n_components
 *   times_dev, lengths       NULL, NULL: every step on its primitive's canonical grid linspace(0, F, F); or times_dev (n_walks, n_steps,
 *                            t_cap) float64 on the device with lengths (n_walks, n_steps): rows as mg_time_function_sample leaves them
 *   frame_offset             (n_walks, n_steps): the first output row of every step inside its walk (NULL with canonical grids: back to back)
 *   alignment                of the FIRST step: NULL (it stays as it is), a previous-frame record, or a start-pose record.  Every later
 *                            step is aligned to the ALIGNED last sample of the step before it (the last entry of its time row) through
 *                            the record's joint and ref_dir -- the root and (0, 0, 1) without a previous-frame record.  skeleton: needed
 *                            only when that joint is not the root
 *   frames_dev               (n_walks, walk_stride, n_dim) float64; rows no step owns are not written
 *   transforms_dev           NULL or (n_walks, n_steps, 4) float64 = (c, s, tx, tz) of every step; (1, 0, 0, 0) for an unaligned one
 * latent_offset, lengths and frame_offset are HOST tables: the call checks them before any launch (a length < 1 or > t_cap, steps that
 * overlap or pass walk_stride, primitives of two contexts or widths, a non-root aligning joint without a skeleton:
 * MG_ERR_INVALID_ARGUMENT) and carries them to the device itself.  One step without an alignment record aligns nothing: n_dim may then
 * be 3 .. 6, no aligning chain is formed and a skeleton passed along is not looked at.
 * Arithmetic: a step's unaligned frames are mg_back_project_frames_f64's (canonical grid) or mg_back_project_frames_at's (given times), bit
 * for bit; its transform is the one mg_align_frames applies -- h the heading it is aligned to, b its own in its first control point:
 * c = h.b, s = h x b, a position becomes (c x + s z + tx, y, -s x + c z + tz), the root quaternion is multiplied from the left by the
 * rotation about y, a start pose raises the heights of the first step by position[1].  A walk's frames do not depend on the batch.
 * At most MG_WALK_MAX_STEPS steps per call: a longer walk is assembled in pieces, the last frame of one piece giving the previous-frame
 * record of the next (graph_walk.py in the Python package does).  Profile slot 12 times mg_walk_frames_kernel. */
#define MG_WALK_MAX_STEPS 64
int mg_walk_frames(int32_t n_steps, mg_primitive *const *prims, const int64_t *latent_offset, const void *latents_dev, int latent_dtype,
                   int64_t n_walks, int64_t ld, const double *times_dev, const int32_t *lengths, int32_t t_cap, const int64_t *frame_offset,
                   const mg_alignment_desc *alignment, const mg_skeleton_desc *skeleton, double *frames_dev, int64_t walk_stride,
                   double *transforms_dev);

/* ---- a population of walks with their own node sequences (csrc/mg_walks_mixed.hip) ---------------------------------
 * What MotionStateGraph.generate_random_walk produces (reference motion_model/motion_state_graph.py:52-71, motion_state_group.py:
 * 107-129, 177-214): every walk has its own nodes, its own number of steps and its own frame count per step.  Shared tables:
 *   prims[n_nodes]           the primitives of the nodes that occur, all of one context and one n_dim
 *   node_of                  HOST int32 (n_walks, s_max): indices into prims; entries at or past n_steps[w] are not read
 *   n_steps                  HOST int32 (n_walks), 1 <= n_steps[w] <= s_max
 * Both calls check the tables before any launch (a node index outside [0, n_nodes), n_steps[w] outside [1, s_max], ld too small for a
 * node that occurs, primitives of two contexts or widths: MG_ERR_INVALID_ARGUMENT, nothing launched) and carry them to the device in
 * a cached table of their own (MG_TABLE_WALKS_SAMPLE, MG_TABLE_WALKS_MIXED), rewritten only when it differs from the last call's.
 * Caps, MG_ERR_UNSUPPORTED: n_walks * s_max of 2^31 on; for the frames, 2^31 tiles of 32 frames on and a node whose control points
 * do not fit LDS (mg_walk_frames' limit); for the sampler, a mixture of more than 299 dimensions.  s_max itself has no cap.
 *
 * mg_walks_sample_latents: ONE launch.  x_dev (n_walks, s_max, ld) of x_dtype; row (w, i), i < n_steps[w], is a draw from the mixture
 * of node node_of[w][i] over its n_gmm_dims columns; the columns behind them and the rows of steps at or past n_steps[w] are 0.
 * component_dev: NULL or int32 (n_walks, s_max), -1 for such steps.  With r = w * s_max + i the row's global index:
 *   component   one Philox4x32-10 word: key (seed & 0xffffffff, seed >> 32), counter (r & 0xffffffff, r >> 32, 0, 1), the first of
 *               the four outputs (the normals of row r use the counters (r & 0xffffffff, r >> 32, column group, 0)); u = (word +
 *               0.5) * 2^-32 in float64; the first c with u < cum[c], cum[c] = cum[c - 1] + weights[c] in float64 from cum[0] =
 *               weights[0] (the weights as given to mg_primitive_create, not normalised); the last component takes what is left;
 *   values      the normals and x = mu_c + z L_c^T are mg_gmm_sample's statement for global row r under `seed`: the bits of
 *               mg_gmm_sample_rows(prim, n_walks * s_max, counts = all rows in component c, seed, r, 1, ..).
 * A row's values depend on (seed, r, its node) only.  Like mg_gmm_sample the draw is validated distributionally against the
 * reference; it is deterministic on gfx950.
 *
 * mg_walks_frames: TWO launches, canonical grids (time-warped steps: mg_walks_time_functions, then mg_walks_frames_at, below).  latents_dev (n_walks, s_max,
 * ld): step (w, i) reads the first n_components columns of its own row, the layout the sampler leaves.  frame_offset: HOST int64
 * (n_walks, s_max), the first output row of every step inside its walk, or NULL: back to back.  alignment, skeleton, frames_dev,
 * walk_stride as in mg_walk_frames; the alignment is that of every walk's first step.  transforms_dev: NULL or (n_walks, s_max, 4);
 * the entries of steps at or past n_steps[w] are not written, nor are rows of frames_dev no step owns.  Further
 * MG_ERR_INVALID_ARGUMENT: steps that overlap or pass walk_stride, a non-root aligning joint without a skeleton.
 * Contract: walk w's frames and transforms are, bit for bit, those of mg_walk_frames called for that walk alone (n_walks = 1, its
 * node sequence, its latents packed into one row, the same alignment). */
int mg_walks_sample_latents(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, int64_t n_walks,
                            int32_t s_max, uint64_t seed, void *x_dev, int x_dtype, int64_t ld, int32_t *component_dev);
int mg_walks_frames(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents_dev,
                    int latent_dtype, int64_t n_walks, int32_t s_max, int64_t ld, const int64_t *frame_offset,
                    const mg_alignment_desc *alignment, const mg_skeleton_desc *skeleton, double *frames_dev, int64_t walk_stride,
                    double *transforms_dev);

/* The time-warped motion of such a population: what GraphWalk.convert_graph_walk_to_quaternion_frames(use_time_parameters=True) hands
 * back (reference motion_generator/graph_walk.py:154-176, back_project(s, True) per step).  The tables and their checks are those above;
 * each call has a cached table of its own (MG_TABLE_WALKS_TIME, MG_TABLE_WALKS_WARPED).
 *
 * mg_walks_time_functions: ONE launch, one wave per (walk, step).  times_dev (n_walks, s_max, t_cap) float64, lengths_dev int32
 * (n_walks, s_max).  Row (w, i) of a node WITH a time model: gamma = columns n_components .. n_components + n_time_components of the
 * step's own latent row (the layout the sampler leaves); the row and its length are, bit for bit, mg_time_function_sample_rows' for
 * that primitive, gamma, speed and t_cap.  Of a node WITHOUT one: numpy.linspace(0, F, int(F * (1 / speed))) -- q * (F / (count - 1)),
 * the last entry F itself, the single value 0 for a count of 1.  Lengths as in mg_time_function_sample: T where T <= t_cap; -T, the row
 * not written, where it does not fit; 0 for a time function that is not finite; 0, the row not written, for steps at or past
 * n_steps[w].  Before any launch, MG_ERR_INVALID_ARGUMENT: speed <= 0 or not finite, a node without a time model whose count is below 1,
 * ld below a node's n_components + n_time_components; MG_ERR_UNSUPPORTED: a node with a time model and more than 2048 canonical frames
 * (or fewer than 4), a count above 2^24, n_walks * s_max of 2^31 on.  Does not synchronise.
 *
 * mg_walks_frames_at: TWO launches, mg_walks_frames with every step at its own time row.  times_dev (n_walks, s_max, t_cap); lengths and
 * frame_offset: HOST tables (n_walks, s_max) as in mg_walk_frames, both required.  A step's exit pose -- what the next step is aligned
 * to -- is taken at the LAST entry of its row; each frame's basis row comes from the FITPACK recurrence at its own time.  Further
 * MG_ERR_INVALID_ARGUMENT: a length below 1 or above t_cap on a step the walk has; NULL times_dev, lengths or frame_offset; what
 * mg_walks_frames refuses.  MG_ERR_UNSUPPORTED: the caps of mg_walks_frames.
 * Contract: walk w's frames and transforms are, bit for bit, those of mg_walk_frames called for that walk alone (n_walks = 1, its node
 * sequence, its latents packed into one row, its time rows as times_dev (1, n_steps, t_cap), the same lengths, offsets and alignment).
 * Rows no step owns and transforms of steps the walk does not have are not written.
 * mg_walks_time_functions_smoothed: mg_walks_time_functions with smooth_of_node, one byte per node (HOST): the rows of a node with a time
 * model and a byte other than 0 are mg_time_function_sample_smoothed_rows' for that primitive, bit for bit (a row of 0 < T < 15 samples
 * reports T and is not written); every other row has the bits of mg_walks_time_functions.  A cached table of its own
 * (MG_TABLE_WALKS_TIME_SMOOTHED).
 * Out of scope: parameters predicted by transition models. */
int mg_walks_time_functions(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps,
                            const void *latents_dev, int latent_dtype, int64_t n_walks, int32_t s_max, int64_t ld, double speed,
                            double *times_dev, int32_t *lengths_dev, int32_t t_cap);
int mg_walks_time_functions_smoothed(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps,
                                     const uint8_t *smooth_of_node, const void *latents_dev, int latent_dtype, int64_t n_walks, int32_t s_max,
                                     int64_t ld, double speed, double *times_dev, int32_t *lengths_dev, int32_t t_cap);
int mg_walks_frames_at(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps,
                       const void *latents_dev, int latent_dtype, int64_t n_walks, int32_t s_max, int64_t ld,
                       const double *times_dev, const int32_t *lengths, int32_t t_cap, const int64_t *frame_offset,
                       const mg_alignment_desc *alignment, const mg_skeleton_desc *skeleton, double *frames_dev,
                       int64_t walk_stride, double *transforms_dev);

/* The objective of a whole graph walk in ONE launch (csrc/mg_walk_score.hip): what n_steps calls of mg_score_constraint_residuals
 * [_chained] give when each step's four exit values (MG_CONSTRAINT_VALUE_HEADING x, z; MG_CONSTRAINT_VALUE_POSITION x, z at the step's
 * exit time) are the next step's per-candidate alignment (obj_global_error_sum and its residual-vector forms, reference
 * optimization/objective_functions.py:290-380), bit for bit: the same residual statements on the same k-ordered chains, the state
 * handed on as unrounded float64 -- in the wave's LDS instead of through the host.
 *   steps[n_steps]           HOST table, one record per step (a primitive may repeat, with the same or other sets)
 *   latents_dev              (n_samples, ld) float32 / float64; step i reads columns latent_offset .. + its primitive's n_components
 *   residuals_dev            NULL or (n_samples, ld_res) float64; step i's own residuals go to columns column_offset .. + n_own, columns
 *                            no step owns are not written
 *   errors_dev               NULL or (n_samples): per step, in step order, the step's own residuals added in constraint order; the
 *                            step sums added in step order
 *   exit_state_dev           NULL or (n_samples, 4): the LAST step's exit values
 * Step 0 uses the alignment its sets were created with (a previous-frame record, a start-pose record, none).  In every later step a
 * set with an alignment must carry a previous-frame record: it supplies the node, the chain and ref_dir, its values are replaced per
 * candidate by the exit values of that candidate's previous step; a set without one is scored unaligned (a local step).
 * Checked before any launch, MG_ERR_INVALID_ARGUMENT: n_steps outside 1 .. MG_WALK_MAX_STEPS, primitives of two contexts, a set of
 * another primitive, a later step whose exit-carrying set has no previous-frame alignment, n_own inconsistent with the sets, own
 * column ranges that overlap or pass ld_res, latent_offset + n_components > ld.  MG_ERR_UNSUPPORTED where a step's tables do not fit
 * LDS (the per-step calls remain).  Apart from the step table (kept on the device, rewritten only when it differs from the last
 * call's) the call allocates nothing and does not synchronise.  A candidate's values do not depend on the batch. */
typedef struct {
    mg_primitive *prim;
    const mg_constraint_set *scored; /* constraints whose residuals are the step's own columns; NULL = none.  May END with the four
                                        exit values */
    const mg_constraint_set *exit;   /* NULL when `scored` ends with the four exit values, else a set of exactly those four (a local
                                        step: scored unaligned, exits aligned) */
    int64_t latent_offset;           /* first column of the step's latents in a row */
    int32_t n_own;                   /* columns of `scored` that are the step's own (its n, minus 4 if it carries the exits) */
    int64_t column_offset;           /* where they go in a residual row */
} mg_walk_score_step;
int mg_score_walk_residuals(int32_t n_steps, const mg_walk_score_step *steps, const void *latents_dev, int latent_dtype, int64_t n_samples,
                            int64_t ld, double *residuals_dev, int64_t ld_res, double *errors_dev, double *exit_state_dev);
/* The same launch, which also writes the exit values EVERY step hands on: step_exits_dev NULL (mg_score_walk_residuals, the same
 * bits) or (n_samples, n_steps, 4) float64 -- row [i] is the state step i + 1 is aligned to, row [n_steps - 1] is exit_state_dev's.
 * What a step's trajectory constraints are aligned to per candidate (mg_score_trajectory_chained on the same stream, behind this
 * launch; a column block of it is gathered with mg_memcpy_d2d_rows). */
int mg_score_walk_residuals_steps(int32_t n_steps, const mg_walk_score_step *steps, const void *latents_dev, int latent_dtype, int64_t n_samples,
                                  int64_t ld, double *residuals_dev, int64_t ld_res, double *errors_dev, double *exit_state_dev,
                                  double *step_exits_dev);

/* The TIME objective of a graph walk in ONE launch (csrc/mg_walk_time.hip): obj_time_error_sum over TimeConstraints (reference
 * optimization/objective_functions.py:270-287, constraints/time_constraints.py:40-102) for n_samples rows of concatenated time latents,
 * bit for bit what mg_time_function_canonical and mg_gmm_log_prob (float64) per step and the reference's host arithmetic give:
 *   error      per constraint (step_index, keyframe_index, desired_time) in list order, starting from 0: n_frames = start_keyframe, then
 *              += t_k(F_k - 1) for the steps k < step_index in step order, then += (double)(int64)t_k(keyframe_index) + 1 at k == step_index
 *              (truncation towards zero), the constraint adds (desired_time - n_frames * frame_time)^2; 0 where keyframe_index >= F_k;
 *              10000 where step_index >= n_steps; -F_k <= keyframe_index < 0 counts from the end; a negative step_index reads step 0;
 *   loglik     log p of step k's mixture on [spatial latents of the step | the row's time latents of the step], added in step order
 *              from 0, divided by n_steps;
 *   objective  error_scale * error + (-loglik) * quality_scale; every product and sum above rounded on its own.
 * t_k is the canonical time function of step k (t(i) = i for a primitive without time model).  Where a kept value of it -- t_k(F_k - 1) of
 * any step, t_k at a constrained keyframe -- is not finite, the row's error and objective are NaN (its loglik is not affected).
 * steps[k].latent_offset: first column of the step's n_time_components time latents in a row; steps[k].spatial_dev: n_components float64
 * on the device.  error_dev, loglik_dev: (n_samples) float64 or NULL.  Profile slot 13.
 * MG_ERR_INVALID_ARGUMENT: NULL pointers, latent_offset + n_time_components > ld, keyframe_index < -F_k.  MG_ERR_UNSUPPORTED, never an
 * approximate answer: MG_F32 latents, more than MG_WALK_MAX_STEPS steps, primitives of two contexts, a mixture that mg_gmm_log_prob does
 * not score on the matrix pipe at this batch (no packed matrix: more than 64 dimensions, or more than 240 components) or that does not
 * span exactly n_components + n_time_components columns, a window whose tables do not fit LDS.  n_samples == 0: MG_OK, no launch.
 * Apart from the table of steps and constraints (kept on the device, rewritten only when it differs from the last call's:
 * mg_walk_time_table_uploads counts the uploads of a context) the call allocates nothing and does not synchronise. */
typedef struct {
    mg_primitive *prim;
    int64_t latent_offset;
    const double *spatial_dev;
} mg_walk_time_step;
typedef struct {
    int32_t step_index;              /* counted from the window's first step */
    int32_t keyframe_index;          /* canonical frame of that step */
    double desired_time;             /* seconds */
} mg_walk_time_constraint;
int mg_score_walk_time(int32_t n_steps, const mg_walk_time_step *steps, const void *latents_dev, int latent_dtype, int64_t n_samples, int64_t ld,
                       int32_t n_constraints, const mg_walk_time_constraint *constraints, double start_keyframe, double frame_time,
                       double error_scale, double quality_scale, double *objective_dev, double *error_dev, double *loglik_dev);
int mg_walk_time_table_uploads(mg_context *ctx, int64_t *uploads);   /* mg_context_table_uploads(ctx, MG_TABLE_WALK_TIME, uploads) */

/* The per-call descriptor tables a context keeps on the device, each rewritten only when a call's table differs from the last call's:
 * of mg_options_step's one-launch path, mg_cluster_tree_search, mg_walk_frames, mg_score_walk_residuals, mg_score_walk_time and
 * mg_step_lengths, of mg_feature_points, of mg_feature_points_warped, of mg_mixture_scores, of mg_point_cloud_features, of mg_walks_frames,
 * of mg_walks_sample_latents, of mg_walks_frames_at and of mg_walks_time_functions.  mg_context_table_uploads: how often table `which` of the context went to the device so far. */
enum { MG_TABLE_FUSED = 0, MG_TABLE_TREE = 1, MG_TABLE_WALK = 2, MG_TABLE_WALK_SCORE = 3, MG_TABLE_WALK_TIME = 4, MG_TABLE_STEP_LENGTH = 5,
       MG_TABLE_FEATURE_POINTS = 6, MG_TABLE_FEATURE_POINTS_WARPED = 7, MG_TABLE_MIXTURE_SCORES = 8, MG_TABLE_POINT_CLOUDS = 9,
       MG_TABLE_WALKS_MIXED = 10, MG_TABLE_WALKS_SAMPLE = 11, MG_TABLE_WALKS_WARPED = 12, MG_TABLE_WALKS_TIME = 13, MG_TABLE_SAVGOL = 14,
       MG_TABLE_WALKS_TIME_SMOOTHED = 15, MG_TABLE_FEATURE_POINTS_SMOOTHED = 16, MG_TABLE_COUNT = 17 };
int mg_context_table_uploads(mg_context *ctx, int which, int64_t *uploads);

/* Step lengths without frames in memory, ONE launch for every candidate of every item (csrc/mg_step_length.hip): what
 * MotionStateGraphNode.get_step_length_for_sample (reference motion_state_graph_node.py:208-230) takes from a back-projected motion,
 * and what MotionStateGroup._update_motion_state_stats (motion_state_group.py:74-105) asks of every node of a graph.  Items may use
 * different primitives, a primitive may repeat; all primitives belong to one context.  Per candidate, float64 throughout, every
 * operation rounded on its own (float32 latents are converted first):
 *   control points  of channels 0, 1, 2: mean' then fma(E'[k], s[k], .) for k ascending, translation_maxima included: the statement
 *                   and the bits of mg_back_project_coeffs(MG_F64);
 *   positions       p_f, f = 0 .. F - 1, on the primitive's canonical grid linspace(0, F, F) with the primitive's own tap rows (the
 *                   FITPACK ext=0 row of the last sample included), four taps w0 c0, fma(w1, c1, .), ..: the bits of
 *                   mg_back_project_frames_f64;
 *   arc_length      d_1 + d_2 + .. + d_{F-1} added in frame order from d_1, d_f = sqrt((x_f - x_{f-1})^2 + (z_f - z_{f-1})^2); 0 for F = 1;
 *   distance        sqrt((dx^2 + dy^2) + dz^2), d = p_{F-1} - p_0.
 * A candidate with a latent that is not finite gets NaN for both, and nothing else does; a candidate's values depend on neither the
 * batch nor the other items nor its position in either.  Nothing per candidate goes to device memory but the two results.
 * latent_offset: first column of the item's n_components latents in a row of ld elements, so the steps of a walk can be items over one
 * shared matrix.  arc_length_dev / distance_dev: (n_samples) float64, one of them may be NULL.
 * Everything is checked before any launch.  MG_ERR_INVALID_ARGUMENT: NULL item table with n_items > 0, a NULL primitive, NULL latents
 * with n_samples > 0, latent_offset < 0 or latent_offset + n_components > ld, negative counts, both outputs NULL, primitives of two
 * contexts.  MG_ERR_UNSUPPORTED, never an approximate answer: a primitive with fewer than 3 channels, or whose root tables do not fit
 * LDS.  n_items == 0 or all items empty: MG_OK, no launch; empty items among others are skipped.  A launch takes
 * MG_STEP_LENGTH_MAX_ITEMS non-empty items; a call with more goes through them in slices itself, whatever their number.  Apart from
 * the item table (kept on the device, rewritten only when it differs from the last call's) the call allocates nothing and does not
 * synchronise.  Profile slot 14. */
#define MG_STEP_LENGTH_MAX_ITEMS 256
typedef struct {
    mg_primitive *prim;
    const void *latents_dev;    /* (n_samples, ld) float32 / float64 */
    int64_t latent_offset;      /* first column of this item's n_components latents in a row */
    int64_t n_samples, ld;
    double *arc_length_dev;     /* (n_samples) or NULL */
    double *distance_dev;       /* (n_samples) or NULL */
} mg_step_length_item;
int mg_step_lengths(int32_t n_items, const mg_step_length_item *items, int latent_dtype);

/* Feature points without frames in memory, ONE launch for every candidate of every item (csrc/mg_feature_points.hip): what the
 * reference's FeaturePointModel (construction/feature_point_model.py: create_feature_points :58-84, create_root_pos_ori :86-95)
 * takes from a whole back-projected motion, and what FeaturePointModelBuilder.build asks of every primitive of a model directory.
 * Items may use different primitives, skeletons, joint lists and frames; a primitive may repeat; all primitives belong to one
 * context.  Per candidate, float64 throughout, every operation rounded on its own (float32 latents are converted first):
 *   control points  only the channels and basis rows the frames 0, frame_idx and F - 1 touch: mean' then fma(E'[k], s[k], .) for k
 *                   ascending, translation_maxima included: the statement and the bits of mg_back_project_coeffs(MG_F64);
 *   frames          0, frame_idx and F - 1 on the primitive's canonical grid linspace(0, F, F) with the primitive's own tap rows (the
 *                   FITPACK ext=0 row of the last sample included), four taps w0 c0, fma(w1, c1, .), ..: the bits of
 *                   mg_back_project_frames_f64;
 *   start_root      (n, 3): the root position of frame 0;
 *   points          (n, 3 n_joints): the global position of every listed joint at frame_idx by forward kinematics along its chain --
 *                   the statement and the bits of mg_joint_positions on that frame -- minus start_root;
 *   root_end        (n, 2): x and z of the root at frame F - 1;
 *   heading_end     (n, 2): the root quaternion of frame F - 1, made unit as every chain quaternion is, applied to (0, 0, 1); its x and z
 *                   divided by their length (the accumulated orientation is not normalised again);
 *   heading_len     (n): that length before the division, so that a caller sees a degenerate heading.
 * No transcendental function runs on the device; the reference's angle (convert_ori_to_angle_deg) is formed on the host from heading_end.
 * A candidate with a latent that is not finite gets NaN in all its outputs, and nothing else does; a candidate's values depend on
 * neither the batch nor the other items nor its position in either.  Nothing per candidate goes to device memory but the outputs.
 * skeleton / joints: HOST pointers, read during the call; skeleton may be NULL with n_joints = 0.  n_joints <=
 * MG_FEATURE_POINTS_MAX_JOINTS = 32: with chains of MG_MAX_CHAIN links the joints' records are 34 KB of a workgroup's LDS, which leaves
 * 116 KB of the 150 KB a workgroup may take for the listed rows of E' and the tile's control points.
 * Everything is checked before any launch or copy.  MG_ERR_INVALID_ARGUMENT: NULL item table with n_items > 0, a NULL primitive, NULL
 * latents with n_samples > 0, latent_offset < 0 or latent_offset + n_components > ld, negative counts, frame_idx outside 0 .. F - 1,
 * a joint outside the skeleton (or n_joints outside 0 .. the cap, joints without a skeleton), n_joints > 0 without points_dev or
 * points_dev with n_joints = 0, all outputs NULL, primitives of two contexts.  MG_ERR_UNSUPPORTED, never an approximate answer: a
 * primitive with fewer than 7 channels, a skeleton with a quaternion channel beyond the primitive's channels, a chain of more than
 * MG_MAX_CHAIN links, tables that do not fit LDS even with the large-LDS opt-in.  n_items == 0 or all items empty: MG_OK, no launch;
 * empty items among others are skipped.  A launch takes MG_FEATURE_POINTS_MAX_ITEMS non-empty items; a call with more goes through them
 * in slices itself.  Apart from the item table (kept on the device, rewritten only when it differs from the last call's) the call
 * allocates nothing and does not synchronise.  Profile slot 15. */
#define MG_FEATURE_POINTS_MAX_ITEMS 256
#define MG_FEATURE_POINTS_MAX_JOINTS 32
typedef struct {
    mg_primitive *prim;
    const void *latents_dev;            /* (n_samples, ld) float32 / float64 */
    int64_t latent_offset;              /* first column of this item's n_components latents in a row */
    int64_t n_samples, ld;
    const mg_skeleton_desc *skeleton;   /* HOST; NULL allowed with n_joints = 0 */
    const int32_t *joints;              /* HOST (n_joints) indices into the skeleton */
    int32_t n_joints;
    int32_t frame_idx;                  /* canonical frame of `points` */
    double *start_root_dev;             /* (n_samples, 3) or NULL */
    double *points_dev;                 /* (n_samples, 3 n_joints); NULL exactly when n_joints = 0 */
    double *root_end_dev;               /* (n_samples, 2) or NULL */
    double *heading_end_dev;            /* (n_samples, 2) or NULL */
    double *heading_len_dev;            /* (n_samples) or NULL */
} mg_feature_point_item;
int mg_feature_points(int32_t n_items, const mg_feature_point_item *items, int latent_dtype);

/* The point clouds a feature cluster tree's "euclidean_pca" features are made of (reference space_partitioning/features.py:133-153,
 * map_motions_to_euclidean_space), WITHOUT frames in memory and in one launch: out_dev (n, F, n_joints, 3) float64, entry [i, f, j, :] the
 * global position of joints[j] in frame step * (f / step) of latent row i -- a frame whose index is not a multiple of step
 * repeats the cloud of the last one that is; each kept frame is evaluated once.  grid: the F frames' times (the cluster-tree builder
 * evaluates the integer canonical frames 0 .. F - 1, `spline.evaluate(frame_idx)`); NULL: the primitive's canonical grid.  latents_dev: n rows of ld elements (float32 or
 * float64), the primitive's n_components first.  Bit for bit what mg_back_project_frames_f64 on the same grid followed by
 * mg_joint_positions gives.  Does not synchronise; allocates nothing but the context's cached table (MG_TABLE_POINT_CLOUDS).
 * MG_ERR_INVALID_ARGUMENT: NULL pointers, n < 0, ld below n_components, step < 1, n_joints outside 1 .. MG_FEATURE_POINTS_MAX_JOINTS, an
 * incomplete skeleton, a joint out of range.  MG_ERR_UNSUPPORTED, never an approximate answer: fewer than 7 channels, chains of more
 * than MG_MAX_CHAIN links, a skeleton channel beyond the primitive's, control points that do not fit LDS even with the large-LDS
 * opt-in (4 candidates x n_basis x the channels the chains read).  n == 0: MG_OK, no launch. */
int mg_point_cloud_features(mg_primitive *prim, const mg_time_grid *grid, const mg_skeleton_desc *skeleton, const int32_t *joints, int32_t n_joints, int32_t step,
                            const void *latents_dev, int latent_dtype, int64_t n, int64_t ld, double *out_dev);

/* Feature points of the TIME-WARPED motion, no time function and no frame in memory, ONE launch for every candidate of every item
 * (csrc/mg_feature_points.hip): what the reference's FeaturePointModel takes from back_project(s, use_time_parameters=True) -- its
 * default -- on a primitive with a time model.  A latent row holds the item's n_components spatial latents from latent_offset on and
 * its n_time_components time latents gamma from time_offset on (the reference's layout: time_offset = latent_offset + n_components).
 * Per candidate, float64 throughout, every operation rounded on its own (float32 latents are converted first):
 *   time function   x(i) = t(i), i = 0 .. F - 1: the running sum of exp(mean_t(i) + phi(i) . gamma) minus 1: the statement and the
 *                   bits of mg_time_function_canonical;
 *   n_frames        num + 2, num = int(round(x(F - 2))): the length of the warped motion (speed 1); 0 for a time function that is not
 *                   finite or asks for more than 2^24 samples (mg_time_function_sample's test);
 *   time_mid        the canonical time of frame frame_idx of the warped motion: 0 for frame_idx = 0, F - 1 for frame_idx =
 *                   n_frames - 1, else the not-a-knot cubic through (x(i), i) at numpy.linspace(1, x(F - 2), num)[frame_idx - 1]: the
 *                   statements and the bits of mg_time_function_sample's times[frame_idx] (csrc/mg_timewarp_device.h states both);
 *                   NaN for frame_idx >= n_frames (the reference's indexing raises IndexError there);
 *   frames          at the times 0, time_mid and F - 1 (NOT F, the canonical grid's last sample): control points mean' then
 *                   fma(E'[k], s[k], .) for k ascending, the basis row by the FITPACK recurrence, four taps: the statements and the
 *                   bits of mg_back_project_frames_at at those times;
 *   start_root, points, root_end, heading_end, heading_len   as in mg_feature_points, on those three frames.
 * n_frames = 0: NaN in every output of the candidate.  A spatial latent that is not finite: NaN in start_root, points, root_end,
 * heading_end and heading_len; n_frames and time_mid are stated.  frame_idx >= n_frames: NaN in points and time_mid only.  Nothing
 * else is NaN for such a row, and a candidate's values depend on neither the batch nor the other items nor its position in either.
 * Nothing per candidate goes to device memory but the outputs: no time function, no frame.
 * Everything is checked before any launch or copy.  MG_ERR_INVALID_ARGUMENT: what mg_feature_points refuses so (but frame_idx has no
 * upper bound here: the warped length is the candidate's), frame_idx < 0, time_offset < 0 or time_offset + n_time_components > ld,
 * spatial and time columns that overlap, a primitive without a time model, all outputs NULL.  MG_ERR_UNSUPPORTED, never an
 * approximate answer: what mg_feature_points refuses so, fewer than 4 or more than MG_FEATURE_POINTS_WARPED_MAX_F canonical frames (a
 * workgroup keeps 3 F doubles of each of its 16 candidates in LDS for the inversion), tables that do not fit LDS.  Empty items,
 * slices of MG_FEATURE_POINTS_MAX_ITEMS items and the device table (MG_TABLE_FEATURE_POINTS_WARPED) as in mg_feature_points; the
 * call allocates nothing else and does not synchronise.  Profile slot 16. */
#define MG_FEATURE_POINTS_WARPED_MAX_F 256
typedef struct {
    mg_primitive *prim;
    const void *latents_dev;            /* (n_samples, ld) float32 / float64 */
    int64_t latent_offset;              /* first column of this item's n_components spatial latents in a row */
    int64_t n_samples, ld;
    const mg_skeleton_desc *skeleton;   /* HOST; NULL allowed with n_joints = 0 */
    const int32_t *joints;              /* HOST (n_joints) indices into the skeleton */
    int32_t n_joints;
    int32_t frame_idx;                  /* frame of `points` in the WARPED motion, >= 0 */
    double *start_root_dev;             /* (n_samples, 3) or NULL */
    double *points_dev;                 /* (n_samples, 3 n_joints); NULL exactly when n_joints = 0 */
    double *root_end_dev;               /* (n_samples, 2) or NULL */
    double *heading_end_dev;            /* (n_samples, 2) or NULL */
    double *heading_len_dev;            /* (n_samples) or NULL */
    int64_t time_offset;                /* first column of this item's n_time_components time latents in a row */
    double *time_mid_dev;               /* (n_samples) or NULL */
    int32_t *n_frames_dev;              /* (n_samples) or NULL */
} mg_warped_feature_point_item;
int mg_feature_points_warped(int32_t n_items, const mg_warped_feature_point_item *items, int latent_dtype);
/* The same over a SMOOTHED time function (smooth_time_parameters; the statement: mg_time_function_sample_smoothed above).  smooth: one
 * byte per item (HOST).  An item whose byte is 0 has the bits of mg_feature_points_warped.  For the others smoothing moves all three
 * times of a candidate: the first becomes row 0 of the hat matrix on the first 15 samples of its time function (it can be negative), the
 * last one row 14 on the last 15 (no longer F - 1), time_mid is smoothed sample frame_idx; the frames are the spline at those times, by
 * the statements of the mid frame above (the bits of mg_back_project_frames_at at them; outside [0, F - 1] the end piece's polynomial).
 * The lane evaluates the <= 45 unsmoothed samples itself; nothing new goes to device memory.  A candidate of fewer than 15 frames is NaN
 * in every output but n_frames; frame_idx >= n_frames: NaN in points and time_mid only.  A device table (MG_TABLE_FEATURE_POINTS_SMOOTHED)
 * and a profile slot (19) of its own. */
int mg_feature_points_warped_smoothed(int32_t n_items, const mg_warped_feature_point_item *items, const uint8_t *smooth, int latent_dtype);

/* Targets scored against the reachability mixtures of many nodes, ONE launch for every target of every item
 * (csrc/mg_mixture_scores.hip): what the reference's FeaturePointModel asks of its stored mixture in check_reachability,
 * evaluate_target_point and score_trajectory_target (construction/feature_point_model.py) -- sklearn's score_samples of a
 * full-covariance mixture over 3, 4 or 3 J features -- and what a planner asks of every node of a graph.
 *
 * A feature mixture is formed once, on the host, in float64 (csrc/mg_mixture_image.h, plain host code).  Per component k:
 *   P   the upper-triangular precision Cholesky factor inv(chol_lower(C))^T (sklearn's _compute_precision_cholesky): the Cholesky
 *       factor row by row and its inverse by forward substitution, every product and difference rounded on its own (no fma), the sums
 *       in ascending index order; only the triangle is kept;
 *   m   m_j = mu_0 P[0][j], then fma(mu_i, P[i][j], .) for i = 1 .. j;
 *   c   (-0.5 dim log(2 pi) + (log P[0][0] + log P[1][1] + ..)) + log w.
 * weights, means (n_components, dim), covars (n_components, dim, dim): HOST arrays; of a covariance the lower triangle is read.
 * MG_ERR_INVALID_ARGUMENT: NULL pointers, a weight that is negative or not finite, a mean or a threshold that is NaN, a covariance that
 * is not positive definite (with sklearn's text for it).  A component of weight 0 is legal: its c is -inf.  MG_ERR_UNSUPPORTED, never an
 * approximate answer: dim outside 1 .. MG_FEATURE_MIXTURE_MAX_DIM (3 x MG_FEATURE_POINTS_MAX_JOINTS), n_components outside 1 ..
 * MG_FEATURE_MIXTURE_MAX_COMPONENTS.  ctx NULL makes a mixture without a device copy: mg_mixture_scores_host and the two getters take
 * it, mg_mixture_scores refuses it.  Otherwise the image goes to the device once (one allocation, freed by _destroy). */
#define MG_FEATURE_MIXTURE_MAX_DIM 96
#define MG_FEATURE_MIXTURE_MAX_COMPONENTS 64
typedef struct mg_feature_mixture mg_feature_mixture;
int mg_feature_mixture_create(mg_context *ctx, int32_t n_components, int32_t dim, const double *weights, const double *means,
                              const double *covars, double threshold, mg_feature_mixture **out);
void mg_feature_mixture_destroy(mg_feature_mixture *m);
int mg_feature_mixture_info(const mg_feature_mixture *m, int32_t *n_components, int32_t *dim, double *threshold);
/* The image as formed: prec_chol (n_components, dim, dim) with zeros below the diagonal, m (n_components, dim), c (n_components);
 * HOST arrays, each may be NULL. */
int mg_feature_mixture_get_image(const mg_feature_mixture *m, double *prec_chol, double *mean_prec, double *log_const);

/* The scores.  Per target x (the mixture's dim columns of a row from target_offset on) and component k, float64, every operation
 * rounded on its own:
 *   y_j   = (x_0 P[0][j], then fma(x_i, P[i][j], .) for i = 1 .. j) - m_j
 *   q     = y_0 y_0, then fma(y_j, y_j, .) for j = 1 .. dim - 1
 *   wlp_k = fma(-0.5, q, c_k)                                    (sklearn's _estimate_weighted_log_prob)
 *   logp  = max + log(exp(wlp_0 - max) + exp(wlp_1 - max) + ..), max the largest wlp_k, the sum in component order; -inf where
 *           every wlp_k is -inf                                  (score_samples)
 *   reachable = !(logp < threshold): the reference's `if score < threshold: False else: True`, so a NaN score reads as reachable.
 * wlp carries no transcendental function of the target: the device's and the host twin's are the same bits; logp differs by the
 * exp and log of the two maths libraries.  A target with a coordinate that is not finite gets NaN in logp and in its wlp row, and
 * nothing else does; a target's values depend on neither the batch nor the other items nor its position in either.  Items may share a
 * target matrix (N nodes against one set of targets), a mixture may repeat.
 * Everything is checked before any launch or copy.  MG_ERR_INVALID_ARGUMENT: a NULL context, a NULL item table with n_items > 0, a
 * NULL mixture, a mixture of another context (or without a device copy), negative counts, target_offset < 0 or target_offset + dim >
 * ld, all outputs NULL, NULL targets with n_targets > 0.  n_items == 0 or all items empty: MG_OK, no launch; empty items among others
 * are skipped.  A launch takes MG_MIXTURE_SCORES_MAX_ITEMS non-empty items; a call with more goes through them in slices itself.  Apart
 * from the item table (MG_TABLE_MIXTURE_SCORES: kept on the device, rewritten only when it differs from the last call's) the call
 * allocates nothing and does not synchronise.  Profile slot 17.
 * mg_mixture_scores_host: the same checks and the same statements (csrc/mg_mixture_image.h) on the HOST, every pointer of an item a host
 * pointer; no device is touched, ctx may be NULL and so may the mixtures' contexts. */
#define MG_MIXTURE_SCORES_MAX_ITEMS 256
typedef struct {
    const mg_feature_mixture *mixture;
    const double *targets_dev;     /* (n_targets, ld) float64 */
    int64_t target_offset;         /* first of the mixture's `dim` columns in a row */
    int64_t n_targets, ld;
    double *logp_dev;              /* (n_targets) or NULL */
    double *wlp_dev;               /* (n_targets, n_components) weighted log-probabilities, or NULL */
    int32_t *reachable_dev;        /* (n_targets): !(logp < threshold), or NULL */
} mg_mixture_score_item;
int mg_mixture_scores(mg_context *ctx, int32_t n_items, const mg_mixture_score_item *items);
int mg_mixture_scores_host(mg_context *ctx, int32_t n_items, const mg_mixture_score_item *items);

/* ---- host-pointer convenience variants (H2D, launch, D2H, synchronise) ---------------- */
/* mg_step_lengths with every item's latents and outputs in host memory (the `_dev` members are host pointers here); items that name
 * the same latent matrix (pointer, n_samples and ld) share one copy of it on the device */
int mg_step_lengths_host(int32_t n_items, const mg_step_length_item *items, int latent_dtype);
/* mg_feature_points with every item's latents and outputs in host memory (the `_dev` members are host pointers here); items that
 * name the same latent matrix (pointer, n_samples and ld) share one copy of it on the device */
int mg_feature_points_host(int32_t n_items, const mg_feature_point_item *items, int latent_dtype);
/* mg_feature_points_warped in the same way */
int mg_feature_points_warped_host(int32_t n_items, const mg_warped_feature_point_item *items, int latent_dtype);
int mg_feature_points_warped_smoothed_host(int32_t n_items, const mg_warped_feature_point_item *items, const uint8_t *smooth, int latent_dtype);
/* mg_score_walk_time with host arrays: latents, outputs and every step's spatial latents (`spatial_dev` is a host pointer here) */
int mg_score_walk_time_host(int32_t n_steps, const mg_walk_time_step *steps, const void *latents, int latent_dtype, int64_t n_samples, int64_t ld,
                            int32_t n_constraints, const mg_walk_time_constraint *constraints, double start_keyframe, double frame_time,
                            double error_scale, double quality_scale, double *objective, double *error, double *loglik);
/* mg_score_walk_residuals with host arrays; `residuals` is read first, so columns no step owns keep their values */
int mg_score_walk_residuals_host(int32_t n_steps, const mg_walk_score_step *steps, const void *latents, int latent_dtype, int64_t n_samples,
                                 int64_t ld, double *residuals, int64_t ld_res, double *errors, double *exit_state);
/* mg_score_walk_residuals_steps with host arrays; step_exits NULL or (n_samples, n_steps, 4) */
int mg_score_walk_residuals_steps_host(int32_t n_steps, const mg_walk_score_step *steps, const void *latents, int latent_dtype, int64_t n_samples,
                                       int64_t ld, double *residuals, int64_t ld_res, double *errors, double *exit_state, double *step_exits);
/* mg_walk_frames with latents, times, frames and transforms in host memory; `frames` is read first, so rows no step owns keep their values */
int mg_walk_frames_host(int32_t n_steps, mg_primitive *const *prims, const int64_t *latent_offset, const void *latents, int latent_dtype,
                        int64_t n_walks, int64_t ld, const double *times, const int32_t *lengths, int32_t t_cap, const int64_t *frame_offset,
                        const mg_alignment_desc *alignment, const mg_skeleton_desc *skeleton, double *frames, int64_t walk_stride,
                        double *transforms);
/* mg_walks_sample_latents with x and component in host memory: the device's draw copied back, as mg_gmm_sample_host is mg_gmm_sample's
 * (the same bits as the device-pointer form) */
int mg_walks_sample_latents_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, int64_t n_walks,
                                 int32_t s_max, uint64_t seed, void *x, int x_dtype, int64_t ld, int32_t *component);
/* mg_walks_frames with latents, frames and transforms in host memory; `frames` and `transforms` are read first, so what no step owns
 * keeps its values */
int mg_walks_frames_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents,
                         int latent_dtype, int64_t n_walks, int32_t s_max, int64_t ld, const int64_t *frame_offset,
                         const mg_alignment_desc *alignment, const mg_skeleton_desc *skeleton, double *frames, int64_t walk_stride,
                         double *transforms);
/* mg_walks_time_functions with latents, times and lengths in host memory; `times` is read first, so rows that are not written keep
 * their values.  mg_walks_frames_at with latents, times, frames and transforms in host memory, as mg_walks_frames_host. */
int mg_walks_time_functions_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps,
                                 const void *latents, int latent_dtype, int64_t n_walks, int32_t s_max, int64_t ld, double speed,
                                 double *times, int32_t *lengths, int32_t t_cap);
/* mg_walks_time_functions_smoothed in the same way (smooth_of_node is a host table in both) */
int mg_walks_time_functions_smoothed_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps,
                                          const uint8_t *smooth_of_node, const void *latents, int latent_dtype, int64_t n_walks, int32_t s_max,
                                          int64_t ld, double speed, double *times, int32_t *lengths, int32_t t_cap);
int mg_walks_frames_at_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents,
                            int latent_dtype, int64_t n_walks, int32_t s_max, int64_t ld, const double *times, const int32_t *lengths,
                            int32_t t_cap, const int64_t *frame_offset, const mg_alignment_desc *alignment,
                            const mg_skeleton_desc *skeleton, double *frames, int64_t walk_stride, double *transforms);
int mg_back_project_frames_host(mg_primitive *prim, const mg_time_grid *grid, const void *latents,
                                int latent_dtype, int64_t n_samples, int64_t ld, float *frames, int path);
int mg_back_project_frames_f64_host(mg_primitive *prim, const mg_time_grid *grid, const void *latents,
                                    int latent_dtype, int64_t n_samples, int64_t ld, double *frames);
int mg_back_project_coeffs_host(mg_primitive *prim, const void *latents, int latent_dtype,
                                int64_t n_samples, int64_t ld, void *coeffs, int out_dtype);
int mg_spline_evaluate_host(mg_primitive *prim, const mg_time_grid *grid, const double *coeffs,
                            int64_t n_splines, double *frames);
int mg_gmm_log_prob_host(mg_primitive *prim, const void *x, int x_dtype, int64_t n_samples, int64_t ld,
                         void *logp, int out_dtype);
int mg_gmm_sample_host(mg_primitive *prim, int64_t n_samples, const int64_t *counts, uint64_t seed,
                       void *x, int x_dtype, int64_t ld, int32_t *component);
int mg_score_constraints_host(mg_primitive *prim, const mg_constraint_set *cs, const void *latents,
                              int latent_dtype, int64_t n_samples, int64_t ld, void *errors, int out_dtype);
int mg_best_candidate_host(mg_primitive *prim, const mg_constraint_set *cs, const void *latents, int latent_dtype,
                           int64_t n_samples, int64_t ld, int64_t *best_index, double *min_error);
int mg_score_constraint_residuals_host(mg_primitive *prim, const mg_constraint_set *cs, const void *latents,
                                       int latent_dtype, int64_t n_samples, int64_t ld, double *residuals);
int mg_gmm_log_prob_jac_host(mg_primitive *prim, const void *x, int x_dtype, int64_t n_samples, int64_t ld,
                             double *jac);
int mg_cluster_tree_search_host(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                const mg_constraint_set *const *csets, int32_t n_candidates, mg_tree_search_record *records);
int mg_cluster_tree_search_trajectories_host(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                             const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                             const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                             const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_search_record *records);
int mg_cluster_tree_search_frames_host(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                       const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                       const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                       const mg_alignment_desc *const *alignments, const mg_tree_frame_lists *lists, int32_t n_candidates,
                                       void *scratch_dev, int64_t scratch_bytes, mg_tree_search_record *records);

#ifdef __cplusplus
}
#endif
#endif /* MG_HIP_H */
