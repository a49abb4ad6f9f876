"""Batched objective functions for the numerical optimizers: the GPU forms of
reference morphablegraphs/motion_generator/optimization/objective_functions.py for root-joint keyframe
constraints, in local coordinates or aligned to the previous motion on the device.

Every function keeps the reference's name, `data` tuple layout and return scaling, but takes a whole batch of
latent vectors (n, L) instead of one `s` and returns one row / value per sample, so that a finite-difference
Jacobian (scipy `leastsq` / `approx_fprime` evaluate the objective L+1 times per iteration,
reference least_squares.py:35-64) or a population of starting points is ONE launch.  A 1-D `s` is accepted and
gives the reference's shapes back.

`data[0]` is the motion primitive (anything exposing the HIP primitive as `._prim` or `.motion_primitive._prim`),
`data[1]` the constraint list (or an object with `.constraints`), `data[2]` the previous frames or None: with
previous frames and constraints that are not `is_local` every sample is aligned to the previous motion on the device
(candidate_scoring.alignment_from_prev_frames).  There is no CPU fallback.
"""
import numpy as np

from . import _capi
from .candidate_scoring import (constraints_to_device_form, cached_constraint_set, alignment_from_prev_frames, group_residuals,
                                split_trajectories, cached_trajectory, release_trajectory)


def _prim_of(motion_primitive):
    if hasattr(motion_primitive, "_prim"):
        return motion_primitive._prim
    if hasattr(motion_primitive, "motion_primitive") and hasattr(motion_primitive.motion_primitive, "_prim"):
        return motion_primitive.motion_primitive._prim
    if isinstance(motion_primitive, _capi.Primitive):
        return motion_primitive
    raise TypeError("objective_functions: %r does not wrap a HIP primitive" % (type(motion_primitive).__name__,))


def _constraint_list(mp_constraints):
    return mp_constraints.constraints if hasattr(mp_constraints, "constraints") else mp_constraints


def _batch(s):
    s = np.asarray(s)
    return (s[None, :], True) if s.ndim == 1 else (s, False)


def _note(mp_constraints, min_error, n):
    if hasattr(mp_constraints, "min_error"):
        mp_constraints.min_error = min_error
    if hasattr(mp_constraints, "evaluations"):
        mp_constraints.evaluations += n


def _residuals(prim, mp_constraints, S, prev_frames=None, sums=False):
    """(n, n_columns) weighted residuals like MotionPrimitiveConstraints.get_residual_vector
    (motion_primitive_constraints.py:124-144): one column per keyframe residual, then -- the optimizers are invariant to
    the order -- one column per canonical frame for every trajectory constraint (trajectory_constraint.py:91-115).
    sums=True: (n,) what MotionPrimitiveConstraints.evaluate adds up (:100-122) -- a keyframe constraint's weighted
    error, a trajectory constraint's weighted AVERAGE distance (:79-86)."""
    clist = constraints_to_device_form(_constraint_list(mp_constraints))
    if len(clist) == 0:
        return np.zeros(len(S)) if sums else np.zeros((len(S), 0))
    skeleton = getattr(mp_constraints, "hip_skeleton", None)
    alignment = alignment_from_prev_frames(prev_frames, mp_constraints, skeleton)
    from .frame_constraints import split_frame_constraints, frame_constraints_errors
    clist, frame_list = split_frame_constraints(clist)
    keyframes, trajectories = split_trajectories(clist)
    if trajectories and alignment is not None and alignment.get("joint", 0) not in (0, _capi.MG_ALIGN_START_POSE):
        raise NotImplementedError("trajectory constraints in global coordinates need the root joint as aligning node")
    blocks, total = [], np.zeros(len(S))
    if keyframes:
        cset = cached_constraint_set(prim, keyframes, skeleton, alignment)
        res = group_residuals(keyframes, prim.score_constraint_residuals(cset, S))
        blocks.append(res)
        total = total + res.sum(axis=1)
    for c in trajectories:
        err, res = prim.score_trajectory(cached_trajectory(prim, c), S, c.get("min_u", 0.0), c.get("weight", 1.0), alignment, residuals=True)
        blocks.append(res)
        total = total + err
    if frame_list:   # per-frame constraints (other joints' trajectories, collision avoidance, ...): tracks from the device, arithmetic on the host
        err, fblocks = frame_constraints_errors(prim, S, frame_list, skeleton, alignment)
        blocks += fblocks
        total = total + err
    if sums:
        return total
    return np.hstack(blocks) if blocks else np.zeros((len(S), 0))


def obj_spatial_error_sum(s, data):
    """objective_functions.py:141-159: MotionPrimitiveConstraints.evaluate per sample -> (n,) (float for 1-D s)."""
    motion_primitive, mp_constraints, prev_frames = data[:3]
    S, single = _batch(s)
    err = _residuals(_prim_of(motion_primitive), mp_constraints, S, prev_frames, sums=True)
    _note(mp_constraints, float(err[-1]) if len(err) else 0.0, len(S))
    return float(err[0]) if single else err


def log_likelihood_jac(s, gmm_or_primitive):
    """objective_functions.py:95-107: sum_k N_k(s) w_k Sigma_k^-1 (s - mu_k) / p(s) per row (= -grad log p)."""
    S, single = _batch(s)
    jac = _prim_of(gmm_or_primitive).gmm_log_prob_jac(S)
    return jac[0] if single else jac


def _objective_in_one_launch(prim, mp_constraints, S, prev_frames, error_scale, quality_scale):
    """(objective, constraint errors) from mg_objective_error_and_naturalness -- the mixture kernel scores the keyframe constraints
    on the latent tile it holds: one launch, the latents read once -- for the sets that kernel carries (root position / 2-D
    direction constraints, local or aligned through the root joint); None for everything else (the caller then makes the two
    calls, which give the same numbers)."""
    clist = constraints_to_device_form(_constraint_list(mp_constraints))
    if len(clist) == 0 or any(c.get("type") not in ("position", "direction") for c in clist):
        return None
    skeleton = getattr(mp_constraints, "hip_skeleton", None)
    alignment = alignment_from_prev_frames(prev_frames, mp_constraints, skeleton)
    cset = cached_constraint_set(prim, clist, skeleton, alignment)
    try:
        obj, err, _ = prim.objective(cset, np.asarray(S, dtype=np.float64), error_scale, quality_scale)
    except _capi.MGError as e:
        if e.status != -4:        # MG_ERR_UNSUPPORTED: a shape the one-launch kernel does not carry
            raise
        return None
    return obj, err


def obj_spatial_error_sum_and_naturalness(s, data):
    """objective_functions.py:162-184: error_scale * spatial_error + quality_scale * (-log p(s)).
    (The reference function computes this value and then falls off its end without `return`, so scipy receives
    None there; the batched form returns the value it computes.)"""
    motion_primitive, mp_constraints, prev_frames, error_scale, quality_scale = data[0], data[1], data[2], data[-3], data[-2]
    S, single = _batch(s)
    prim = _prim_of(motion_primitive)
    fused = _objective_in_one_launch(prim, mp_constraints, S, prev_frames, error_scale, quality_scale)
    if fused is not None:
        err, spatial = fused
    else:
        spatial = _residuals(prim, mp_constraints, S, prev_frames, sums=True)
        err = error_scale * spatial + (-prim.gmm_log_prob(S.astype(np.float64))) * quality_scale
    _note(mp_constraints, float(spatial[-1]) if len(spatial) else 0.0, len(S))
    return float(err[0]) if single else err


def spatial_error_jac(s, data, epsilon=1e-7):
    """The kinematic part of obj_spatial_error_sum_and_naturalness_jac (objective_functions.py:207):
    scipy approx_fprime's forward differences of obj_spatial_error_sum, (f(s + eps e_i) - f(s)) / eps, with all
    n * (L + 1) evaluations in one launch -> (n, L)."""
    motion_primitive, mp_constraints, prev_frames = data[:3]
    S, single = _batch(s)
    S = np.asarray(S, dtype=np.float64)
    n, L = S.shape
    pert = np.repeat(S[:, None, :], L + 1, axis=1)           # (n, L+1, L): row 0 unperturbed
    pert[:, np.arange(1, L + 1), np.arange(L)] += epsilon
    f = _residuals(_prim_of(motion_primitive), mp_constraints, pert.reshape(n * (L + 1), L), prev_frames, sums=True).reshape(n, L + 1)
    if hasattr(mp_constraints, "evaluations"):
        mp_constraints.evaluations += n * (L + 1)
    jac = (f[:, 1:] - f[:, :1]) / epsilon
    return jac[0] if single else jac


def obj_spatial_error_sum_and_naturalness_jac(s, data, epsilon=1e-7):
    """objective_functions.py:187-208: logLikelihood_jac * quality_scale + kinematic_jac * error_scale, the first
    analytic (mixture), the second by forward differences.  NB the reference reads error_scale = data[-1] and
    quality_scale = data[-2] here (not [-3], [-2] as in the objective); kept."""
    error_scale, quality_scale = data[-1], data[-2]
    S, single = _batch(s)
    jac = log_likelihood_jac(S, data[0]) * quality_scale + spatial_error_jac(S, data, epsilon) * error_scale
    return jac[0] if single else jac


def _pad(res, n_variables):
    if res.shape[1] < n_variables:   # `while n_error_values < n_variables: residual_vector.append(0)`
        res = np.hstack([res, np.zeros((res.shape[0], n_variables - res.shape[1]))])
    return res


def obj_spatial_error_residual_vector(s, data):
    """objective_functions.py:209-236: weighted residual of every constraint, zero-padded to n_variables columns,
    divided by init_error_sum -> (n, max(n_constraints, L))."""
    motion_primitive, mp_constraints, prev_frames, error_scale, quality_scale, init_error_sum = data
    S, single = _batch(s)
    res = _residuals(_prim_of(motion_primitive), mp_constraints, S, prev_frames)
    _note(mp_constraints, float(res[-1].sum()) if len(res) else 0.0, len(S))
    out = _pad(res, S.shape[1]) / init_error_sum
    return out[0] if single else out


def obj_spatial_error_residual_vector_and_naturalness(s, data):
    """objective_functions.py:239-267: (residual_i * error_scale - log p(s) * quality_scale), zero-padded to
    n_variables columns, divided by init_error_sum."""
    mp, mp_constraints, prev_frames, error_scale, quality_scale, init_error_sum = data
    S, single = _batch(s)
    prim = _prim_of(mp)
    nll = -prim.gmm_log_prob(S.astype(np.float64)) * quality_scale
    res = _residuals(prim, mp_constraints, S, prev_frames)
    _note(mp_constraints, float(res[-1].sum()) if len(res) else 0.0, len(S))
    out = _pad(res * error_scale + nll[:, None], S.shape[1]) / init_error_sum
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------------
# Graph-walk (global) objectives: reference optimization/objective_functions.py:290-380, driven by
# motion_generator/graph_walk_optimizer.py:78-105.  `s` concatenates the spatial latents of the walk's steps; per step the
# reference back-projects, evaluates the step's constraints against the PREVIOUS step's aligned frames and aligns this step's
# motion for the next one -- a chain.  Batched: S (n, sum L_i); a candidate's chain is its own (its step i is aligned to ITS
# step i - 1), so per step ONE launch scores all n candidates with a per-candidate alignment record
# (mg_score_constraint_residuals_chained) and returns, beside the residuals, the four numbers of the aligned motion's last
# frame the next step is aligned to (MG_CONSTRAINT_VALUE_*): the chain never leaves the device arithmetic, the host only
# slices.  Alignment itself is PARITY UNPINNED (anim_utils absent), as for the per-primitive objectives.
# ---------------------------------------------------------------------------------------------------------------------
def _aligning_node(motion_primitive_graph):
    sk = getattr(motion_primitive_graph, "skeleton", None)
    node = getattr(sk, "aligning_root_node", None)
    ref_dir = tuple(float(v) for v in getattr(sk, "aligning_root_dir", (0.0, 0.0, 1.0)))
    if node is not None and node == getattr(sk, "root", None):
        node = None
    return node, ref_dir


def _trajectory_alignment_check(trajectories, alignment):
    if trajectories and alignment is not None and alignment.get("joint", 0) not in (0, _capi.MG_ALIGN_START_POSE):
        raise NotImplementedError("trajectory constraints in global coordinates need the root joint as aligning node")


def _global_blocks(s, motion_primitive_graph, graph_walk_steps, prev_frames, exit_from="frames", states=None):
    """Per step the (n, n_residuals_i) matrix of a batch of concatenated latent vectors, every candidate's steps chained, and per
    step the (n,) error MotionPrimitiveConstraints.evaluate adds up -> (S, single, blocks, errors).  A step's block is its grouped
    keyframe columns, then T columns per trajectory constraint in list order (the order of _residuals); its error is the keyframe
    columns' sum plus every trajectory's weighted AVERAGE distance -- not the sum of its T columns.  A trajectory is scored like
    the step's keyframe set: against the walk's record on the first step (score_trajectory), unaligned on a local step, and on a
    later step against every candidate's own previous step (score_trajectory_chained on the state the keyframe route carries).
    exit_from: "frames" -- the next step is aligned to the last FRAME of this step's aligned motion (obj_global_error_sum,
    obj_global_residual_vector: get_motion_vector()[-1], canonical time F); "coeffs" -- to its last CONTROL POINT
    (obj_global_residual_vector_and_naturalness hands `.coeffs` on, objective_functions.py:373: the spline at its last knot).
    states: a list that receives the (n, 4) exit state every step hands on."""
    S, single = _batch(s)
    S = np.asarray(S, dtype=np.float64)
    n = len(S)
    hip_sk = getattr(motion_primitive_graph, "hip_skeleton", None)
    node_name, ref_dir = _aligning_node(motion_primitive_graph)
    if node_name is not None and hip_sk is None:
        raise NotImplementedError("aligning node %r is not the root joint: the graph needs a _capi.Skeleton as .hip_skeleton" % (node_name,))
    joint = 0 if node_name is None else node_name
    state, offset, blocks, errors = None, 0, [], []
    for step in graph_walk_steps:
        node = motion_primitive_graph.nodes[step.node_key]
        prim = _prim_of(node)
        Li = int(step.n_spatial_components)
        alpha = np.ascontiguousarray(S[:, offset:offset + Li])
        offset += Li
        cons = step.motion_primitive_constraints
        keyframes, trajectories = split_trajectories(constraints_to_device_form(_constraint_list(cons)))
        sk = getattr(cons, "hip_skeleton", None) or hip_sk
        F = float(prim.n_canonical_frames)
        t_exit = F if exit_from == "frames" else F - 1.0
        exits = [{"type": "value_heading", "t": t_exit, "weight": 1.0, "axis": 0, "joint": joint, "ref_dir": ref_dir},
                 {"type": "value_heading", "t": t_exit, "weight": 1.0, "axis": 2, "joint": joint, "ref_dir": ref_dir},
                 {"type": "value_position", "t": t_exit, "weight": 1.0, "axis": 0},
                 {"type": "value_position", "t": t_exit, "weight": 1.0, "axis": 2}]
        local = bool(getattr(cons, "is_local", False))
        if state is None:
            # first step: the walk's previous frames (or start pose, or nothing) -- the same record for every candidate
            al_motion = alignment_from_prev_frames(prev_frames, type("_NotLocal", (), {"start_pose": getattr(cons, "start_pose", None), "is_local": False,
                                                                                      "skeleton": getattr(cons, "skeleton", getattr(motion_primitive_graph, "skeleton", None))})(), sk)
            al_cons = None if local else al_motion
            _trajectory_alignment_check(trajectories, al_cons)
            traj = [prim.score_trajectory(cached_trajectory(prim, c), alpha, c.get("min_u", 0.0), c.get("weight", 1.0), al_cons, residuals=True)
                    for c in trajectories]
            if al_cons is al_motion:
                res = prim.score_constraint_residuals(cached_constraint_set(prim, keyframes + exits, sk, al_motion), alpha)
                res_k, new_state = res[:, :len(keyframes)], res[:, len(keyframes):]
            else:
                res_k = prim.score_constraint_residuals(cached_constraint_set(prim, keyframes, sk, None), alpha) if keyframes else np.zeros((n, 0))
                new_state = prim.score_constraint_residuals(cached_constraint_set(prim, exits, sk, al_motion), alpha)
        else:
            template = {"joint": joint, "position": (0.0, 0.0, 0.0), "heading": (0.0, 1.0), "ref_dir": ref_dir}
            _trajectory_alignment_check(trajectories, None if local else template)
            traj = [prim.score_trajectory(cached_trajectory(prim, c), alpha, c.get("min_u", 0.0), c.get("weight", 1.0), None, residuals=True) if local else
                    prim.score_trajectory_chained(cached_trajectory(prim, c), alpha, state, template, c.get("min_u", 0.0), c.get("weight", 1.0), residuals=True)
                    for c in trajectories]
            if local:
                res_k = prim.score_constraint_residuals(cached_constraint_set(prim, keyframes, sk, None), alpha) if keyframes else np.zeros((n, 0))
                new_state = prim.score_constraint_residuals_chained(cached_constraint_set(prim, exits, sk, template), alpha, state)
            else:
                res = prim.score_constraint_residuals_chained(cached_constraint_set(prim, keyframes + exits, sk, template), alpha, state)
                res_k, new_state = res[:, :len(keyframes)], res[:, len(keyframes):]
        block = group_residuals(keyframes, res_k) if keyframes else res_k
        err = block.sum(axis=1)
        for e, _ in traj:
            err = err + e
        blocks.append(np.hstack([block] + [r for _, r in traj]) if traj else block)
        errors.append(err)
        state = np.ascontiguousarray(new_state)
        if states is not None:
            states.append(state)
        if hasattr(cons, "evaluations"):
            cons.evaluations += n
    return S, single, blocks, errors


def obj_global_error_sum(s, data):
    """objective_functions.py:290-316: the sum over the walk's steps of MotionPrimitiveConstraints.evaluate, each step scored
    against the previous step's aligned frames -> (n,) (float for 1-D s).  (The reference prints the value on every call.)"""
    motion_primitive_graph, graph_walk_steps, error_scale, quality_scale, prev_frames = data
    S, single, _, errors = _global_blocks(s, motion_primitive_graph, graph_walk_steps, prev_frames, "frames")
    err = np.zeros(len(S))
    for e in errors:
        err = err + e
    return float(err[0]) if single else err


def obj_global_residual_vector(s, data):
    """objective_functions.py:319-345: the steps' residual vectors (each zero-padded to its number of variables) side by side,
    divided by init_error_sum.  NB the reference hands obj_spatial_error_residual_vector a FIVE-element step_data where that
    function unpacks six (:341 vs :220), so the reference raises ValueError here; this is the evident intent, with the missing
    per-step init_error_sum = 1 as in the _and_naturalness form (:369)."""
    motion_primitive_graph, graph_walk_steps, error_scale, quality_scale, prev_frames, init_error_sum = data
    S, single, blocks, _ = _global_blocks(s, motion_primitive_graph, graph_walk_steps, prev_frames, "frames")
    cols = [_pad(b, int(step.n_spatial_components)) for b, step in zip(blocks, graph_walk_steps)]
    out = np.hstack(cols) / init_error_sum
    return out[0] if single else out


def obj_global_residual_vector_and_naturalness(s, data):
    """objective_functions.py:348-380: per step residual_i * error_scale - log p(concat(alpha, the step's time latents)) *
    quality_scale, zero-padded to the step's FULL number of latents, side by side, divided by init_error_sum; the next step is
    aligned to this step's aligned CONTROL POINTS (the reference passes `.coeffs` on as frames, :362,:373)."""
    motion_primitive_graph, graph_walk_steps, error_scale, quality_scale, prev_frames, init_error_sum = data
    S, single, blocks, _ = _global_blocks(s, motion_primitive_graph, graph_walk_steps, prev_frames, "coeffs")
    cols, offset = [], 0
    for b, step in zip(blocks, graph_walk_steps):
        Li = int(step.n_spatial_components)
        node = motion_primitive_graph.nodes[step.node_key]
        prim = _prim_of(node)
        tail = np.asarray(step.parameters, dtype=np.float64)[Li:]
        concat = np.hstack([S[:, offset:offset + Li], np.tile(tail, (len(S), 1))]) if len(tail) else S[:, offset:offset + Li]
        offset += Li
        nll = -prim.gmm_log_prob(np.ascontiguousarray(concat, dtype=np.float64)) * quality_scale
        cols.append(_pad(b * error_scale + nll[:, None], concat.shape[1]))
    out = np.hstack(cols) / init_error_sum
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------------
# The same objectives with the whole walk in ONE launch (mg_score_walk_residuals, csrc/mg_walk_score.hip): a wave keeps its 16
# candidates for all steps and hands the four exit values on in its LDS, where _global_blocks makes a launch, three copies and
# a synchronisation per step.  The residuals are the chain's, bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
def _exit_constraints(t_exit, joint, ref_dir):
    return [{"type": "value_heading", "t": t_exit, "weight": 1.0, "axis": 0, "joint": joint, "ref_dir": ref_dir},
            {"type": "value_heading", "t": t_exit, "weight": 1.0, "axis": 2, "joint": joint, "ref_dir": ref_dir},
            {"type": "value_position", "t": t_exit, "weight": 1.0, "axis": 0},
            {"type": "value_position", "t": t_exit, "weight": 1.0, "axis": 2}]


class HipGraphWalkObjective(object):
    """The chained objective of graph_walk_steps over motion_primitive_graph, its device sets built once.  Per call: one upload
    of S (n, sum L_i), one launch, one download.  The sets are the ones _global_blocks asks for (the same `keyframes + exits`
    lists, the same local-step split, the same first-step record), so blocks(S) equals _global_blocks(S, ...)[2].

    A step's trajectory constraints are one launch each on the same stream behind the walk's (mg_score_trajectory; on a later
    step that is not local mg_score_trajectory_chained on the exit values the walk's launch wrote for the step before,
    mg_score_walk_residuals_steps): still one upload and one download, n_launches grows by 1 + the number of trajectories per
    call.  The trajectories are pinned for the life of the objective (close() releases them).

    Raises NotImplementedError where _global_blocks does, ValueError for more than MG_WALK_MAX_STEPS steps; a call raises
    _capi.MGError(-4) where a step's tables do not fit LDS (the callers then take the chain)."""

    def __init__(self, motion_primitive_graph, graph_walk_steps, prev_frames=None, exit_from="frames"):
        self.graph, self.steps, self.prev_frames, self.exit_from = motion_primitive_graph, list(graph_walk_steps), prev_frames, exit_from
        if not 1 <= len(self.steps) <= _capi.MG_WALK_MAX_STEPS:
            raise ValueError("%d steps: 1 .. %d per launch" % (len(self.steps), _capi.MG_WALK_MAX_STEPS))
        self._private, self._shared, self._buf, self._cap = [], [], None, 0
        self._trajectories = []      # [(pinned trajectory, min_u, weight, step index, column offset in the step's block, alignment, chained)]
        self.n_launches = 0
        try:
            self._build()
        except Exception:
            self.close()      # (nothing stays pinned behind a refused walk)
            raise

    def _set(self, prim, clist, sk, alignment, taken):
        """cached_constraint_set, unless the shared set of this structure already serves another step of this walk with other
        values (one launch reads all steps' sets at once): then a set of the objective's own."""
        from .candidate_scoring import _structure_key, _values_key
        key, values = _structure_key(prim, clist, sk, alignment), _values_key(clist, alignment)
        if taken.setdefault(key, values) != values:
            cs = _capi.ConstraintSet(prim, clist, sk, alignment)
            self._private.append(cs)
            return cs
        cs = cached_constraint_set(prim, clist, sk, alignment)
        self._shared.append((cs, values))
        return cs

    def _build(self):
        graph = self.graph
        hip_sk = getattr(graph, "hip_skeleton", None)
        node_name, ref_dir = _aligning_node(graph)
        if node_name is not None and hip_sk is None:
            raise NotImplementedError("aligning node %r is not the root joint: the graph needs a _capi.Skeleton as .hip_skeleton" % (node_name,))
        joint = 0 if node_name is None else node_name
        for cs in self._private:
            cs.close()
        self._release_trajectories()
        self._private, self._shared = [], []
        taken, records, self._info = {}, [], []
        offset = column = 0
        for i, step in enumerate(self.steps):
            prim = _prim_of(graph.nodes[step.node_key])
            Li = int(step.n_spatial_components)
            cons = step.motion_primitive_constraints
            keyframes, trajectories = split_trajectories(constraints_to_device_form(_constraint_list(cons)))
            sk = getattr(cons, "hip_skeleton", None) or hip_sk
            F = float(prim.n_canonical_frames)
            exits = _exit_constraints(F if self.exit_from == "frames" else F - 1.0, joint, ref_dir)
            local = bool(getattr(cons, "is_local", False))
            if i == 0:
                al_motion = alignment_from_prev_frames(self.prev_frames, type("_NotLocal", (), {
                    "start_pose": getattr(cons, "start_pose", None), "is_local": False,
                    "skeleton": getattr(cons, "skeleton", getattr(graph, "skeleton", None))})(), sk)
            else:
                al_motion = {"joint": joint, "position": (0.0, 0.0, 0.0), "heading": (0.0, 1.0), "ref_dir": ref_dir}
            if local and not (i == 0 and al_motion is None):      # (a local first step without a record: one unaligned set, as in _global_blocks)
                scored = self._set(prim, keyframes, sk, None, taken) if keyframes else None
                exit_set = self._set(prim, exits, sk, al_motion, taken)
            else:
                scored, exit_set = self._set(prim, keyframes + exits, sk, al_motion, taken), None
            # (a trajectory is aligned like the step's scored set: the walk's record, nothing on a local step, the candidate's own state)
            al_traj = None if local else al_motion
            _trajectory_alignment_check(trajectories, al_traj)
            width = len(keyframes) if not keyframes else group_residuals(keyframes, np.zeros((0, len(keyframes)))).shape[1]
            for c in trajectories:
                self._trajectories.append((cached_trajectory(prim, c, pin=True), c.get("min_u", 0.0), c.get("weight", 1.0), i, width, al_traj,
                                           i > 0 and not local))
                width += prim._grid_size(None)
            records.append((prim, scored, exit_set, offset, len(keyframes), column))
            self._info.append((prim, keyframes, Li, offset, column, cons))
            offset += Li
            column += len(keyframes)
        self.n_latents, self.n_columns = offset, column
        self.table = _capi.WalkScoreTable(records)
        self.ctx = self.table.ctx

    def _ensure(self):
        """A shared set may have been rewritten for another caller's values, or closed by the cache, since the table was made."""
        if any(not cs.handle or cs.cached_values != values for cs, values in self._shared):
            self._build()

    def _release_trajectories(self):
        while self._trajectories:
            release_trajectory(self._trajectories.pop()[0])

    def close(self):
        for cs in self._private:
            cs.close()
        self._private = []
        self._release_trajectories()
        if self._buf is not None:
            self._buf.free()
        self._buf, self._cap = None, 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, S, logp=False):
        """-> (residuals (n, n_columns), errors (n), exit state (n, 4), {step: log p (n)} for the steps whose mixture has no time
        latents, [(n, T) residuals per trajectory]).  One device block: the latents, then everything that comes back, then what
        stays on the device (every step's exit values and the (n, 4) block of them a chained trajectory launch reads)."""
        self._ensure()
        S = _capi._latents(S)
        if S.shape[1] < self.n_latents:
            raise ValueError("latent rows of %d columns, the walk's steps need %d" % (S.shape[1], self.n_latents))
        n, ld, m = S.shape[0], S.shape[1], len(self._info)
        on_device = [i for i, (prim, _, Li, _, _, _) in enumerate(self._info)
                     if logp and len(np.asarray(self.steps[i].parameters)) <= Li and prim.n_gmm_dims == Li]
        lat_bytes = (S.nbytes + 255) & ~255
        traj_T = [t[0].prim._grid_size(None) for t in self._trajectories]
        chained = any(t[6] for t in self._trajectories)      # some step past the first follows a trajectory from its candidates' states
        n_out = n * (self.n_columns + 5 + len(on_device) + sum(traj_T))
        need = lat_bytes + 8 * max(n_out, 1) + (8 * n * 4 * (m + 1) if chained else 0)
        if need > self._cap:
            if self._buf is not None:
                self._buf.free()
            self._buf, self._cap = self.ctx.malloc(2 * need), 2 * need
        base = self._buf.address
        d_res = base + lat_bytes
        d_err = d_res + 8 * n * self.n_columns
        d_exit = d_err + 8 * n
        d_logp = d_exit + 8 * n * 4
        d_traj = d_logp + 8 * n * len(on_device)
        d_steps = base + lat_bytes + 8 * max(n_out, 1)      # (n, m, 4), then the (n, 4) rows of one step gathered from it
        d_state = d_steps + 8 * n * 4 * m
        if n == 0:
            return np.zeros((0, self.n_columns)), np.zeros(0), np.zeros((0, 4)), {i: np.zeros(0) for i in on_device}, [np.zeros((0, T)) for T in traj_T]
        self.ctx.upload_into(base, S)
        self.table.score_dev(base, S.dtype, n, ld, d_res if self.n_columns else None, self.n_columns, d_err, d_exit, d_steps if chained else None)
        self.n_launches += 1
        gathered, d_r = None, d_traj
        for (t, min_u, weight, i, _, al, chain), T in zip(self._trajectories, traj_T):     # stream ordered behind the walk's launch
            prim, _, _, offset, _, _ = self._info[i]
            lat = base + offset * S.dtype.itemsize
            if chain:
                if gathered != i:      # the state step i is aligned to: step i - 1's exit values of every candidate, side by side
                    self.ctx.copy_rows_dev(d_state, 32, d_steps + 32 * (i - 1), 32 * m, 32, n)
                    gathered = i
                prim.score_trajectory_chained_dev(t, lat, S.dtype, n, ld, d_state, al, d_err, min_u, weight, True, d_r)
            else:
                prim.score_trajectory_dev(t, lat, S.dtype, n, ld, d_err, min_u, weight, al, True, d_r)
            self.n_launches += 1
            d_r += 8 * n * T
        for j, i in enumerate(on_device):      # stream ordered behind the walk's launch, on the latents already there
            prim, _, Li, offset, _, _ = self._info[i]
            prim.gmm_log_prob_dev(base + offset * S.dtype.itemsize, S.dtype, n, ld, d_logp + 8 * n * j, np.float64)
        out = self.ctx.download(d_res, (n_out,), np.float64)
        res = out[:n * self.n_columns].reshape(n, self.n_columns)
        err = out[n * self.n_columns:n * (self.n_columns + 1)]
        ex = out[n * (self.n_columns + 1):n * (self.n_columns + 5)].reshape(n, 4)
        lp = {i: out[n * (self.n_columns + 5 + j):n * (self.n_columns + 6 + j)] for j, i in enumerate(on_device)}
        tres, at = [], n * (self.n_columns + 5 + len(on_device))
        for T in traj_T:
            tres.append(out[at:at + n * T].reshape(n, T))
            at += n * T
        for _, _, _, _, _, cons in self._info:
            if hasattr(cons, "evaluations"):
                cons.evaluations += n
        return res, err, ex, lp, tres

    def _blocks_of(self, res, tres=()):
        out = []
        for i, (_, keyframes, _, _, column, _) in enumerate(self._info):
            res_k = res[:, column:column + len(keyframes)]
            block = group_residuals(keyframes, res_k) if keyframes else res_k
            mine = [r for t, r in zip(self._trajectories, tres) if t[3] == i]     # in list order, at the columns _build recorded
            out.append(np.hstack([block] + mine) if mine else block)
        return out

    def blocks(self, S):
        """Per step the (n, n_residuals_i) matrix: _global_blocks(S, ...)[2]."""
        run = self._run(S)
        return self._blocks_of(run[0], run[4])

    def exit_state(self, S):
        """(n, 4): the last step's exit values (unit heading x, z; root position x, z)."""
        return self._run(S)[2]

    def error_sum(self, S):
        """(n,): per step the residuals added in constraint order, the step sums added in step order (on the device); then every
        trajectory's error in step and list order."""
        return self._run(S)[1].copy()

    def residual_vector(self, S, init_error_sum):
        """obj_global_residual_vector's rows for the batch S."""
        run = self._run(S)
        blocks = self._blocks_of(run[0], run[4])
        cols = [_pad(b, int(step.n_spatial_components)) for b, step in zip(blocks, self.steps)]
        return np.hstack(cols) / init_error_sum

    def residual_vector_and_naturalness(self, S, error_scale, quality_scale, init_error_sum):
        """obj_global_residual_vector_and_naturalness' rows for the batch S: the mixtures of the steps without time latents are
        scored on the latents the walk's launch has read (mg_gmm_log_prob at the step's column), everything comes back in one
        download; a step with time latents (its tail is concatenated) goes through the host for its mixture."""
        S = np.asarray(_batch(S)[0], dtype=np.float64)
        res, _, _, lp, tres = self._run(S, logp=True)
        cols = []
        for i, (b, step) in enumerate(zip(self._blocks_of(res, tres), self.steps)):
            prim, _, Li, offset, _, _ = self._info[i]
            width = Li
            if i in lp:
                nll = -lp[i] * quality_scale
            else:
                tail = np.asarray(step.parameters, dtype=np.float64)[Li:]
                concat = np.hstack([S[:, offset:offset + Li], np.tile(tail, (len(S), 1))]) if len(tail) else S[:, offset:offset + Li]
                nll = -prim.gmm_log_prob(np.ascontiguousarray(concat, dtype=np.float64)) * quality_scale
                width = concat.shape[1]
            cols.append(_pad(b * error_scale + nll[:, None], width))
        return np.hstack(cols) / init_error_sum


_WALK_OBJECTIVES = []      # [(graph, steps, constraint lists, prev_frames, exit_from, objective)], most recent last
_WALK_OBJECTIVES_SIZE = 4


def _walk_objective(motion_primitive_graph, graph_walk_steps, prev_frames, exit_from):
    """The HipGraphWalkObjective of these very objects (the step list, every step's constraint list and prev_frames, by identity:
    an optimiser hands the same `data` tuple over hundreds of times), built on first use.  None for a walk of more than
    MG_WALK_MAX_STEPS steps."""
    if len(graph_walk_steps) > _capi.MG_WALK_MAX_STEPS:
        return None
    lists = [_constraint_list(step.motion_primitive_constraints) for step in graph_walk_steps]
    for k, (g, st, ls, pf, ef, obj) in enumerate(_WALK_OBJECTIVES):
        if g is motion_primitive_graph and st is graph_walk_steps and pf is prev_frames and ef == exit_from and len(ls) == len(lists) and \
                all(a is b for a, b in zip(ls, lists)):
            _WALK_OBJECTIVES.append(_WALK_OBJECTIVES.pop(k))
            return obj
    obj = HipGraphWalkObjective(motion_primitive_graph, graph_walk_steps, prev_frames, exit_from)
    _WALK_OBJECTIVES.append((motion_primitive_graph, graph_walk_steps, lists, prev_frames, exit_from, obj))
    while len(_WALK_OBJECTIVES) > _WALK_OBJECTIVES_SIZE:
        _WALK_OBJECTIVES.pop(0)[-1].close()
    return obj


def clear_walk_objectives():
    """Drop the cached walk objectives (call before closing a primitive they belong to)."""
    while _WALK_OBJECTIVES:
        _WALK_OBJECTIVES.pop()[-1].close()
    while _WALK_TIME_OBJECTIVES:
        _WALK_TIME_OBJECTIVES.pop()[-1].close()


def _one_launch(s, motion_primitive_graph, graph_walk_steps, prev_frames, exit_from, method, args, chain):
    """method(S, *args) of the walk's objective; the chain's function where the walk has more than MG_WALK_MAX_STEPS steps or a
    step's tables do not fit the kernel's LDS (MG_ERR_UNSUPPORTED)."""
    obj = _walk_objective(motion_primitive_graph, graph_walk_steps, prev_frames, exit_from)
    if obj is None:
        return chain()
    S, single = _batch(s)
    try:
        out = getattr(obj, method)(S, *args)
    except _capi.MGError as e:
        if e.status != _capi.MG_ERR_UNSUPPORTED:
            raise
        return chain()
    return (float(out[0]) if out.ndim == 1 else out[0]) if single else out


def obj_global_error_sum_one_launch(s, data):
    """obj_global_error_sum with the walk in one launch.  (The steps' sums are added on the device one by one, NumPy's row sums
    are pairwise: the last bits may differ from the chain's.)"""
    motion_primitive_graph, graph_walk_steps, error_scale, quality_scale, prev_frames = data
    return _one_launch(s, motion_primitive_graph, graph_walk_steps, prev_frames, "frames", "error_sum", (), lambda: obj_global_error_sum(s, data))


def obj_global_residual_vector_one_launch(s, data):
    """obj_global_residual_vector with the walk in one launch: the same bits."""
    motion_primitive_graph, graph_walk_steps, error_scale, quality_scale, prev_frames, init_error_sum = data
    return _one_launch(s, motion_primitive_graph, graph_walk_steps, prev_frames, "frames", "residual_vector", (init_error_sum,),
                       lambda: obj_global_residual_vector(s, data))


def obj_global_residual_vector_and_naturalness_one_launch(s, data):
    """obj_global_residual_vector_and_naturalness with the walk in one launch: the same bits."""
    motion_primitive_graph, graph_walk_steps, error_scale, quality_scale, prev_frames, init_error_sum = data
    return _one_launch(s, motion_primitive_graph, graph_walk_steps, prev_frames, "coeffs", "residual_vector_and_naturalness",
                       (error_scale, quality_scale, init_error_sum), lambda: obj_global_residual_vector_and_naturalness(s, data))


# ---------------------------------------------------------------------------------------------------------------------
# Time constraints (reference constraints/time_constraints.py:25-110, objective optimization/objective_functions.py:270-287)
# ---------------------------------------------------------------------------------------------------------------------
class HipTimeConstraints(object):
    """TimeConstraints for batches: `s` concatenates the TIME latents of the steps start_step .. end_step; per step the
    canonical time functions of all candidates come from one launch (mg_time_function_canonical), their inversion runs on the
    host with scipy as in the reference, the naturalness term is one mixture launch per step."""

    def __init__(self, motion_primitive_graph, graph_walk, start_step, end_step, constraint_list):
        self.start_step, self.end_step, self.constraint_list = start_step, end_step, constraint_list
        self.start_keyframe = self._get_start_frame(motion_primitive_graph, graph_walk, start_step)

    def _get_start_frame(self, graph, graph_walk, start_step):
        start_keyframe = 0
        for i in range(0, max(start_step, 0)):
            tf = graph.nodes[graph_walk.steps[i].node_key].back_project_time_function(graph_walk.steps[i].parameters)
            start_keyframe += tf[-1]
        return start_keyframe

    def _time_functions(self, S, graph, graph_walk):
        """[step][candidate] -> time function t'(t) (1-D array)"""
        out, offset = [], 0
        for step in graph_walk.steps[self.start_step:self.end_step]:
            nt = int(step.n_time_components)
            base = np.asarray(step.parameters, dtype=np.float64)
            vecs = np.tile(base, (len(S), 1))
            vecs[:, int(step.n_spatial_components):] = S[:, offset:offset + nt]
            offset += nt
            node = graph.nodes[step.node_key]
            # the wrapper's back_project_time_function (motion_primitive_wrapper.py:233-249, legacy branch) for every candidate:
            # one launch where the node offers the batched form
            out.append(node.back_project_time_functions(vecs) if hasattr(node, "back_project_time_functions")
                       else [node.back_project_time_function(v) for v in vecs])
        return out

    def evaluate_graph_walk(self, s, graph, graph_walk):
        """time_constraints.py:40-50,68-91 for every candidate -> (n,)"""
        S, single = _batch(s)
        S = np.asarray(S, dtype=np.float64)
        tfs = self._time_functions(S, graph, graph_walk)
        frame_time = graph.skeleton.frame_time
        err = np.zeros(len(S))
        for b in range(len(S)):
            for step_index, keyframe_index, desired_time in self.constraint_list:
                n_frames, e = self.start_keyframe, 10000.0        # (the reference's value when the constrained step is beyond the walk)
                for k, per_step in enumerate(tfs):
                    tf = per_step[b]
                    if k < step_index:
                        n_frames += tf[-1]
                    else:
                        if keyframe_index >= len(tf):
                            e = 0.0
                        else:
                            n_frames += int(tf[keyframe_index]) + 1
                            e = (desired_time - n_frames * frame_time) ** 2
                        break
                err[b] += e
        return float(err[0]) if single else err

    def get_average_loglikelihood(self, s, graph, graph_walk):
        """time_constraints.py:93-102 for every candidate -> (n,)"""
        S, single = _batch(s)
        S = np.asarray(S, dtype=np.float64)
        total, count, offset = np.zeros(len(S)), 0, 0
        for step in graph_walk.steps[self.start_step:self.end_step]:
            nt, ns = int(step.n_time_components), int(step.n_spatial_components)
            X = np.hstack([np.tile(np.asarray(step.parameters, dtype=np.float64)[:ns], (len(S), 1)), S[:, offset:offset + nt]])
            offset += nt
            total += _prim_of(graph.nodes[step.node_key]).gmm_log_prob(np.ascontiguousarray(X))
            count += 1
        out = total / max(count, 1)
        return float(out[0]) if single else out

    def get_initial_guess(self, graph_walk):
        parameters = []
        for step in graph_walk.steps[self.start_step:self.end_step]:
            parameters += np.asarray(step.parameters)[int(step.n_spatial_components):].tolist()
        return parameters


def obj_time_error_sum(s, data):
    """objective_functions.py:270-287: error_scale * time_error + quality_scale * (-average log-likelihood) -> (n,)"""
    motion_primitive_graph, graph_walk, time_constraints, error_scale, quality_scale = data
    time_error = time_constraints.evaluate_graph_walk(s, motion_primitive_graph, graph_walk)
    nll = -np.asarray(time_constraints.get_average_loglikelihood(s, motion_primitive_graph, graph_walk))
    out = error_scale * np.asarray(time_error) + nll * quality_scale
    return float(out) if np.ndim(out) == 0 else out


# ---------------------------------------------------------------------------------------------------------------------
# The time objective with the whole window in ONE launch (mg_score_walk_time, csrc/mg_walk_time.hip): a workgroup keeps its 16
# candidates for all steps -- the time functions, the entries the constraints read and the mixtures' scores meet in its LDS --
# where obj_time_error_sum makes two launches, two uploads and two downloads per step and loops over candidates, constraints
# and steps on the host.  The values are the chain's, bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
def walk_time_objective_host(time_functions, log_likelihoods, constraint_list, start_keyframe, frame_time, error_scale, quality_scale, parts=False):
    """The arithmetic of mg_score_walk_time in NumPy, float64, no device.  time_functions: per step of the window the canonical
    time functions of the candidates (n, F_k); log_likelihoods: per step the mixture's log p of every candidate (n,);
    constraint_list: (step counted from the window's first step, canonical keyframe, desired time).  -> objective (n,), or with
    parts (objective, error, average log-likelihood).  time_constraints.py:68-102, objective_functions.py:270-287: constraints in
    list order, steps in step order, int() towards zero; a candidate with a non-finite entry among those read has error and
    objective NaN; a keyframe below -F_k raises IndexError."""
    tfs = [np.atleast_2d(np.asarray(tf, dtype=np.float64)) for tf in time_functions]
    if not tfs:
        raise ValueError("a window has at least one step")
    n, m = tfs[0].shape[0], len(tfs)
    before, finite = [], np.ones(n, dtype=bool)
    n_before = np.full(n, float(start_keyframe))
    for tf in tfs:                                   # frames before step k: start_keyframe + t_0(F - 1) + ... in step order
        before.append(n_before)
        finite &= np.isfinite(tf[:, -1])
        n_before = n_before + tf[:, -1]
    err = np.zeros(n)
    for step_index, keyframe_index, desired_time in constraint_list:
        k = max(int(step_index), 0)                  # (the reference's loop takes the first step it meets for a negative index)
        if k >= m:
            e = 10000.0
        elif keyframe_index >= tfs[k].shape[1]:
            e = 0.0
        else:
            t = tfs[k][:, keyframe_index]            # IndexError below -F, as in the reference
            finite &= np.isfinite(t)
            n_frames = before[k] + (np.trunc(np.where(np.isfinite(t), t, 0.0)) + 1.0)
            d = desired_time - n_frames * frame_time
            e = d * d
        err = err + e
    total = np.zeros(n)
    for lp in log_likelihoods:
        total = total + np.asarray(lp, dtype=np.float64)
    avg = total / m
    obj = error_scale * err + (-avg) * quality_scale
    err, obj = np.where(finite, err, np.nan), np.where(finite, obj, np.nan)
    return (obj, err, avg) if parts else obj


class HipWalkTimeObjective(object):
    """obj_time_error_sum of the steps start_step .. end_step of graph_walk under `time_constraints` (a HipTimeConstraints: its
    start_step, end_step, constraint_list and start_keyframe are read), its tables built once: the step table and every step's
    fixed spatial latents go to the device here.  evaluate(): one upload of S, one launch, one download.

    Raises NotImplementedError for a window the launch does not state (no step, a static primitive, a node without HIP primitive,
    a step whose widths are not its primitive's) and IndexError for a keyframe below -n_canonical_frames; evaluate() raises
    _capi.MGError(MG_ERR_UNSUPPORTED) where the entry point refuses (the callers then take the chain)."""

    def __init__(self, motion_primitive_graph, graph_walk, time_constraints):
        from .motion_primitive_wrapper import HipStaticMotionPrimitive
        self.graph, self.graph_walk, self.time_constraints = motion_primitive_graph, graph_walk, time_constraints
        self.start_step, self.end_step = time_constraints.start_step, time_constraints.end_step
        self.steps = list(graph_walk.steps[self.start_step:self.end_step])
        self.constraint_list = [tuple(c) for c in time_constraints.constraint_list]
        self.start_keyframe = float(time_constraints.start_keyframe)
        self.frame_time = float(motion_primitive_graph.skeleton.frame_time)
        if not self.steps:
            raise NotImplementedError("an empty window")
        records, offset = [], 0
        for step in self.steps:
            node = motion_primitive_graph.nodes[step.node_key]
            if isinstance(getattr(node, "motion_primitive", None), HipStaticMotionPrimitive):
                raise NotImplementedError("step %r is a static primitive" % (step.node_key,))
            try:
                prim = _prim_of(node)
            except TypeError as e:
                raise NotImplementedError(str(e))
            ns, nt = int(step.n_spatial_components), int(step.n_time_components)
            if ns != prim.n_components or nt != prim.n_time_components or len(np.asarray(step.parameters)) < ns:
                raise NotImplementedError("step %r: %d spatial and %d time latents, its primitive has %d and %d" %
                                          (step.node_key, ns, nt, prim.n_components, prim.n_time_components))
            records.append((prim, offset, np.array(np.asarray(step.parameters, dtype=np.float64)[:ns])))
            offset += nt
        for step_index, keyframe_index, _ in self.constraint_list:
            k = max(int(step_index), 0)
            if k < len(records) and keyframe_index < -records[k][0].n_canonical_frames:
                raise IndexError("index %d is out of bounds for a time function of %d canonical frames" % (keyframe_index, records[k][0].n_canonical_frames))
        self.n_latents = offset
        self.table = _capi.WalkTimeTable(records, self.constraint_list, self.start_keyframe, self.frame_time)
        self.ctx = self.table.ctx
        self._buf, self._cap = None, 0
        self.n_launches = 0

    def matches(self, graph_walk, time_constraints):
        """Still the objective of this window: the same steps, constraints and start frame, the steps' spatial latents unchanged."""
        tc = time_constraints
        steps = graph_walk.steps[tc.start_step:tc.end_step]
        if self.table is None or tc.start_step != self.start_step or tc.end_step != self.end_step or len(steps) != len(self.steps) or \
                any(a is not b for a, b in zip(steps, self.steps)) or float(tc.start_keyframe) != self.start_keyframe or \
                [tuple(c) for c in tc.constraint_list] != self.constraint_list or float(self.graph.skeleton.frame_time) != self.frame_time:
            return False
        return all(np.array_equal(np.asarray(step.parameters, dtype=np.float64)[:len(sp)], sp) for step, (_, _, sp) in zip(steps, self.table.steps))

    def table_uploads(self):
        return self.table.table_uploads()

    def close(self):
        if getattr(self, "table", None) is not None:
            self.table.close()
        self.table = None
        if getattr(self, "_buf", None) is not None:
            self._buf.free()
        self._buf, self._cap = None, 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, S, error_scale, quality_scale, parts=False):
        """S (n, >= the window's time latents) -> objective (n,), or with parts (objective, error, average log-likelihood)."""
        if self.table is None:
            raise ValueError("the objective is closed")
        S = _capi._latents(S)
        if S.shape[1] < self.n_latents:
            raise ValueError("latent rows of %d columns, the window's steps need %d" % (S.shape[1], self.n_latents))
        n, ld = S.shape
        if n == 0:
            return (np.zeros(0), np.zeros(0), np.zeros(0)) if parts else np.zeros(0)
        lat_bytes = (S.nbytes + 255) & ~255
        need = lat_bytes + 8 * 3 * n
        if need > self._cap:
            if self._buf is not None:
                self._buf.free()
            self._buf, self._cap = self.ctx.malloc(2 * need), 2 * need
        base = self._buf.address
        d_out = base + lat_bytes
        if S.nbytes:
            self.ctx.upload_into(base, S)
        self.table.score_dev(base, S.dtype, n, ld, error_scale, quality_scale, d_out, d_out + 8 * n if parts else None, d_out + 16 * n if parts else None)
        self.n_launches += 1
        out = self.ctx.download(d_out, (3 * n if parts else n,), np.float64)
        return (out[:n], out[n:2 * n], out[2 * n:]) if parts else out


_WALK_TIME_OBJECTIVES = []      # [(graph, graph_walk, time_constraints, objective)], most recent last
_WALK_TIME_OBJECTIVES_SIZE = 4


def _walk_time_objective(motion_primitive_graph, graph_walk, time_constraints):
    """The HipWalkTimeObjective of these very objects (by identity: an optimiser hands the same `data` tuple over hundreds of
    times), built on first use and again when the window, the constraints or a step's spatial latents have changed."""
    for k, (g, w, t, obj) in enumerate(_WALK_TIME_OBJECTIVES):
        if g is motion_primitive_graph and w is graph_walk and t is time_constraints:
            _WALK_TIME_OBJECTIVES.pop(k)
            if obj.matches(graph_walk, time_constraints):
                _WALK_TIME_OBJECTIVES.append((g, w, t, obj))
                return obj
            obj.close()
            break
    obj = HipWalkTimeObjective(motion_primitive_graph, graph_walk, time_constraints)
    _WALK_TIME_OBJECTIVES.append((motion_primitive_graph, graph_walk, time_constraints, obj))
    while len(_WALK_TIME_OBJECTIVES) > _WALK_TIME_OBJECTIVES_SIZE:
        _WALK_TIME_OBJECTIVES.pop(0)[-1].close()
    return obj


def obj_time_error_sum_one_launch(s, data):
    """obj_time_error_sum with the window in one launch: the same bits.  The chain where the launch does not state the window
    (a static primitive, MG_ERR_UNSUPPORTED).  ValueError names the first candidate whose time function is not finite at an entry
    the objective reads (the minimisers take it as a failed evaluation, as the reference's does); IndexError for a keyframe
    below -n_canonical_frames, as indexing the time function would."""
    motion_primitive_graph, graph_walk, time_constraints, error_scale, quality_scale = data
    S, single = _batch(s)
    S = np.asarray(S, dtype=np.float64)
    try:
        objective = _walk_time_objective(motion_primitive_graph, graph_walk, time_constraints)
        out, err, _ = objective.evaluate(S, error_scale, quality_scale, parts=True)
    except NotImplementedError:
        return obj_time_error_sum(s, data)
    except _capi.MGError as e:
        if e.status != _capi.MG_ERR_UNSUPPORTED:
            raise
        return obj_time_error_sum(s, data)
    bad = np.flatnonzero(np.isnan(err))
    if len(bad):
        raise ValueError("candidate %d: the time function is not finite" % int(bad[0]))
    return float(out[0]) if single else out


# ---------------------------------------------------------------------------------------------------------------------
# Step goals (reference optimization/objective_functions.py:59-140).  The reference reads the LAST control point's root position
# straight from the projection (`sfpca.project(s)[idx:idx+3]`, idx = (n_coeffs - 1) * n_dims) of an MGRD model; here the same
# three numbers are rows of E' and mean' of the legacy primitive: pos = E_last . s + mean_last, y dropped.
# ---------------------------------------------------------------------------------------------------------------------
def _last_control_point_rows(motion_primitive):
    mp = motion_primitive.motion_primitive if hasattr(motion_primitive, "motion_primitive") else motion_primitive
    sp = mp.s_pca
    NB, D = int(sp["n_basis"]), int(sp["n_dim"])
    E = np.asarray(sp["eigen_vectors"], dtype=np.float64)            # (NB * D, L) as loaded (motion_primitive.py:156)
    mean = np.asarray(sp["mean_vector"], dtype=np.float64)
    scale = np.asarray(getattr(mp, "translation_maxima", (1.0, 1.0, 1.0)), dtype=np.float64)
    idx = (NB - 1) * D
    return E[idx:idx + 3] * scale[:, None], mean[idx:idx + 3] * scale


def _step_goal(s, data):
    motion_primitive, mp_constraints = data[0], data[1]
    target = np.asarray(_constraint_list(mp_constraints)[0].position, dtype=np.float64)
    S, single = _batch(s)
    S = np.asarray(S, dtype=np.float64)
    E3, m3 = _last_control_point_rows(motion_primitive)
    n_spatial = E3.shape[1]
    pos = S[:, :n_spatial] @ E3.T + m3
    pos[:, 1] = 0.0
    delta = target[None, :] - pos
    return S, single, E3, delta, n_spatial


def step_goal_error(s, data):
    """objective_functions.py:59-71 -> (n,)"""
    S, single, E3, delta, _ = _step_goal(s, data)
    err = np.einsum("ij,ij->i", delta, delta)
    return float(err[0]) if single else err


def step_goal_jac(s, data):
    """objective_functions.py:73-90 -> (n, len(s)): 2 * E_last^T (pos - target) on the spatial latents, zeros elsewhere"""
    S, single, E3, delta, n_spatial = _step_goal(s, data)
    jac = np.zeros_like(S)
    jac[:, :n_spatial] = 2.0 * (-delta) @ E3
    return jac[0] if single else jac


def step_goal_and_naturalness(s, data):
    """objective_functions.py:94-107: step_goal_error - log p(s)"""
    S, single, E3, delta, _ = _step_goal(s, data)
    err = np.einsum("ij,ij->i", delta, delta) - _prim_of(data[0]).gmm_log_prob(np.ascontiguousarray(S))
    return float(err[0]) if single else err


def step_goal_and_naturalness_jac(s, data):
    """objective_functions.py:122-140: step_goal_jac - log_likelihood_jac"""
    S, single = _batch(s)
    jac = np.atleast_2d(step_goal_jac(S, data)) - np.atleast_2d(log_likelihood_jac(S, data[0]))
    return jac[0] if single else jac
