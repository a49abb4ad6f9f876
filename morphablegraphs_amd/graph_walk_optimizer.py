"""GraphWalkOptimizer (reference morphablegraphs/motion_generator/graph_walk_optimizer.py:39-189) over a HipGraphWalk.

The global spatial optimisation evaluates its objective over the concatenated latents of all steps with the whole walk in ONE
launch (objective_functions.obj_global_residual_vector_and_naturalness_one_launch, csrc/mg_walk_score.hip), writes the result
back with update_spatial_parameters and rebuilds the frames on the device (HipGraphWalk.convert_graph_walk_to_quaternion_frames:
mg_walk_frames).  The time optimisation evaluates its objective over a window's time latents in one launch as well
(objective_functions.obj_time_error_sum_one_launch, csrc/mg_walk_time.hip).  The method table, the algorithm_config keys and the constants are the reference's; constraint construction
stays in the reference.

The module imports without a device and works on a HipGraphWalk(host=True) as far as no objective is evaluated.
"""
import numpy as np

from . import objective_functions as of

GRAPH_WALK_OPTIMIZATION_ALL = "all"                        # graph_walk_optimizer.py:32-35
GRAPH_WALK_OPTIMIZATION_TWO_HANDS = "two_hands"
GRAPH_WALK_OPTIMIZATION_END_POINT = "trajectory_end"
SPATIAL_CONSTRAINT_TYPE_TRAJECTORY = "trajectory"          # constraints/spatial_constraints/__init__.py:23-31
SPATIAL_CONSTRAINT_TYPE_KEYFRAME_POSITION = "keyframe_position"
SPATIAL_CONSTRAINT_TYPE_KEYFRAME_DIR_2D = "keyframe_2d_direction"
SPATIAL_CONSTRAINT_TYPE_KEYFRAME_POSE = "keyframe_pose"
SPATIAL_CONSTRAINT_TYPE_TRAJECTORY_SET = "trajectory_set"
SPATIAL_CONSTRAINT_TYPE_CA_CONSTRAINT = "ca_constraint"
CONSTRAINT_FILTER_LIST = [SPATIAL_CONSTRAINT_TYPE_KEYFRAME_POSE, SPATIAL_CONSTRAINT_TYPE_TRAJECTORY, SPATIAL_CONSTRAINT_TYPE_TRAJECTORY_SET,
                          SPATIAL_CONSTRAINT_TYPE_CA_CONSTRAINT]


class TimeConstraintsBuilder(object):
    """constraints/time_constraints_builder.py:27-63: the keyframe-position constraints with a desired time of the steps
    start_step .. end_step (inclusive; clipped to the walk) as (step counted from start_step, canonical keyframe, desired time);
    build() makes HipTimeConstraints of them, or None without any."""

    def __init__(self, graph_walk, start_step, end_step):
        self.start_step = start_step
        self.end_step = min(end_step + 1, len(graph_walk.steps))
        self.time_constraint_list = []
        self.n_time_constraints = 0
        for count, step_index in enumerate(range(self.start_step, self.end_step)):
            mp_constraints = graph_walk.steps[step_index].motion_primitive_constraints
            if mp_constraints is None:
                continue
            for constraint in mp_constraints.constraints:
                if getattr(constraint, "constraint_type", None) == SPATIAL_CONSTRAINT_TYPE_KEYFRAME_POSITION and getattr(constraint, "desired_time", None) is not None:
                    self.time_constraint_list.append((count, constraint.canonical_keyframe, constraint.desired_time))
                    self.n_time_constraints += 1

    def build(self, motion_primitive_graph, graph_walk):
        if self.n_time_constraints > 0:
            return of.HipTimeConstraints(motion_primitive_graph, graph_walk, self.start_step, self.end_step, self.time_constraint_list)
        return None


class _CollisionAvoidanceConstraints(object):
    """What the reference's empty MotionPrimitiveConstraints() amounts to for the objective: a list, global coordinates."""

    def __init__(self, skeleton=None, hip_skeleton=None):
        self.constraints, self.is_local, self.start_pose = [], False, None
        self.skeleton, self.hip_skeleton = skeleton, hip_skeleton
        self.min_error, self.evaluations = None, 0


class HipGraphWalkOptimizer(object):
    """minimizers: None, or a dict with any of "time", "global", "collision_avoidance" -- objects with
    set_objective_function_parameters(data) and run(initial_guess) (and, for "global", `_objective_function`) that take the
    place of the ones built from algorithm_config (tests inject stubs)."""

    def __init__(self, motion_primitive_graph, algorithm_config, minimizers=None):
        self.motion_primitive_graph = motion_primitive_graph
        minimizers = dict(minimizers or {})
        self.time_error_minimizer = minimizers.get("time")
        self.global_error_minimizer = minimizers.get("global")
        self.collision_avoidance_error_minimizer = minimizers.get("collision_avoidance")
        if None in (self.time_error_minimizer, self.global_error_minimizer, self.collision_avoidance_error_minimizer):
            from .motion_primitive_generator import HipLeastSquares, HipNumericalMinimizer, HipOptimizerBuilder
            if self.time_error_minimizer is None:      # build_time_error_minimizer's settings on the one-launch objective
                self.time_error_minimizer = HipNumericalMinimizer(algorithm_config["global_time_optimization_settings"],
                                                                  of.obj_time_error_sum_one_launch)
            if self.global_error_minimizer is None:    # build_global_error_minimizer_residual's settings on the one-launch objective
                self.global_error_minimizer = HipLeastSquares(algorithm_config["global_spatial_optimization_settings"],
                                                              of.obj_global_residual_vector_and_naturalness_one_launch)
            if self.collision_avoidance_error_minimizer is None:
                self.collision_avoidance_error_minimizer = HipOptimizerBuilder(algorithm_config).build_spatial_error_minimizer()
        self.set_algorithm_config(algorithm_config)

    def set_algorithm_config(self, algorithm_config):
        self._algorithm_config = algorithm_config
        self.spatial_mode = algorithm_config["global_spatial_optimization_mode"]
        self.optimize_collision_avoidance_constraints_extra = algorithm_config["optimize_collision_avoidance_constraints_extra"]
        self._global_spatial_optimization_steps = algorithm_config["global_spatial_optimization_settings"]["max_steps"]
        self._position_weight_factor = algorithm_config["global_spatial_optimization_settings"]["position_weight"]
        self._orientation_weight_factor = algorithm_config["global_spatial_optimization_settings"]["orientation_weight"]
        self.optimized_actions_for_time_constraints = algorithm_config["global_time_optimization_settings"]["optimized_actions"]

    def _is_optimization_required(self, action_constraints):
        return self.spatial_mode == GRAPH_WALK_OPTIMIZATION_ALL and action_constraints.contains_user_constraints or \
               self.spatial_mode == GRAPH_WALK_OPTIMIZATION_TWO_HANDS and action_constraints.contains_two_hands_constraints

    def optimize(self, graph_walk, action_state, action_constraints):
        if self._is_optimization_required(action_constraints):
            start_step = max(action_state.start_step - self._global_spatial_optimization_steps, 0)
            graph_walk = self.optimize_spatial_parameters_over_graph_walk(graph_walk, start_step)
        elif self.spatial_mode == GRAPH_WALK_OPTIMIZATION_END_POINT and action_constraints.root_trajectory is not None:
            start_step = max(len(graph_walk.steps) - self._global_spatial_optimization_steps, 0)
            graph_walk = self.optimize_spatial_parameters_over_graph_walk(graph_walk, start_step)
        ca = getattr(action_constraints, "collision_avoidance_constraints", None)
        if self.optimize_collision_avoidance_constraints_extra and ca is not None and len(ca) > 0:
            graph_walk = self.optimize_for_collision_avoidance_constraints(graph_walk, action_constraints, action_state.start_step)
        return graph_walk

    def optimize_spatial_parameters_over_graph_walk(self, graph_walk, start_step=0):
        initial_guess = graph_walk.get_global_spatial_parameter_vector(start_step)
        constraint_count = self._filter_constraints(graph_walk, start_step)
        self._adapt_constraint_weights(graph_walk, start_step)
        if constraint_count > 0:
            if start_step == 0:
                prev_frames = None
            else:      # the last rows before the first optimised step, from the walk's store
                prev_frames = graph_walk.get_quat_frames()[:graph_walk.steps[start_step].start_frame]
            settings = self._algorithm_config["global_spatial_optimization_settings"]
            steps = graph_walk.steps[start_step:]
            data = (self.motion_primitive_graph, steps, settings["error_scale_factor"], settings["quality_scale_factor"], prev_frames, 1.0)
            init_error_sum = max(abs(np.sum(self.global_error_minimizer._objective_function(initial_guess, data))), 1.0)
            data = (self.motion_primitive_graph, steps, settings["error_scale_factor"], settings["quality_scale_factor"], prev_frames, init_error_sum)
            self.global_error_minimizer.set_objective_function_parameters(data)
            optimal_parameters = self.global_error_minimizer.run(initial_guess)
            graph_walk.update_spatial_parameters(optimal_parameters, start_step)
            graph_walk.convert_graph_walk_to_quaternion_frames(start_step, use_time_parameters=False)
        return graph_walk

    def _filter_constraints(self, graph_walk, start_step):
        constraint_count = 0
        for step in graph_walk.steps[start_step:]:
            mp_constraints = step.motion_primitive_constraints
            mp_constraints.constraints = [c for c in mp_constraints.constraints if c.constraint_type not in CONSTRAINT_FILTER_LIST]
            constraint_count += len(mp_constraints.constraints)
        return constraint_count

    def _adapt_constraint_weights(self, graph_walk, start_step):
        if self.spatial_mode == GRAPH_WALK_OPTIMIZATION_ALL or self.spatial_mode == GRAPH_WALK_OPTIMIZATION_TWO_HANDS:
            for step in graph_walk.steps[start_step:]:
                for constraint in step.motion_primitive_constraints.constraints:
                    if "generated" not in list(constraint.semantic_annotation.keys()):
                        constraint.weight_factor = self._position_weight_factor
        else:      # GRAPH_WALK_OPTIMIZATION_END_POINT
            for constraint in graph_walk.steps[-1].motion_primitive_constraints.constraints:
                if constraint.constraint_type == SPATIAL_CONSTRAINT_TYPE_KEYFRAME_POSITION:
                    constraint.weight_factor = self._position_weight_factor
                elif constraint.constraint_type == SPATIAL_CONSTRAINT_TYPE_KEYFRAME_DIR_2D:
                    constraint.weight_factor = self._orientation_weight_factor

    def optimize_time_parameters_over_graph_walk(self, graph_walk):
        settings = self._algorithm_config["global_time_optimization_settings"]
        for idx, ea in enumerate(graph_walk.elementary_action_list):
            prev_action_idx = max(idx - (self.optimized_actions_for_time_constraints - 1), 0)
            start_step = graph_walk.elementary_action_list[prev_action_idx].start_step
            end_step = ea.end_step
            time_constraints = TimeConstraintsBuilder(graph_walk, start_step, end_step).build(self.motion_primitive_graph, graph_walk)
            if time_constraints is not None:
                data = (self.motion_primitive_graph, graph_walk, time_constraints, settings["error_scale_factor"], settings["quality_scale_factor"])
                self.time_error_minimizer.set_objective_function_parameters(data)
                optimal_parameters = self.time_error_minimizer.run(time_constraints.get_initial_guess(graph_walk))
                graph_walk.update_time_parameters(optimal_parameters, start_step, end_step)
        return graph_walk

    def optimize_for_collision_avoidance_constraints(self, graph_walk, action_constraints, start_step=0):
        """graph_walk_optimizer.py:156-189.  The reference grows a copy of the motion vector step by step; here the walk's own store
        is that vector: the rows before a step are what it is aligned to and measured against, and the step's new parameters reach
        the frames through convert_graph_walk_to_quaternion_frames(step_index).  (The reference hands the minimiser a five-element
        tuple where obj_spatial_error_residual_vector unpacks six; init_error_sum = 1 is added, as in the global objectives.)"""
        settings = self._algorithm_config["local_optimization_settings"]
        ref_sk = getattr(self.motion_primitive_graph, "skeleton", None)
        hip_sk = getattr(self.motion_primitive_graph, "hip_skeleton", None)
        for step_index in range(start_step, len(graph_walk.steps)):
            step = graph_walk.steps[step_index]
            node = self.motion_primitive_graph.nodes[step.node_key]
            frames = graph_walk.get_quat_frames()
            prev_frames = None if frames is None or step.start_frame == 0 else frames[:step.start_frame]
            mp_constraints = _CollisionAvoidanceConstraints(ref_sk, hip_sk)
            for trajectory in action_constraints.collision_avoidance_constraints:
                if prev_frames is not None:
                    trajectory.set_min_arc_length_from_previous_frames(prev_frames)
                else:
                    trajectory.min_arc_length = 0.0
                trajectory.set_number_of_canonical_frames(node.n_canonical_frames)
                mp_constraints.constraints.append(trajectory)
            if mp_constraints.constraints:
                data = (node, mp_constraints, prev_frames, settings["error_scale_factor"], settings["quality_scale_factor"], 1.0)
                self.collision_avoidance_error_minimizer.set_objective_function_parameters(data)
                step.parameters = self.collision_avoidance_error_minimizer.run(step.parameters)
            graph_walk.convert_graph_walk_to_quaternion_frames(step_index)
        return graph_walk
