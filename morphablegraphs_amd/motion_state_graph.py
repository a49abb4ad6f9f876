"""A minimal container for BASELINE.json config 3: the ~16 primitives of a MotionStateGraph resident on
one GPU, and the batched form of GraphWalkPlanner's option evaluation
(reference morphablegraphs/motion_generator/graph_walk_planner.py:184-226): for every outgoing option draw
n candidates, score them against the path-following constraints, keep the first minimum per option, pick
the option with the smallest error (np.argmin over options, graph_walk_planner.py:191-192).
Graph loading / transitions / control flow stay in the reference; only the scoring is replaced."""
import ctypes as C
import random
from collections import namedtuple

import numpy as np

from . import candidate_scoring as _cs

from . import _capi
from .candidate_scoring import constraints_to_device_form, evaluate_samples_using_constraints
from .cluster_tree import HipFeatureClusterTree, TreeSearchSet, search_on_device
from .kd_cluster_tree import HipClusterTree

_SEARCH_TREES = (HipFeatureClusterTree, HipClusterTree)   # the trees a search descends (the others hold samples only)
from .frame_constraints import is_frame_constraint
from .motion_primitive import HipMotionPrimitive, get_context
from .motion_primitive_wrapper import HipMotionPrimitiveModelWrapper

NODE_TYPE_START = "start"
NODE_TYPE_STANDARD = "standard"
NODE_TYPE_END = "end"


def random_edge(outgoing_edges, accept, rng=random):
    """One of the edges of `outgoing_edges` (in its order) that `accept(edge_key)` keeps, drawn the way the reference draws it
    (motion_state_graph_node.py:152-160, 170-181: rng.randrange(0, len(edges), 1)); None without such an edge, and then nothing
    is drawn."""
    edges = [edge_key for edge_key in outgoing_edges.keys() if accept(edge_key)]
    if len(edges) > 0:
        return edges[rng.randrange(0, len(edges), 1)]
    return None


def arc_length_xz(root_positions):
    """Length of the root path on the ground plane (x, z) -- what the reference gets from anim_utils'
    extract_root_positions_from_frames + get_arc_length_from_points (motion_state_graph_node.py:222-224;
    PARITY UNPINNED: anim_utils is not under /root/reference)."""
    p = np.asarray(root_positions, dtype=np.float64)[..., [0, 2]]
    return np.sqrt(((p[..., 1:, :] - p[..., :-1, :]) ** 2).sum(axis=-1)).sum(axis=-1)


def step_lengths_host(root_positions):
    """(arc_length, distance) of root paths (..., F, 3) in NumPy: the statement of mg_step_lengths' two reductions
    (csrc/mg_step_length.hip).  arc_length = d_1 + .. + d_{F-1} added in frame order (np.cumsum: np.sum adds pairwise, which is
    not the kernel's order) with d_f = sqrt(dx^2 + dz^2) on the ground plane; distance = sqrt((dx^2 + dy^2) + dz^2) between the
    first and the last position (np.linalg.norm of motion_state_graph_node.py:225-229)."""
    p = np.asarray(root_positions, dtype=np.float64)
    d = p[..., 1:, :] - p[..., :-1, :]
    seg = np.sqrt(d[..., 0] * d[..., 0] + d[..., 2] * d[..., 2])
    arc = np.cumsum(seg, axis=-1)[..., -1] if seg.shape[-1] else np.zeros(seg.shape[:-1])
    e = p[..., -1, :] - p[..., 0, :]
    return arc, np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])


class HipMotionStateGraphNode(HipMotionPrimitiveModelWrapper):
    """The hot-path call sites of MotionStateGraphNode (reference motion_model/motion_state_graph_node.py:45-275)
    on top of the HIP-backed wrapper: step-length statistics, transition-model dispatch, best-sample search.
    Edges / groups / cluster trees are plain host data exactly as in the reference."""

    def __init__(self, motion_state_group=None, context=None, device=0):
        super(HipMotionStateGraphNode, self).__init__(context=context, device=device)
        self.motion_state_group = motion_state_group
        self.motion_state_graph = None     # the graph that holds the node (HipMotionStateGraph._build_nodes)
        self.outgoing_edges = dict()
        self.node_type = NODE_TYPE_STANDARD
        self.n_standard_transitions = 0
        self.parameter_bb = None
        self.cartesian_bb = None
        self.velocity_data = None
        self.average_step_length = 0
        self.action_name = None
        self.name = None
        self.node_key = None
        self.cluster_tree = None

    def init_from_dict(self, action_name, desc):
        self.name = desc["name"]
        self.action_name = action_name
        self.node_key = (action_name, self.name)       # motion_state_graph_node.py: the key the graph holds the node under
        self._initialize_from_json(None, desc["mm"])
        if "stats" in desc:
            self.parameter_bb = desc["stats"]["pose_bb"]
            self.cartesian_bb = desc["stats"]["cartesian_bb"]
            self.velocity_data = desc["stats"]["pose_velocity"]

    # ---- step length (motion_state_graph_node.py:183-230) ------------------------------------------
    def update_motion_stats(self, n_samples=5, method="median"):
        self.n_standard_transitions = len([e for e in self.outgoing_edges
                                           if getattr(self.outgoing_edges[e], "transition_type", None) == NODE_TYPE_STANDARD])
        sample_lengths = [self._get_random_sample_step_length() for _ in range(n_samples)]
        if method == "average":
            self.average_step_length = sum(sample_lengths) / n_samples
        else:
            self.average_step_length = np.median(sample_lengths)

    def _get_random_sample_step_length(self, method="arc_length"):
        current_parameters = np.ravel(self.sample_low_dimensional_vector())
        return self.get_step_length_for_sample(current_parameters, method)

    def get_step_length_for_sample(self, parameters, method="arc_length"):
        quat_frames = self.back_project(parameters, use_time_parameters=False).get_motion_vector()
        if method == "arc_length":
            return float(arc_length_xz(quat_frames[:, :3]))
        elif method == "distance":
            return float(np.linalg.norm(quat_frames[-1][:3] - quat_frames[0][:3]))
        raise NotImplementedError

    def get_step_lengths_for_samples(self, samples, method="arc_length"):
        """Batched form: one frames launch for all rows."""
        frames = self.motion_primitive.back_project_frames_batch(np.asarray(samples))
        if method == "arc_length":
            return arc_length_xz(frames[:, :, :3])
        elif method == "distance":
            return np.linalg.norm(frames[:, -1, :3].astype(np.float64) - frames[:, 0, :3], axis=1)
        raise NotImplementedError

    def step_lengths_on_device(self, samples, method="arc_length"):
        """get_step_lengths_for_samples without frames in memory (mg_step_lengths): (n,) float64, float64 arithmetic on the
        root's three channels alone; 8 bytes per candidate come back.  samples (n, >= n_spatial_components)."""
        return self.motion_primitive._prim.step_lengths(samples, method)

    # ---- transitions (motion_state_graph_node.py:232-272) -----------------------------------------
    def has_transition_model(self, to_node_key):
        return to_node_key in self.outgoing_edges and getattr(self.outgoing_edges[to_node_key], "transition_model", None) is not None

    def generate_random_transition(self, transition_type=NODE_TYPE_STANDARD):
        """The key of a random transition of that type, or None (motion_state_graph_node.py:144-160); draws from the global
        `random`, as there."""
        return random_edge(self.outgoing_edges, lambda key: self.outgoing_edges[key].transition_type == transition_type)

    def generate_random_action_transition(self, elementary_action_name, cycle=False):
        """The key of a random transition to a start state (with cycle: or a cycle state) of that action, or None
        (motion_state_graph_node.py:162-181; the reference's `+=` also lengthens the action's own start_states, which is not
        repeated here)."""
        info = self.motion_state_graph.node_groups[elementary_action_name]["info"]
        states = list(info.get("start_states", [])) + (list(info.get("cycle_states", [])) if cycle else [])
        return random_edge(self.outgoing_edges, lambda key: key[0] == elementary_action_name and key[1] in states)

    def predict_parameters(self, to_node_key, current_parameters):
        gmm = self.outgoing_edges[to_node_key].transition_model.predict(current_parameters)
        s = gmm.sample()           # ONE draw, as motion_state_graph_node.py:252-253: every call consumes NumPy's global stream
        return np.ravel(s[0] if isinstance(s, tuple) else s)

    def predict_gmm(self, to_node_key, current_parameters):
        edge = self.outgoing_edges.get(to_node_key)
        if edge is not None and getattr(edge, "transition_model", None) is not None:
            return edge.transition_model.predict(current_parameters)
        return self.get_gaussian_mixture_model()

    # ---- best-sample search (motion_state_graph_node.py:119-142) -------------------------------------
    def search_best_sample(self, obj, data, n_candidates=2):
        if self.cluster_tree is not None:
            return self.cluster_tree.find_best_example_excluding_search_candidates(obj, data, n_candidates)
        return np.inf, None

    def _tree_search_set(self, constraints, prev_frames=None, skeleton=None, per_frame=False):
        """What a one-launch tree search scores against (cluster_tree.TreeSearchSet: the device keyframe set, the root
        trajectory constraints as pinned device trajectories, the alignment and, with per_frame, the per-frame constraint list), or
        None when the launch does not cover the constraints: more than MG_TREE_MAX_TRAJECTORIES trajectories, trajectories
        aligned to another joint than the root, and per-frame constraints -- all of them by default (per_frame=False: the
        routing there always was); with per_frame=True only a list longer than MG_FRAME_LIST_MAX (or over more than
        MG_TRACK_MAX_REQUESTS requests) and a plan no rung of the kernel's LDS ladder takes.  The caller release()s the set after
        its call."""
        from . import cluster_tree as _ct, frame_constraints as _fc
        from .candidate_scoring import alignment_from_prev_frames, cached_constraint_set, cached_trajectory, split_trajectories
        from .frame_constraints import is_frame_constraint
        clist = constraints.constraints if hasattr(constraints, "constraints") else constraints
        skeleton = skeleton if skeleton is not None else getattr(constraints, "hip_skeleton", None)
        form = constraints_to_device_form(clist)
        frames = [c for c in form if is_frame_constraint(c)]
        if frames and (not per_frame or len(frames) > _capi.MG_FRAME_LIST_MAX):
            return None
        keyframes, trajectories = split_trajectories([c for c in form if not is_frame_constraint(c)])
        if len(trajectories) > _capi.MG_TREE_MAX_TRAJECTORIES:
            return None
        alignment = alignment_from_prev_frames(prev_frames, constraints, skeleton)
        if trajectories and alignment is not None and alignment.get("joint", 0) not in (0, _capi.MG_ALIGN_START_POSE):
            return None
        prim = self.motion_primitive._prim
        cset = cached_constraint_set(prim, keyframes, skeleton, alignment)
        sset = TreeSearchSet(cset, alignment=alignment)
        try:
            for c in trajectories:
                sset.trajectories.append((cached_trajectory(prim, c, pin=True), c.get("min_u", 0.0), c.get("weight", 1.0)))
            if frames:
                sset.frame_constraints = _fc.tree_frame_list(prim, frames, skeleton, alignment)
                if sset.frame_constraints is None or _ct.frames_search_plan([(self._search_tree(), prim, sset)], 1)["refused"]:
                    sset.release()
                    return None
        except Exception:
            sset.release()
            raise
        return sset

    def _search_tree(self):
        if not isinstance(self.cluster_tree, _SEARCH_TREES):
            raise NotImplementedError("node %r has no cluster tree to descend (only stored samples)" % (self.name,))
        return self.cluster_tree

    def search_best_sample_on_device(self, constraints, n_candidates, prev_frames=None, skeleton=None, search_set=None, per_frame=False):
        """search_best_sample with the reference's objective (the constraints' summed weighted errors, aligned to prev_frames
        outside local mode) as ONE launch (mg_cluster_tree_search[_trajectories | _frames]): (error, sample).  Adds the objectives
        scored to constraints.evaluations.  search_set: what _tree_search_set returned for these arguments, where the caller has
        asked already; it is released here either way.  per_frame: per-frame constraint lists take the launch as well
        (_tree_search_set's flag)."""
        sset = search_set
        try:
            tree = self._search_tree()
            if sset is None:
                sset = self._tree_search_set(constraints, prev_frames, skeleton, per_frame=per_frame)
            if sset is None:
                raise NotImplementedError("the one-launch tree search scores keyframe constraints, up to %d root trajectories and, with "
                                          "per_frame, up to %d per-frame constraints" % (_capi.MG_TREE_MAX_TRAJECTORIES, _capi.MG_FRAME_LIST_MAX))
            rec = search_on_device([(tree, self.motion_primitive._prim, sset)], n_candidates)[0]
        finally:
            if sset is not None:
                sset.release()
        if hasattr(constraints, "evaluations"):
            constraints.evaluations += int(rec["evaluations"])
        return tree.result_of_record(rec)

    def search_best_sample_batched(self, constraints, n_candidates, prev_frames=None, skeleton=None):
        """The same descent driven from the host: every level's children scored by one call of the general scoring path
        (keyframe, trajectory and per-frame constraints alike).  (error, sample); adds to constraints.evaluations."""
        from .candidate_scoring import alignment_from_prev_frames, errors_of_samples
        tree = self._search_tree()
        clist = constraints.constraints if hasattr(constraints, "constraints") else constraints
        skeleton = skeleton if skeleton is not None else getattr(constraints, "hip_skeleton", None)
        form = constraints_to_device_form(clist)
        alignment = alignment_from_prev_frames(prev_frames, constraints, skeleton)
        L = self.get_n_spatial_components()
        table = tree.points if isinstance(tree, HipClusterTree) else tree.means   # what descend's ids index
        value, row, _, n_eval = tree.descend(lambda ids: errors_of_samples(self.motion_primitive._prim, form, skeleton, alignment, table[ids, :L]),
                                             n_candidates)
        if hasattr(constraints, "evaluations"):
            constraints.evaluations += n_eval
        return value, row

    def search_best_sample_gpu(self, constraints, n_samples):
        """Brute-force replacement of the cluster-tree search at GPU batch sizes: draw n_samples latents, score
        them in one launch, return (error, parameters) like search_best_sample."""
        samples = self.sample_low_dimensional_vectors(n_samples)
        best, err = evaluate_samples_using_constraints(samples, self, constraints, None)
        return err, best


class HipMotionStateTransition(object):
    """MotionStateTransition (reference motion_model/motion_state_transition.py): plain host data."""

    def __init__(self, from_node_key, to_node_key, transition_type, transition_model=None):
        self.from_node_key, self.to_node_key = from_node_key, to_node_key
        self.transition_type, self.transition_model = transition_type, transition_model


class _StoredSamples(object):
    """What the brute-force search needs of a FeatureClusterTree: its stored samples."""

    def __init__(self, data):
        self.data = np.asarray(data, dtype=np.float64)


NODE_TYPE_SINGLE = "single_primitive"
NODE_TYPE_CYCLE_END = "cycle_end"
NODE_TYPE_IDLE = "idle"


class HipMotionStateGraph(object):
    """All primitives of a motion state graph resident on one GPU (BASELINE.json config 3), built the way
    MotionStateGraphLoader._build_from_zip_file does (reference motion_model/motion_state_graph_loader.py:184-242):
    node groups from the "subgraphs" of the zip, node types from each action's meta information
    (motion_state_group.py:46-62), transitions from the "transitions" table (loader :244-263, types :265-289),
    the start node, cached or recomputed step statistics.  Skeleton, hand poses and PFNN data are not read."""

    def __init__(self, context=None, device=0):
        self.ctx = context or get_context(device)
        self.nodes = {}
        self.node_groups = {}
        self.start_node = None
        self.action_definitions = {}

    def load_from_zip(self, path, recalculate_stats=False, pickle_objects=False):
        """pickle_objects: read the pickled cluster trees of formatVersion < 4 or usePickle zips (model_io.read_graph_zip)."""
        from .model_io import read_graph_zip
        return self.build_from_graph_data(read_graph_zip(path, pickle_objects), recalculate_stats)

    def build_from_graph_data(self, graph_data, recalculate_stats=False):
        # every primitive of the graph lives in one device arena (a few 64 MiB blocks instead of ~20 allocations each)
        self.ctx.arena_begin()
        try:
            self._build_nodes(graph_data)
        finally:
            self.ctx.arena_end()
        self._set_transitions_from_dict(graph_data.get("transitions", {}))
        for group in self.node_groups.values():
            stats = group["info"].get("stats", {})
            for mp_name in group["nodes"]:
                node = self.nodes[(group["name"], mp_name)]
                if recalculate_stats or mp_name not in stats:
                    node.update_motion_stats()
                else:   # motion_state_group.py:88-99: cached values from meta_information.json
                    node.average_step_length = stats[mp_name]["average_step_length"]
                    node.n_standard_transitions = stats[mp_name]["n_standard_transitions"]
        if "actionDefinitions" in graph_data:
            self.action_definitions = graph_data["actionDefinitions"]
        if "startNode" in graph_data:
            start_node = list(graph_data["startNode"])
            if start_node[1].startswith("walk"):
                start_node[1] = start_node[1][5:]
            self.start_node = tuple(start_node)
        return self

    def update_all_motion_stats(self, n_samples=5, method="median", node_keys=None):
        """update_motion_stats of the given nodes (default: all, in self.nodes order) with ONE mg_step_lengths call for all of
        them (MotionStateGroup._update_motion_state_stats, motion_state_group.py:74-105, pays a back-projection per sample).
        The latents are drawn node after node with node.sample_low_dimensional_vector(), n_samples each: the draws, in the
        order, of calling update_motion_stats on each node.  Static primitives keep the per-node path."""
        keys = list(self.nodes) if node_keys is None else list(node_keys)
        items, scored = [], []
        for key in keys:
            node = self.nodes[key]
            if not isinstance(node.motion_primitive, HipMotionPrimitive):
                node.update_motion_stats(n_samples, method)
                continue
            node.n_standard_transitions = len([e for e in node.outgoing_edges
                                               if getattr(node.outgoing_edges[e], "transition_type", None) == NODE_TYPE_STANDARD])
            rows = [np.ravel(node.sample_low_dimensional_vector()) for _ in range(n_samples)]
            S = np.asarray(rows, dtype=np.float64).reshape(n_samples, -1)
            items.append((node.motion_primitive._prim, S))
            scored.append(node)
        for node, lengths in zip(scored, _capi.step_lengths(items, "arc_length")):
            if method == "average":
                node.average_step_length = sum(lengths.tolist()) / n_samples
            else:
                node.average_step_length = np.median(lengths)

    def _build_nodes(self, graph_data):
        for action_name, action_data in graph_data["subgraphs"].items():
            group = {"name": action_data["name"], "info": action_data.get("info", {}), "nodes": []}
            for mp_name, desc in action_data["nodes"].items():
                if "spatial_coeffs" in desc["mm"]:
                    continue   # static primitives carry no statistical model (motion_primitive_wrapper.py:61-66)
                node = HipMotionStateGraphNode(group, context=self.ctx)
                node.motion_state_graph = self
                node.init_from_dict(action_data["name"], desc)
                if "space_partition_pickle" in desc:   # motion_state_graph_node.py:96-97
                    node.cluster_tree = desc["space_partition_pickle"]
                    node.cluster_tree.validate(node.get_n_spatial_components())
                if "space_partition_json" in desc:
                    tree_data = desc["space_partition_json"]
                    if isinstance(tree_data.get("root"), dict) and len(tree_data["root"]) > 0:
                        node.cluster_tree = HipFeatureClusterTree.from_json(tree_data, node.get_n_spatial_components())
                    else:   # a stub without nodes: the stored samples for the exhaustive search
                        node.cluster_tree = _StoredSamples(tree_data["data"])
                self.nodes[(action_data["name"], mp_name)] = node
                group["nodes"].append(mp_name)
            self._set_node_types(group)
            self.node_groups[action_data["name"]] = group
            idle = group["info"].get("idle_states", [])
            if action_name == "walk" and len(idle) > 0:
                self.start_node = (action_name, idle[0])

    def _set_node_types(self, group):
        keys = [(group["name"], n) for n in group["nodes"]]
        if len(keys) == 1:
            self.nodes[keys[0]].node_type = NODE_TYPE_SINGLE
            return
        info = group["info"]
        for field, node_type in (("start_states", NODE_TYPE_START), ("end_states", NODE_TYPE_END),
                                 ("cycle_states", NODE_TYPE_CYCLE_END), ("idle_states", NODE_TYPE_IDLE)):
            for k in info.get(field, []):
                if (group["name"], k) in self.nodes:
                    self.nodes[(group["name"], k)].node_type = node_type

    def _get_transition_type(self, from_node_key, to_node_key):
        t_type = "action_transition"
        if to_node_key[0] == from_node_key[0]:
            to_type = self.nodes[to_node_key].node_type
            if self.nodes[from_node_key].node_type == NODE_TYPE_IDLE:
                if to_type in (NODE_TYPE_START, NODE_TYPE_IDLE, NODE_TYPE_END):
                    t_type = to_type
            else:
                t_type = to_type if to_type in (NODE_TYPE_STANDARD, NODE_TYPE_START, NODE_TYPE_CYCLE_END, NODE_TYPE_IDLE) else NODE_TYPE_END
        return t_type

    def _set_transitions_from_dict(self, transition_dict):
        if len(transition_dict) == 0:
            return
        split_key = ":" if ":" in list(transition_dict.keys())[0] else "_"
        for node_key in transition_dict:
            from_node_key = tuple(node_key.split(split_key)[:2])
            if from_node_key not in self.nodes:
                continue
            for to_key in transition_dict[node_key]:
                to_node_key = tuple(to_key.split(split_key)[:2])
                if to_node_key in self.nodes:
                    self.nodes[from_node_key].outgoing_edges[to_node_key] = HipMotionStateTransition(
                        from_node_key, to_node_key, self._get_transition_type(from_node_key, to_node_key), None)

    def evaluate_options(self, options, constraints_per_option, n_samples, rng_seed=None, use_cluster_trees=False, prev_frames=None,
                         skeleton=None, per_frame=False):
        """GraphWalkPlanner._evaluate_options over this graph's nodes (reference graph_walk_planner.py:184-226): options are node
        keys.  With use_cluster_trees every option whose node has a cluster tree is searched with n_candidates = 1, as
        _evaluate_option does (:205-207), ALL of them in one launch; the other options draw n_samples candidates, score them and
        keep the first minimum.  per_frame: options whose lists carry per-frame constraints take that launch too
        (_tree_search_set's flag; off: they take the host-driven descent, as before).  Returns (best_option, {option: (best_sample, min_error)})."""
        results, searches, general = {}, [], []
        try:
            for key in options:
                node = self.nodes[key]
                cons = constraints_per_option[key]
                if use_cluster_trees and isinstance(node.cluster_tree, _SEARCH_TREES):
                    sset = node._tree_search_set(cons, prev_frames, skeleton, per_frame=per_frame) if per_frame else \
                        node._tree_search_set(cons, prev_frames, skeleton)
                    if sset is not None:
                        searches.append((key, (node.cluster_tree, node.motion_primitive._prim, sset)))
                        continue
                    results[key] = node.search_best_sample_batched(cons, 1, prev_frames, skeleton)[::-1]
                    continue
                general.append(key)
            for kind in _SEARCH_TREES:   # one launch per tree kind, trajectory constraints included
                group = [s for s in searches if isinstance(s[1][0], kind)]
                if not group:
                    continue
                records = search_on_device([s for _, s in group], 1)
                for (key, (tree, _, _)), rec in zip(group, records):
                    cons = constraints_per_option[key]
                    if hasattr(cons, "evaluations"):
                        cons.evaluations += int(rec["evaluations"])
                    err, row = tree.result_of_record(rec)
                    results[key] = (row, err)
        finally:
            for _, (_, _, sset) in searches:
                sset.release()
        for key in general:
            node = self.nodes[key]
            if rng_seed is not None:
                np.random.seed(rng_seed)
            samples = node.sample_low_dimensional_vectors(n_samples)
            results[key] = evaluate_samples_using_constraints(samples, node, constraints_per_option[key], prev_frames, skeleton)
        errors = [results[k][1] for k in options]
        return options[int(np.argmin(errors))], results

    # ---- random walks (motion_state_graph.py:52-71; random_walks.py) -------------------------------------------------
    def generate_random_walk(self, start_action, number_of_steps, use_transition_model=True):
        """MotionStateGraph.generate_random_walk: a list of {"node_key", "parameters"}; the nodes by the reference's rule from the
        global `random`, the parameters from the device sampler (one launch for the walk), keyed by a seed taken from NumPy's
        global stream -- the stream the reference's sampling consumes."""
        from . import random_walks
        return random_walks.generate_random_walk(self, start_action, number_of_steps, use_transition_model)

    def generate_random_walks(self, start_action, number_of_steps, n_walks, seed, rng=None, dtype=np.float64):
        """A population of n_walks random walks (random_walks.RandomWalks): the node sequences from `rng` (a random.Random;
        default: the global `random`), every step's parameters from ONE mg_walks_sample_latents launch under `seed`."""
        from . import random_walks
        return random_walks.generate_random_walks(self, start_action, number_of_steps, n_walks, seed, rng, dtype)

    def close(self):
        for node in self.nodes.values():
            if isinstance(node.cluster_tree, _SEARCH_TREES):
                node.cluster_tree.close()
            prim = getattr(node.motion_primitive, "_prim", None)
            if prim is not None:
                prim.close()
        self.nodes = {}


def _fp_value(v):
    t = type(v)
    if v is None or t is float or t is int or t is str or t is bool:
        return v
    if t is list or t is tuple:
        return tuple([x if type(x) is float else _fp_value(x) for x in v])
    if t is np.ndarray:
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, np.generic):
        return v.item()
    if t is dict:
        return tuple([(k, _fp_value(x)) for k, x in v.items()])
    raise TypeError(t)


_FLAT = frozenset((float, int, str, bool, type(None)))
_DTYPES = {np.float32: np.dtype(np.float32), np.float64: np.dtype(np.float64)}


def flat_constraint_copy(clist):
    """A value copy of a list of plain device-form constraint dicts whose every value is a scalar or a flat list of scalars (the
    usual form: targets as lists of floats / None), for the planner step's "same constraints as last step?" test; None for
    anything else -- arrays, nested lists, reference objects -- which takes the general route every step.  The copy shares
    nothing mutable with the caller's dicts: a target rewritten in place changes the comparison's outcome."""
    if type(clist) is not list:
        return None
    out = []
    for c in clist:
        if type(c) is not dict:
            return None
        d = {}
        for k, v in c.items():
            t = type(v)
            if t in _FLAT:
                d[k] = v
            elif t is list:
                for x in v:
                    if type(x) not in _FLAT:
                        return None
                d[k] = v[:]
            else:
                return None
        out.append(d)
    return out


def _same_mapping(cons, remembered):
    """{option: constraint list} == the remembered flat copy, by value, in one comparison."""
    try:
        return cons == remembered
    except (ValueError, TypeError):
        return False


def _same_constraints(clist, remembered):
    """clist == remembered by value (the interpreter's own recursive comparison of lists, dicts and scalars: key names, lengths
    and values; NaN compares unequal, so a NaN target is "changed" every step -- safe).  Values that cannot be compared this way
    (arrays) are "not the same"."""
    try:
        return type(clist) is list and clist == remembered
    except (ValueError, TypeError):
        return False


def constraint_fingerprint(clist):
    """A value copy of a list of plain device-form constraint dicts, for "same as last step?" comparisons: key names and
    values, nested lists and arrays copied element by element (a caller that rewrites a target list or array IN PLACE changes
    the next fingerprint, not the remembered one).  None when the list holds anything else (reference constraint objects,
    values of unknown types): such lists take the general route."""
    if type(clist) is not list:
        return None
    try:
        return [tuple([(k, _fp_value(v)) for k, v in c.items()]) for c in clist]
    except (AttributeError, TypeError):
        return None


def _options_frame_lists(plan, fast, extras):
    """mg_options_frame_lists for the options in `fast` [(k, TrackScorer | None)]: their result records (_capi.option_records)."""
    vp, m = C.c_void_p, len(fast)
    R, Q = _capi.MG_TRACK_MAX_REQUESTS, _capi.MG_FRAME_LIST_MAX
    prims, plans, lats, errs = (vp * m)(), (vp * m)(), (vp * m)(), (vp * m)()
    lds, ncons = (C.c_int64 * m)(), (C.c_int32 * m)()
    grids, tracks, cons = (vp * (m * R))(), (vp * (m * R))(), (vp * (m * Q))()
    req_of = (C.c_int32 * (m * Q))()
    als, al_ptrs = [], (vp * m)()
    ctx = plan.options[fast[0][0]].ctx
    for j, (k, scorer) in enumerate(fast):
        opt = plan.options[k]
        prims[j], lats[j], errs[j], lds[j] = opt.prim.handle, _capi._dev_ptr(opt.x), _capi._dev_ptr(opt.errors), opt.width
        alignment = extras[k].alignment
        if scorer is not None:
            if not scorer.valid():
                raise _capi.MGError("a track scorer's plan or trajectories were closed under it")
            plans[j], ncons[j] = scorer.plan.handle, scorer.m
            bufs = scorer._track_buffers(plan.n)
            for q, (g, b) in enumerate(zip(scorer.grids, bufs)):
                grids[j * R + q] = g.handle if g is not None else None
                tracks[j * R + q] = _capi._dev_ptr(b)
            for i in range(scorer.m):
                cons[j * Q + i] = C.addressof(scorer.descs[i])
                req_of[j * Q + i] = scorer.req_of[i]
            if alignment is not None:
                al = _capi.ConstraintSet._marshal_alignment(alignment, scorer.plan.skeleton)
                als.append(al)
                al_ptrs[j] = C.addressof(al)
    stride = 16 + 8 * max(plan.options[k].width for k, _ in fast)
    bufs = plan.frame_lists.get((m, stride))
    if bufs is None:
        bufs = plan.frame_lists[(m, stride)] = (ctx.malloc(m * stride), np.empty(m * stride, dtype=np.uint8))
    d_res, host = bufs
    _capi._check(ctx.lib.mg_options_frame_lists(m, prims, plans, lats, plan.code, plan.n, lds, al_ptrs, grids, tracks, ncons, cons, req_of, errs,
                                                 d_res.ptr, stride, host.ctypes.data_as(vp)))
    return _capi.option_records(host, m, stride)


# one option of a planner step: the device buffers of its candidates (n x width), their errors and its result record; its full
# latent width and the normalised mixture weights its component counts are drawn with
_Option = namedtuple("_Option", "name node prim ctx x errors record width weights")
# the whole step's shortcut: a flat copy of the constraint mapping, CSET_GENERATION, the sets and general routes made from it
_Whole = namedtuple("_Whole", "mapping generation csets general")
# an option's memo: a flat copy of its constraints at the last step, the set made from them and that set's cached_values then
_Memo = namedtuple("_Memo", "constraints cset values")
# what _mixed_step adds to an option's keyframe errors
_Extras = namedtuple("_Extras", "trajectories frames alignment skeleton")


class _StepPlan(object):
    """Everything about a planner step that does not change from step to step, built once per (options, n, dtype): the options'
    device buffers (no allocation inside a step), the argument arrays of the C calls (no ctypes object is made inside a step),
    the host block the result records land in, the counts.  Only its methods write the argument arrays."""

    def __init__(self, options, n, dtype):
        self.options, self.n, self.dtype = options, n, dtype
        self.code = _capi.MG_F64 if dtype == np.float64 else _capi.MG_F32
        m = len(options)
        # all primitives in one context: the whole step is one C call (mg_options_step & co.), else mg_option_step per option
        self.fused = m > 0 and all(opt.ctx is options[0].ctx for opt in options)
        self.counts = np.zeros((max(m, 1), max([len(opt.weights) for opt in options] + [1])), dtype=np.int64)
        self.memo = [None] * m          # per option: _Memo, or None
        self.whole = None               # _Whole, or None
        self.track_scorers = {}         # _mixed_step's TrackScorers
        self.frame_lists = {}           # _options_frame_lists' result blocks
        self._bound = None
        vp, mm = C.c_void_p, max(m, 1)
        self.prims = (vp * mm)(*[opt.prim.handle for opt in options])
        self.csets, self.seeds = (vp * mm)(), (C.c_uint64 * mm)()
        self.cnts = (vp * mm)(*[self.counts[k].ctypes.data for k in range(m)])
        self.xs = (vp * mm)(*[_capi._dev_ptr(opt.x).value for opt in options])
        self.errs = (vp * mm)(*[_capi._dev_ptr(opt.errors).value for opt in options])
        self.lds = (C.c_int64 * mm)(*[opt.width for opt in options])
        self._karange, self._seeds_np = np.arange(m, dtype=np.uint64), np.ctypeslib.as_array(self.seeds)[:m]
        if self.fused:
            self.lib = options[0].prim.lib
            self.stride = 16 + 8 * max(opt.width for opt in options)
            self.shared = options[0].ctx.malloc(m * self.stride)
            self.host = np.empty(m * self.stride, dtype=np.uint8)
            self.device_counts = np.zeros((m, 16), dtype=np.int64)
            self.shared_ptr, self.host_ptr = self.shared.ptr, self.host.ctypes.data_as(vp)
            self.device_counts_ptr = self.device_counts.ctypes.data_as(vp)

    def option(self, name):
        return next(opt for opt in self.options if opt.name == name)

    def bind(self, csets):
        """Make `csets` (a ConstraintSet per option) the sets the next launch scores against.  The only writer of the sets' argument
        array: binding other sets than the whole-step shortcut's drops the shortcut, which would otherwise score against them."""
        if csets is self._bound:
            return
        if self.whole is not None and csets is not self.whole.csets:
            self.whole = None
        for k, cs in enumerate(csets):
            self.csets[k] = cs.handle.value
        self._bound = csets

    def seed(self, seed):
        """Option k's candidates are drawn with the key seed + k (modulo 2^64)."""
        np.add(self._karange, np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), out=self._seeds_np)

    def draw_counts(self):
        """Every option's component counts, in option order, from NumPy's global stream."""
        counts, multinomial, n = self.counts, np.random.multinomial, self.n
        for k, opt in enumerate(self.options):
            counts[k, :len(opt.weights)] = multinomial(n, opt.weights)

    def launch(self, device_counts=False, rows=None):
        """mg_options_step, or mg_options_step_device_counts (counts left in self.device_counts), or for rows = (n of the whole draw,
        first row) mg_options_step_rows; without one context mg_option_step per option.  Returns MG_OK or MG_ERR_UNSUPPORTED (the
        one-launch kernel does not take the step, nothing has run); any other status raises."""
        m, n = len(self.options), self.n
        if not self.fused:
            for k, opt in enumerate(self.options):
                _capi._check(opt.prim.lib.mg_option_step(opt.prim.handle, self.csets[k], n, self.counts[k].ctypes.data, self.seeds[k], opt.x.ptr,
                                                         self.code, opt.width, opt.errors.ptr, opt.record.ptr))
            return _capi.MG_OK
        if rows is not None:
            rc = self.lib.mg_options_step_rows(m, self.prims, self.csets, rows[0], self.cnts, self.seeds, rows[1], n, self.xs, self.code, self.lds,
                                               self.errs, self.shared_ptr, self.stride, self.host_ptr)
        elif device_counts:
            rc = self.lib.mg_options_step_device_counts(m, self.prims, self.csets, n, self.seeds, self.xs, self.code, self.lds, self.errs,
                                                        self.shared_ptr, self.stride, self.host_ptr, self.device_counts_ptr)
        else:
            rc = self.lib.mg_options_step(m, self.prims, self.csets, n, self.cnts, self.seeds, self.xs, self.code, self.lds, self.errs,
                                          self.shared_ptr, self.stride, self.host_ptr)
        if rc != _capi.MG_OK and rc != _capi.MG_ERR_UNSUPPORTED:
            _capi._check(rc)
        return rc

    def results(self):
        """({option: (winning latent as float64, error)}, the index of the first minimum over the options, np.argmin's) of the last launch."""
        if self.fused:
            rec = _capi.option_records(self.host, len(self.options), self.stride)     # a copy: the next step reuses the host block
            lat, errors = rec["latent"], rec["error"]      # lat: (m, widest L), the winners already rounded to the caller's type
            errs = errors.tolist()
            return {opt.name: (lat[k, :opt.width], errs[k]) for k, opt in enumerate(self.options)}, int(errors.argmin())
        results = {}
        for opt in self.options:
            size = 16 + 8 * opt.width
            rec = _capi.option_records(opt.ctx.download(opt.record, (size,), np.uint8), 1, size)     # synchronises this option's stream
            results[opt.name] = (rec["latent"][0].astype(self.dtype).astype(np.float64), float(rec["error"][0]))
        return results, int(np.argmin([results[opt.name][1] for opt in self.options]))


class HipPrimitiveSet(object):
    """separate_streams: every primitive gets its own libmg_hip context, i.e. its own HIP stream, so that the small,
    latency-bound launches of different options overlap on the GPU (evaluate_options_on_device)."""

    def __init__(self, primitives_json, context=None, device=0, separate_streams=False):
        self.ctx = context or get_context(device)
        self.nodes = {}
        self._plans = {}
        self._buffers = {}          # (option, n, dtype.str) -> (candidates, errors, result record), shared by the plans holding it
        self._last_counts = None
        for data in primitives_json:
            ctx = _capi.Context(device) if separate_streams else self.ctx
            p = HipMotionPrimitive(None, context=ctx)
            p._initialize_from_json(data)
            self.nodes[p.name] = p

    @property
    def last_counts(self):
        """{option: component counts} the device drew in the last step with device_counts=True."""
        plan = self._last_counts
        if plan is None:
            return None
        return {opt.name: plan.device_counts[k, :len(opt.weights)].copy() for k, opt in enumerate(plan.options)}

    def step_plan(self, options, n, dtype):
        """The _StepPlan of a step over `options` with n candidates each, made on first use: per option (.options, .option(name))
        the device buffers the step leaves its candidates, errors and result record in."""
        dtype = _DTYPES.get(dtype) or np.dtype(dtype)
        key = (options if type(options) is tuple else tuple(options), int(n), dtype.str)
        plan = self._plans.get(key)
        if plan is None:
            n, opts = key[1], []
            for name in key[0]:
                node = self.nodes[name]
                prim = node._prim
                L = prim.n_gmm_dims          # the winner comes back at full width (spatial + time latents)
                bkey = (name, n, dtype.str)
                bufs = self._buffers.get(bkey)
                if bufs is None:
                    bufs = self._buffers[bkey] = (prim.ctx.malloc(max(n, 1) * L * dtype.itemsize), prim.ctx.malloc(max(n, 1) * 8),
                                                  prim.ctx.malloc(16 + 8 * L))
                weights = np.asarray(node.gaussian_mixture_model.weights_, dtype=np.float64)
                opts.append(_Option(name, node, prim, prim.ctx, bufs[0], bufs[1], bufs[2], L, weights / weights.sum()))
            plan = self._plans[key] = _StepPlan(opts, n, dtype)
        return plan

    def evaluate_options_on_device(self, options, constraints_per_option, n_samples, seed=0, dtype=np.float32,
                                   prev_frames=None, skeleton=None, communicator=None, device_counts=False):
        """GraphWalkPlanner's option evaluation (reference graph_walk_planner.py:184-226) without host round trips:
        for every option the component counts come from NumPy's stream, the candidates from the device sampler,
        scoring, first-minimum argmin and the copy of the winner stay on the device (mg_options_step: one C call enqueues
        every option without synchronisation and reads all (16 + 8 L)-byte result records back in one copy; with a
        context per primitive: mg_option_step per option, then one read-back each).
        With `prev_frames` every candidate is aligned to the last previous frame before scoring, which is how the
        planner scores (its constraints stay global, graph_walk_planner.py:179; `skeleton`: a _capi.Skeleton when
        the aligning node is not the root or joints other than the root are constrained).
        communicator (distributed.MgCommunicator / FileCommunicator; rank 0 calls, the other ranks sit in
        distributed.worker_loop with their own HipPrimitiveSet under "__primitive_set__"): rank 0 draws the counts and broadcasts
        them with the constraint values and the seed, every rank runs the step on its block of the rows of every option's draw
        (mg_options_step_rows), one all-gather of the result records, per option the first minimum over the ranks: the
        single-GPU result.
        device_counts: the component counts of every option's draw come from the device as well (mg_options_step_device_counts:
        a Philox-keyed multinomial per option, distributed like NumPy's, not NumPy's stream -- the status the device sampler has
        anyway) instead of 16 x np.random.multinomial on the host, which is most of a step's host time; steps the one-launch
        kernel does not cover fall back to the host draw.  self.last_counts holds the counts of the last such step.
        Returns (best_option, {name: (best_sample, min_error)})."""
        if communicator is not None and communicator.world > 1:
            return self._distributed_step(options, constraints_per_option, int(n_samples), seed, dtype, prev_frames, skeleton, communicator)
        plan = self.step_plan(options, n_samples, dtype)
        csets, general = self._constraint_sets(plan, constraints_per_option, prev_frames, skeleton)
        if None in csets:      # an option with trajectory or per-frame constraints: the mixed step, else option by option
            plan.draw_counts()
            results = self._mixed_step(plan, csets, general, seed) if plan.fused else None
            if results is None:
                results = self._option_chains(plan, constraints_per_option, general, seed)
            return options[int(np.argmin([results[nm][1] for nm in options]))], results
        plan.bind(csets)
        plan.seed(seed)
        # device_counts: the whole step on the device -- counts (mg_options_counts_kernel), candidates, scores, first minima; records
        # and counts arrive in pinned host memory, one synchronisation.  MG_ERR_UNSUPPORTED (an option the one-launch kernel does
        # not cover, nothing has run): the host draw.
        if device_counts and plan.fused and len(plan.options) <= _capi.MG_FUSED_MAX_OPTIONS and plan.launch(device_counts=True) == _capi.MG_OK:
            self._last_counts = plan
        else:
            plan.draw_counts()
            _capi._check(plan.launch())
        results, best = plan.results()
        return options[best], results

    def _constraint_sets(self, plan, constraints_per_option, prev_frames, skeleton):
        """The step's keyframe constraint sets, one per option (None for an option with trajectory or per-frame constraints), and per
        option what the general chain scores with, (device form, alignment, skeleton) or None where the memo gave the set."""
        local = prev_frames is None and skeleton is None
        # The whole step's shortcut.  A planner that asks the same questions as at the last step -- every option's constraints plain
        # device-form dicts with the values they had (ONE comparison by value of the whole mapping against a copy that shares nothing
        # mutable with the caller's: a target rewritten in place is seen), no shared set created, rewritten or closed since (one
        # integer) -- scores against the sets the last step used: no per-option host work at all.
        whole = plan.whole
        if whole is not None and local and whole.generation == _cs.CSET_GENERATION[0] and type(constraints_per_option) is dict and \
                len(constraints_per_option) == len(whole.mapping) and _same_mapping(constraints_per_option, whole.mapping):
            return whole.csets, whole.general
        plan.whole = None
        memo, csets, general = plan.memo, [], []
        for k, opt in enumerate(plan.options):
            cons = constraints_per_option[opt.name]
            clist = cons.constraints if hasattr(cons, "constraints") else cons
            # A planner asks the same questions step after step: when an option's constraints are plain device-form dicts whose
            # every value is what it was at the last step (compared value by value: callers rewrite targets in place), the set of
            # the last step is the set of this one.  Anything else -- reference objects, a previous motion to align to -- takes the
            # general route (device form, structure and values keys, the shared cache).
            last = memo[k]
            if last is not None and local and _same_constraints(clist, last.constraints) and last.cset.handle and \
                    last.cset.cached_values is last.values and getattr(cons, "hip_skeleton", None) is None and getattr(cons, "is_local", True):
                csets.append(last.cset)      # (cached_values: nobody else rewrote the shared set)
                general.append(None)
                continue
            fp = flat_constraint_copy(clist) if local else None
            sk = skeleton if skeleton is not None else getattr(cons, "hip_skeleton", None)
            form = constraints_to_device_form(clist)
            alignment = _cs.alignment_from_prev_frames(prev_frames, cons, sk)
            general.append((form, alignment, sk))
            if any(is_frame_constraint(c) or c.get("type") == "trajectory" for c in form):
                # trajectory and per-frame constraints are not keyframe channels: this option is scored by the mixed step or the
                # general chain (device sampler, fused scorers, the per-frame kernels adding to the same errors, first minimum)
                csets.append(None)
                memo[k] = None
                continue
            cs = _cs.cached_constraint_set(opt.prim, form, sk, alignment)
            csets.append(cs)
            memo[k] = _Memo(fp, cs, cs.cached_values) if fp is not None else None
        if local and type(constraints_per_option) is dict and len(constraints_per_option) == len(plan.options) and None not in memo and \
                None not in csets and all(getattr(constraints_per_option[opt.name], "hip_skeleton", None) is None for opt in plan.options):
            plan.whole = _Whole({opt.name: last.constraints for opt, last in zip(plan.options, memo)}, _cs.CSET_GENERATION[0], csets, general)
        return csets, general

    def _option_chains(self, plan, constraints_per_option, general, seed):
        """The step option by option through the general chain (sample_rows_and_first_minimum): the same draws -- the sampler is keyed
        by seed + option index, the counts are the plan's."""
        from .candidate_scoring import sample_rows_and_first_minimum
        results = {}
        for k, opt in enumerate(plan.options):
            if general[k] is not None:
                form, alignment, sk = general[k]
            else:
                cons = constraints_per_option[opt.name]
                form, alignment, sk = constraints_to_device_form(cons.constraints if hasattr(cons, "constraints") else cons), None, None
            idx, err, lat = sample_rows_and_first_minimum(opt.node, form, alignment, plan.counts[k, :len(opt.weights)].copy(), int(seed) + k, 0,
                                                          plan.n, skeleton=sk, dtype=plan.dtype)
            results[opt.name] = (np.asarray(lat, dtype=np.float64), err)
        return results

    def _distributed_step(self, options, constraints_per_option, n, seed, dtype, prev_frames, skeleton, communicator):
        """evaluate_options_on_device over communicator.world > 1 ranks."""
        from . import distributed
        cmd = {"op": "options_step", "options": list(options), "n_samples": n, "seed": int(seed), "dtype": np.dtype(dtype).name,
               "skeleton": skeleton is not None, "counts": {}, "constraints": {}, "alignments": {}, "widths": {}}
        for name in options:
            node = self.nodes[name]
            cons = constraints_per_option[name]
            clist = cons.constraints if hasattr(cons, "constraints") else cons
            sk = skeleton if skeleton is not None else getattr(cons, "hip_skeleton", None)
            w = np.asarray(node.gaussian_mixture_model.weights_, dtype=np.float64)
            cmd["counts"][name] = np.random.multinomial(n, w / w.sum()).astype(np.int64)
            cmd["constraints"][name] = constraints_to_device_form(clist)
            cmd["alignments"][name] = _cs.alignment_from_prev_frames(prev_frames, cons, sk)
            cmd["widths"][name] = node._prim.n_gmm_dims
        local = {"__primitive_set__": self, "__skeleton__": skeleton}
        if any(is_frame_constraint(c) or c.get("type") == "trajectory" for name in options for c in cmd["constraints"][name]):
            # an option with a trajectory or per-frame constraint: the step as one sample-and-evaluate command per option (every
            # rank holds the primitives under their names), the same draws
            local.update(self.nodes)
            out = {}
            for k, name in enumerate(options):
                _, err, lat = distributed.run_command(communicator, local, {
                    "op": "sample_and_evaluate", "node": name, "constraints": cmd["constraints"][name], "alignment": cmd["alignments"][name],
                    "skeleton": cmd["skeleton"], "counts": cmd["counts"][name], "seed": int(seed) + k, "dtype": cmd["dtype"],
                    "width": cmd["widths"][name]})
                out[name] = (np.asarray(lat, dtype=np.float64), err)
        else:
            out = distributed.run_command(communicator, local, cmd)
        results = {name: (out[name][0].astype(dtype).astype(np.float64), out[name][1]) for name in options}
        errors = [results[nm][1] for nm in options]
        return options[int(np.argmin(errors))], results

    def _mixed_step(self, plan, csets, general, seed):
        """A planner step in which some options carry trajectory or per-frame constraints (csets[k] is None for them): ONE launch
        still draws every option's candidates and scores their KEYFRAME constraints (mg_options_step, component counts already in
        the plan); the options with more then add the rest to their errors where the launch left them -- one launch per root
        trajectory, two per list of per-frame constraints (mg_joint_tracks + mg_score_frame_constraints) -- and take their own first
        minimum (one launch, one small read-back).  The additions are the general chain's, in its order: the same errors and
        winners, bit for bit (round 3 ran such a step option by option: sampler, scorer, ... per option).  None: not covered (an
        option without keyframe constraints, a trajectory aligned by another node than the root) -- the caller goes option by option."""
        from .candidate_scoring import cached_constraint_set, cached_trajectory, release_trajectory, split_trajectories
        from .frame_constraints import TrackScorer, split_frame_constraints, add_frame_constraints_dev
        opts, n, dtype = plan.options, plan.n, plan.dtype
        extras, sets = {}, list(csets)
        for k, opt in enumerate(opts):
            if sets[k] is not None:
                continue
            form, alignment, sk = general[k]
            fused, frames = split_frame_constraints(form)
            keyframes, trajectories = split_trajectories(fused)
            if not keyframes:
                return None
            if alignment is not None and trajectories and alignment.get("joint", 0) not in (0, _capi.MG_ALIGN_START_POSE):
                return None
            sets[k] = cached_constraint_set(opt.prim, keyframes, sk, alignment)
            extras[k] = _Extras(trajectories, frames, alignment, sk)
        plan.bind(sets)
        plan.seed(seed)
        if plan.launch() == _capi.MG_ERR_UNSUPPORTED:      # an option the one-launch kernel does not take
            return None
        results = plan.results()[0]       # (the options in `extras` are replaced below)
        scorers = plan.track_scorers
        # the options' trajectory constraints round by round (the j-th of every option that has one): ONE launch per round
        # (mg_score_trajectories) -- an option's own additions stay in its list's order
        for j in range(max(len(e.trajectories) for e in extras.values())):
            ks = [k for k, e in extras.items() if len(e.trajectories) > j]
            cj = [extras[k].trajectories[j] for k in ks]
            # (pinned while the list is built and enqueued: more distinct trajectories than the cache holds must not close the first)
            trs = [cached_trajectory(opts[k].prim, c, pin=True) for k, c in zip(ks, cj)]
            try:
                _capi.Primitive.score_trajectories_dev([opts[k].prim for k in ks], trs, [opts[k].x for k in ks], dtype, n, [opts[k].width for k in ks],
                                                       [opts[k].errors for k in ks], [c.get("min_u", 0.0) for c in cj], [c.get("weight", 1.0) for c in cj],
                                                       [extras[k].alignment for k in ks], accumulate=True)
            finally:
                for t in trs:
                    release_trajectory(t)
        # the options' per-frame lists and first minima: every option's joint tracks in ONE launch, every option's list + first minimum
        # in a second one, one read-back (mg_options_frame_lists; round 4: two launches per option + a first-minimum launch and two
        # synchronising reads per option).  An option whose list the call does not take (a joint-rotation constraint, more than four
        # constraints or requests) goes the per-option way below.
        fast, slow = [], []
        for k, (trajectories, frames, alignment, sk) in extras.items():
            scorer = None
            if frames:
                key = (k, _cs._freeze(frames), _cs._freeze(alignment), None if sk is None else sk.serial)
                scorer = scorers.get(key)
                if scorer and not scorer.valid():      # a cache was cleared under it
                    scorer.close()
                    scorer = None
                if scorer is None:
                    if len(scorers) > 64:
                        for old in scorers.values():
                            if old:
                                old.close()
                        scorers.clear()
                    try:
                        scorer = TrackScorer(opts[k].prim, frames, sk, alignment)
                    except NotImplementedError:
                        scorer = False        # (a joint-rotation constraint, more than four requests: the frames chain)
                    scorers[key] = scorer
            if not frames or (scorer and scorer.m <= _capi.MG_FRAME_LIST_MAX):
                fast.append((k, scorer if frames else None))
            else:
                slow.append((k, scorer))
        if fast:
            rec = _options_frame_lists(plan, fast, extras)
            for j, (k, _) in enumerate(fast):
                results[opts[k].name] = (rec["latent"][j, :opts[k].width].copy(), float(rec["error"][j]))
        for k, scorer in slow:
            trajectories, frames, alignment, sk = extras[k]
            opt = opts[k]
            if scorer:
                scorer.score_dev(opt.x, dtype, n, opt.width, opt.errors, accumulate=True)
            else:
                add_frame_constraints_dev(opt.prim, opt.ctx.download(opt.x, (n, opt.width), dtype), frames, sk, alignment, opt.errors, accumulate=True)
            idx, err = opt.ctx.argmin_first(opt.errors, n, np.float64)
            row = opt.ctx.download(opt.x.ptr.value + idx * opt.width * dtype.itemsize, (opt.width,), dtype)
            results[opt.name] = (row.astype(np.float64), err)
        return results

    def options_step_rows(self, cmd, row_begin, row_end, skeleton=None):
        """One rank's share of a sharded planner step (distributed._cmd_options_step): the global rows [row_begin, row_end) of
        every option's draw, through mg_options_step_rows.  Returns {option: (global index, error, winning latent)}."""
        from .candidate_scoring import cached_constraint_set
        plan = self.step_plan(tuple(cmd["options"]), int(row_end) - int(row_begin), cmd.get("dtype", "float32"))   # buffers sized for the block
        if not plan.fused:
            raise NotImplementedError("sharded planner steps need all primitives in one context")
        plan.bind([cached_constraint_set(opt.prim, cmd["constraints"][opt.name], skeleton, cmd["alignments"][opt.name]) for opt in plan.options])
        plan.seed(cmd["seed"])
        for k, opt in enumerate(plan.options):
            c = np.asarray(cmd["counts"][opt.name], dtype=np.int64)
            plan.counts[k, :len(c)] = c
        _capi._check(plan.launch(rows=(int(cmd["n_samples"]), int(row_begin))))
        rec = _capi.option_records(plan.host, len(plan.options), plan.stride)
        return {opt.name: (int(rec["index"][k]), float(rec["error"][k]), rec["latent"][k, :opt.width].copy()) for k, opt in enumerate(plan.options)}

    def evaluate_options(self, options, constraints_per_option, n_samples, rng_seed=None):
        """options: node names; constraints_per_option: name -> constraint list.  Returns
        (best_option, {name: (best_sample, min_error)})."""
        results = {}
        for name in options:
            node = self.nodes[name]
            prim = node._prim
            if rng_seed is not None:
                np.random.seed(rng_seed)
            samples = node.sample_low_dimensional_vector(n_samples)
            cset = _capi.ConstraintSet(prim, constraints_to_device_form(constraints_per_option[name]))
            try:
                S = _capi._latents(samples)
                d_s = self.ctx.upload(S)
                d_e = self.ctx.malloc(len(S) * 8)
                prim.score_constraints_dev(cset, d_s, S.dtype, len(S), S.shape[1], d_e, np.float64)
                idx, err = self.ctx.argmin_first(d_e, len(S), np.float64)
                d_s.free()
                d_e.free()
            finally:
                cset.close()
            results[name] = (samples[idx], err)
        errors = [results[n][1] for n in options]
        return options[int(np.argmin(errors))], results
