"""Writes tests/golden/random_walks.npz: the node sequences the reference's own random-walk lines give on a small synthetic graph.

The reference's unmodified files motion_model/action_meta_info.py (get_random_start_state), motion_state_group.py
(generate_random_walk) and motion_state_graph_node.py (generate_random_transition) are imported through stub parents, as
oracle/gen_golden.py does: the parents supply the NODE_TYPE_* constants of motion_model/__init__.py, the anim_utils names the files
import, and a MotionPrimitiveModelWrapper whose sample_low_dimensional_vector returns a fixed vector (the parameters are not
recorded).  MotionStateGraph.generate_random_walk itself passes its group one argument too many (motion_state_graph.py:71), so
its two lines are called here: the group's get_random_start_state, then its generate_random_walk.

The graph: two actions, six nodes; nodes with 3, 1 and 0 standard transitions, one node without an end transition, an edge into
another action.  Recorded: the edge lists (in outgoing_edges order), the start states, and for random.seed(0 .. 4) x
number_of_steps in (0, 1, 5) x both actions the node keys of the walk.  Names and integers only.

Run in the build container only:   python tools/gen_random_walk_golden.py
"""
import importlib
import json
import os
import random
import sys
import types

import numpy as np

REFERENCE = "/root/reference/morphablegraphs"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (from, to, transition type) in the order the edges are added to outgoing_edges
EDGES = [
    (("walk", "begin"), ("walk", "left"), "standard"), (("walk", "begin"), ("walk", "stop"), "end"), (("walk", "begin"), ("walk", "right"), "standard"),
    (("walk", "begin"), ("walk", "begin"), "standard"),
    (("walk", "left"), ("walk", "stop"), "end"), (("walk", "left"), ("walk", "right"), "standard"),
    (("walk", "right"), ("walk", "left"), "standard"),
    (("walk", "stop"), ("pick", "reach"), "action_transition"),
    (("pick", "reach"), ("pick", "retrieve"), "end"), (("pick", "reach"), ("walk", "begin"), "action_transition"),
    (("pick", "grasp"), ("pick", "retrieve"), "end"),
]
NODES = {"walk": ["begin", "left", "right", "stop"], "pick": ["reach", "grasp", "retrieve"]}
START_STATES = {"walk": ["begin"], "pick": ["reach", "grasp"]}
END_STATES = {"walk": ["stop"], "pick": ["retrieve"]}
SEEDS, STEPS = (0, 1, 2, 3, 4), (0, 1, 5)


def import_reference():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    quiet = lambda *a, **k: None
    module("anim_utils"), module("anim_utils.utilities"), module("anim_utils.animation_data")
    module("anim_utils.utilities.log", write_log=quiet, write_message_to_log=quiet, LOG_MODE_DEBUG=0, LOG_MODE_INFO=1, LOG_MODE_ERROR=2)
    module("anim_utils.utilities.io_helper_functions", write_to_json_file=quiet)
    module("anim_utils.animation_data.utils", get_arc_length_from_points=quiet)
    top = module("mg_ref_graph")
    top.__path__ = []
    module("mg_ref_graph.space_partitioning", ClusterTree=object, FeatureClusterTree=object)
    pkg = module("mg_ref_graph.motion_model", NODE_TYPE_START="start", NODE_TYPE_STANDARD="standard", NODE_TYPE_END="end", NODE_TYPE_IDLE="idle",
                 NODE_TYPE_SINGLE="single_primitive", NODE_TYPE_CYCLE_END="cycle_end", META_INFORMATION_FILE_NAME="meta_information.json")
    pkg.__path__ = [os.path.join(REFERENCE, "motion_model")]

    class MotionPrimitiveModelWrapper(object):
        def sample_low_dimensional_vector(self, use_time=True):
            return np.zeros(3)
    module("mg_ref_graph.motion_model.motion_primitive_wrapper", MotionPrimitiveModelWrapper=MotionPrimitiveModelWrapper)
    return (importlib.import_module("mg_ref_graph.motion_model.motion_state_group").MotionStateGroup,
            importlib.import_module("mg_ref_graph.motion_model.motion_state_graph_node").MotionStateGraphNode,
            importlib.import_module("mg_ref_graph.motion_model.motion_state_transition").MotionStateTransition)


def build_groups():
    Group, Node, Transition = import_reference()
    groups, nodes = {}, {}
    for action, names in NODES.items():
        group = groups[action] = Group(action, None, None)
        for name in names:
            node = Node(group)
            node.action_name, node.name = action, name
            group.nodes[(action, name)] = nodes[(action, name)] = node
    for a, b, kind in EDGES:
        nodes[a].outgoing_edges[b] = Transition(a, b, kind, None)
    for action, group in groups.items():
        group.set_meta_information({"start_states": START_STATES[action], "end_states": END_STATES[action]})
        for key in group.nodes:      # MotionStateGroup._update_motion_state_stats' count (motion_state_group.py:85)
            group.nodes[key].n_standard_transitions = len(group.get_n_standard_transitions(key))
    return groups


def main():
    groups = build_groups()
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")     # (the reference prints every draw)
    try:
        walks = []
        for action in sorted(groups):
            for seed in SEEDS:
                for steps in STEPS:
                    random.seed(seed)
                    start = groups[action].get_random_start_state()
                    walk = groups[action].generate_random_walk(start, steps, True)
                    walks.append({"action": action, "seed": seed, "number_of_steps": steps, "node_keys": [list(e["node_key"]) for e in walk]})
    finally:
        sys.stdout = stdout
    graph = {"nodes": NODES, "start_states": START_STATES, "end_states": END_STATES,
             "edges": [[list(a), list(b), kind] for a, b, kind in EDGES],
             "n_standard_transitions": {"%s:%s" % key: node.n_standard_transitions for g in groups.values() for key, node in g.nodes.items()}}
    path = os.path.join(ROOT, "tests", "golden", "random_walks.npz")
    np.savez_compressed(path, graph=np.array(json.dumps(graph, sort_keys=True)), walks=np.array(json.dumps(walks, sort_keys=True)))
    lengths = sorted({len(w["node_keys"]) for w in walks})
    print("wrote %s: %d walks of %s nodes, %d bytes" % (path, len(walks), lengths, os.path.getsize(path)))


if __name__ == "__main__":
    main()
