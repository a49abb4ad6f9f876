"""Random walks without a device (tests/random_walk_cases.py; the device half is tests/test_gpu_random_walks.py).

1. choose_random_walks gives every node sequence recorded in tests/golden/random_walks.npz -- the reference's own
   get_random_start_state / generate_random_walk / generate_random_transition lines on the same graph (tools/gen_random_walk_golden.py)
   -- from random.Random(seed) and from the global `random`.
2. generate_random_walk refuses transition models before anything is drawn.
3. walk_tables' checks, and the NumPy restatement of the component draw.
4. assemble_walks_mixed_host is assemble_walk_host walk by walk.
"""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
from morphablegraphs_amd import random_walks as rw
from morphablegraphs_amd.graph_walk import assemble_walk_host
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode, HipMotionStateTransition


def test_the_fixture_holds_the_cases_the_rule_has():
    graph, walks = rc.load_golden()
    assert {(w["action"], w["seed"], w["number_of_steps"]) for w in walks} == {(a, s, n) for a in ("walk", "pick") for s in range(5) for n in (0, 1, 5)}
    assert sorted({node.n_standard_transitions for node in graph.nodes.values()}) == [0, 1, 3]
    # a start node without standard transitions: a start and an end only, whatever number_of_steps
    assert all(len(w["node_keys"]) == 2 for w in walks if w["action"] == "pick")
    # a walk that stops on the node without an end transition has no end entry: 1 + number_of_steps nodes
    short = [w for w in walks if w["action"] == "walk" and len(w["node_keys"]) == 1 + w["number_of_steps"]]
    assert short and all(w["node_keys"][-1] == ["walk", "right"] for w in short)
    assert any(len(w["node_keys"]) == 2 + w["number_of_steps"] for w in walks if w["action"] == "walk" and w["number_of_steps"] == 5)
    assert {tuple(w["node_keys"][-1]) for w in walks if w["number_of_steps"] == 0 and w["action"] == "walk"} == {("walk", "stop")}


def test_choose_random_walks_reproduces_every_recorded_sequence():
    graph, walks = rc.load_golden()
    for w in walks:
        want = [tuple(k) for k in w["node_keys"]]
        assert rw.choose_random_walks(graph, w["action"], w["number_of_steps"], 1, random.Random(w["seed"])) == [want], w
        random.seed(w["seed"])                       # the default: the module's global stream, as in the reference
        assert rw.choose_random_walks(graph, w["action"], w["number_of_steps"]) == [want], w


def test_a_population_consumes_one_stream_walk_after_walk():
    graph, _ = rc.load_golden()
    rng = random.Random(7)
    one_by_one = [rw.choose_random_walks(graph, "walk", 5, 1, rng)[0] for _ in range(4)]
    assert rw.choose_random_walks(graph, "walk", 5, 4, random.Random(7)) == one_by_one
    assert len({tuple(w) for w in one_by_one}) > 1
    with pytest.raises(KeyError):
        rw.choose_random_walks(graph, "jump", 1)
    graph.node_groups["walk"]["info"]["start_states"] = []
    with pytest.raises(ValueError):
        rw.choose_random_walks(graph, "walk", 1)


def test_the_nodes_methods_draw_like_the_reference():
    graph, _ = rc.load_golden()
    node = HipMotionStateGraphNode.__new__(HipMotionStateGraphNode)
    node.outgoing_edges = {key: HipMotionStateTransition(("walk", "begin"), key, edge.transition_type) for key, edge in graph.nodes[("walk", "begin")].outgoing_edges.items()}
    node.motion_state_graph = graph
    standard = [k for k, e in node.outgoing_edges.items() if e.transition_type == "standard"]
    random.seed(3)
    want = [standard[random.randrange(0, len(standard), 1)] for _ in range(8)]
    random.seed(3)
    assert [node.generate_random_transition() for _ in range(8)] == want and len(set(want)) > 1
    assert node.generate_random_transition("end") == ("walk", "stop") and node.generate_random_transition("cycle_end") is None
    stop = HipMotionStateGraphNode.__new__(HipMotionStateGraphNode)
    stop.outgoing_edges, stop.motion_state_graph = dict(graph.nodes[("walk", "stop")].outgoing_edges), graph
    assert stop.generate_random_action_transition("pick") == ("pick", "reach") and stop.generate_random_action_transition("walk") is None
    state = random.getstate()
    assert stop.generate_random_transition("standard") is None and random.getstate() == state     # nothing to choose from: nothing drawn


def test_transition_models_are_refused_before_anything_is_drawn():
    graph, _ = rc.load_golden()
    graph.nodes[("walk", "left")].outgoing_edges[("walk", "right")].transition_model = object()
    state, np_state = random.getstate(), np.random.get_state()[1].copy()
    with pytest.raises(NotImplementedError):
        rw.generate_random_walk(graph, "walk", 3, use_transition_model=True)
    assert random.getstate() == state and np.array_equal(np.random.get_state()[1], np_state)
    assert rw.has_transition_models(graph, "walk") and not rw.has_transition_models(graph, "pick")
    with pytest.raises(KeyError):
        rw.generate_random_walk(graph, "jump", 3)


def test_walk_tables():
    a, b, c = ("walk", "a"), ("walk", "b"), ("walk", "c")
    nodes, node_of, n_steps = rw.walk_tables([[b], [a, b, b], [c, a]], known={a, b, c})
    assert nodes == [b, a, c] and n_steps.tolist() == [1, 3, 2] and node_of.dtype == np.int32 and n_steps.dtype == np.int32
    assert node_of.tolist() == [[0, -1, -1], [1, 0, 0], [2, 1, -1]]
    assert rw.walk_tables([[["walk", "a"]]], known={a})[0] == [a]        # keys as lists, as JSON gives them
    for bad, error in (([], ValueError), ([[a], []], ValueError), ([[a, ("walk", "z")]], KeyError)):
        with pytest.raises(error):
            rw.walk_tables(bad, known={a, b, c})


def test_the_component_draw_restated():
    # Philox4x32-10 with counter and key zero, and with all bits set: the known-answer vectors of the Random123 distribution
    out = rc.philox4x32_10(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], dtype=np.uint32), np.array([[0, 0], [0xFFFFFFFF] * 2], dtype=np.uint32))
    assert out.tolist() == [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]]
    weights = [[1.0], [0.25, 0.75], [0.2, 0.3, 0.5]]
    node_of, n_steps = rc.tables([[2] * 500, [1] * 400, [0] * 3])
    comp = rc.walk_components(weights, node_of, n_steps, 99)
    assert (comp[2, :3] == 0).all() and (comp[2, 3:] == -1).all() and (comp[1, 400:] == -1).all()
    # shares within four standard deviations of the weights
    for row, n, w in ((0, 500, weights[2]), (1, 400, weights[1])):
        share = np.bincount(comp[row, :n], minlength=len(w)) / n
        assert np.all(np.abs(share - w) <= 4.0 * np.sqrt(np.array(w) * (1.0 - np.array(w)) / n)), share
    assert not np.array_equal(comp, rc.walk_components(weights, node_of, n_steps, 100))


@pytest.mark.parametrize("kind", ["none", "previous", "start_pose", "previous_spine"])
def test_assemble_walks_mixed_host_is_assemble_walk_host_per_walk(kind):
    jsons, sk = rc.primitive_jsons(), rc.skeleton()
    _, alignment, skeleton = next(a for a in rc.alignments(sk, jsons) if a[0] == kind)
    node_of, n_steps = rc.tables(rc.CONTRACT_WALKS)
    P = rc.latents(node_of, 14)
    frames, offsets, transforms = rw.assemble_walks_mixed_host(jsons, node_of, n_steps, P, alignment, skeleton)
    for w, seq in enumerate(rc.CONTRACT_WALKS):
        steps = [jsons[k] for k in seq]
        S = np.concatenate([P[w, i, :rc.SHAPES[k][0]] for i, k in enumerate(seq)])[None, :]
        fr, offs, tr = assemble_walk_host(steps, S, alignment=alignment, skeleton=skeleton)
        assert np.array_equal(frames[w], fr[0]) and np.array_equal(offsets[w], offs[0]) and np.array_equal(transforms[w, :len(seq)], tr[0])
        assert frames[w].shape == (sum(rc.SHAPES[k][1] for k in seq), 11) and np.isnan(transforms[w, len(seq):]).all()
    assert frames[1].shape == frames[5].shape and not np.array_equal(frames[1], frames[5])     # the shared sequence: the latents differ
