"""Shared builders of the random-walk tests (tests/test_random_walks_host.py, tests/test_gpu_random_walks.py).

Three synthetic primitives of one n_dim (11: Hips and Spine) whose shapes differ in everything the mixed-sequence kernels index by
node: 31, 33 and 65 canonical frames (one tile of MG_WALK_TILE = 32 less one frame, one tile and one frame, two tiles and one
frame), 7 / 9 / 12 basis functions, 5 / 8 / 12 latents and mixtures of 1 / 2 / 3 components; the third has two time latents, so
its mixture (14 dimensions) is wider than what its frames read.  The graph puts them into one action
with the edge types a random walk follows.  philox4x32_10 and walk_components restate the sampler's component draw
(include/mg_hip.h, mg_walks_sample_latents) in NumPy.
"""
import json
import os

import numpy as np

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose

N_ANIMATED = 2
SHAPES = [(5, 31, 7, 1, 0), (8, 33, 9, 2, 0), (12, 65, 12, 3, 2)]     # (n_components, n_canonical_frames, n_basis, n_gmm, n_time_components)
NAMES = ["a", "b", "c"]
START_POSE = {"position": [35.0, 7.0, -12.0], "orientation": [0.0, 40.0, 0.0]}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_walks.npz")

# the frames contract's population: six walks of 1, 2, 3, 4, 4, 2 steps; node 1 twice in a row in walk 3; walks 1 and 5 share a sequence
CONTRACT_WALKS = [[2], [0, 1], [1, 2, 0], [2, 1, 1, 0], [0, 2, 1, 2], [0, 1]]


def primitive_jsons():
    return [synthetic.make_primitive(seed=170 + i, n_components=L, n_frames=F, n_basis=NB, n_dim=3 + 4 * N_ANIMATED, n_gmm=K, name=NAMES[i],
                                     dirichlet_weights=True, n_time_components=Lt)
            for i, (L, F, NB, K, Lt) in enumerate(SHAPES)]


def skeleton():
    joints, animated = synthetic.make_skeleton(N_ANIMATED)
    return _capi.Skeleton(joints, animated)


def tables(walks):
    """(node_of int32 (n_walks, s_max) padded with -1, n_steps int32) of lists of node indices."""
    n_steps = np.array([len(w) for w in walks], dtype=np.int32)
    node_of = np.full((len(walks), int(n_steps.max())), -1, dtype=np.int32)
    for w, seq in enumerate(walks):
        node_of[w, :len(seq)] = seq
    return node_of, n_steps


def latents(node_of, ld, seed=5, dtype=np.float64):
    """(n_walks, s_max, ld): every entry drawn, so that a kernel reading past a step's own columns or steps would show."""
    return (0.7 * np.random.default_rng(seed).standard_normal(node_of.shape + (ld,))).astype(dtype)


def alignments(sk, jsons):
    """The first-step records of the contract test: (name, alignment, skeleton or None)."""
    from oracle import mg_oracle as orc
    prev = orc.OraclePrimitive(jsons[1]).back_project_frames(np.random.default_rng(3).standard_normal(SHAPES[1][0]))[-1].copy()
    prev[0] += 120.0
    prev[2] -= 40.0
    return [("none", None, None), ("previous", sk.alignment_to(prev, "Hips"), None), ("start_pose", alignment_from_start_pose(START_POSE), None),
            ("previous_spine", sk.alignment_to(prev, "Spine", (0.6, 0.0, 0.8)), sk)]


def graph_data(jsons=None, transition_models=False):
    """One action "walk" over the three primitives: a is the start state with three standard transitions (b, c, a) and an end
    transition; b has one standard transition (c) and an end transition; c has one (b) and no end transition; e, a second node
    of primitive a's shape, is the end state."""
    jsons = primitive_jsons() if jsons is None else jsons
    mms = dict(zip(NAMES, jsons))
    mms["e"] = dict(jsons[0], name="e")
    stats = {name: {"average_step_length": 1.0, "n_standard_transitions": n} for name, n in (("a", 3), ("b", 1), ("c", 1), ("e", 0))}
    info = {"start_states": ["a"], "end_states": ["e"], "stats": stats}
    return {"subgraphs": {"walk": {"name": "walk", "info": info, "nodes": {name: {"name": name, "mm": mm} for name, mm in mms.items()}}},
            "transitions": {"walk:a": ["walk:b", "walk:e", "walk:c", "walk:a"], "walk:b": ["walk:e", "walk:c"], "walk:c": ["walk:b"]}}


# ---- the fixture's graph without a device ---------------------------------------------------------------------------------
class FixtureEdge(object):
    def __init__(self, transition_type, transition_model=None):
        self.transition_type, self.transition_model = transition_type, transition_model


class FixtureNode(object):
    def __init__(self):
        self.outgoing_edges, self.n_standard_transitions = {}, 0


class FixtureGraph(object):
    """What choose_random_walks reads of a graph -- nodes with outgoing_edges and n_standard_transitions, node_groups with the
    start states -- from the recorded edge lists of tests/golden/random_walks.npz."""

    def __init__(self, graph):
        self.nodes, self.node_groups = {}, {}
        for action, names in graph["nodes"].items():
            self.node_groups[action] = {"name": action, "nodes": list(names), "info": {"start_states": graph["start_states"][action],
                                                                                         "end_states": graph["end_states"][action]}}
            for name in names:
                self.nodes[(action, name)] = FixtureNode()
        for a, b, kind in graph["edges"]:
            self.nodes[tuple(a)].outgoing_edges[tuple(b)] = FixtureEdge(kind)
        for key, n in graph["n_standard_transitions"].items():
            self.nodes[tuple(key.split(":"))].n_standard_transitions = n


def load_golden():
    """(FixtureGraph, the recorded walks: dicts with action, seed, number_of_steps, node_keys)."""
    data = np.load(GOLDEN)
    return FixtureGraph(json.loads(str(data["graph"]))), json.loads(str(data["walks"]))


# ---- the component draw in NumPy ------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 for arrays of counters (n, 4) and keys (n, 2) of uint32: (n, 4) uint32."""
    c = [np.asarray(counter)[:, j].astype(np.uint64) for j in range(4)]
    k = [np.asarray(key)[:, j].astype(np.uint64) for j in range(2)]
    M0, M1, W0, W1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [h1 ^ c[1] ^ k[0], l1, h0 ^ c[3] ^ k[1], l0]
        k = [(k[0] + W0) & mask, (k[1] + W1) & mask]
    return np.stack(c, axis=1).astype(np.uint32)


def walk_components(weights, node_of, n_steps, seed):
    """The component of every (walk, step), -1 behind a walk's end: key (seed low, seed high), counter (r low, r high, 0, 1) with
    r = w * s_max + i, the first output word; u = (word + 0.5) 2^-32; the first c with u < cumsum(weights)[c], else the last."""
    n, s_max = node_of.shape
    r = np.arange(n * s_max, dtype=np.uint64)
    counter = np.stack([r & np.uint64(0xFFFFFFFF), r >> np.uint64(32), np.zeros_like(r), np.ones_like(r)], axis=1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.tile(np.array([[seed & 0xFFFFFFFF, seed >> 32]], dtype=np.uint64), (len(r), 1))
    u = (philox4x32_10(counter, key)[:, 0].astype(np.float64) + 0.5) * 2.0 ** -32
    comp = np.full(n * s_max, -1, dtype=np.int32)
    for w in range(n):
        for i in range(int(n_steps[w])):
            cum = np.cumsum(np.asarray(weights[node_of[w, i]], dtype=np.float64))
            below = np.nonzero(u[w * s_max + i] < cum)[0]
            comp[w * s_max + i] = below[0] if len(below) else len(cum) - 1
    return comp.reshape(n, s_max)
