"""Probe: the frames of a population of random walks from ONE mg_walks_frames call (random_walks.RandomWalks.frames: two launches,
one download) against the only route there was before it: graph_walk.assemble_walks once per DISTINCT node sequence, on the same
latents.  64 walks x 8 steps over 6 nodes of the 'walk' shape family (n_dim 79), the sequences drawn at random, so nearly every
walk has its own.  Wall clock of a synchronised call; the two routes alternate inside one run, 3 warm-up rounds, then the median of
30 rounds each, with the quartiles.  The routes' frames are compared bit for bit first.
usage: python tools/probes/random_walks_latency.py [out.json]"""
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import synthetic  # noqa: E402
from morphablegraphs_amd import graph_walk as gw  # noqa: E402
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph  # noqa: E402

N_WALKS, N_STEPS, D = 64, 8, 79
SHAPES = [(40, 156), (32, 120), (24, 96), (40, 140), (16, 64), (28, 180)]      # (n_components, n_canonical_frames) of the six nodes
WARMUP, ROUNDS = 3, 30

names = ["n%d" % i for i in range(len(SHAPES))]
mms = {name: synthetic.make_primitive(seed=300 + i, n_components=L, n_frames=F, n_dim=D, n_gmm=4, name=name) for i, (name, (L, F)) in enumerate(zip(names, SHAPES))}
stats = {name: {"average_step_length": 1.0, "n_standard_transitions": len(names)} for name in names}
data = {"subgraphs": {"walk": {"name": "walk", "info": {"start_states": names[:1], "end_states": [], "stats": stats},
                               "nodes": {name: {"name": name, "mm": mm} for name, mm in mms.items()}}},
        "transitions": {"walk:%s" % a: ["walk:%s" % b for b in names] for a in names}}
graph = HipMotionStateGraph().build_from_graph_data(data)
ctx = graph.ctx
# n0 is the start state, every edge into another node a standard transition, none an end transition: 1 + 7 steps per walk
walks = graph.generate_random_walks("walk", N_STEPS - 1, N_WALKS, seed=1, rng=random.Random(1))
assert set(walks.n_steps.tolist()) == {N_STEPS}
params = walks.parameters_host()
groups = {}
for w, keys in enumerate(walks.node_keys):
    groups.setdefault(tuple(keys), []).append(w)
packed = {seq: np.concatenate([params[ws, i, :graph.nodes[key].get_n_spatial_components()] for i, key in enumerate(seq)], axis=1)
          for seq, ws in groups.items()}


def mixed():
    return walks.frames()


def per_sequence():
    out = [None] * N_WALKS
    for seq, ws in groups.items():
        frames, offsets = gw.assemble_walks(graph, list(seq), packed[seq])
        for j, w in enumerate(ws):
            out[w] = frames[j, :int(offsets[j, -1])]
    return out


a, b = mixed(), per_sequence()
same = all(x.shape == y.shape and np.array_equal(x.view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a, b))
times = {"mixed": [], "per_sequence": []}
for r in range(WARMUP + ROUNDS):
    for name, fn in (("mixed", mixed), ("per_sequence", per_sequence)):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if r >= WARMUP:
            times[name].append(1e3 * (time.perf_counter() - t0))
row = {"n_walks": N_WALKS, "n_steps": N_STEPS, "n_nodes": len(names), "distinct_sequences": len(groups), "same_bits": bool(same), "rounds": ROUNDS}
for name, ts in times.items():
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    row[name + "_ms"] = {"median": float(med), "q1": float(q1), "q3": float(q3)}
    print("%-13s median %8.3f ms (quartiles %.3f .. %.3f) over %d rounds" % (name, med, q1, q3, ROUNDS), flush=True)
print("%d walks x %d steps over %d nodes, %d distinct sequences; same bits: %s; per_sequence / mixed = %.1f" % (
    N_WALKS, N_STEPS, len(names), len(groups), same, row["per_sequence_ms"]["median"] / row["mixed_ms"]["median"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"device": ctx.device_info()["name"], "result": row}, f, indent=1)
walks.close()
graph.close()
