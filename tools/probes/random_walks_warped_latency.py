"""Probe: the TIME-WARPED frames of a population of random walks from RandomWalks.frames(use_time_parameters=True) -- one
mg_walks_time_functions launch, one download of the lengths, one mg_walks_frames_at call (two launches), one download -- against the
route there was before it: graph_walk.assemble_walks(time_parameters=...) once per DISTINCT node sequence, on the same latents (per
sequence one mg_time_function_sample_rows call per timed step, a download, two launches, a download).  64 walks x 8 steps over 6
nodes of the 'walk' shape family (n_dim 79), three of them with a time model of two time latents, the sequences drawn at random,
so nearly every walk has its own.  Wall clock of a synchronised call; the two routes alternate inside one run, 3 warm-up rounds,
then the median of 30 rounds each, with the quartiles.  The routes' frames are compared bit for bit first.
usage: python tools/probes/random_walks_warped_latency.py [out.json]"""
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
SHAPES = [(40, 156, 2), (32, 120, 0), (24, 96, 2), (40, 140, 0), (16, 64, 2), (28, 180, 0)]      # (n_components, n_canonical_frames, n_time_components)
WARMUP, ROUNDS = 3, 30
SPEED = 1.0

names = ["n%d" % i for i in range(len(SHAPES))]
mms = {name: synthetic.make_primitive(seed=300 + i, n_components=L, n_frames=F, n_dim=D, n_gmm=4, name=name, n_time_components=Lt)
       for i, (name, (L, F, Lt)) in enumerate(zip(names, SHAPES))}
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


def _columns(ws, seq, part):
    cols = []
    for i, key in enumerate(seq):
        mp = graph.nodes[key].motion_primitive
        n_s, n_t = mp.get_n_spatial_components(), mp.get_n_time_components()
        cols.append(params[ws, i, :n_s] if part == "spatial" else params[ws, i, n_s:n_s + n_t])
    return np.ascontiguousarray(np.concatenate(cols + [np.zeros((len(ws), 1))], axis=1))      # (a trailing column: no row is empty)


packed = {seq: (_columns(ws, seq, "spatial"), _columns(ws, seq, "time")) for seq, ws in groups.items()}


def mixed():
    return walks.frames(use_time_parameters=True, speed=SPEED)


def per_sequence():
    out = [None] * N_WALKS
    for seq, ws in groups.items():
        S, G = packed[seq]
        frames, offsets = gw.assemble_walks(graph, list(seq), S, time_parameters=G, speed=SPEED)
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
row = {"n_walks": N_WALKS, "n_steps": N_STEPS, "n_nodes": len(names), "timed_nodes": sum(1 for s in SHAPES if s[2]), "speed": SPEED,
       "distinct_sequences": len(groups), "frames": int(sum(len(x) for x in a)), "same_bits": bool(same), "rounds": ROUNDS}
for name, ts in times.items():
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    row[name + "_ms"] = {"median": float(med), "q1": float(q1), "q3": float(q3)}
    print("%-13s median %8.3f ms (quartiles %.3f .. %.3f) over %d rounds" % (name, med, q1, q3, ROUNDS), flush=True)
print("%d walks x %d steps over %d nodes, %d distinct sequences, %d frames; same bits: %s; per_sequence / mixed = %.1f" % (
    N_WALKS, N_STEPS, len(names), len(groups), row["frames"], same, row["per_sequence_ms"]["median"] / row["mixed_ms"]["median"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"device": ctx.device_info()["name"], "result": row}, f, indent=1)
walks.close()
graph.close()
