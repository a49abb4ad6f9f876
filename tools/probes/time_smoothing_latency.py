"""Probe: the SMOOTHED time-warped frames of a population of random walks (smooth_time_parameters on every node).  The device
route: RandomWalks.frames(use_time_parameters=True) with smooth_on_device -- one mg_walks_time_functions_smoothed launch, one download
of the lengths, one mg_walks_frames_at call, one download; no time row crosses the bus.  The host-pass route, the only one there was:
graph_walk.assemble_walks(time_parameters=...) once per DISTINCT node sequence with smooth_on_device off -- per sequence the sampling
launches, a download of every time row, scipy's savgol_filter per (walk, step) in a Python loop, an upload, two launches, a download.
Both run in this process on the same latents: 64 walks x 8 steps over 6 nodes of the 'walk' shape family (n_dim 79), every node with
two time latents, the sequences drawn at random.  Wall clock of a synchronised call; the routes alternate inside one run, 3 warm-up
rounds, then the median of 30 rounds each, with the quartiles.  The routes' frames differ by the rounding of the Savitzky-Golay sums
(the table against scipy's convolution and polynomial fits): the largest difference is reported, not held to bits.
usage: python tools/probes/time_smoothing_latency.py [out.json]"""
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
SHAPES = [(40, 156, 2), (32, 120, 2), (24, 96, 2), (40, 140, 2), (16, 64, 2), (28, 180, 2)]      # (n_components, n_canonical_frames, n_time_components)
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
primitives = [graph.nodes[("walk", name)].motion_primitive for name in names]
for mp in primitives:
    mp.smooth_time_parameters = True


def on_device(flag):
    for mp in primitives:
        mp.smooth_on_device = flag

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
    on_device(True)
    return walks.frames(use_time_parameters=True, speed=SPEED)


def per_sequence():
    on_device(False)
    out = [None] * N_WALKS
    for seq, ws in groups.items():
        S, G = packed[seq]
        frames, offsets = gw.assemble_walks(graph, list(seq), S, time_parameters=G, speed=SPEED)
        for j, w in enumerate(ws):
            out[w] = frames[j, :int(offsets[j, -1])]
    return out


a, b = mixed(), per_sequence()
assert all(x.shape == y.shape for x, y in zip(a, b))
worst = max(float(np.abs(x - y).max()) for x, y in zip(a, b))
scale = max(float(np.abs(y).max()) for y in b)
times = {"device": [], "host_pass": []}
for r in range(WARMUP + ROUNDS):
    for name, fn in (("device", mixed), ("host_pass", per_sequence)):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if r >= WARMUP:
            times[name].append(1e3 * (time.perf_counter() - t0))
row = {"n_walks": N_WALKS, "n_steps": N_STEPS, "n_nodes": len(names), "timed_nodes": sum(1 for s in SHAPES if s[2]), "speed": SPEED,
       "distinct_sequences": len(groups), "frames": int(sum(len(x) for x in a)), "largest_difference": worst, "largest_value": scale, "rounds": ROUNDS}
for name, ts in times.items():
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    row[name + "_ms"] = {"median": float(med), "q1": float(q1), "q3": float(q3)}
    print("%-10s median %8.3f ms (quartiles %.3f .. %.3f) over %d rounds" % (name, med, q1, q3, ROUNDS), flush=True)
print("%d walks x %d steps over %d nodes, %d distinct sequences, %d frames; largest difference %.3g of %.4g; host_pass / device = %.1f" % (
    N_WALKS, N_STEPS, len(names), len(groups), row["frames"], worst, scale, row["host_pass_ms"]["median"] / row["device_ms"]["median"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"device": ctx.device_info()["name"], "result": row}, f, indent=1)
walks.close()
graph.close()
