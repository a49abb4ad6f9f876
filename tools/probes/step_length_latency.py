"""Probe: step lengths without frames in memory (mg_step_lengths, csrc/mg_step_length.hip) against the routes through whole
motions, on the 'walk' primitive at the benchmark's 8192 candidates, and update_all_motion_stats against the per-node loop on a
16-node synthetic graph.  Host wall clock around calls that end in a synchronise, alternating the arms; the kernel's own time
from the library's event pairs (profile slot "step_lengths").

usage: python tools/probes/step_length_latency.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraph, HipMotionStateGraphNode, step_lengths_host

B, ROUNDS = 8192, 12
ctx = _capi.Context(0)
node = HipMotionStateGraphNode(context=ctx)
node.init_from_dict("walk", {"name": "walk", "mm": synthetic.make_walk_primitive(seed=0)})
prim = node.motion_primitive._prim
S = np.random.default_rng(0).standard_normal((B, 40))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


arms = {"step_lengths_on_device": lambda: node.step_lengths_on_device(S),
        "get_step_lengths_for_samples": lambda: node.get_step_lengths_for_samples(S),
        "frames_f64_then_download": lambda: step_lengths_host(prim.back_project_frames_f64(S)[:, :, :3])[0]}
times = {k: [] for k in arms}
values = {}
for r in range(ROUNDS + 2):
    for k, fn in arms.items():
        ms, values[k] = wall(fn)
        if r >= 2:
            times[k].append(ms)
result = {"batch": B, "rounds": ROUNDS, "device": ctx.device_info()["name"],
          "ms_median": {k: float(np.median(v)) for k, v in times.items()}, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
          "max_abs_difference_from_frames_f64": float(np.abs(values["step_lengths_on_device"] - values["frames_f64_then_download"]).max()),
          "max_abs_difference_of_the_float32_route": float(np.abs(values["get_step_lengths_for_samples"] - values["frames_f64_then_download"]).max())}

# the kernel alone, device buffers: event pairs around the launch
with ctx.buffers() as bufs:
    d_S, d_arc = bufs.upload(S), bufs.malloc(8 * B)
    table = (_capi.StepLengthItem * 1)()
    table[0].prim, table[0].latents, table[0].n_samples, table[0].ld, table[0].arc_length = prim.handle.value, d_S.address, B, 40, d_arc.address
    for _ in range(20):
        _capi.step_lengths_table(prim.lib, 1, table, np.float64, host=False)
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(200):
        _capi.step_lengths_table(prim.lib, 1, table, np.float64, host=False)
    ctx.synchronize()
    samples = np.asarray(ctx.profile_samples(_capi.PROFILE_SLOTS["step_lengths"]), dtype=np.float64)
    ctx.profile_enable(False)
    result["kernel_us_median"], result["kernel_us_min"], result["kernel_launches_timed"] = float(1e3 * np.median(samples)), float(1e3 * samples.min()), int(len(samples))
    result["bytes_written_per_call"] = 8 * B
    result["bytes_written_by_the_frames_route"] = 4 * B * 156 * 79

# a 16-node graph: one call for all nodes against the per-node loop
mms = {p["name"]: p for p in synthetic.make_graph_primitives(16)}
stats = {name: {"average_step_length": 0.0, "n_standard_transitions": 0} for name in mms}
graph = HipMotionStateGraph(context=ctx).build_from_graph_data(
    {"subgraphs": {"walk": {"name": "walk", "info": {"stats": stats}, "nodes": {n: {"name": n, "mm": mm} for n, mm in mms.items()}}}, "transitions": {}})


def per_node():
    for n in graph.nodes.values():
        n.update_motion_stats(5)


garms = {"update_all_motion_stats": lambda: graph.update_all_motion_stats(5), "per_node_update_motion_stats": per_node}
gtimes = {k: [] for k in garms}
for r in range(ROUNDS + 2):
    for k, fn in garms.items():
        np.random.seed(r)
        ms, _ = wall(fn)
        if r >= 2:
            gtimes[k].append(ms)
result["graph_nodes"] = len(graph.nodes)
result["graph_ms_median"] = {k: float(np.median(v)) for k, v in gtimes.items()}
result["graph_ms_min"] = {k: float(np.min(v)) for k, v in gtimes.items()}
print(json.dumps(result, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
