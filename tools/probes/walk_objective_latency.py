"""Probe: the objective of a whole graph walk in one launch (objective_functions.obj_global_residual_vector_and_naturalness_one_launch:
mg_score_walk_residuals + one mg_gmm_log_prob per step on the resident latents, one upload, one download) against the step-by-step
chain it stands beside (obj_global_residual_vector_and_naturalness: per step a launch, three copies, three allocations and a
synchronisation, then the mixture through the host) -- 'walk'-shaped primitives (L = 40, F = 156, D = 79; a position, a direction
and a joint-position constraint per step), walks of 3 and 16 steps, batches of n = 1 (a residual call) and n = sum L + 1 (a
finite-difference Jacobian).  Wall clock of a synchronised evaluation; the two paths take turns inside one process on one box, one
warm-up each, then the median of REPS >= 5; the spread reported is the interquartile range of each side.  Where the medians differ by
less than the larger spread the verdict is "no difference", not a ratio.
usage: python tools/probes/walk_objective_latency.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import objective_functions as of  # noqa: E402
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode  # noqa: E402

REPS = 9
L, F, D = 40, 156, 79


class _Skeleton(object):
    aligning_root_node, aligning_root_dir, root = "Hips", (0.0, 0.0, 1.0), "Hips"


class _Constraints(object):
    def __init__(self, cons, hip_sk, ref_sk):
        self.constraints, self.is_local, self.hip_skeleton, self.skeleton, self.start_pose, self.evaluations = cons, False, hip_sk, ref_sk, None, 0


class _Step(object):
    def __init__(self, key, parameters, cons):
        self.node_key, self.parameters, self.n_spatial_components, self.n_time_components, self.motion_primitive_constraints = key, parameters, L, 0, cons


class _Graph(object):
    pass


joints, animated = synthetic.make_skeleton()
graph = _Graph()
graph.hip_skeleton, graph.skeleton, graph.nodes = _capi.Skeleton(joints, animated), _Skeleton(), {}
keys = []
for i in range(3):
    node = HipMotionStateGraphNode()
    node.init_from_dict("walk", {"name": "w%d" % i, "mm": synthetic.make_walk_primitive(seed=i)})
    graph.nodes[node.node_key] = node
    keys.append(node.node_key)
ctx = of._prim_of(graph.nodes[keys[0]]).ctx
prev = np.concatenate(([20.0, 90.0, -10.0], np.tile([1.0, 0.0, 0.0, 0.0], (D - 3) // 4)))[None, :]


def walk(n_steps):
    rng = np.random.default_rng(n_steps)
    steps = []
    for i in range(n_steps):
        cons = [{"type": "position", "t": F - 1.0, "weight": 1.0, "target": [30.0 * (i % 3 + 1), None, -20.0 * (i % 3)]},
                {"type": "direction", "t": (F - 1.0) / 2.0, "weight": 0.5, "target": [0.3, 1.0]},
                {"type": "joint_position", "joint": "LeftHand", "t": F - 1.0, "weight": 2.0, "target": [25.0 * (i % 3 + 1), 95.0, -15.0 * (i % 3)]}]
        steps.append(_Step(keys[i % 3], rng.standard_normal(L), _Constraints(cons, graph.hip_skeleton, graph.skeleton)))
    return steps


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return time.perf_counter() - t0


results = []
for n_steps in (3, 16):
    steps = walk(n_steps)
    data = (graph, steps, 0.8, 0.05, prev, 2.0)
    for n in (1, n_steps * L + 1):
        S = 0.7 * np.random.default_rng(n).standard_normal((n, n_steps * L))
        one = lambda: of.obj_global_residual_vector_and_naturalness_one_launch(S, data)
        chain = lambda: of.obj_global_residual_vector_and_naturalness(S, data)
        same = bool(np.array_equal(one().view(np.uint64), chain().view(np.uint64)))      # (also the warm-up of both)
        t_one, t_chain = [], []
        for _ in range(REPS):           # interleaved: a drift of the box meets both sides alike
            t_one.append(timed(one))
            t_chain.append(timed(chain))
        q = lambda t: [1e3 * float(v) for v in np.percentile(t, [25, 50, 75])]
        (o25, o50, o75), (c25, c50, c75) = q(t_one), q(t_chain)
        spread = max(o75 - o25, c75 - c25)
        verdict = "no difference" if abs(c50 - o50) < spread else "one launch x%.2f %s" % (c50 / o50 if o50 < c50 else o50 / c50, "faster" if o50 < c50 else "SLOWER")
        row = {"n_steps": n_steps, "n": n, "one_launch_ms": o50, "one_launch_iqr_ms": o75 - o25, "chain_ms": c50, "chain_iqr_ms": c75 - c25, "reps": REPS,
               "same_bits": same, "verdict": verdict}
        results.append(row)
        print("steps %2d n %4d: one launch %8.3f ms (iqr %.3f) | chain %8.3f ms (iqr %.3f) | %s | same bits: %s" % (
            n_steps, n, o50, o75 - o25, c50, c75 - c25, verdict, same), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"device": ctx.device_info()["name"], "primitive": {"L": L, "F": F, "D": D}, "reps": REPS, "results": results}, f, indent=1)
