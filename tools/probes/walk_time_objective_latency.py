"""Probe: a graph walk's time objective in one launch (objective_functions.obj_time_error_sum_one_launch: mg_score_walk_time, one
upload, one download) against the step-by-step chain it stands beside (obj_time_error_sum over HipTimeConstraints: per step
mg_time_function_canonical and mg_gmm_log_prob, each with an upload and a download, then the error in a Python loop over
candidates, constraints and steps) -- synthetic.make_primitive(n_time_components=3) ('walk' sized otherwise: L = 40, F = 156),
windows of 1, 3, 8 and 16 steps with a timed keyframe on every other step, at the batch of a finite-difference Jacobian
(len(s) + 1 rows).  Wall clock of a synchronised evaluation; the two paths take turns inside one process on one box, one warm-up
each (which also checks that their results are equal), then the median of REPS; the spread reported is the interquartile range of
each side.  Where the medians differ by less than the larger spread the verdict is "no difference", not a ratio.
usage: python tools/probes/walk_time_objective_latency.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import synthetic  # noqa: E402
from morphablegraphs_amd import objective_functions as of  # noqa: E402
from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode  # noqa: E402

REPS = 15
L, LT, F = 40, 3, 156


class _Skeleton(object):
    frame_time = 1.0 / 30.0


class _Step(object):
    def __init__(self, key, parameters):
        self.node_key, self.parameters, self.n_spatial_components, self.n_time_components = key, parameters, L, LT


class _Graph(object):
    pass


class _Walk(object):
    pass


graph = _Graph()
graph.skeleton, graph.nodes = _Skeleton(), {}
keys = []
for i in range(3):
    node = HipMotionStateGraphNode()
    node.init_from_dict("walk", {"name": "w%d" % i, "mm": synthetic.make_primitive(seed=i, n_time_components=LT, name="w%d" % i)})
    graph.nodes[node.node_key] = node
    keys.append(node.node_key)
ctx = of._prim_of(graph.nodes[keys[0]]).ctx


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return time.perf_counter() - t0


results = []
for n_steps in (1, 3, 8, 16):
    rng = np.random.default_rng(n_steps)
    walk = _Walk()
    walk.steps = [_Step(keys[i % 3], 0.5 * rng.standard_normal(L + LT)) for i in range(n_steps)]
    clist = [(k, F - 1, (k + 1) * F / 30.0) for k in range(0, n_steps, 2)]
    tc = of.HipTimeConstraints(graph, walk, 0, n_steps, clist)
    data = (graph, walk, tc, 2.0, 0.3)
    n = n_steps * LT + 1
    S = 0.5 * np.random.default_rng(n).standard_normal((n, n_steps * LT))
    one = lambda: of.obj_time_error_sum_one_launch(S, data)
    chain = lambda: of.obj_time_error_sum(S, data)
    a, b = one(), chain()                                   # (also the warm-up of both)
    same, close = bool(np.array_equal(a, b)), bool(np.allclose(a, b, rtol=1e-12, atol=0.0))
    t_one, t_chain = [], []
    for _ in range(REPS):           # interleaved: a drift of the box meets both sides alike
        t_one.append(timed(one))
        t_chain.append(timed(chain))
    q = lambda t: [1e3 * float(v) for v in np.percentile(t, [25, 50, 75])]
    (o25, o50, o75), (c25, c50, c75) = q(t_one), q(t_chain)
    spread = max(o75 - o25, c75 - c25)
    verdict = "no difference" if abs(c50 - o50) < spread else "one launch x%.2f %s" % (c50 / o50 if o50 < c50 else o50 / c50, "faster" if o50 < c50 else "SLOWER")
    row = {"n_steps": n_steps, "n": n, "n_constraints": len(clist), "one_launch_ms": o50, "one_launch_iqr_ms": o75 - o25, "chain_ms": c50,
           "chain_iqr_ms": c75 - c25, "reps": REPS, "equal": same, "equal_to_1e-12": close, "verdict": verdict}
    results.append(row)
    print("steps %2d n %3d: one launch %8.3f ms (iqr %.3f) | chain %8.3f ms (iqr %.3f) | %s | equal: %s" % (
        n_steps, n, o50, o75 - o25, c50, c75 - c25, verdict, same), flush=True)
of.clear_walk_objectives()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"device": ctx.device_info()["name"], "primitive": {"L": L, "Lt": LT, "F": F}, "reps": REPS, "results": results}, f, indent=1)
