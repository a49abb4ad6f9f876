"""Probe: which of a graph's nodes reach each of a set of targets -- log p of every target under every node's reachability mixture --
for 64 nodes x 4096 root targets (3 dimensions) and 16 nodes x 4096 feature-point targets (24 dimensions, 8 joints):
HipReachabilityIndex.scores, ONE mg_mixture_scores launch over one upload of the targets, against the host loop of the parent
commit, FeatureMixture.score_samples per node.  Host wall clock around arms that end with the (nodes, targets) matrix in host
memory -- the upload of the targets and the download of the scores are inside the device arm's clock --, the arms taking turns in
one process, two warm-up rounds; the kernel's own time from the library's event pairs (profile slot "mixture_scores").

usage: python tools/probes/reachability_scores_latency.py [out.json]"""
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import _capi
from morphablegraphs_amd import feature_point_model as fpm

ROUNDS, N_TARGETS = 7, 4096
WORKLOADS = {"root_64_nodes_dim3": (64, 3), "points_16_nodes_dim24": (16, 24)}
ctx = _capi.Context(0)


def mixture(rng, K, dim):
    a = rng.standard_normal((K, dim, dim)) * 0.3
    return fpm.FeatureMixture(rng.dirichlet(np.full(K, 2.0)), rng.uniform(-3.0, 3.0, (K, dim)), a @ a.transpose(0, 2, 1) + 0.4 * np.eye(dim))


def node(name, dist):
    model = fpm.HipFeaturePointModel(types.SimpleNamespace(name=name, has_time_parameters=False, t_pca={"n_components": 0}), None, ctx=ctx)
    model.feature_point_dist, model.threshold = dist, -20.0
    return model


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


result = {"targets": N_TARGETS, "rounds": ROUNDS, "device": ctx.device_info()["name"], "workloads": {}}
for name, (n_nodes, dim) in WORKLOADS.items():
    rng = np.random.default_rng(dim)
    # GMMTrainer's sweep ends at 40 components; the AIC minimum of the reachability features is usually far below
    nodes = {"n%02d" % i: node("n%02d" % i, mixture(rng, int(rng.integers(2, 13)), dim)) for i in range(n_nodes)}
    index = fpm.HipReachabilityIndex(nodes, which="points", ctx=ctx)
    X = rng.uniform(-4.0, 4.0, (N_TARGETS, dim))
    arms = {"one_mg_mixture_scores_call": lambda: index.scores(X),
            "host_loop_score_samples_per_node": lambda: np.stack([m.feature_point_dist.score_samples(X) for m in nodes.values()])}
    times, values = {k: [] for k in arms}, {}
    for r in range(ROUNDS + 2):
        for k, fn in arms.items():
            ms, values[k] = wall(fn)
            if r >= 2:
                times[k].append(ms)
    a, b = values["one_mg_mixture_scores_call"], values["host_loop_score_samples_per_node"]
    w = {"nodes": n_nodes, "dim": dim, "components": [int(m.feature_point_dist.n_components) for m in nodes.values()],
         "ms_median": {k: float(np.median(v)) for k, v in times.items()}, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
         "max_relative_difference": float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())}
    w["ratio_of_medians"] = w["ms_median"]["host_loop_score_samples_per_node"] / w["ms_median"]["one_mg_mixture_scores_call"]
    # the kernel alone: event pairs around the launch, on buffers that stay
    with ctx.buffers() as bufs:
        d_x = bufs.upload(X)
        table = (_capi.MixtureScoreItem * n_nodes)()
        for rec, mix in zip(table, index.mixtures):
            rec.mixture, rec.targets, rec.target_offset, rec.n_targets, rec.ld = mix.handle.value, d_x.address, 0, N_TARGETS, dim
            rec.logp = bufs.malloc(8 * N_TARGETS).address
        for _ in range(5):
            _capi.mixture_scores_table(ctx, n_nodes, table)
        ctx.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(50):
            _capi.mixture_scores_table(ctx, n_nodes, table)
        ctx.synchronize()
        samples = np.asarray(ctx.profile_samples(_capi.PROFILE_SLOTS["mixture_scores"]), dtype=np.float64)
        ctx.profile_enable(False)
    w["kernel_us_median"], w["kernel_us_min"], w["kernel_launches_timed"] = float(1e3 * np.median(samples)), float(1e3 * samples.min()), int(len(samples))
    result["workloads"][name] = w
print(json.dumps(result, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
