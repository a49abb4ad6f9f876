"""Probe: the feature step of HipFeaturePointModelBuilder -- the root's ground position and heading at the last frame of every
candidate -- for 16 'walk'-sized primitives x 10 000 device-sampled candidates: ONE mg_feature_points call on device buffers
against the composed path of the parent commit (per primitive: whole float64 motions by mg_back_project_frames_f64, the last
frames gathered, mg_joint_positions of the root, the heading on the host).  Host wall clock around arms that end in the download
of their results, the arms taking turns in one process, two warm-up rounds; the kernel's own time from the library's event pairs
(profile slot "feature_points").

usage: python tools/probes/feature_points_latency.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import feature_point_model as fpm

NODES, N, ROUNDS = 16, 10000, 7
ctx = _capi.Context(0)
datas = [synthetic.make_walk_primitive(seed=400 + i) for i in range(NODES)]
prims = [_capi.Primitive(ctx, d) for d in datas]
L, F, D = prims[0].n_components, prims[0].n_canonical_frames, prims[0].n_dim
root_only = _capi.Skeleton([("Hips", None, (0.0, 0.0, 0.0))], ["Hips"])
root_index = root_only.indices(["Hips"])

bufs = ctx.buffers().__enter__()
d_S = [bufs.malloc(8 * N * L) for _ in prims]
rng = np.random.default_rng(0)
for i, (prim, data) in enumerate(zip(prims, datas)):          # device-sampled latents, drawn once: both arms read the same
    counts = rng.multinomial(N, np.asarray(data["gmm_weights"]))
    prim.gmm_sample_dev(counts, 1000 + i, d_S[i], np.float64, L)
d_out = [(bufs.malloc(8 * N * 2), bufs.malloc(8 * N * 2), bufs.malloc(8 * N)) for _ in prims]
table = (_capi.FeaturePointItem * NODES)()
for rec, prim, s, (a, b, c) in zip(table, prims, d_S, d_out):
    rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = prim.handle.value, s.address, 0, N, L
    rec.root_end, rec.heading_end, rec.heading_len = a.address, b.address, c.address
d_frames, d_last, d_pos = bufs.malloc(8 * N * F * D), bufs.malloc(8 * N * D), bufs.malloc(8 * N * 3)


def one_call():
    _capi.feature_points_table(prims[0].lib, NODES, table, np.float64, host=False)
    out = []
    for a, b, c in d_out:
        end, heading = ctx.download(a, (N, 2), np.float64), ctx.download(b, (N, 2), np.float64)
        out.append((end, heading, np.array(fpm.orientations_to_angles(heading))))
    return out


def composed():
    out = []
    for prim, s in zip(prims, d_S):
        _capi._check(prim.lib.mg_back_project_frames_f64(prim.handle, None, s.ptr, _capi.MG_F64, N, L, d_frames.ptr))
        ctx.copy_rows_dev(d_last, 8 * D, d_frames.address + 8 * (F - 1) * D, 8 * F * D, 8 * D, N)
        ctx.joint_positions_dev(root_only, root_index, d_last, N, D, d_pos)
        last, pos = ctx.download(d_last, (N, D), np.float64), ctx.download(d_pos, (N, 3), np.float64)
        q = last[:, 3:7] / np.linalg.norm(last[:, 3:7], axis=1, keepdims=True)
        v = np.array([0.0, 0.0, 1.0]) + 2.0 * (q[:, :1] * np.cross(q[:, 1:], [0.0, 0.0, 1.0]) + np.cross(q[:, 1:], np.cross(q[:, 1:], [0.0, 0.0, 1.0])))
        heading = v[:, [0, 2]] / np.linalg.norm(v[:, [0, 2]], axis=1, keepdims=True)
        out.append((pos[:, [0, 2]], heading, np.array(fpm.orientations_to_angles(heading))))
    return out


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


arms = {"one_mg_feature_points_call": one_call, "composed_frames_then_joint_positions": composed}
times, values = {k: [] for k in arms}, {}
for r in range(ROUNDS + 2):
    for k, fn in arms.items():
        ms, values[k] = wall(fn)
        if r >= 2:
            times[k].append(ms)
a, b = values["one_mg_feature_points_call"], values["composed_frames_then_joint_positions"]
result = {"nodes": NODES, "samples_per_node": N, "rounds": ROUNDS, "device": ctx.device_info()["name"],
          "ms_median": {k: float(np.median(v)) for k, v in times.items()}, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
          "root_end_same_bits": bool(all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))),
          "max_heading_difference": float(max(np.abs(x[1] - y[1]).max() for x, y in zip(a, b))),
          "bytes_written_per_node": {"one_call": 8 * N * 5, "composed": 8 * N * F * D}}
result["ratio_of_medians"] = result["ms_median"]["composed_frames_then_joint_positions"] / result["ms_median"]["one_mg_feature_points_call"]

# the kernel alone: event pairs around the launch
for _ in range(5):
    _capi.feature_points_table(prims[0].lib, NODES, table, np.float64, host=False)
ctx.synchronize()
ctx.profile_enable(True)
ctx.profile_reset()
for _ in range(50):
    _capi.feature_points_table(prims[0].lib, NODES, table, np.float64, host=False)
ctx.synchronize()
samples = np.asarray(ctx.profile_samples(_capi.PROFILE_SLOTS["feature_points"]), dtype=np.float64)
ctx.profile_enable(False)
result["kernel_us_median"], result["kernel_us_min"], result["kernel_launches_timed"] = float(1e3 * np.median(samples)), float(1e3 * samples.min()), int(len(samples))
print(json.dumps(result, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
bufs.__exit__(None, None, None)
