"""Probe: the TIME-WARPED features of a reachability model -- the root's start, two joints at warped frame 77, the root's ground
position and heading at the last frame -- for 16 'walk'-sized primitives with time models x 10 000 device-sampled float64
candidates (full rows, spatial then time latents): ONE mg_feature_points_warped call on device buffers against the composed route,
the parent commit's only way to these numbers (per primitive: mg_time_function_sample, the whole warped motions by
mg_back_project_frames_at, rows 0 / frame_idx / last of every candidate gathered on the device, mg_joint_positions, the heading on
the host).  The last row's index differs per candidate, so the gather is an indexed one (torch, on the context's stream), not a
strided copy.  Host wall clock around arms that end in the download of their results, the arms taking turns in one process, two
warm-up rounds, median of 7; the kernel's own time from the library's event pairs (profile slot "feature_points_warped").

usage: python tools/probes/feature_points_warped_latency.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import feature_point_model as fpm

NODES, N, ROUNDS, FRAME, N_TIME = 16, 10000, 7, 77, 3
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = _capi.Context(0, stream=stream.cuda_stream)
datas = [synthetic.make_walk_primitive(seed=400 + i, n_time_components=N_TIME) for i in range(NODES)]
prims = [_capi.Primitive(ctx, d) for d in datas]
L, Lt, F, D = prims[0].n_components, prims[0].n_time_components, prims[0].n_canonical_frames, prims[0].n_dim
LD = L + Lt
skeleton = _capi.Skeleton(*synthetic.make_skeleton(19))
JOINTS = ["LeftHand", "RightFoot"]
J = len(JOINTS)
joint_index = skeleton.indices(JOINTS)
lib = prims[0].lib


def f64(*shape):
    return torch.empty(shape, dtype=torch.float64, device=dev)


d_S = [f64(N, LD) for _ in prims]
rng = np.random.default_rng(0)
for i, (prim, data) in enumerate(zip(prims, datas)):          # device-sampled latents, drawn once: both arms read the same
    counts = rng.multinomial(N, np.asarray(data["gmm_weights"]))
    prim.gmm_sample_dev(counts, 1000 + i, d_S[i].data_ptr(), np.float64, LD)
OUT = (("start_root", 3), ("points", 3 * J), ("root_end", 2), ("heading_end", 2), ("heading_len", 1))
d_out = [{name: f64(N, w) for name, w in OUT} for _ in prims]
d_nf = [torch.empty(N, dtype=torch.int32, device=dev) for _ in prims]
desc = skeleton.desc()
table = (_capi.WarpedFeaturePointItem * NODES)()
for rec, prim, s, outs, nf in zip(table, prims, d_S, d_out, d_nf):
    rec.prim, rec.latents, rec.latent_offset, rec.time_offset, rec.n_samples, rec.ld = prim.handle.value, s.data_ptr(), 0, L, N, LD
    rec.skeleton, rec.joints, rec.n_joints, rec.frame_idx = C.addressof(desc), joint_index.ctypes.data, J, FRAME
    for name, _ in OUT:
        setattr(rec, name, outs[name].data_ptr())
    rec.n_frames = nf.data_ptr()

# the composed route's tables: the row capacity from the longest warped motion of the batch (one sampling pass, outside the clock)
d_len = torch.empty(N, dtype=torch.int32, device=dev)
cap = 0
probe_times = f64(N, 4 * F + 8)
for prim, s in zip(prims, d_S):
    _capi._check(lib.mg_time_function_sample(prim.handle, C.c_void_p(s.data_ptr() + 8 * L), _capi.MG_F64, N, LD, C.c_double(1.0),
                                             C.c_void_p(probe_times.data_ptr()), C.c_void_p(d_len.data_ptr()), 4 * F + 8, None))
    lens = d_len.cpu().numpy()
    assert lens.min() > FRAME + 1, "a candidate's warped motion has no frame %d" % FRAME
    cap = max(cap, int(lens.max()))
del probe_times
d_times, d_frames, d_pos = f64(N, cap), f64(N, cap, D), f64(3 * N, J, 3)
row = torch.arange(N, device=dev)


def one_call():
    _capi.feature_points_warped_table(lib, NODES, table, np.float64, host=False)
    ctx.synchronize()
    out = []
    for outs, nf in zip(d_out, d_nf):
        got = {name: t.cpu().numpy() for name, t in outs.items()}
        got["n_frames"] = nf.cpu().numpy()
        got["angles"] = np.array(fpm.orientations_to_angles(got["heading_end"]))
        out.append(got)
    return out


def composed():
    out = []
    for prim, s in zip(prims, d_S):
        _capi._check(lib.mg_time_function_sample(prim.handle, C.c_void_p(s.data_ptr() + 8 * L), _capi.MG_F64, N, LD, C.c_double(1.0),
                                                 C.c_void_p(d_times.data_ptr()), C.c_void_p(d_len.data_ptr()), cap, None))
        _capi._check(lib.mg_back_project_frames_at(prim.handle, C.c_void_p(s.data_ptr()), _capi.MG_F64, N, LD, C.c_void_p(d_times.data_ptr()),
                                                   C.c_void_p(d_len.data_ptr()), cap, C.c_void_p(d_frames.data_ptr()), _capi.MG_F64))
        last = d_len.long() - 1
        three = torch.stack((d_frames[:, 0], d_frames[:, FRAME], d_frames[row, last]), dim=0).contiguous()      # (3, N, D)
        ctx.joint_positions_dev(skeleton, joint_index, three.data_ptr(), 3 * N, D, d_pos.data_ptr())
        ctx.synchronize()
        pos, end, lens = d_pos.cpu().numpy().reshape(3, N, J, 3), three[2].cpu().numpy(), d_len.cpu().numpy()
        start = three[0, :, :3].cpu().numpy()
        q = end[:, 3:7] / np.linalg.norm(end[:, 3:7], axis=1, keepdims=True)
        v = np.array([0.0, 0.0, 1.0]) + 2.0 * (q[:, :1] * np.cross(q[:, 1:], [0.0, 0.0, 1.0]) + np.cross(q[:, 1:], np.cross(q[:, 1:], [0.0, 0.0, 1.0])))
        length = np.linalg.norm(v[:, [0, 2]], axis=1)
        heading = v[:, [0, 2]] / length[:, None]
        out.append({"start_root": start, "points": (pos[1] - start[:, None, :]).reshape(N, 3 * J), "root_end": end[:, [0, 2]], "heading_end": heading,
                    "heading_len": length[:, None], "n_frames": lens, "angles": np.array(fpm.orientations_to_angles(heading))})
    return out


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


arms = {"one_mg_feature_points_warped_call": one_call, "composed_sample_frames_gather_joint_positions": composed}
times, values = {k: [] for k in arms}, {}
for r in range(ROUNDS + 2):
    for k, fn in arms.items():
        ms, values[k] = wall(fn)
        if r >= 2:
            times[k].append(ms)
a, b = values["one_mg_feature_points_warped_call"], values["composed_sample_frames_gather_joint_positions"]
per_candidate_out = 8 * sum(w for _, w in OUT) + 4
result = {"nodes": NODES, "samples_per_node": N, "rounds": ROUNDS, "frame_idx": FRAME, "joints": J, "t_cap": cap, "device": ctx.device_info()["name"],
          "ms_median": {k: float(np.median(v)) for k, v in times.items()}, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
          "n_frames_equal": bool(all(np.array_equal(x["n_frames"], y["n_frames"]) for x, y in zip(a, b))),
          "same_bits": {key: bool(all(np.array_equal(x[key], y[key]) for x, y in zip(a, b))) for key in ("start_root", "points", "root_end")},
          "max_heading_difference": float(max(np.abs(x["heading_end"] - y["heading_end"]).max() for x, y in zip(a, b))),
          "bytes_written_per_node": {"one_call": N * per_candidate_out,
                                     "composed": int(8 * sum(int(x["n_frames"].sum()) for x in b) / NODES * (D + 1)) + 4 * N + 8 * 3 * N * D + 8 * 3 * N * J * 3}}
result["ratio_of_medians"] = result["ms_median"]["composed_sample_frames_gather_joint_positions"] / result["ms_median"]["one_mg_feature_points_warped_call"]

# the kernel alone: event pairs around the launch
for _ in range(5):
    _capi.feature_points_warped_table(lib, NODES, table, np.float64, host=False)
ctx.synchronize()
ctx.profile_enable(True)
ctx.profile_reset()
for _ in range(50):
    _capi.feature_points_warped_table(lib, NODES, table, np.float64, host=False)
ctx.synchronize()
samples = np.asarray(ctx.profile_samples(_capi.PROFILE_SLOTS["feature_points_warped"]), dtype=np.float64)
ctx.profile_enable(False)
result["kernel_us_median"], result["kernel_us_min"], result["kernel_launches_timed"] = float(1e3 * np.median(samples)), float(1e3 * samples.min()), int(len(samples))
print(json.dumps(result, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
