"""Probe: a graph walk's frames from mg_walk_frames (graph_walk.assemble_walks: two launches, one download) against the step-by-step
chain of the entry points that existed before it (per step mg_back_project_frames_f64 -> mg_score_constraint_residuals ->
mg_align_frames, one download, the record for the next step built on the host, host concatenation) -- the 'walk' primitive
(L = 40, F = 156, D = 79), a 16-step walk, n_walks = 1 and 256.  Wall clock of a synchronised run, median of 5 after 1 warm-up;
mg_walk_frames_kernel's own time by its dispatch-attached events (profile slot "walk_frames") and the share of the HBM peak
(8 TB/s) its 8 * n_dim * frames bytes amount to.
usage: python tools/probes/walk_frames_latency.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import graph_walk as gw  # noqa: E402
from morphablegraphs_amd.frame_constraints import _Batch  # noqa: E402
from morphablegraphs_amd.motion_state_graph import HipPrimitiveSet  # noqa: E402

HBM_PEAK = 8.0e12
N_STEPS, L, F, D = 16, 40, 156, 79

pset = HipPrimitiveSet([synthetic.make_walk_primitive(seed=0)])
mp = pset.nodes["walk"]
ctx = mp._prim.ctx
keys = ["walk"] * N_STEPS
prev = np.concatenate(([20.0, 90.0, -10.0], np.tile([1.0, 0.0, 0.0, 0.0], (D - 3) // 4)))
alignment = gw._ROOT_ONLY.alignment_to(prev)


def chain(S):
    """what the parent offers: one walk after the other is not needed -- every step's batch of n_walks candidates is one call, but
    each walk has its own previous frame, so mg_align_frames (one record per call) runs per walk"""
    n = len(S)
    out = np.empty((n, N_STEPS * F, D))
    for w in range(n):
        al = alignment
        for i in range(N_STEPS):
            batch = _Batch(mp._prim, S[w:w + 1, i * L:(i + 1) * L], None, al)
            try:
                d_f, T = batch.frames(None)
                fr = ctx.download(d_f, (T, D), np.float64)
            finally:
                batch.close()
            out[w, i * F:(i + 1) * F] = fr
            al = gw._ROOT_ONLY.alignment_to(fr[-1])
    return out


def median_wall(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


results = []
for n_walks in (1, 256):
    rng = np.random.default_rng(n_walks)
    S = 0.7 * rng.standard_normal((n_walks, N_STEPS * L))
    t_new = median_wall(lambda: gw.assemble_walks(pset, keys, S, alignment=alignment))
    n_chain = n_walks                               # every walk goes through the chain; at 256 it takes seconds, so it is timed ONCE after the warm-up
    t_chain = median_wall(lambda: chain(S), reps=5 if n_walks == 1 else 1)
    frames, _ = gw.assemble_walks(pset, keys, S[:4], alignment=alignment)
    worst = float(np.max(np.abs(frames - chain(S[:4])))) / float(np.max(np.abs(frames[..., :3])))
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(6):
        gw.assemble_walks(pset, keys, S, alignment=alignment)
    ctx.synchronize()
    samples = ctx.profile_samples("walk_frames")
    ctx.profile_enable(False)
    kernel_us = 1e3 * float(np.median(samples[1:]))
    nbytes = 8.0 * D * n_walks * N_STEPS * F
    row = {"n_walks": n_walks, "n_steps": N_STEPS, "assemble_walks_ms": 1e3 * t_new, "chain_ms": 1e3 * t_chain, "chain_walks_timed": n_chain, "chain_reps": 5 if n_walks == 1 else 1,
           "speedup": t_chain / t_new, "frames_kernel_us": kernel_us, "frames_bytes": nbytes, "fraction_of_hbm_peak": nbytes / (kernel_us * 1e-6) / HBM_PEAK,
           "disagreement_with_chain": worst}
    results.append(row)
    print("n_walks %4d: assemble_walks %9.3f ms | step-by-step chain %10.3f ms (%d walks timed) | x%.1f | mg_walk_frames_kernel %8.1f us = %.3f of HBM peak | "
          "disagreement %.2g" % (n_walks, row["assemble_walks_ms"], row["chain_ms"], n_chain, row["speedup"], kernel_us, row["fraction_of_hbm_peak"], worst), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"device": ctx.device_info()["name"], "primitive": {"L": L, "F": F, "D": D}, "results": results}, f, indent=1)
