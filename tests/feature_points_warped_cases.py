"""What the time-warped feature point tests share (the host statement's and the device's): the models and recorded arrays of
tests/golden/feature_points_warped.npz (tools/gen_feature_point_warped_golden.py), and timewarp_cases' time tolerance for a
model that is not in its table.  Not a test module."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import timewarp_cases as twc
from conftest import load_golden
from morphablegraphs_amd import _capi


@functools.lru_cache(maxsize=None)
def golden_cases():
    """((model JSON dict, _capi.Skeleton, recorded arrays), ...) of the fixture; read once."""
    g = load_golden("feature_points_warped")
    out = []
    for k in range(int(g["n_models"])):
        p = "m%d_" % k
        rec = {key[len(p):]: g[key] for key in g.files if key.startswith(p)}
        data = {key[len("model_"):]: rec[key] for key in rec if key.startswith("model_")}
        data["n_basis_spatial"], data["n_dim_spatial"], data["n_basis_time"] = int(data.pop("n_basis")), int(data.pop("n_dim")), int(data["n_basis_time"])
        data["n_canonical_frames"], data["name"] = int(rec["n_canonical_frames"]), str(data["name"])
        names = [str(n) for n in rec["joint_names"]]
        joints = [(n, None if par < 0 else names[par], tuple(off)) for n, par, off in zip(names, rec["joint_parents"], rec["joint_offsets"])]
        out.append((data, _capi.Skeleton(joints, [str(n) for n in rec["animated_joints"]]), rec))
    return tuple(out)


def case_ids():
    return [c[0]["name"] for c in golden_cases()]


def time_tolerance_of(data, gammas):
    """timewarp_cases.time_tolerance's formula for a model that is not in its table: max(16 e_fit, 4 ulp of F), never above 1e-11 F,
    e_fit FITPACK's largest deviation from the 50-digit twin over the rows `gammas`.  The bound grows with the rows it is given, so a
    caller that passes only some of the rows it checks (the twin is slow) holds all of them to the smaller bound."""
    F = int(data["n_canonical_frames"])
    e_fit = 0.0
    for g in gammas:
        c = twc.canonical_time_function(data, g)
        e_fit = max(e_fit, float(np.max(np.abs(twc.reference_time_function(c, 1.0) - twc.twin_time_function(c, 1.0)))))
    return min(max(16.0 * e_fit, 4.0 * np.spacing(float(F))), 1.0e-11 * F)
