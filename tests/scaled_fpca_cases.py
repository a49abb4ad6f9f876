"""The cases of tests/test_scaled_fpca_host.py and tests/test_gpu_scaled_fpca.py, and of tools/gen_scaled_fpca_golden.py: seeded spline
coefficients on a 5-joint chain-and-branch skeleton (D = 23) and the weight vectors scored on them.  Each case varies one edge
from the base n = 24, n_basis = 7, F = 20, npc = 3, step = 1, m = 3, all joints.  Pure NumPy: no library, no GPU."""
import hashlib

import numpy as np

from morphablegraphs_amd import _capi
from morphablegraphs_amd.synthetic import cubic_b_spline_knots

N_JOINTS, N_DIMS, N_WEIGHTS = 5, 23, 8
MIN_GAP = 1e-3            # relative gap between singular values npc and npc + 1 of the weighted centred matrix, every tested weight vector
BASE = {"n": 24, "n_basis": 7, "F": 20, "npc": 3, "step": 1, "m": 3, "joints": None, "weights": "random", "constant_joint": None}


def skeleton():
    """root - spine - chest, two arms and a head off the chest; hands and head are end sites (not animated)."""
    joints = [("root", None, (0.0, 0.0, 0.0)), ("spine", "root", (0.0, 10.0, 0.5)), ("chest", "spine", (0.0, 12.0, 1.0)),
              ("armL", "chest", (8.0, 3.0, 0.0)), ("armR", "chest", (-8.0, 3.0, 0.0)), ("handL", "armL", (15.0, -1.0, 2.0)),
              ("handR", "armR", (-15.0, -1.0, 2.0)), ("head", "chest", (0.0, 9.0, -1.0))]
    return _capi.Skeleton(joints, ["root", "spine", "chest", "armL", "armR"])


def _case(name, **changes):
    c = dict(BASE, name=name)
    c.update(changes)
    return c


CASES = [
    _case("base"),
    _case("n15", n=15), _case("n16", n=16), _case("n17", n=17),            # both sides of the 16-row tile; odd n: the Jacobi bye
    _case("n2_npc1", n=2, npc=1),
    _case("npc1", npc=1), _case("npc4", npc=4), _case("npc5", npc=5), _case("npc_n_minus_1", npc=23),   # every K mod 4
    _case("step4_F20", step=4), _case("step1_F21", F=21), _case("step4_F21", F=21, step=4),            # where the last sampled frame falls
    _case("m1", m=1), _case("m_gradient", m=N_WEIGHTS + 1), _case("m65", m=65),
    _case("weight_bounds", weights="bounds"),                               # 1e-4 beside 1e3
    _case("constant_joint", constant_joint=3),                              # armL's quaternion the same in all samples: its G_g = 0
    _case("joint_subset", joints=("handL", "head")),
]
NAMES = [c["name"] for c in CASES]
OPTIMISER_CASE = _case("optimiser", n=16, m=1, weights="ones")
DEVICE_ROUTE_CASE = "base"      # the case checked against mg_pca_fit / mg_pca_backproject / mg_joint_positions


def case(name):
    return OPTIMISER_CASE if name == "optimiser" else CASES[NAMES.index(name)]


def joints_of(c):
    sk = skeleton()
    return list(range(len(sk.names))) if c["joints"] is None else [sk.index(j) for j in c["joints"]]


def draw(c, seed):
    """(coeffs (n, n_basis, D), weights (m, 3 + J)) of case c from `seed`: a mean motion, a few modes of falling size and
    noise; root translations in tens of units, quaternions near a common rotation per joint."""
    rng = np.random.default_rng(seed)
    n, nb = c["n"], c["n_basis"]
    mean = np.zeros((nb, N_DIMS))
    mean[:, :3] = rng.normal(0.0, 20.0, (1, 3)) + np.linspace(0.0, 1.0, nb)[:, None] * rng.normal(0.0, 30.0, (1, 3))
    for j in range(N_JOINTS):
        q = rng.normal(0.0, 1.0, 4) + np.array([2.0, 0.0, 0.0, 0.0])
        mean[:, 3 + 4 * j:7 + 4 * j] = q / np.linalg.norm(q)
    n_modes = 8
    modes = rng.normal(0.0, 1.0, (n_modes, nb, N_DIMS))
    modes[:, :, :3] *= 25.0
    modes[:, :, 3:] *= 0.12
    scales = 0.7 ** np.arange(n_modes)
    latents = rng.normal(0.0, 1.0, (n, n_modes)) * scales
    noise = rng.normal(0.0, 1.0, (n, nb, N_DIMS)) * 0.01
    noise[:, :, :3] *= 50.0
    coeffs = mean + np.tensordot(latents, modes, axes=1) + noise
    if c["constant_joint"] is not None:
        j = c["constant_joint"]
        coeffs[:, :, 3 + 4 * j:7 + 4 * j] = mean[:, 3 + 4 * j:7 + 4 * j]
    if c["weights"] == "ones":
        weights = np.ones((c["m"], N_WEIGHTS))
    else:
        weights = np.exp(rng.normal(0.0, 0.7, (c["m"], N_WEIGHTS)))
        weights[0] = 1.0
        if c["weights"] == "bounds":
            weights[1, 0], weights[1, 1], weights[1, 4], weights[1, 5] = 1e-4, 1e3, 1e-4, 1e3
            weights[2, :] = 1e-4
            weights[2, 3] = 1e3
    return np.ascontiguousarray(coeffs), np.ascontiguousarray(weights)


def relative_gaps(coeffs, weights, npc):
    """(s_npc - s_{npc + 1}) / s_npc of the weighted centred matrix, per weight vector (1 where s_{npc + 1} does not exist)."""
    from morphablegraphs_amd.scaled_fpca import spread_weights
    n = len(coeffs)
    out = []
    for ext in spread_weights(weights, coeffs.shape[2]):
        xw = (coeffs * ext).reshape(n, -1)
        s = np.linalg.svd(xw - xw.mean(axis=0), compute_uv=False)
        out.append(1.0 if npc >= len(s) else (s[npc - 1] - s[npc]) / s[npc - 1])
    return np.array(out)


def knots_of(c):
    return cubic_b_spline_knots(c["n_basis"], c["F"])


def digest(coeffs, weights):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(coeffs).tobytes())
    h.update(np.ascontiguousarray(weights).tobytes())
    return h.hexdigest()
