"""The trajectory scorers across every kernel route and shape edge, against the Python oracle.

mg_trajectory.hip holds eight kernels that must give the same bits: the staged one-lane kernel with the target spline's polynomials
in LDS or in global memory, the streaming one-lane kernel, the 8- and 4-lane cooperative kernels and the side-by-side forms of
the last three.  One host function (mg_traj_plan) picks among them from L, rows = 3 NB + 4, the spline's n_seg, B, the candidates in
flight and two options.  ROWS below is a table of the smallest shapes on both sides of every comparison in that function.

traj_plan restates the dispatch; the CPU tests pin it to the C source line by line, assert that the table straddles every
boundary and that every kernel is chosen by some row.  coop_walk_k and wave_help_k restate the two cooperative index maps (the
W-lane windows of mg_traj_closest_dist_coop and the WAVE_HELP rounds of mg_traj_closest_dist) and are held to the k of
oracle.mg_oracle.closest_point_walk on the sweep's own splines and paths.

The GPU sweep runs both searches, the forced lane counts, both latent dtypes, the three alignment modes, three bounds, four time
grids and the tail batch sizes on every row: every call's plan as the library reports it equals the restated one; every route
returns the same bits for the same input; NaN-payload guards around every output come back untouched; candidates 0, 63, 64 and
B - 1 are held to the oracle (closest_point_walk at 1e-9, closest_point_lbfgsb(formk_rule=True) at the search's stated
tolerance).  LEDGER records which (kernel, search) ran; test_the_ledger_covers_every_kernel fails when a route stops being reached.
"""
import math
import os
import re

import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
from oracle import mg_oracle as orc

MG_ERR_UNSUPPORTED = -4
WALK_TOL = 1.0e-9                 # the walk against its restatement (tests/test_gpu_adaptors.py)
U_TOL, D_TOL = 2.0e-6, 1.0e-6     # the reference's search (tests/test_gpu_closest_point.py)

# ---- the dispatch, restated (kept in step with mg_trajectory.hip by test_restatement_matches_the_source) -------------------------
MG_TRAJ_BLOCK = 64
MG_TRAJ_COOP_BLOCK = 64
MG_TRAJ_COOP_MAX_B = 65536
MG_TRAJ_W8_MAX_TOTAL = 28672
MG_TRAJ_W4_MAX_TOTAL = 40960
MG_TRAJ_MULTI_MAX = 16
MG_TRAJ_WALK_ALONE = 16
KB60, KB150, KB158 = 60 * 1024, 150 * 1024, 158 * 1024
KERNELS = _capi.MG_TRAJ_KERNELS


def traj_lanes(search, opt, B, total):
    """mg_traj_lanes."""
    if search != 1:
        return 1
    if opt == 1 or B > MG_TRAJ_COOP_MAX_B:
        return 1
    if opt in (8, 4):
        return opt
    return 8 if total <= MG_TRAJ_W8_MAX_TOTAL else (4 if total <= MG_TRAJ_W4_MAX_TOTAL else 1)


def traj_plan(L, rows, n_seg, B, total=None, points=False, search=0, opt=0):
    """mg_traj_plan: what Context.trajectory_plan returns, or None where the library reports MG_ERR_UNSUPPORTED."""
    total = B if total is None else total
    poly_bytes = (n_seg * 12 + 3) * 8

    def plan(kernel, lanes, cands, poly_lds, needs_paths, together, lds):
        return dict(kernel=kernel, lanes=lanes, poly_lds=poly_lds, needs_paths=needs_paths, together=together,
                    candidates_per_workgroup=cands, lds_bytes=lds)
    if points:
        lanes = traj_lanes(search, opt, B, B) if poly_bytes <= KB60 else 1
        poly_lds = lanes > 1 or poly_bytes <= KB158
        kernel = "coop8" if lanes == 8 else "coop4" if lanes == 4 else "staged_lds" if poly_lds else "staged_global"
        return plan(kernel, lanes, MG_TRAJ_COOP_BLOCK // lanes, poly_lds, False, False, poly_bytes if poly_lds else 0)
    if total > B:
        lanes = traj_lanes(search, opt, B, total)
        coop = lanes > 1
        coop_cands = MG_TRAJ_COOP_BLOCK // lanes
        need = coop_cands * (L + rows) * 8 + poly_bytes if coop else L * MG_TRAJ_BLOCK * 8 + poly_bytes
        if need <= KB60:
            kernel = "coop8_multi" if lanes == 8 else "coop4_multi" if lanes == 4 else "stream_multi"
            return plan(kernel, lanes, coop_cands if coop else MG_TRAJ_BLOCK, True, (not coop) and search == 0, True, need)
    lds = (L + rows) * MG_TRAJ_BLOCK * 8
    if lds > KB150:
        return None
    poly_lds = lds + poly_bytes <= KB158
    if poly_lds:
        lds += poly_bytes
    lanes = traj_lanes(search, opt, B, B)
    coop_cands = MG_TRAJ_COOP_BLOCK // max(lanes, 1)
    coop_lds = coop_cands * (L + rows) * 8 + poly_bytes
    if coop_lds > KB60:
        lanes = 1
    stream_lds = L * MG_TRAJ_BLOCK * 8 + poly_bytes
    if lanes > 1:
        return plan("coop8" if lanes == 8 else "coop4", lanes, MG_TRAJ_COOP_BLOCK // lanes, True, False, False, coop_lds)
    if stream_lds <= KB60:
        return plan("stream", 1, MG_TRAJ_BLOCK, True, search == 0, False, stream_lds)
    return plan("staged_lds" if poly_lds else "staged_global", 1, MG_TRAJ_BLOCK, poly_lds, False, False, lds)


# ---- the cooperative index maps, restated --------------------------------------------------------------------------------------
def _first_k(min_u, G):
    return min(G, int(math.ceil(min_u * G - 1e-12)))


def coop_walk_k(d2, min_u, G, W):
    """mg_traj_closest_dist_coop<W>'s grid walk: d2(u) the squared distance.  Returns (k, windows) and asserts what the device
    relies on: every stop comes from a lane that holds a grid value, the parabola's neighbour lanes lie inside the group and hold
    the grid values k - 1 and k + 1."""
    k = _first_k(min_u, G)
    base, last = k - 1, W - 2
    idxs = [min(G, max(0, base + sub)) if sub < W - 1 else None for sub in range(W)]     # (None: the value at the bound itself)
    mine = [d2(min_u) if i is None else d2(i / G) for i in idxs]
    windows = 1
    while True:
        group = 0
        for sub in range(W):
            idx = base + sub
            if sub <= last and (idx >= G or (sub < last and mine[sub + 1] >= mine[sub])):
                group |= 1 << sub
        group &= ~((1 << (k - base)) - 1)
        if group:
            k = base + (group & -group).bit_length() - 1
            break
        k = base + last
        base, last = k - 1, W - 1
        idxs = [min(G, base + sub) for sub in range(W)]
        mine = [d2(i / G) for i in idxs]
        windows += 1
    assert 0 <= k - base < W and idxs[k - base] == k, (k, base, idxs)
    if 0 < k < G:
        assert k - base - 1 >= 0 and k - base + 1 < W, (k, base, W)
        assert idxs[k - base - 1] == k - 1 and idxs[k - base + 1] == k + 1, (k, base, idxs)
    return k, windows


def wave_help_k(d2, min_u, G):
    """mg_traj_closest_dist<WAVE_HELP = true> for one lane: MG_TRAJ_WALK_ALONE steps alone, then rounds of 64 grid values side by
    side.  Returns (k, steps taken alone, rounds)."""
    k = _first_k(min_u, G)
    dk = d2(k / G)
    done, alone = False, 0
    for _ in range(MG_TRAJ_WALK_ALONE):
        if k >= G:
            done = True
            break
        dn = d2((k + 1) / G)
        if dn >= dk:
            done = True
            break
        k, dk, alone = k + 1, dn, alone + 1
    rounds = 0
    if not done:
        ks, dks = k, dk
        while True:
            rounds += 1
            idx = [ks + 1 + lane for lane in range(64)]
            val = [d2(min(i, G) / G) for i in idx]
            stop = [idx[lane] > G or val[lane] >= (dks if lane == 0 else val[lane - 1]) for lane in range(64)]
            if any(stop):
                first = stop.index(True)
                k = ks + first
                break
            ks += 64
            dks = val[63]
    return k, alone, rounds


# ---- the table ------------------------------------------------------------------------------------------------------------------
F = 24
BATCHES = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130)
B_MAX = max(BATCHES)
ORACLE_CANDS = (0, 63, 64, B_MAX - 1)
MIN_US = (0.0, 0.37, 1.0)


def _row(name, L, NB, D, n_cp, oracle_configs=3):
    return dict(name=name, L=L, NB=NB, D=D, n_cp=n_cp, rows=3 * NB + 4, n_seg=n_cp - 1, oracle_configs=oracle_configs)


ROWS = [
    _row("stream_last_width", 118, 7, 7, 7),
    _row("staged_root_rows", 119, 7, 7, 7),
    _row("long_spline_640", 40, 31, 79, 640, 1),
    _row("long_spline_641", 40, 31, 79, 641, 1),
    _row("poly_global_root_955", 40, 31, 79, 955, 1),
    _row("poly_global_root_956", 40, 31, 79, 956, 1),
    _row("poly_global_points_1686", 8, 7, 7, 1686, 1),
    _row("poly_global_points_1687", 8, 7, 7, 1687, 1),
    _row("forced_four_to_stream", 8, 96, 7, 241, 1),
    _row("forced_four_to_staged", 40, 31, 79, 459, 1),
    _row("no_quaternion_D3", 8, 7, 3, 5),
    _row("no_quaternion_D6", 8, 7, 6, 5),
    _row("tiny", 3, 7, 7, 2),
]
ROW_IDS = [r["name"] for r in ROWS]
BY_NAME = {r["name"]: r for r in ROWS}
UNSUPPORTED_NB = 7
# L + rows = 494: sixteen candidates' rows (four forced lanes) do not fit 60 KB, eight candidates' do, and the latents alone fit the
# streaming kernel -- but (L + rows) * 512 > 150 KB is tested before any of that, so the shape is refused whatever the lanes.  The
# fall-back of four forced lanes is reached through the spline's length instead (forced_four_to_stream, forced_four_to_staged).
ROWS_REFUSED = [_row("forced_four_falls_back", 40, 150, 7, 7)]
# (dtype, alignment mode, min_u, grid): every dtype with every mode, every bound, every grid
CONFIGS = [(np.float64, 0, 0.0, "frames"), (np.float32, 1, 0.37, "frames"), (np.float64, 2, 0.0, "strided"),
           (np.float32, 0, 1.0, "frames"), (np.float64, 1, 0.0, "backwards"), (np.float32, 2, 0.37, "one")]
WEIGHT = 1.5


def _unsupported_L():
    rows = 3 * UNSUPPORTED_NB + 4
    L = 1
    while not ((L + rows) * 512 > KB150 and L * 512 > KB60):
        L += 1
    return L


def _lane_options(search):
    return (0, 1, 4, 8) if search == 1 else (0, 8)       # (the reference's search is one lane whatever is asked for)


def _root_plans(r, B=B_MAX, total=None):
    return [(s, o, traj_plan(r["L"], r["rows"], r["n_seg"], B, total, False, s, o)) for s in (0, 1) for o in _lane_options(s)]


def _point_plans(r, B=B_MAX):
    return [(s, o, traj_plan(r["L"], r["rows"], r["n_seg"], B, None, True, s, o)) for s in (0, 1) for o in _lane_options(s)]


def _curve(t):
    t = np.asarray(t, dtype=np.float64)
    return np.stack([160.0 * t, 90.0 + 2.0 * np.sin(6.0 * t), 40.0 * np.sin(2.0 * t)], axis=-1)


def _control_points(n):
    """A target spline beside the candidates' root paths (a few units off, like tests/test_gpu_adaptors.py)."""
    t = np.linspace(0.0, 1.0, n)
    cps = _curve(t)
    cps[:, 0] += 6.0 * t
    cps[:, 2] -= 4.0 * t
    return cps


def _model(r, D=None):
    """The row's primitive: root control points on _curve, varied by a few units by the latents."""
    if r["name"] == "tiny":
        return synthetic.make_tiny_primitive()
    L, NB, D = r["L"], r["NB"], r["D"] if D is None else D
    data = synthetic.make_primitive(seed=9000 + L + NB, name=r["name"], n_components=L, n_frames=F, n_basis=NB, n_dim=D, n_gmm=1)
    mean = np.array(data["mean_spatial_vector"]).reshape(NB, D)
    eig = np.array(data["eigen_vectors_spatial"]).reshape(L, NB, D)
    mean[:, :3] = _curve(np.linspace(0.0, 1.0, NB))
    eig[:, :, :3] *= 0.03
    data["mean_spatial_vector"] = mean.reshape(-1).tolist()
    data["eigen_vectors_spatial"] = eig.reshape(L, -1).tolist()
    return data


def _n_frames(r):
    return 12 if r["name"] == "tiny" else F


def _grids(r):
    n = _n_frames(r)
    return {"frames": np.linspace(0.0, n - 1.0, 24), "one": np.array([0.4 * n]), "strided": np.array([0.0, 0.5 * n + 0.25, n - 1.0]),
            "backwards": np.linspace(n - 1.0, 0.0, 24)}


def _cps_of(r):
    if r["name"] == "tiny":
        return np.array([[-80.0, 0.0, -60.0], [90.0, 5.0, 70.0]])
    return _control_points(r["n_cp"])


HIPS = ([("Hips", None, (0.0, 0.0, 0.0))], ["Hips"])
PREV7 = np.array([30.0, 88.0, -15.0, 0.9, 0.05, 0.42, 0.03])
PREV7[3:] /= np.linalg.norm(PREV7[3:])
START_POSE = {"position": [3.0, 2.0, 1.0], "orientation": [0.0, 25.0, 0.0]}


def _alignment(mode):
    if mode == 0:
        return None
    if mode == 2:
        return alignment_from_start_pose(START_POSE)
    al = _capi.Skeleton(*HIPS).alignment_to(PREV7, 0)
    return {"joint": 0, "position": al["position"], "heading": al["heading"]}


def _oracle_path(op, s, mode, times):
    """The candidate's aligned root path as the oracle forms it (a primitive without a root quaternion is padded with the identity)."""
    coeffs = op.back_project_spatial_coeffs(s)
    if coeffs.shape[1] < 7:
        coeffs = np.concatenate([coeffs[:, :3], np.tile([1.0, 0.0, 0.0, 0.0], (len(coeffs), 1))], axis=1)
    if mode == 1:
        coeffs = orc.align_coeffs_to_previous_frame(coeffs, PREV7, HIPS[0], HIPS[1], "Hips")
    elif mode == 2:
        coeffs = orc.align_coeffs_to_start_pose(coeffs, {"position": list(START_POSE["position"]), "orientation": list(START_POSE["orientation"])})
    return orc.spline_frames(op.knots, coeffs, times)[:, :3]


def _oracle_chain(cps, path, min_u, search, info=None):
    """(parameters, distances) of the chained search over a path."""
    us, ds = [], []
    for p in path:
        if search == 1:
            rec = {}
            pt, min_u = orc.closest_point_walk(cps, p, min_u, info=rec)
            if info is not None:
                info.append(rec)
        else:
            pt, min_u = orc.closest_point_lbfgsb(cps, p, min_u, formk_rule=True)
        us.append(min_u)
        ds.append(float(np.linalg.norm(np.asarray(p) - pt)))
    return np.array(us), np.array(ds)


def _d2_of(cps, p):
    def d2(u):
        v = orc.catmull_rom_point(cps, u) - p
        return float(v @ v)
    return d2


# ---- WAVE_HELP tracks ---------------------------------------------------------------------------------------------------------------
HELP_G = 1000
HELP_B = 70
HELP_FAR = {3: (0.004, 0.05, 0.2, 0.21, 0.6, 1.4), 40: (0.01, 0.06, 0.1, 0.45, 0.46, 0.47)}     # lane: curve parameter per frame


def _help_tracks():
    """Point tracks for the one-lane walk: lanes 3 and 40 of the first wave jump far ahead of their bound (more than 16 and more
    than 80 grid steps in a frame, both in frame 1, lane 3 past the spline's end in the last frame), the others move a few steps."""
    cps = _control_points(7)
    rng = np.random.default_rng(77)
    T = len(HELP_FAR[3])
    tracks = np.empty((HELP_B, T, 3))
    for b in range(HELP_B):
        t = np.array(HELP_FAR[b]) if b in HELP_FAR else 0.002 * b + 0.008 * np.arange(T)
        tracks[b] = _curve(t) + rng.normal(0.0, 0.4, (T, 3))
    return cps, tracks


# ---- CPU checks -----------------------------------------------------------------------------------------------------------------
def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "morphablegraphs_amd", "csrc", name)).read()


def test_restatement_matches_the_source():
    """Every constant and every comparison restated above, pinned to its line in mg_trajectory.hip / mg_traj_device.h."""
    src, dev = _source("mg_trajectory.hip"), _source("mg_traj_device.h")
    for name, value in (("MG_TRAJ_BLOCK", MG_TRAJ_BLOCK), ("MG_TRAJ_COOP_BLOCK", MG_TRAJ_COOP_BLOCK), ("MG_TRAJ_COOP_MAX_B", MG_TRAJ_COOP_MAX_B),
                        ("MG_TRAJ_W8_MAX_TOTAL", MG_TRAJ_W8_MAX_TOTAL), ("MG_TRAJ_W4_MAX_TOTAL", MG_TRAJ_W4_MAX_TOTAL),
                        ("MG_TRAJ_MULTI_MAX", MG_TRAJ_MULTI_MAX)):
        m = re.search(r"#define %s (\d+)\b" % name, src)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"#define MG_TRAJ_WALK_ALONE (\d+)\b", dev).group(1) == str(MG_TRAJ_WALK_ALONE)
    plan = src[src.index("static int mg_traj_plan("):src.index('extern "C" int mg_trajectory_plan(')]
    lanes = src[src.index("static int mg_traj_lanes("):src.index("// THE DISPATCH")]
    assert sorted(set(re.findall(r"(\d+) \* 1024", plan))) == ["150", "158", "60"] and (KB60, KB150, KB158) == (61440, 153600, 161792)
    for line in ("if (ctx->opt[MG_OPT_TRAJECTORY_SEARCH] != 1) return 1;", "if (opt == 1 || B > MG_TRAJ_COOP_MAX_B) return 1;",
                 "if (opt == 8 || opt == 4) return opt;",
                 "return total <= MG_TRAJ_W8_MAX_TOTAL ? 8 : (total <= MG_TRAJ_W4_MAX_TOTAL ? 4 : 1);"):
        assert line in lanes, line
    for line in ("const size_t poly_bytes = ((size_t)n_seg * 12 + 3) * 8;",
                 "pl.lanes = poly_bytes <= 60 * 1024 ? mg_traj_lanes(ctx, B, B) : 1;",
                 "pl.poly_lds = pl.lanes > 1 || poly_bytes <= 158 * 1024;", "pl.lds_bytes = pl.poly_lds ? poly_bytes : 0;",
                 "pl.cands = MG_TRAJ_COOP_BLOCK / pl.lanes;",
                 "if (total > B) {", "const int lanes = mg_traj_lanes(ctx, B, total);", "const int coop_cands = MG_TRAJ_COOP_BLOCK / lanes;",
                 "const size_t need = coop ? (size_t)coop_cands * (L + rows) * 8 + poly_bytes",
                 ": (size_t)L * MG_TRAJ_BLOCK * 8 + poly_bytes;", "if (need <= 60 * 1024) {",
                 "pl.needs_paths = !coop && search == 0; pl.together = true;",
                 "size_t lds = (size_t)(L + rows) * MG_TRAJ_BLOCK * 8;", "if (lds > 150 * 1024) {",
                 "const bool poly_lds = lds + poly_bytes <= 158 * 1024;", "if (poly_lds) lds += poly_bytes;",
                 "int lanes = mg_traj_lanes(ctx, B, B);", "const int coop_cands = MG_TRAJ_COOP_BLOCK / std::max(lanes, 1);",
                 "const size_t coop_lds = (size_t)coop_cands * (L + rows) * 8 + poly_bytes;", "if (coop_lds > 60 * 1024) lanes = 1;",
                 "const size_t stream_lds = (size_t)L * MG_TRAJ_BLOCK * 8 + poly_bytes;",
                 "else if (stream_lds <= 60 * 1024) { pl.kernel = MG_TRAJ_KERNEL_STREAM; pl.lds_bytes = stream_lds; pl.needs_paths = search == 0; }"):
        assert line in plan, line
    # the entry points call it and hold no arithmetic of their own
    rest = src[src.index('extern "C" int mg_trajectory_plan('):]
    assert rest.count("mg_traj_plan(") == 4 and "* 1024" not in rest.replace("160 * 1024", "")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mg_hip.h")).read()
    for i, k in enumerate(KERNELS):
        assert "#define MG_TRAJ_KERNEL_%s %d " % (k.upper(), i) in header, k
    # the two index maps
    for line in ("int base = k - 1, last = W - 2;", "idx = idx < 0 ? 0 : (idx > G ? G : idx);",
                 "mine = mg_traj_d2(poly, n_seg, sub == W - 1 ? min_u : idx * invG, q);",
                 "const bool stop = sub <= last && (idx >= G || (sub < last && next >= mine));",
                 "const unsigned group = (unsigned)(__ballot(stop) >> g0) & ((1u << W) - 1u) & ~((1u << (k - base)) - 1u);",
                 "if (group) { k = base + (__ffs(group) - 1); break; }", "k = base + last;", "base = k - 1; last = W - 1;",
                 "i2 = i2 > G ? G : i2;", "const double da = __shfl(mine, g0 + (k - base) - 1), dc = __shfl(mine, g0 + (k - base) + 1);",
                 "for (int step = 0; step < MG_TRAJ_WALK_ALONE && !done; step++) {", "const int idx = ks + 1 + lane;",
                 "const double val = mg_traj_d2(a.poly, a.n_seg, (idx < G ? idx : G) * invG, qs);",
                 "const double before = lane == 0 ? dks : up;", "const unsigned long long stop = __ballot(idx > G || val >= before);",
                 "if (lane == src) { k = ks + first; dk = first > 0 ? dfirst : dks; }", "ks += 64;", "dks = __shfl(val, 63);"):
        assert line in dev, line


def test_the_table_lands_on_both_sides_of_every_comparison():
    """Each comparison of the dispatch is taken both ways by some call the sweep makes, at the smallest shapes that do so."""
    R = BY_NAME

    def root(name, search, opt, B=B_MAX, total=None):
        r = R[name]
        return traj_plan(r["L"], r["rows"], r["n_seg"], B, total, False, search, opt)

    def pts(name, search, opt, B=B_MAX):
        r = R[name]
        return traj_plan(r["L"], r["rows"], r["n_seg"], B, None, True, search, opt)
    # stream_lds <= 60 KB: L = 118 at seven control points is the last width that streams (one lane), 119 is staged
    assert root("stream_last_width", 0, 0)["kernel"] == "stream" and root("stream_last_width", 0, 0)["lds_bytes"] == 118 * 512 + 600 <= KB60
    assert root("staged_root_rows", 0, 0) == dict(kernel="staged_lds", lanes=1, poly_lds=True, needs_paths=False, together=False,
                                                  candidates_per_workgroup=64, lds_bytes=(119 + 25) * 512 + 600)
    assert root("stream_last_width", 1, 1)["kernel"] == "stream" and root("staged_root_rows", 1, 1)["kernel"] == "staged_lds"
    assert root("stream_last_width", 0, 0)["needs_paths"] and not root("stream_last_width", 1, 1)["needs_paths"]
    # poly_bytes <= 60 KB on the points route: 640 control points keep the cooperative kernels, 641 fall to one lane
    assert pts("long_spline_640", 1, 0)["kernel"] == "coop8" and pts("long_spline_640", 1, 4)["kernel"] == "coop4"
    assert all(pts("long_spline_641", 1, o)["kernel"] == "staged_lds" for o in (0, 1, 4, 8))
    assert (639 * 12 + 3) * 8 <= KB60 < (640 * 12 + 3) * 8
    # ... and both long splines are staged on the root rows (the cooperative and the streaming forms do not hold them)
    assert all(p["kernel"] == "staged_lds" for n in ("long_spline_640", "long_spline_641") for _, _, p in _root_plans(R[n]))
    # lds + poly_bytes <= 158 KB on the root rows: 955 control points stay in LDS, 956 go to global memory
    assert all(p["kernel"] == "staged_lds" and p["lds_bytes"] <= KB158 for _, _, p in _root_plans(R["poly_global_root_955"]))
    assert all(p["kernel"] == "staged_global" and not p["poly_lds"] and p["lds_bytes"] == 137 * 512 for _, _, p in _root_plans(R["poly_global_root_956"]))
    # poly_bytes <= 158 KB on the points route: 1686 / 1687
    assert all(p["kernel"] == "staged_lds" and p["lds_bytes"] == (1685 * 12 + 3) * 8 <= KB158 for _, _, p in _point_plans(R["poly_global_points_1686"]))
    assert all(p["kernel"] == "staged_global" and p["lds_bytes"] == 0 for _, _, p in _point_plans(R["poly_global_points_1687"]))
    # coop_lds <= 60 KB: sixteen candidates' rows and the polynomials (four forced lanes) do not fit, eight candidates' do; the one lane
    # that is left streams where the latents and the polynomials fit 60 KB and is staged where they do not
    r = R["forced_four_to_stream"]
    assert r["L"] + r["rows"] == 300 and 16 * 300 * 8 + 23064 > KB60 >= 16 * 300 * 8 + 23064 - 96 and 300 * 512 <= KB150
    assert root("forced_four_to_stream", 1, 8)["kernel"] == "coop8" and root("forced_four_to_stream", 1, 0)["kernel"] == "coop8"
    assert root("forced_four_to_stream", 1, 4) == dict(kernel="stream", lanes=1, poly_lds=True, needs_paths=False, together=False,
                                                       candidates_per_workgroup=64, lds_bytes=8 * 512 + 23064)
    assert root("forced_four_to_staged", 1, 8)["kernel"] == "coop8" and root("forced_four_to_staged", 1, 4)["kernel"] == "staged_lds"
    assert root("stream_last_width", 1, 4)["kernel"] == "coop4"
    # the issue's row for this fall-back (L = 40, NB = 150: L + rows = 494) never gets that far: 494 * 512 > 150 KB
    r = ROWS_REFUSED[0]
    assert r["L"] + r["rows"] == 494 and 16 * 494 * 8 + 600 > KB60 >= 8 * 494 * 8 + 600 and r["L"] * 512 + 600 <= KB60
    assert all(traj_plan(r["L"], r["rows"], r["n_seg"], B_MAX, None, False, s, o) is None for s in (0, 1) for o in (0, 1, 4, 8))
    # lds <= 150 KB
    Lu = _unsupported_L()
    rows_u = 3 * UNSUPPORTED_NB + 4
    assert Lu == 276 and traj_plan(Lu, rows_u, 6, B_MAX, search=1) is None and traj_plan(Lu - 1, rows_u, 6, B_MAX, search=1) is not None
    # lanes by candidates in flight, B > 65 536
    assert [traj_lanes(1, 0, 64, t) for t in (28672, 28673, 40960, 40961)] == [8, 4, 4, 1]
    assert traj_lanes(1, 8, 65536, 65536) == 8 and traj_lanes(1, 8, 65537, 65537) == 1 and traj_lanes(0, 8, 64, 64) == 1
    assert root("tiny", 1, 8, B=65537)["kernel"] == "stream" and root("tiny", 1, 8, B=65536)["kernel"] == "coop8"
    # side by side: need <= 60 KB per scorer, cooperative or streaming
    assert root("long_spline_640", 1, 0, total=3 * B_MAX)["together"] is False
    assert root("tiny", 1, 0, total=3 * B_MAX)["kernel"] == "coop8_multi" and root("tiny", 1, 4, total=3 * B_MAX)["kernel"] == "coop4_multi"
    assert root("tiny", 1, 1, total=3 * B_MAX)["kernel"] == "stream_multi" and not root("tiny", 1, 1, total=3 * B_MAX)["needs_paths"]
    assert root("tiny", 0, 0, total=3 * B_MAX)["kernel"] == "stream_multi" and root("tiny", 0, 0, total=3 * B_MAX)["needs_paths"]
    assert root("staged_root_rows", 0, 0, total=3 * B_MAX)["together"] is False and root("stream_last_width", 0, 0, total=3 * B_MAX)["together"]


def _reachable():
    """(kernel, search) pairs some call of the sweep must take."""
    want = {(k, 1) for k in KERNELS}
    want |= {(k, 0) for k in ("staged_lds", "staged_global", "stream", "stream_multi")}
    return want


def test_every_kernel_is_chosen_by_some_row():
    chosen = set()
    for r in ROWS:
        for s, o, p in _root_plans(r) + _point_plans(r):
            chosen.add((p["kernel"], s))
        for s in (0, 1):
            for o in _lane_options(s):
                p = traj_plan(r["L"], r["rows"], r["n_seg"], B_MAX, 3 * B_MAX, False, s, o)
                chosen.add((p["kernel"], s))
    assert chosen == _reachable(), sorted(_reachable() ^ chosen)
    # the grids: a knot span that jumps by two and more, one that goes backwards, a single sample
    for r in ROWS:
        knots = orc.cubic_b_spline_knots(r["NB"], _n_frames(r))
        g = _grids(r)
        assert np.diff(orc.basis_rows(knots, g["strided"])[0]).max() >= 2, r["name"]
        assert np.diff(orc.basis_rows(knots, g["backwards"])[0]).min() < 0 and len(g["one"]) == 1 and len(g["frames"]) == 24
    assert {c[0] for c in CONFIGS} == {np.float32, np.float64} and {c[1] for c in CONFIGS} == {0, 1, 2}
    assert {c[2] for c in CONFIGS} == set(MIN_US) and {c[3] for c in CONFIGS} == {"frames", "one", "strided", "backwards"}
    assert {(np.dtype(c[0]).name, c[1]) for c in CONFIGS} == {(d, m) for d in ("float32", "float64") for m in (0, 1, 2)}
    assert set(BATCHES) >= {1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130}


@pytest.mark.parametrize("name", ["stream_last_width", "long_spline_641", "no_quaternion_D3", "tiny"])
def test_index_maps_give_the_walks_k(name):
    """coop_walk_k (W = 4, 8) and wave_help_k against closest_point_walk's k, frame by frame, on the sweep's own splines and paths."""
    r = BY_NAME[name]
    data = _model(r)
    op = orc.OraclePrimitive(data)
    cps = _cps_of(r)
    S = _latents_of(r)
    G = 1000
    windows = set()
    for b, (mode, min_u, grid) in zip((0, 63, 129), ((0, 0.0, "frames"), (2, 0.37, "backwards"), (0, 1.0, "strided"))):
        path = _oracle_path(op, S[b], mode, _grids(r)[grid])
        info = []
        us, _ = _oracle_chain(cps, path, min_u, 1, info)
        bound = min_u
        for f, p in enumerate(path):
            d2 = _d2_of(cps, p)
            for W in (4, 8):
                k, nw = coop_walk_k(d2, bound, G, W)
                windows.add(min(nw, 3))
                assert k == info[f]["k"], (name, b, f, W, k, info[f])
            assert wave_help_k(d2, bound, G)[0] == info[f]["k"], (name, b, f)
            bound = us[f]
    assert 1 in windows and (name == "tiny" or max(windows) >= 2), windows     # the first window alone, and refills


def test_wave_help_tracks_exercise_the_rounds():
    """The WAVE_HELP tracks against closest_point_walk's k -- and the counts that make them a test of the rounds: a frame with more
    than 16 grid steps, one with more than 80 (a second round), one that ends at k = G, one wave in which two lanes need help."""
    cps, tracks = _help_tracks()
    over16 = over80 = at_end = 0
    helped = np.zeros(tracks.shape[:2], dtype=int)
    max_rounds = 0
    for b in list(HELP_FAR) + [0, 63, 64, 69]:
        info = []
        us, _ = _oracle_chain(cps, tracks[b], 0.0, 1, info)
        bound = 0.0
        for f, p in enumerate(tracks[b]):
            d2 = _d2_of(cps, p)
            k, alone, rounds = wave_help_k(d2, bound, HELP_G)
            assert k == info[f]["k"], (b, f, k, info[f])
            for W in (4, 8):
                assert coop_walk_k(d2, bound, HELP_G, W)[0] == k, (b, f, W)
            steps = k - info[f]["k0"]
            over16 += steps > 16
            over80 += steps > 80
            at_end += k == HELP_G
            assert (rounds > 0) == (steps >= 16) and (steps <= 80 or rounds >= 2), (b, f, steps, rounds)
            helped[b, f] = rounds > 0
            max_rounds = max(max_rounds, rounds)
            bound = us[f]
    assert over16 >= 1 and over80 >= 1 and at_end >= 1 and max_rounds >= 2, (over16, over80, at_end, max_rounds)
    assert helped[:64].sum(axis=0).max() >= 2, "no frame in which two lanes of the first wave need help"
    assert helped[0].sum() == 0 and helped[3, 1] and helped[40, 1]     # a lane that never needs help; the two far lanes in one frame


# ---- GPU sweep ------------------------------------------------------------------------------------------------------------------
GUARD_A, GUARD_B, FILL = 0x7FF8DEADBEEF0A0A, 0x7FF8FEEDFACE0B0B, 0x7FF8000000C0FFEE
GUARD_WORDS = 8
LEDGER = set()          # (kernel, search) that ran and matched
WORST = {0: [0.0, 0.0], 1: [0.0, 0.0]}     # per search: worst |du| (points route), worst |dd| / max(1, d) against the oracle
_CACHE = {}


class Guarded(object):
    """A device buffer with NaN-payload guard words before and after the payload the library is handed."""

    def __init__(self, ctx, nbytes, prefill=None):
        self.ctx = ctx
        self.words = (nbytes + 7) // 8
        host = np.full(self.words + 2 * GUARD_WORDS, FILL, dtype=np.uint64)
        host[:GUARD_WORDS] = GUARD_A + np.arange(GUARD_WORDS, dtype=np.uint64)
        host[-GUARD_WORDS:] = GUARD_B + np.arange(GUARD_WORDS, dtype=np.uint64)
        if prefill is not None:
            host[GUARD_WORDS:GUARD_WORDS + self.words] = np.ascontiguousarray(prefill).view(np.uint64).reshape(-1)
        self.buf = ctx.upload(host)
        self.ptr = self.buf.address + 8 * GUARD_WORDS

    def read(self, shape, dtype, tag=""):
        whole = self.ctx.download(self.buf, (self.words + 2 * GUARD_WORDS,), np.uint64)
        assert np.array_equal(whole[:GUARD_WORDS], GUARD_A + np.arange(GUARD_WORDS, dtype=np.uint64)), ("the guard before", tag)
        assert np.array_equal(whole[-GUARD_WORDS:], GUARD_B + np.arange(GUARD_WORDS, dtype=np.uint64)), ("the guard after", tag)
        n = int(np.prod(shape))
        out = whole[GUARD_WORDS:GUARD_WORDS + self.words].view(dtype)[:n].reshape(shape).copy()
        return out

    def free(self):
        self.buf.free()


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _written(a, tag):
    """No element still holds the pattern the payload was filled with (evaluation counts: every one a small positive number)."""
    if a.dtype == np.int32:
        assert ((a > 0) & (a < 100000)).all(), ("evaluation counts the kernel never wrote", tag)
        return
    bad = _bits64(a) == np.uint64(FILL)
    assert not bad.any(), ("elements the kernel never wrote", tag, int(bad.sum()))


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _default_options(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        if c.handle:
            c.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
            c.set_option(_capi.MG_OPT_TRAJECTORY_LANES, 0)


def _set(ctx, search, opt):
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
    ctx.set_option(_capi.MG_OPT_TRAJECTORY_LANES, opt)


def _latents_of(r, n=B_MAX):
    return np.random.default_rng(500 + r["L"] + r["NB"]).standard_normal((n, r["L"]))


def _check_plan(ctx, r, B, search, opt, points=False, total=None):
    want = traj_plan(r["L"], r["rows"], r["n_seg"], B, total, points, search, opt)
    got = ctx.trajectory_plan(r["L"], r["rows"], r["n_seg"], B, total, points)
    assert got == want, (r["name"], B, search, opt, points, got, want)
    return want


def _score_root(ctx, prim, traj, S, grid, T, min_u, al, tag, prefill=None):
    """mg_score_trajectory on guarded buffers; prefill: accumulate onto it, then run again without and check the overwrite."""
    B = len(S)
    d_S = ctx.upload(S)
    e, r = Guarded(ctx, B * 8, prefill), Guarded(ctx, B * T * 8)
    try:
        prim.score_trajectory_dev(traj, d_S, S.dtype, B, S.shape[1], e.ptr, min_u, WEIGHT, al, prefill is not None, r.ptr, grid)
        err, res = e.read((B,), np.float64, tag), r.read((B, T), np.float64, tag)
        _written(err, tag)
        _written(res, tag)
        if prefill is not None:
            prim.score_trajectory_dev(traj, d_S, S.dtype, B, S.shape[1], e.ptr, min_u, WEIGHT, al, False, None, grid)
            plain = e.read((B,), np.float64, tag)
            np.testing.assert_array_equal(_bits64(err), _bits64(prefill + plain), err_msg="accumulate %s" % (tag,))
            err = plain
        return err, res
    finally:
        for b in (d_S, e, r):
            b.free()


def _score_points(ctx, prim, traj, P, min_u, tag, search, prefill=None):
    """mg_score_trajectory_points and mg_trajectory_closest_points on guarded buffers: (errors, residuals, parameters, evaluations)."""
    B, T = P.shape[:2]
    lib = prim.lib
    d_P = ctx.upload(P)
    e, r, u, d, n = (Guarded(ctx, B * 8, prefill), Guarded(ctx, B * T * 8), Guarded(ctx, B * T * 8), Guarded(ctx, B * T * 8),
                     Guarded(ctx, B * T * 4))
    try:
        _capi._check(lib.mg_score_trajectory_points(prim.handle, traj.handle, d_P.ptr, B, T, float(min_u), WEIGHT, e.ptr,
                                                    1 if prefill is not None else 0, r.ptr))
        err, res = e.read((B,), np.float64, tag), r.read((B, T), np.float64, tag)
        if prefill is not None:
            _capi._check(lib.mg_score_trajectory_points(prim.handle, traj.handle, d_P.ptr, B, T, float(min_u), WEIGHT, e.ptr, 0, None))
            plain = e.read((B,), np.float64, tag)
            np.testing.assert_array_equal(_bits64(err), _bits64(prefill + plain), err_msg="accumulate %s" % (tag,))
            err = plain
        _capi._check(lib.mg_trajectory_closest_points(prim.handle, traj.handle, d_P.ptr, B, T, float(min_u), u.ptr, d.ptr, n.ptr if search == 0 else None))
        us, ds = u.read((B, T), np.float64, tag), d.read((B, T), np.float64, tag)
        ns = n.read((B, T), np.int32, tag)
        for a in (err, res, us, ds) + ((ns,) if search == 0 else ()):
            _written(a, tag)
        np.testing.assert_array_equal(_bits64(res), _bits64(WEIGHT * ds), err_msg=str(tag))
        return err, res, us, ns
    finally:
        for b in (d_P, e, r, u, d, n):
            b.free()


def _hold_to_oracle(r, op, cps, S, mode, min_u, times, search, res, us=None, path_of=None, tag=""):
    """Candidates 0, 63, 64 and B - 1 against the chained oracle search over the oracle's own root paths."""
    for b in ORACLE_CANDS:
        path = path_of(b) if path_of is not None else _oracle_path(op, S[b], mode, times)
        u_ref, d_ref = _oracle_chain(cps, path, min_u, search)
        d_dev = res[b] / WEIGHT
        if search == 1:
            WORST[1][1] = max(WORST[1][1], float((np.abs(d_dev - d_ref) / np.maximum(1.0, d_ref)).max()))
            np.testing.assert_allclose(d_dev, d_ref, rtol=WALK_TOL, atol=WALK_TOL, err_msg="%s candidate %d" % (tag, b))
            if us is not None:
                WORST[1][0] = max(WORST[1][0], float(np.abs(us[b] - u_ref).max()))
                np.testing.assert_allclose(us[b], u_ref, rtol=WALK_TOL, atol=WALK_TOL, err_msg="%s candidate %d" % (tag, b))
        else:
            dd = np.abs(d_dev - d_ref) / np.maximum(1.0, d_ref)
            WORST[0][1] = max(WORST[0][1], float(dd.max()))
            assert dd.max() <= D_TOL, (tag, b, float(dd.max()))
            if us is not None:
                WORST[0][0] = max(WORST[0][0], float(np.abs(us[b] - u_ref).max()))
                assert np.abs(us[b] - u_ref).max() <= U_TOL, (tag, b, float(np.abs(us[b] - u_ref).max()))


def _twin_with_identity_quaternion(r):
    """The D = 7 primitive with the row's root rows and the quaternion rows mean (1, 0, 0, 0), zero eigenvectors."""
    data = _model(r)
    L, NB, D = r["L"], r["NB"], r["D"]
    mean = np.array(data["mean_spatial_vector"]).reshape(NB, D)
    eig = np.array(data["eigen_vectors_spatial"]).reshape(L, NB, D)
    mean7, eig7 = np.zeros((NB, 7)), np.zeros((L, NB, 7))
    mean7[:, :3], eig7[:, :, :3] = mean[:, :3], eig[:, :, :3]
    mean7[:, 3] = 1.0
    twin = dict(data, n_dim_spatial=7, mean_spatial_vector=mean7.reshape(-1).tolist(), eigen_vectors_spatial=eig7.reshape(L, -1).tolist(),
                animated_joints=["joint_0"])
    return twin


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_IDS)
def test_every_route_returns_the_same_bits_and_the_oracles_numbers(ctx, name):
    """One row of the table through mg_score_trajectory, mg_score_trajectory_points and mg_trajectory_closest_points: both searches,
    every lane option, every configuration, every tail batch size."""
    r = BY_NAME[name]
    data = _model(r)
    op = orc.OraclePrimitive(data)
    cps = _cps_of(r)
    S_all = _latents_of(r)
    prim = _capi.Primitive(ctx, data)
    traj = _capi.Trajectory(prim, cps, granularity=1000)
    twin = twin_traj = None
    if r["D"] < 7:
        twin = _capi.Primitive(ctx, _twin_with_identity_quaternion(r))
        twin_traj = _capi.Trajectory(twin, cps, granularity=1000)
    grids = {k: (prim.time_grid(t), t) for k, t in _grids(r).items()}
    rng = np.random.default_rng(31)
    try:
        for ci, (dtype, mode, min_u, gname) in enumerate(CONFIGS):
            grid, times = grids[gname]
            T = len(times)
            S = S_all.astype(dtype)
            S64 = S.astype(np.float64)
            al = _alignment(mode)
            for search in (0, 1):
                base = None
                for opt in _lane_options(search):
                    _set(ctx, search, opt)
                    for B in BATCHES[::-1]:
                        tag = (name, ci, search, opt, B)
                        plan = _check_plan(ctx, r, B, search, opt)
                        pre = rng.standard_normal(B) if B in (65, 9) else None
                        err, res = _score_root(ctx, prim, traj, S[:B], grid, T, min_u, al, tag, pre)
                        if base is None:
                            base = (err, res)
                            np.testing.assert_allclose(err, res.mean(axis=1), rtol=1e-13, atol=1e-13)
                        np.testing.assert_array_equal(_bits64(err), _bits64(base[0][:B]), err_msg=str(tag))
                        np.testing.assert_array_equal(_bits64(res), _bits64(base[1][:B]), err_msg=str(tag))
                        LEDGER.add((plan["kernel"], search))
                if twin is not None and mode == 1:
                    # no root quaternion: the identity -- the same bits as a primitive that carries the identity in its rows
                    _set(ctx, search, 0)
                    tgrid = twin.time_grid(times)
                    e7, r7 = _score_root(ctx, twin, twin_traj, S, tgrid, T, min_u, al, (name, "twin", ci, search))
                    tgrid.close()
                    np.testing.assert_array_equal(_bits64(base[0]), _bits64(e7))
                    np.testing.assert_array_equal(_bits64(base[1]), _bits64(r7))
                elif ci < r["oracle_configs"] or (twin is not None and mode != 1):
                    _hold_to_oracle(r, op, cps, S64, mode, min_u, times, search, base[1], tag=(name, ci, search))
                if mode != 0:
                    continue
                # the points route, fed with the positions of the root route: the same bits
                P = prim.back_project_frames_f64(S, grid=grid)[:, :, :3].copy()
                pbase = None
                for opt in _lane_options(search):
                    _set(ctx, search, opt)
                    for B in BATCHES[::-1]:
                        tag = (name, "points", ci, search, opt, B)
                        plan = _check_plan(ctx, r, B, search, opt, points=True)
                        pre = rng.standard_normal(B) if B in (65, 9) else None
                        out = _score_points(ctx, prim, traj, P[:B], min_u, tag, search, pre)
                        if pbase is None:
                            pbase = out
                        for a, b in zip(out, pbase):
                            np.testing.assert_array_equal(a, b[:B], err_msg=str(tag))
                        LEDGER.add((plan["kernel"], search))
                np.testing.assert_array_equal(_bits64(pbase[1]), _bits64(base[1]), err_msg="points against root rows %s" % ((name, ci, search),))
                np.testing.assert_array_equal(_bits64(pbase[0]), _bits64(base[0]), err_msg="points against root rows %s" % ((name, ci, search),))
                if ci < r["oracle_configs"]:
                    _hold_to_oracle(r, op, cps, S64, mode, min_u, times, search, pbase[1], us=pbase[2], path_of=lambda b: P[b],
                                    tag=(name, "points", ci, search))
    finally:
        for g, _ in grids.values():
            g.close()
        for h in (traj, prim, twin_traj, twin):
            if h is not None:
                h.close()
    print("%s: worst against the oracle so far: reference search |du| %.2e |dd| %.2e, walk |du| %.2e |dd| %.2e" % (
        name, WORST[0][0], WORST[0][1], WORST[1][0], WORST[1][1]))


@pytest.mark.gpu
def test_shapes_that_fit_no_kernel_are_reported(ctx):
    """(L + rows) * 512 > 150 KB: MG_ERR_UNSUPPORTED from the plan and from the launch, with the launch's message, under every option;
    the smallest such L at NB = 7, and the row whose rows would fit the cooperative and the streaming kernels."""
    L = _unsupported_L()
    for r in [_row("unsupported", L, UNSUPPORTED_NB, 7, 7)] + ROWS_REFUSED:
        prim = _capi.Primitive(ctx, _model(r))
        traj = _capi.Trajectory(prim, _cps_of(r), granularity=1000)
        S = np.zeros((16, r["L"]))
        try:
            for search in (0, 1):
                for opt in _lane_options(search):
                    _set(ctx, search, opt)
                    assert traj_plan(r["L"], r["rows"], r["n_seg"], 16, None, False, search, opt) is None
                    with pytest.raises(_capi.MGError) as e:
                        ctx.trajectory_plan(r["L"], r["rows"], r["n_seg"], 16)
                    assert e.value.status == MG_ERR_UNSUPPORTED
                    with pytest.raises(_capi.MGError) as e:
                        prim.score_trajectory(traj, S)
                    assert e.value.status == MG_ERR_UNSUPPORTED
                    assert "%d basis functions x %d components do not fit LDS" % (r["NB"], r["L"]) in str(e.value)
            # (given points need no rows: the same primitive scores them)
            _set(ctx, 1, 0)
            assert _check_plan(ctx, r, 16, 1, 0, points=True)["kernel"] == "coop8"
        finally:
            traj.close()
            prim.close()


@pytest.mark.gpu
def test_wave_help_rounds_against_the_oracle(ctx):
    """The one-lane walk's WAVE_HELP rounds (and the cooperative windows on the same tracks) against closest_point_walk itself."""
    cps, tracks = _help_tracks()
    r = BY_NAME["tiny"]
    prim = _capi.Primitive(ctx, _model(r))
    traj = _capi.Trajectory(prim, cps, granularity=HELP_G)
    rr = dict(r, n_seg=len(cps) - 1)
    try:
        outs = []
        for opt in (1, 8, 4):
            _set(ctx, 1, opt)
            plan = _check_plan(ctx, rr, HELP_B, 1, opt, points=True)
            assert plan["kernel"] == {1: "staged_lds", 8: "coop8", 4: "coop4"}[opt]
            outs.append(_score_points(ctx, prim, traj, tracks, 0.0, ("help", opt), 1))
            LEDGER.add((plan["kernel"], 1))
        for o in outs[1:]:
            for a, b in zip(o, outs[0]):
                np.testing.assert_array_equal(a, b)
        for b in list(HELP_FAR) + [0, 63, 64, 69]:
            u_ref, d_ref = _oracle_chain(cps, tracks[b], 0.0, 1)
            np.testing.assert_allclose(outs[0][2][b], u_ref, rtol=WALK_TOL, atol=WALK_TOL, err_msg="lane %d" % b)
            np.testing.assert_allclose(outs[0][1][b] / WEIGHT, d_ref, rtol=WALK_TOL, atol=WALK_TOL, err_msg="lane %d" % b)
            WORST[1][0] = max(WORST[1][0], float(np.abs(outs[0][2][b] - u_ref).max()))
    finally:
        traj.close()
        prim.close()


def _multi(ctx, prims, trajs, Ss, B, min_us, als, accumulate_onto=None):
    """mg_score_trajectories on guarded buffers: one (B,) error vector per scorer."""
    n = len(prims)
    d_S = [ctx.upload(S[:B]) for S in Ss]
    es = [Guarded(ctx, B * 8, None if accumulate_onto is None else accumulate_onto[k][:B]) for k in range(n)]
    try:
        _capi.Primitive.score_trajectories_dev(prims, trajs, d_S, Ss[0].dtype, B, [S.shape[1] for S in Ss], [e.ptr for e in es], min_us,
                                               [WEIGHT] * n, als, accumulate_onto is not None)
        out = [e.read((B,), np.float64, ("multi", k, B)) for k, e in enumerate(es)]
        for o in out:
            _written(o, "multi")
        return out
    finally:
        for b in d_S + es:
            b.free()


@pytest.mark.gpu
def test_side_by_side_launches_equal_single_launches(ctx):
    """mg_score_trajectories with three scorers of different shapes: the three side-by-side kernels, with and without accumulation,
    and the fall-back to single launches when one scorer's spline is too long -- the bits of mg_score_trajectory every time."""
    names = ("stream_last_width", "no_quaternion_D3", "tiny")
    rs = [BY_NAME[n] for n in names]
    prims = [_capi.Primitive(ctx, _model(r)) for r in rs]
    trajs = [_capi.Trajectory(p, _cps_of(r), granularity=1000) for p, r in zip(prims, rs)]
    long_traj = _capi.Trajectory(prims[2], _control_points(641), granularity=1000)
    als = [_alignment(1), _alignment(2), None]
    min_us = [0.0, 0.37, 0.1]
    rng = np.random.default_rng(5)
    try:
        for dtype in (np.float64, np.float32):
            Ss = [_latents_of(r).astype(dtype) for r in rs]
            for search in (0, 1):
                for opt in _lane_options(search):
                    _set(ctx, search, opt)
                    for B in (130, 65, 7):
                        singles = [p.score_trajectory(t, S[:B], min_u=m, weight=WEIGHT, alignment=a) for p, t, S, m, a in zip(prims, trajs, Ss, min_us, als)]
                        plans = [_check_plan(ctx, r, B, search, opt, total=3 * B) for r in rs]
                        assert all(p["together"] for p in plans) and len({p["kernel"] for p in plans}) == 1
                        got = _multi(ctx, prims, trajs, Ss, B, min_us, als)
                        pre = [rng.standard_normal(B) for _ in rs]
                        acc = _multi(ctx, prims, trajs, Ss, B, min_us, als, pre)
                        for k in range(3):
                            np.testing.assert_array_equal(_bits64(got[k]), _bits64(singles[k]), err_msg=str((search, opt, B, k)))
                            np.testing.assert_array_equal(_bits64(acc[k]), _bits64(pre[k] + singles[k]), err_msg=str((search, opt, B, k)))
                        LEDGER.add((plans[0]["kernel"], search))
                    # one long spline among the scorers: every scorer through single launches
                    B = 65
                    trajs2 = trajs[:2] + [long_traj]
                    plan_long = _check_plan(ctx, dict(rs[2], n_seg=640), B, search, opt, total=3 * B)
                    assert not plan_long["together"] and plan_long["kernel"] == "staged_lds"
                    singles = [p.score_trajectory(t, S[:B], min_u=m, weight=WEIGHT, alignment=a) for p, t, S, m, a in zip(prims, trajs2, Ss, min_us, als)]
                    got = _multi(ctx, prims, trajs2, Ss, B, min_us, als)
                    for k in range(3):
                        np.testing.assert_array_equal(_bits64(got[k]), _bits64(singles[k]), err_msg=str(("not together", search, opt, k)))
    finally:
        for h in trajs + [long_traj] + prims:
            h.close()


@pytest.mark.gpu
def test_more_than_65536_candidates_take_one_lane():
    """B = 65 537 on the walk with eight lanes forced: the plan reports one lane; rows 0, 65 535 and 65 536 are the bits of a launch
    of those three rows."""
    c = _capi.Context(0)
    r = BY_NAME["tiny"]
    prim = _capi.Primitive(c, _model(r))
    traj = _capi.Trajectory(prim, _cps_of(r), granularity=1000)
    try:
        _set(c, 1, 8)
        B = MG_TRAJ_COOP_MAX_B + 1
        plan = _check_plan(c, r, B, 1, 8)
        assert plan["lanes"] == 1 and plan["kernel"] == "stream"
        assert _check_plan(c, r, B - 1, 1, 8)["kernel"] == "coop8"
        S = np.random.default_rng(3).standard_normal((B, r["L"]))
        T = prim.n_canonical_frames
        err, res = _score_root(c, prim, traj, S, None, T, 0.0, None, "65537")
        pick = [0, B - 2, B - 1]
        e3, r3 = _score_root(c, prim, traj, S[pick], None, T, 0.0, None, "three rows")
        np.testing.assert_array_equal(_bits64(err[pick]), _bits64(e3))
        np.testing.assert_array_equal(_bits64(res[pick]), _bits64(r3))
        LEDGER.add((plan["kernel"], 1))
    finally:
        traj.close()
        prim.close()
        c.close()


@pytest.mark.gpu
def test_the_path_scratch_grows_and_is_shared_out_per_scorer():
    """The reference's search in the streaming kernels writes the candidates' root paths to the context's scratch first: 64
    candidates, then 4608 at 156 frames (above the first 16 MiB: synchronise, free, reallocate), then 64 again -- each the bits of
    the same rows scored 512 at a time on a fresh context; and three scorers of 2048 side by side, each with its own block."""
    data = synthetic.make_path_following_primitive(seed=0)
    rows, L = 3 * 31 + 4, 40
    S = np.random.default_rng(21).standard_normal((4608, L))
    cps3 = [_control_points(7), _control_points(5) + [0.0, 1.0, 2.0], _control_points(9) - [1.0, 0.0, 3.0]]

    def chunks(prim, traj, S, min_u):
        return np.concatenate([prim.score_trajectory(traj, S[i:i + 512], min_u=min_u, weight=WEIGHT) for i in range(0, len(S), 512)])
    c1, c2 = _capi.Context(0), _capi.Context(0)
    p1, p2 = _capi.Primitive(c1, data), _capi.Primitive(c2, data)
    t1, t2 = [_capi.Trajectory(p1, c, 1000) for c in cps3], [_capi.Trajectory(p2, c, 1000) for c in cps3]
    try:
        want = chunks(p2, t2[0], S, 0.0)
        for B in (64, 4608, 64):
            plan = c1.trajectory_plan(L, rows, 6, B)
            assert plan == traj_plan(L, rows, 6, B) and plan["kernel"] == "stream" and plan["needs_paths"]
            assert (B * 156 * 24 > (16 << 20)) == (B == 4608)
            err = p1.score_trajectory(t1[0], S[:B], weight=WEIGHT)
            np.testing.assert_array_equal(_bits64(err), _bits64(want[:B]), err_msg="B = %d" % B)
        LEDGER.add(("stream", 0))
        B = 2048
        c3 = _capi.Context(0)
        p3 = _capi.Primitive(c3, data)
        t3 = [_capi.Trajectory(p3, c, 1000) for c in cps3]
        try:
            Ss = [S[:B], S[B:2 * B], S[1000:1000 + B]]
            min_us = [0.0, 0.2, 0.0]
            plans = [c3.trajectory_plan(L, rows, len(c) - 1, B, 3 * B) for c in cps3]
            assert all(p == traj_plan(L, rows, len(c) - 1, B, 3 * B) for p, c in zip(plans, cps3))
            assert all(p["kernel"] == "stream_multi" and p["needs_paths"] and p["together"] for p in plans) and 3 * B * 156 * 24 > (16 << 20)
            got = _multi(c3, [p3] * 3, t3, Ss, B, min_us, None)
            for k in range(3):
                np.testing.assert_array_equal(_bits64(got[k]), _bits64(chunks(p2, t2[k], Ss[k], min_us[k])), err_msg="scorer %d" % k)
            LEDGER.add(("stream_multi", 0))
        finally:
            for h in t3 + [p3, c3]:
                h.close()
    finally:
        for h in t1 + t2 + [p1, p2, c1, c2]:
            h.close()


@pytest.mark.gpu
def test_the_ledger_covers_every_kernel():
    """Runs last: every kernel, for every search that can reach it, was launched by the sweep above and matched."""
    missing = _reachable() - LEDGER
    assert not missing, sorted(missing)
    print("worst deviation from the oracle: reference search |du| %.3e (tolerance %.1e), |dd| / max(1, d) %.3e (%.1e); "
          "walk |du| %.3e, |dd| / max(1, d) %.3e (%.1e)" % (WORST[0][0], U_TOL, WORST[0][1], D_TOL, WORST[1][0], WORST[1][1], WALK_TOL))
