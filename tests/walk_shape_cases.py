"""The graph-walk kernels' host decisions restated, and the table of shapes on both sides of every one of them.

Shared by tests/test_walk_shapes_host.py (no device: the restatements against the C text, the table against the restatements, the
host statement against the oracle on every row) and tests/test_gpu_walk_shapes.py (the same rows on the device, with a ledger of the
routes they took).

walk_frames_plan restates mg_walk_frames (csrc/mg_walk.hip), walk_score_plan mg_score_walk_residuals_steps (csrc/mg_walk_score.hip),
walk_time_plan mg_score_walk_time (csrc/mg_walk_time.hip).  FRAME_ROWS is the frames kernels' table: every row names the routes it
exists for, and the CPU companion asserts from the plan that it takes them.
"""
import copy

import numpy as np

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
from oracle import mg_oracle as orc

MG_ERR_INVALID_ARGUMENT = _capi.MG_ERR_INVALID_ARGUMENT
MG_ERR_UNSUPPORTED = _capi.MG_ERR_UNSUPPORTED

# ---- constants of the three files (pinned by test_restatements_match_the_source) ---------------------------------------------------
MG_MAX_CHAIN = 32
MG_MAX_KK = 16
MG_WALK_MAX_STEPS = 64
MG_WALK_TILE = 32
MG_WALK_BLOCK = 256
MG_WALK_CHAIN_BLOCK = 64
MG_WALK_LDS_MAX = 160 * 1024 - 64
MG_WSCORE_LDS_MAX = 150 * 1024
MG_WTIME_LDS_MAX = 150 * 1024
MG_WTIME_CHUNK = 64
MG_WTIME_BS = MG_WTIME_CHUNK + 1
KB64 = 64 * 1024


def k_steps(width):
    """mg_primitive_create: the even number of 4-wide k-steps that hold `width` columns, 0 past 64 (p->KK of L, p->KKg of Lg)."""
    return (((width + 3) // 4 + 1) // 2) * 2 if width <= 4 * MG_MAX_KK else 0


class Refused(Exception):
    def __init__(self, status, why):
        Exception.__init__(self, why)
        self.status = status


# ---- mg_walk_frames -------------------------------------------------------------------------------------------------------------
def walk_frames_plan(steps, D, first_aligned=False, start_pose=False, joint=0, skeleton=None, t_cap=None):
    """steps: (L, NB, T) per step; first_aligned: an alignment record is given; start_pose: it is a start pose; joint: the record's
    node; skeleton: None or (parents, quat_channel).  Raises Refused with the status the library answers."""
    lmax = max(L for L, _, _ in steps)
    rmax = max(NB * D for _, NB, _ in steps)
    n_steps = len(steps)
    if not (1 <= n_steps <= MG_WALK_MAX_STEPS):
        raise Refused(MG_ERR_INVALID_ARGUMENT, "steps")
    aligned_any = n_steps > 1 or first_aligned
    if not (D >= 3 and (not aligned_any or D >= 7)):
        raise Refused(MG_ERR_INVALID_ARGUMENT, "no root channels to align")
    if not first_aligned or start_pose:
        joint = 0
    link = []
    if not aligned_any:
        pass
    elif joint == 0 and skeleton is None:
        link = [3]
    else:
        if skeleton is None:
            raise Refused(MG_ERR_INVALID_ARGUMENT, "a skeleton is needed")
        parents, quat_channel = skeleton
        chain, j = [], joint
        while j >= 0:
            chain.insert(0, j)
            j = int(parents[j])
        for j in chain:
            qc = int(quat_channel[j])
            if qc < 0:
                continue
            if not (qc + 4 <= D and len(link) < MG_MAX_CHAIN):
                raise Refused(MG_ERR_INVALID_ARGUMENT, "the aligning chain does not fit")
            link.append(qc)
    n_link = len(link)
    lds_f = (rmax + lmax + MG_WALK_TILE * 4) * 8 + MG_WALK_TILE * 4
    lds_c = (lmax + 5 * (3 + 4 * n_link) + 4) * 8 + 16
    if not lds_f <= MG_WALK_LDS_MAX:
        raise Refused(MG_ERR_UNSUPPORTED, "do not fit LDS")
    tiles = sum(((t_cap if t_cap is not None else T) + MG_WALK_TILE - 1) // MG_WALK_TILE for _, _, T in steps)
    nch = 3 + 4 * n_link
    return dict(n_link=n_link, link=link, lmax=lmax, rmax=rmax, tiles_per_walk=tiles, lds_f=lds_f, lds_c=lds_c, opt_in=True,
                chain_passes=(5 * nch + MG_WALK_CHAIN_BLOCK - 1) // MG_WALK_CHAIN_BLOCK)


# ---- mg_score_walk_residuals_steps ------------------------------------------------------------------------------------------------
def walk_score_plan(steps, force_valu=False):
    """steps: per step (L, [(n constraints, RT or None for a set without packed matrix), ...] the step's one or two sets)."""
    rtmax, nmax, xs, per_step = 0, 1, 0, []
    for L, sets in steps:
        routes = []
        for n, RT in sets:
            if n == 0:
                continue
            packed = RT is not None and not force_valu
            if packed:
                rtmax = max(rtmax, RT)
            else:
                xs = max(xs, L + 1)
            nmax = max(nmax, n)
            routes.append("packed" if packed else "staged")
        per_step.append(dict(KK=k_steps(L), routes=routes))
    vs = rtmax * 16 + 1
    lds = 4 * (16 * vs + nmax * 16 + 64 + 16 * xs) * 8
    if not lds <= MG_WSCORE_LDS_MAX:
        raise Refused(MG_ERR_UNSUPPORTED, "do not fit LDS")
    return dict(steps=per_step, vs=vs, nmax=nmax, xs=xs, lds=lds, opt_in=lds > KB64)


# ---- mg_score_walk_time -----------------------------------------------------------------------------------------------------------
def walk_time_plan(steps, n_constraints):
    """steps: (F, L, Lt, K) per step."""
    kmax, per_step = 1, []
    for F, L, Lt, K in steps:
        Lg = L + Lt
        KKg = k_steps(Lg)
        if K <= 0 or KKg < 2 or KKg > MG_MAX_KK or (KKg & 1) or K * 16 * 16 > 60 * 1024:
            raise Refused(MG_ERR_UNSUPPORTED, "no in-kernel form of this mixture")
        per_step.append(dict(KKg=KKg, JT=(Lg + 15) // 16, chunks=(F + MG_WTIME_CHUNK - 1) // MG_WTIME_CHUNK if Lt > 0 else 0,
                             gamma_from_memory=Lt > 16))
        kmax = max(kmax, K)
    wave_doubles = max(16 * MG_WTIME_BS, 2 * kmax * 16)
    lds = (48 * len(steps) + 16 * n_constraints + 4 * wave_doubles) * 8
    if lds > MG_WTIME_LDS_MAX:
        raise Refused(MG_ERR_UNSUPPORTED, "do not fit LDS")
    return dict(steps=per_step, wave_doubles=wave_doubles, lds=lds, opt_in=lds > KB64, units=2 * len(steps))


# ---- the frames kernels' table ----------------------------------------------------------------------------------------------------
START_POSE = {"position": [35.0, 7.0, -12.0], "orientation": [0.0, 40.0, 0.0]}
OBLIQUE = (0.48, 0.6, 0.64)            # a unit vector: 0.2304 + 0.36 + 0.4096 = 1
N_DEEP = 9                             # Hips .. LeftHand of synthetic.make_skeleton: its deepest chain, seven animated joints
SMALL = [(5, 12, 7), (8, 33, 9), (3, 20, 6)]      # (n_components, n_canonical_frames, n_basis)
# the largest control-point block that fits MG_WALK_LDS_MAX: rmax + lmax = 20328 = 100 * 203 + 28 (a wide pose rather than many
# basis functions: knots much closer than a frame make the grid's last sample, one frame past the last knot, astronomically large)
LDS_NB, LDS_D, LDS_L, LDS_F = 100, 203, 28, 130
PARITY_STRIDE = 70                     # rows per walk of the "parities" row: even, so the walks' parities are their offsets'


def _row(name, D, routes, shapes=SMALL, sequence=(0, 1), kind="previous", node="Hips", ref_dir=(0.0, 0.0, 1.0), skel=None, n_walks=2,
         dtype=np.float64, offsets=None, expect=None, seed=None):
    return dict(name=name, D=D, routes=set(routes), shapes=list(shapes), sequence=list(sequence), kind=kind, node=node, ref_dir=tuple(ref_dir),
                skel=skel if skel is not None else ("humanoid", max(1, (D - 3) // 4)), n_walks=n_walks, dtype=dtype, offsets=offsets, expect=expect,
                seed=seed)


def _frame_rows():
    rows = []
    for D in (3, 4, 6):                  # one unaligned step: the chain kernel reads the root translation alone
        rows.append(_row("single_D%d" % D, D, {"chain:no_links", "frames:unaligned", "D:%d" % D}, sequence=(1,), kind="none", n_walks=3))
    walks, dtypes = (1, 2, 5), (np.float64, np.float32)
    i = 0
    for D in (7, 8, 11, 12, 15):
        for n_steps in (2, 3):
            for kind in ("previous", "start_pose", "none"):
                node = "Spine" if (kind == "previous" and D >= 11) else "Hips"
                dt = dtypes[i % 2]
                routes = {"D:%d" % D, "mode:%s" % kind, "steps:%d" % n_steps, "walks:%d" % walks[i % 3], "lat:%s" % np.dtype(dt).name, "chain:one_pass"}
                routes.add("frames:even_D" if D % 2 == 0 else "frames:odd_D")
                if D == 7:
                    routes.add("frames:root_is_the_whole_row")
                rows.append(_row("D%d_%dsteps_%s" % (D, n_steps, kind), D, routes, sequence=(0, 1, 2)[:n_steps], kind=kind, node=node,
                                 n_walks=walks[i % 3], dtype=dt))
                i += 1
    D = 3 + 4 * N_DEEP
    for node, depth in (("Hips", 1), ("Spine", 2), ("Spine1", 3), ("Neck", 4), ("LeftHand", 7)):
        routes = {"chain:depth_%d" % depth, "chain:one_pass" if depth <= 2 else "chain:more_passes"}
        rows.append(_row("chain_depth_%d" % depth, D, routes, node=node, skel=("humanoid", N_DEEP), seed=8700 if depth == 3 else None))
    rows.append(_row("chain_max", 3 + 4 * MG_MAX_CHAIN, {"chain:max_links", "chain:more_passes"}, node="j%d" % (MG_MAX_CHAIN - 1), skel=("line", MG_MAX_CHAIN),
                     n_walks=1, seed=9760))
    rows.append(_row("chain_one_more", 3 + 4 * (MG_MAX_CHAIN + 1), {"refused:chain"}, node="j%d" % MG_MAX_CHAIN, skel=("line", MG_MAX_CHAIN + 1), n_walks=1,
                     expect=MG_ERR_INVALID_ARGUMENT))
    rows.append(_row("chain_unanimated_joint", 11, {"chain:unanimated_joint", "chain:one_pass"}, node="Spine", skel=("gap",), seed=8800))
    rows.append(_row("ref_dir_x", 11, {"ref_dir:x"}, node="Spine", ref_dir=(1.0, 0.0, 0.0), sequence=(0, 1, 2)))
    rows.append(_row("ref_dir_oblique", 11, {"ref_dir:oblique"}, node="Spine", ref_dir=OBLIQUE, sequence=(0, 1, 2), dtype=np.float32))
    rows.append(_row("pitches", 11, {"frames:below_lmax_rmax"}, shapes=[(1, 12, 4), (64, 40, 12)], sequence=(0, 1, 0), seed=8860))
    # odd n_dim, 33 frames (two tiles): the walks' rows start on even and on odd doubles for every (step, tile)
    rows.append(_row("parities", 11, {"frames:both_parities"}, shapes=[(8, 33, 9), (5, 33, 7)], sequence=(0, 1), n_walks=2,
                     offsets=[[0, 34], [1, 35]]))
    rows.append(_row("lds_largest", LDS_D, {"frames:lds_largest"}, shapes=[(LDS_L, LDS_F, LDS_NB)], sequence=(0,), kind="start_pose", n_walks=2))
    rows.append(_row("lds_one_more", LDS_D, {"refused:lds"}, shapes=[(LDS_L + 1, LDS_F, LDS_NB)], sequence=(0,), kind="start_pose", n_walks=2,
                     expect=MG_ERR_UNSUPPORTED))
    # (seeds given above: the first of seed + 1000, seed + 2000, ... at which the row meets the CPU companion's two input conditions)
    for k, r in enumerate(rows):
        if r["seed"] is None:
            r["seed"] = 7000 + 20 * k          # the row's primitives take seed, seed + 1, ...; its latents seed + 10; its previous frame seed + 11
    return rows


FRAME_ROWS = _frame_rows()
FRAME_IDS = [r["name"] for r in FRAME_ROWS]
FRAME_BY_NAME = {r["name"]: r for r in FRAME_ROWS}
FRAME_ROUTES = set().union(*[r["routes"] for r in FRAME_ROWS])


def skeleton_of(row):
    """(joints, animated) of a row."""
    kind = row["skel"][0]
    if kind == "humanoid":
        return synthetic.make_skeleton(row["skel"][1])
    if kind == "line":                   # a purpose-built chain: every joint animated, one below the other
        n = row["skel"][1]
        joints = [("j%d" % i, None if i == 0 else "j%d" % (i - 1), (0.0, 0.0 if i == 0 else 3.0, 0.0)) for i in range(n)]
        return joints, [j[0] for j in joints]
    # a joint without channels between the root and the aligning node
    return [("Hips", None, (0.0, 0.0, 0.0)), ("Mid", "Hips", (0.0, 5.0, 0.0)), ("Spine", "Mid", (0.0, 6.0, 0.5))], ["Hips", "Spine"]


def frame_models(row):
    """The row's primitives (JSON dicts), each from its own seed."""
    return [synthetic.make_primitive(seed=row["seed"] + i, n_components=L, n_frames=F, n_basis=NB, n_dim=row["D"], n_gmm=1, name="%s_%d" % (row["name"], i))
            for i, (L, F, NB) in enumerate(row["shapes"])]


def frame_case(row, models=None):
    """(models, steps' models, S float64 (n_walks, sum L), alignment record or None, _capi.Skeleton or None, (joints, animated), previous frame or None)."""
    models = frame_models(row) if models is None else models
    joints, animated = skeleton_of(row)
    steps = [models[k] for k in row["sequence"]]
    rng = np.random.default_rng(row["seed"] + 10)
    S = 0.7 * rng.standard_normal((row["n_walks"], sum(row["shapes"][k][0] for k in row["sequence"])))
    if row["dtype"] == np.float32:
        S = S.astype(np.float32).astype(np.float64)        # the values a float32 batch holds
    prev, alignment, hip_sk = None, None, None
    if row["D"] >= 7:
        hip_sk = _capi.Skeleton(joints, animated)
    if row["kind"] == "previous":
        prng = np.random.default_rng(row["seed"] + 11)
        prev = orc.OraclePrimitive(models[-1]).back_project_frames(prng.standard_normal(row["shapes"][len(models) - 1][0]))[-1].copy()
        prev[0] += 120.0
        prev[2] -= 40.0
        alignment = hip_sk.alignment_to(prev, row["node"], row["ref_dir"])
    elif row["kind"] == "start_pose":
        alignment = alignment_from_start_pose(START_POSE)
    needs_sk = row["kind"] == "previous" and row["node"] != joints[0][0]
    return models, steps, S, alignment, (hip_sk if needs_sk else None), (joints, animated), prev


def frame_plan(row):
    """walk_frames_plan of the row as the sweep calls the library."""
    joints, animated = skeleton_of(row)
    steps = [(row["shapes"][k][0], row["shapes"][k][2], row["shapes"][k][1]) for k in row["sequence"]]
    previous = row["kind"] == "previous"
    sk = None
    if previous and row["node"] != joints[0][0]:
        s = _capi.Skeleton(joints, animated)
        sk = (s.parents, s.quat_channel)
    names = [j[0] for j in joints]
    return walk_frames_plan(steps, row["D"], row["kind"] != "none", row["kind"] == "start_pose", names.index(row["node"]) if previous else 0, sk)


def oracle_walk(steps, row_latents, kind, node, skel, prev, ref_dir=(0.0, 0.0, 1.0)):
    """The oracle's control-point chain for one walk (tests/test_graph_walk_host.py's, with the record's reference vector):
    (frames, smallest xz norm of any heading before normalisation, widest turn).  The turn of a step is the oracle's phi, the
    difference of two atan2 values in (-2 pi, 2 pi), of which it takes the half angle as it stands; the host statement and the
    device take the half angle from (cos phi, sin phi), i.e. of phi wrapped into (-pi, pi].  Past pi the two root quaternions are q
    and -q: the same rotation, other numbers.  The rows keep |phi| below pi, and the CPU companion asserts it."""
    joints, animated = skel
    parts, off, least, widest = [], 0, np.inf, 0.0
    start_pose = copy.deepcopy(START_POSE)
    ref = np.asarray(ref_dir, dtype=np.float64)

    def xz_norm(pose):
        p = orc.joint_global_orientation(pose, joints, animated, node) @ ref
        return float(np.hypot(p[0], p[2]))
    if prev is not None:
        least = xz_norm(prev)
    for i, data in enumerate(steps):
        op = orc.OraclePrimitive(data)
        coeffs = op.back_project_spatial_coeffs(row_latents[off:off + op.n_components])
        off += op.n_components
        if prev is not None or kind == "previous":
            least = min(least, xz_norm(coeffs[0]))
        if prev is not None:
            ha, hb = (orc.node_heading(p, joints, animated, node, ref_dir) for p in (prev, coeffs[0]))
            widest = max(widest, abs(np.arctan2(hb[1], hb[0]) - np.arctan2(ha[1], ha[0])))
            coeffs = orc.align_coeffs_to_previous_frame(coeffs, prev, joints, animated, node, ref_dir)
        elif i == 0 and kind == "start_pose":
            coeffs = orc.align_coeffs_to_start_pose(coeffs, start_pose)
        fr = orc.spline_frames(op.knots, coeffs, op.canonical_time_function())
        prev = fr[-1]
        if i + 1 < len(steps):
            least = min(least, xz_norm(prev))
        parts.append(fr)
    return np.concatenate(parts), least, widest


def place(frames, offsets, row, stride):
    """assemble_walk_host's walks moved to the row's frame offsets over a NaN sentinel: (n_walks, stride, D)."""
    if row["offsets"] is None:
        out = np.full((frames.shape[0], stride, frames.shape[2]), np.nan)
        out[:, :frames.shape[1]] = frames
        return out
    out = np.full((frames.shape[0], stride, frames.shape[2]), np.nan)
    for w in range(frames.shape[0]):
        for i, at in enumerate(row["offsets"][w]):
            a, b = offsets[w, i], offsets[w, i + 1]
            out[w, at:at + (b - a)] = frames[w, a:b]
    return out


# ---- the time kernel's table ------------------------------------------------------------------------------------------------------
FRAME_TIME = 0.02
TIME_START_KEYFRAME_STEPS = 1          # every window starts at step 1 of its walk: a start keyframe that is no whole number
# name: (n_canonical_frames, n_components, n_time_components, n_gmm): F on both sides of the 64-frame chunk, Lt on both sides of the
# sixteen registers, L + Lt in every case of the KKg switch, K on both sides of wave_doubles' arms
TIME_SHAPES = {"f2": (2, 3, 1, 1), "f63": (63, 9, 3, 2), "f64": (64, 5, 15, 3), "f65": (65, 12, 16, 2), "f128": (128, 20, 17, 32),
               "f129": (129, 25, 20, 33), "lt0": (65, 50, 0, 40), "wide": (20, 60, 3, 2), "k148": (20, 5, 2, 148), "k149": (20, 5, 2, 149)}
TIME_SEEDS = {name: 9100 + 7 * i for i, name in enumerate(sorted(TIME_SHAPES))}
# name: (the window's steps, candidates)
TIME_ROWS = {"w1": (("f2",), 1), "w2": (("f63", "f64"), 15), "w3": (("f65", "lt0", "f128"), 16), "w4": (("f129", "wide", "f2", "f63"), 17),
             "w5": (("f64", "f65", "lt0", "f128", "f129"), 33), "w8": (("f2", "f63", "f64", "f65", "lt0", "wide", "f2", "f63"), 17),
             "w9": (("wide", "f2", "f63", "f64", "f65", "lt0", "f2", "f63", "f64"), 16), "k148": (("k148",), 17), "k149": (("k149",), 17)}
TIME_IDS = sorted(TIME_ROWS)
TIME_REFUSED = {"k149": MG_ERR_UNSUPPORTED}
FIRST_STEP = "f63"                     # the step before every window: its time function's last entry is the start keyframe


def time_model(name):
    F, L, Lt, K = TIME_SHAPES[name]
    return synthetic.make_primitive(seed=TIME_SEEDS[name], name=name, n_components=L, n_frames=F, n_basis=max(4, min(7, F + 2)), n_dim=7, n_gmm=K,
                                    n_time_components=Lt, n_basis_time=(5 if F < 40 else 8) if Lt else None)


def time_constraints_of(window):
    """Every keyframe edge on every step it can sit on: 0, the chunk's last and first frames, F - 1, from the end, at F (no error), two
    on one keyframe; a step beyond the window (10000)."""
    clist = []
    for k, name in enumerate(window):
        F = TIME_SHAPES[name][0]
        for kf in (0, 62, 63, 64, 65, F - 1, -1, -F, F):
            clist.append((k, kf, round(FRAME_TIME * (40.0 * k + (kf % F) + 3.5), 6)))
    last = len(window) - 1
    clist += [(last, min(1, TIME_SHAPES[window[last]][0] - 1), 0.31), (last, min(1, TIME_SHAPES[window[last]][0] - 1), 0.87), (10000, 1, 1.0), (len(window), 0, 1.0)]
    return clist


def time_case(row):
    """(window, n, parameters of the walk's steps (the step before the window first), S (n, the window's time latents), constraints)."""
    window, n = TIME_ROWS[row]
    rng = np.random.default_rng(9500 + TIME_IDS.index(row))
    names = (FIRST_STEP,) + tuple(window)
    params = [0.5 * rng.standard_normal(TIME_SHAPES[k][1] + TIME_SHAPES[k][2]) for k in names]
    S = 0.5 * rng.standard_normal((n, sum(TIME_SHAPES[k][2] for k in window)))
    return window, n, params, S, time_constraints_of(window)


def time_plan(row):
    window, _ = TIME_ROWS[row]
    return walk_time_plan([TIME_SHAPES[k] for k in window], len(time_constraints_of(window)))


_TIME_ORACLES = {}


def time_oracle(name):
    if name not in _TIME_ORACLES:
        data = time_model(name)
        op = orc.OraclePrimitive(data)
        if TIME_SHAPES[name][2]:
            op.init_time_model(data)
        _TIME_ORACLES[name] = op
    return _TIME_ORACLES[name]


def time_oracle_functions(row):
    """(start keyframe, per step of the window the oracle's canonical time functions (n, F), per step its log p (n,))."""
    window, n, params, S, _ = time_case(row)
    first = time_oracle(FIRST_STEP)
    start = orc.time_constraints_start_keyframe([first.back_transform_gamma_to_canonical_time_function(params[0][TIME_SHAPES[FIRST_STEP][1]:])])
    tfs, lps, off = [], [], 0
    for k, name in enumerate(window):
        F, L, Lt, _ = TIME_SHAPES[name]
        op = time_oracle(name)
        G = S[:, off:off + Lt]
        off += Lt
        tfs.append(np.array([op.back_transform_gamma_to_canonical_time_function(g) for g in G]) if Lt else np.tile(np.arange(F, dtype=np.float64), (n, 1)))
        lps.append(op.score_samples(np.hstack([np.tile(params[k + 1][:L], (n, 1)), G])))
    return start, tfs, lps


# ---- the score kernel's table -----------------------------------------------------------------------------------------------------
SCORE_WIDTHS = (4, 5, 16, 17, 24, 25, 32, 33, 48, 49, 56, 57, 60, 61, 64, 65)
SCORE_F, SCORE_NB = 12, 6
SCORE_REFUSED_L = 280                  # sixteen staged latent rows of 281 doubles alone are 4496 of a wave's 4800 doubles
# name: (the walk's widths, constraints per step beside the exits, candidates, latent dtype, what else the row does)
SCORE_ROWS = {"s1": ((4, 65, 5), 1, 1, np.float64, ()), "s2": ((16, 17, 24), 2, 16, np.float32, ("errors_only",)),
              "s15": ((25, 32, 33), 15, 17, np.float64, ("wide_ld",)), "s16": ((48, 49, 56), 16, 64, np.float32, ("descending",)),
              "s17": ((57, 60, 61), 17, 65, np.float64, ()), "edge": ((64, 65), 3, 17, np.float64, ("force_valu",)),
              "deep": ((65, 33), 2, 17, np.float32, ("deep",)), "refused": ((SCORE_REFUSED_L, 4), 1, 5, np.float64, ("refused",))}
SCORE_IDS = sorted(SCORE_ROWS)


def score_model(L):
    return synthetic.make_primitive(seed=9700 + L, n_components=L, n_frames=SCORE_F, n_basis=SCORE_NB, n_gmm=1, name="L%d" % L)


def score_constraints(n, i, deep=False):
    """n constraints of step i: root positions and directions at spread times, or (deep) joint positions on the deepest chain."""
    tl, out = float(SCORE_F - 1), []
    for c in range(n):
        t = round(tl * (c + 1) / n, 6)
        if deep:
            out.append({"type": "joint_position", "joint": "LeftHand", "t": t, "weight": 2.0, "target": [25.0 * (i + 1), 95.0 + c, -15.0 * i]})
        elif c % 3 == 1:
            out.append({"type": "direction", "t": t, "weight": 0.5 + 0.1 * c, "target": [0.3, 1.0]})
        elif c % 3 == 2:
            out.append({"type": "joint_position", "joint": "Spine", "t": t, "weight": 1.5, "target": [20.0 * (i + 1), 60.0 + c, -10.0 * i]})
        else:
            out.append({"type": "position", "t": t, "weight": 1.0, "target": [30.0 * (i + 1) + c, None, -20.0 * i]})
    return out


def score_latents(row):
    widths, _, n, dtype, _ = SCORE_ROWS[row]
    S = (0.7 * np.random.default_rng(9800 + SCORE_IDS.index(row)).standard_normal((n, sum(widths)))).astype(dtype)
    return S
