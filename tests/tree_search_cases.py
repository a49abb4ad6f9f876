"""mg_cluster_tree_search_trajectories (csrc/mg_cluster_tree.hip) across its LDS ladder and shape edges: both LDS plans and the ladder
of csrc/mg_tree_plan.h restated, the table of shapes, the ledger of the boundaries the table straddles, and an objective that calls
nothing of the library.

Shared by tests/test_tree_search_shapes_host.py (no device: the restatement against the header through tests/native/tree_plan_check,
the table against the ledger, the conditioning of every row for the oracle) and tests/test_gpu_tree_search_shapes.py (the same rows
on the device).

A row is one search on a flat tree -- a root whose children are all leaves, so the launch scores every leaf and the winner is the
argmin over the leaves.  Its shape is the smallest that lands on its rung: the sizes are computed from the restated plan
(_segments_up_to, _keyframes_from), never guessed.  The rungs, in the order mg_tree_plan_fit leaves them:

    all_staged            W, the polynomial tables and the root rows in LDS
    w_memory              s.Wm = a.W: the set's W read from memory (dropped by the ladder, or never known: more than 64 latents)
    polynomials_memory    t.poly = NULL: tr->t[i].poly read from memory
    root_rows_memory      t.cp = NULL: every tap forms its control points from the latents
    refused               no rung fits: MG_ERR_UNSUPPORTED, nothing launched

oracle_objectives is the yardstick that is independent of the library: oracle.mg_oracle's back-projection, alignment, keyframe errors
and chained closest-point search (Catmull-Rom splines: the only type the oracle has, so every table row uses it; the other two types
are held to the batched descent in the GPU file's trajectory-edge tests).
"""
import numpy as np

from morphablegraphs_amd import synthetic
from oracle import mg_oracle as orc

# ---- csrc/mg_tree_plan.h, restated (held to the header by tests/test_tree_search_shapes_host.py) --------------------------------------
CHUNK = 64                       # MG_TREE_CHUNK
KD_GROUP = 32                    # MG_KD_GROUP
HENT, KENT = 24, 16              # MG_TREE_HENT_BYTES, MG_TREE_KENT_BYTES
LDS_MAX = 160 * 1024 - 512       # MG_TREE_LDS_MAX
KB64 = 64 * 1024                 # above it the launch opts in to the large LDS
MAX_TRAJECTORIES = 4             # MG_TREE_MAX_TRAJECTORIES
STATES = ("all_staged", "w_memory", "polynomials_memory", "root_rows_memory")
KINDS = ("feature", "kd")
SEGMENT_BYTES, CONSTRAINT_BYTES, ROOT_ROW_BYTES = 96, 512, 512     # what one more of each moves a plan by (per trajectory slot / rs row / cp row)


def head_bytes(L, nc, traj, wrows, cp_rows, poly_doubles):
    """mg_tree_carve_head: xs [64][L + 1], W and bias [wrows][L + 1], rs [max(nc, 1)][64], cval [64], then with trajectories the root rows
    [cp_rows][64], the polynomial tables [traj][poly_doubles] and the terms [traj][64]; all doubles."""
    cp = cp_rows if traj > 0 else 0
    poly = poly_doubles if traj > 0 else 0
    return 8 * (CHUNK * (L + 1) + wrows * (L + 1) + max(nc, 1) * CHUNK + CHUNK + cp * CHUNK + traj * poly + traj * CHUNK)


def _caps(n_cand, children, depth):
    cap_local = max(children, 1)
    return cap_local, n_cand * min(n_cand, cap_local), n_cand * (depth + 1)


def _ints(n_cand):
    """mg_tree_carve_ints: cid [64], clast [64], fr_n [n_cand], fr_off [n_cand + 1]"""
    return 4 * (CHUNK + CHUNK + n_cand + n_cand + 1)


def feature_plan_bytes(L, nc, n_cand, children, depth, traj, wrows, cp_rows, poly_doubles):
    """mg_tree_plan(...).bytes"""
    cap_local, cap_level, cap_res = _caps(n_cand, children, depth)
    o = head_bytes(L, nc, traj, wrows, cp_rows, poly_doubles)
    o += 8 * (n_cand + cap_level + cap_local + cap_res) + _ints(n_cand) + 4 * (cap_level + cap_local + cap_res)
    return (o + 15) & ~15


def kd_plan_bytes(L, nc, n_cand, children, depth, kd_children, kd_depth, traj, wrows, cp_rows, poly_doubles):
    """mg_kd_plan(...).bytes"""
    cap_local, cap_level, cap_res = _caps(n_cand, children, depth)
    cap_leaf, kcap = max(kd_children, 1), kd_depth + 1
    o = head_bytes(L, nc, traj, wrows, cp_rows, poly_doubles)
    o += HENT * (cap_local + cap_level + cap_res + cap_leaf) + KD_GROUP * kcap * KENT + KD_GROUP * 8 + KD_GROUP * kcap * 4
    o += _ints(n_cand) + 4 * CHUNK + 4 * (n_cand + 1) + 3 * 4 * KD_GROUP
    return (o + 15) & ~15


def plan_bytes(kind, c, wrows, cp_rows, poly_doubles):
    """The plan of call shape c (call_shape) with that much staged."""
    if kind == "kd":
        return kd_plan_bytes(c["L"], c["nc"], c["n_cand"], c["children"], c["depth"], c["kd_children"], c["kd_depth"], c["traj"], wrows, cp_rows, poly_doubles)
    return feature_plan_bytes(c["L"], c["nc"], c["n_cand"], c["children"], c["depth"], c["traj"], wrows, cp_rows, poly_doubles)


def plan_fit(kind, c):
    """mg_tree_plan_fit on the call's maxima: what mg_cluster_tree_search_plan reports, plus the rung's name ("state")."""
    st = [c["wrows"], c["cp_rows"] if c["traj"] > 0 else 0, c["poly_doubles"] if c["traj"] > 0 else 0]

    def size():
        return plan_bytes(kind, c, st[0], st[1], st[2])
    b = size()
    if b > LDS_MAX and st[0] > 0:
        st[0] = 0
        b = size()
    if c["traj"] > 0:
        if b > LDS_MAX and st[2] > 0:
            st[2] = 0
            b = size()
        if b > LDS_MAX and st[1] > 0:
            st[1] = 0
            b = size()
    if b > LDS_MAX:
        state = "refused"
    elif c["traj"] > 0 and st[1] == 0:
        state = "root_rows_memory"
    elif c["traj"] > 0 and st[2] == 0:
        state = "polynomials_memory"
    elif st[0] == 0:
        state = "w_memory"
    else:
        state = "all_staged"
    return dict(lds_bytes=b, w_rows=st[0], root_rows=st[1], poly_doubles=st[2], trajectory_slots=c["traj"], lds_opt_in=b > KB64, refused=b > LDS_MAX,
                state=state)


def ladder_bytes(kind, c):
    """The plan's bytes at each comparison of mg_tree_plan_fit: (as asked for, behind the W step, behind the polynomial step, behind the
    root-row step)"""
    traj = c["traj"] > 0
    st = [c["wrows"], c["cp_rows"] if traj else 0, c["poly_doubles"] if traj else 0]
    out = [plan_bytes(kind, c, *st)]
    for i in (0, 2, 1):
        if out[-1] > LDS_MAX and st[i] > 0 and (i == 0 or traj):
            st[i] = 0
        out.append(plan_bytes(kind, c, *st))
    return tuple(out)


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------
F = 12                   # canonical frames of every primitive here: the grid stays short
ROOT_CHANNELS = 7        # a root keyframe constraint owns one row of W per pose channel (D = 7: the root alone)
ALIGN_ROWS = {0: 0, 1: 7, 2: 3}     # rows the alignment adds to the set: the first control point's root position [+ the root quaternion]
PRIMS = {                # name: (L, NB)
    "tiny": (3, 7),           # synthetic.make_tiny_primitive
    "wide60": (60, 7),        # a W row costs 488 bytes: a few dozen keyframes crowd the plan
    "wide68": (68, 7),        # more than 64 latents: the set has no row count, W is read from memory whatever the plan
    "basis31": (3, 31),       # 97 root rows: a long keyframe list in front of them pushes them out
    "basis104": (3, 104),     # 316 root rows fit no plan: beyond mg_trajectory_plan too, so the oracle alone is the yardstick
}


def model(name):
    if name == "tiny":
        return synthetic.make_tiny_primitive(seed=1)
    L, NB = PRIMS[name]
    return synthetic.make_primitive(seed=7000 + L + NB, n_components=L, n_frames=F, n_basis=NB, n_dim=7, n_gmm=1, name=name)


def canonical_times():
    return np.linspace(0, F, F)


def tree_shape(kind, n_leaves):
    """(children, depth, kd_children, kd_depth) of a flat tree as mg_tree_maxima sees it (a KD leaf without KD trees scores its mean)"""
    return (n_leaves, 1, 1, 0) if kind == "kd" else (n_leaves, 1, 1, 0)


def set_rows(prim, n_keyframes, align):
    """mg_constraint_set::rows of n root keyframe constraints (0: not known, beyond 64 latents or an empty set)"""
    if PRIMS[prim][0] > 64:
        return 0
    return ROOT_CHANNELS * n_keyframes + ALIGN_ROWS[align]


def search_shape(kind, prim, n_keyframes, align, n_segs, n_leaves, n_cand):
    """One search's contribution to a call's maxima"""
    L, NB = PRIMS[prim]
    children, depth, kd_children, kd_depth = tree_shape(kind, n_leaves)
    return dict(L=L, nc=n_keyframes, n_cand=n_cand, children=children, depth=depth, kd_children=kd_children, kd_depth=kd_depth, traj=len(n_segs),
                wrows=set_rows(prim, n_keyframes, align), rows_known=set_rows(prim, n_keyframes, align) > 0,
                cp_rows=(3 * NB + 4) if n_segs else 0, poly_doubles=max([12 * s + 3 for s in n_segs] + [0]))


def call_shape(shapes):
    """mg_tree_gather's maxima over a call's searches (mg_tree_maxima: every maximum starts at its default)"""
    c = dict(L=1, nc=1, children=1, depth=0, kd_children=1, kd_depth=0, wrows=0, traj=0, cp_rows=0, poly_doubles=0)
    for k in c:
        c[k] = max([c[k]] + [s[k] for s in shapes])
    c["n_cand"] = shapes[0]["n_cand"]
    if not all(s["rows_known"] for s in shapes):
        c["wrows"] = 0
    return c


def row_shape(r):
    return search_shape(r["kind"], r["prim"], r["n_keyframes"], r["align"], [t["n_seg"] for t in r["trajectories"]], r["n_leaves"], r["n_cand"])


def row_plan(r):
    return plan_fit(r["kind"], call_shape([row_shape(r)]))


N_LEAVES = 24


def _traj(n_seg, min_u=0.0, weight=1.0, granularity=1000, seed=0):
    return dict(n_seg=n_seg, min_u=min_u, weight=weight, granularity=granularity, seed=seed)


def _row(name, kind, search, prim, n_keyframes, align, trajectories, state, over64, yardstick="batched", n_cand=2):
    return dict(name="%s-%s-s%d" % (name, kind, search), family=name, kind=kind, search=search, prim=prim, n_keyframes=n_keyframes, align=align,
                trajectories=trajectories, n_leaves=N_LEAVES, n_cand=n_cand, state=state, over64=over64, yardstick=yardstick)


def _with(kind, prim, n_keyframes, align, n_segs, n_cand=2):
    return plan_fit(kind, call_shape([search_shape(kind, prim, n_keyframes, align, n_segs, N_LEAVES, n_cand)]))


def _segments_up_to(kind, limit, prim, n_keyframes, align, count):
    """The longest `count` equal trajectories whose plan with everything staged stays within `limit` bytes"""
    n = 1
    c = lambda s: call_shape([search_shape(kind, prim, n_keyframes, align, [s] * count, N_LEAVES, 2)])
    full = lambda s: plan_bytes(kind, c(s), c(s)["wrows"], c(s)["cp_rows"], c(s)["poly_doubles"])
    assert full(1) <= limit
    while full(n + 1) <= limit:
        n += 1
    return n


def _keyframes_from(kind, prim, align, n_segs, state):
    """The shortest keyframe list (at least one) that lands the search on `state`"""
    n = 1
    while _with(kind, prim, n, align, n_segs)["state"] != state:
        n += 1
        assert n < 400, (kind, prim, state)
    return n


def _rows():
    rows = []
    for kind in KINDS:
        # the 64 KiB line and the limit, with everything staged, to the segment: one trajectory around 64 KiB, two around the limit
        s64 = _segments_up_to(kind, KB64, "tiny", 2, 0, 1)
        smax = _segments_up_to(kind, LDS_MAX, "tiny", 1, 0, 2)
        # W leaves alone: wide latents and a few dozen keyframes (the shortest list that does it); with a long staged table the plan
        # stays above 64 KiB
        kw = _keyframes_from(kind, "wide60", 0, [5], "w_memory")
        kw_long = _keyframes_from(kind, "wide60", 0, [600], "w_memory")
        # the root rows leave: 97 of them behind the shortest keyframe list that pushes them out
        kc = _keyframes_from(kind, "basis31", 0, [5, 7], "root_rows_memory")
        for search in (0, 1):
            a = (0, 1, 2)[(search + KINDS.index(kind)) % 3]          # alignment modes spread over the rows, not crossed
            b = (a + 1) % 3
            rows += [
                _row("small", kind, search, "tiny", 2, a, [_traj(5, 0.0, 1.0, seed=1)], "all_staged", False),
                _row("four_trajectories", kind, search, "tiny", 1, b, [_traj(5, 0.15, 0.7, seed=2), _traj(3, 0.0, 2.5, seed=3), _traj(9, 0.05, 1.0, seed=4),
                                                                       _traj(1, 0.0, 0.5, seed=5)], "all_staged", False),
                _row("last_under_64k", kind, search, "tiny", 2, 0, [_traj(s64, seed=6)], "all_staged", False),
                _row("first_over_64k", kind, search, "tiny", 2, 0, [_traj(s64 + 1, seed=6)], "all_staged", True),
                _row("last_under_limit", kind, search, "tiny", 1, 0, [_traj(smax, seed=7), _traj(smax - 200, 0.1, 1.5, seed=8)], "all_staged", True),
                # one segment more: the 7 rows of W leave, and that is enough; two more: the polynomials leave as well
                _row("first_over_limit", kind, search, "tiny", 1, 0, [_traj(smax + 1, seed=7), _traj(smax - 200, 0.1, 1.5, seed=8)], "w_memory", True),
                _row("polynomials_leave", kind, search, "tiny", 1, 0, [_traj(smax + 2, seed=7), _traj(smax - 200, 0.1, 1.5, seed=8)], "polynomials_memory", False),
                _row("three_long", kind, search, "tiny", 1, a, [_traj(641, seed=9), _traj(640, 0.2, 0.8, seed=10), _traj(12, 0.0, 1.2, seed=11)],
                     "polynomials_memory", False),
                _row("w_leaves", kind, search, "wide60", kw, 0, [_traj(5, seed=12)], "w_memory", False),
                _row("w_stays", kind, search, "wide60", kw - 1, 0, [_traj(5, seed=12)], "all_staged", True),
                _row("w_leaves_long_table", kind, search, "wide60", kw_long, 0, [_traj(600, seed=13)], "w_memory", True),
                _row("beyond_64_latents", kind, search, "wide68", 2, b, [_traj(5, 0.1, 1.0, seed=14), _traj(4, 0.0, 2.0, seed=15)], "w_memory", False),
                _row("root_rows_leave", kind, search, "basis31", kc, 0, [_traj(5, seed=16), _traj(7, 0.1, 1.3, seed=17)], "root_rows_memory", True),
                _row("root_rows_stay", kind, search, "basis31", kc - 1, 0, [_traj(5, seed=16), _traj(7, 0.1, 1.3, seed=17)], "polynomials_memory", True),
                _row("root_rows_too_many", kind, search, "basis104", 1, 0, [_traj(5, seed=18)], "root_rows_memory", False, yardstick="oracle"),
            ]
    return rows


ROWS = _rows()
BY_NAME = {r["name"]: r for r in ROWS}
ROW_IDS = [r["name"] for r in ROWS]
# fits on no rung: 64 rows of 281 doubles are 140 KiB before anything else, and 40 keyframes' residuals make up the rest
REFUSED = dict(name="refused", kind=None, search=0, prim=None, L=280, NB=7, n_keyframes=40, align=0, trajectories=[_traj(5, seed=19)], n_leaves=N_LEAVES,
               n_cand=2)


def refused_shape(kind):
    children, depth, kd_children, kd_depth = tree_shape(kind, N_LEAVES)
    return call_shape([dict(L=REFUSED["L"], nc=REFUSED["n_keyframes"], n_cand=2, children=children, depth=depth, kd_children=kd_children, kd_depth=kd_depth,
                            traj=1, wrows=0, rows_known=False, cp_rows=3 * REFUSED["NB"] + 4, poly_doubles=63)])


def refused_model():
    return synthetic.make_primitive(seed=7280, n_components=REFUSED["L"], n_frames=F, n_basis=REFUSED["NB"], n_dim=7, n_gmm=1, name="refused")


# ---- the ledger: every comparison of mg_tree_plan_fit and the 64 KiB test, with the families on each side ----------------------------------
# (family below, family above, what is compared, the step the shapes can move the plan by: the distance from the boundary is at most that)
LEDGER = [
    dict(boundary="bytes > 64 KiB (the opt-in), everything staged", below=["last_under_64k"], above=["first_over_64k"], step=SEGMENT_BYTES),
    dict(boundary="bytes > 64 KiB with W read from memory", below=["w_leaves"], above=["w_leaves_long_table"], step=None),
    dict(boundary="bytes > 64 KiB with the polynomials read from memory", below=["polynomials_leave", "three_long"], above=["root_rows_stay"], step=None),
    dict(boundary="bytes > 64 KiB with the root rows read from memory", below=["root_rows_too_many"], above=["root_rows_leave"], step=None),
    dict(boundary="bytes > MG_TREE_LDS_MAX on the first plan (W leaves)", below=["w_stays", "last_under_limit"], above=["w_leaves", "first_over_limit"],
         step=2 * SEGMENT_BYTES),
    dict(boundary="bytes > MG_TREE_LDS_MAX without W (the polynomials leave)", below=["first_over_limit"], above=["polynomials_leave"], step=2 * SEGMENT_BYTES),
    dict(boundary="bytes > MG_TREE_LDS_MAX without the polynomials (the root rows leave)", below=["root_rows_stay"], above=["root_rows_leave"],
         step=CONSTRAINT_BYTES),
    dict(boundary="bytes > MG_TREE_LDS_MAX without the root rows (the refusal)", below=["root_rows_leave", "root_rows_too_many"], above=["refused"], step=None),
    dict(boundary="st.wrows > 0 (a set without a row count has no W to drop)", below=["beyond_64_latents"], above=["w_leaves"], step=None),
]


def families():
    return sorted({r["family"] for r in ROWS})


def ledger_sides(rows=None):
    """Per ledger entry the rows (of every kind and search) on each side that really lie there, by the restated plan: {boundary: (below, above)}"""
    rows = ROWS if rows is None else rows
    out = {}
    for e in LEDGER:
        out[e["boundary"]] = ([r["name"] for r in rows if r["family"] in e["below"]], [r["name"] for r in rows if r["family"] in e["above"]])
    return out


# ---- the inputs of a row ---------------------------------------------------------------------------------------------------------------------
PREV7 = np.array([30.0, 88.0, -15.0, 0.9, 0.05, 0.42, 0.03])
PREV7[3:] /= np.linalg.norm(PREV7[3:])
START_POSE = {"position": [3.0, 2.0, 1.0], "orientation": [0.0, 25.0, 0.0]}
HIPS = ([("Hips", None, (0.0, 0.0, 0.0))], ["Hips"])
_MEAN_PATHS = {}


def mean_path(prim, data=None):
    """The root path of the zero latent on the canonical frames, by the oracle"""
    if prim not in _MEAN_PATHS:
        op = orc.OraclePrimitive(model(prim) if data is None else data)
        _MEAN_PATHS[prim] = orc.spline_frames(op.knots, op.back_project_spatial_coeffs(np.zeros(op.n_components)), canonical_times())[:, :3]
    return _MEAN_PATHS[prim]


def control_points(path, n_seg, seed):
    """n_seg + 1 Catmull-Rom control points beside `path`: the path resampled evenly, moved off it by a smooth seeded wave of a few
    units (no jitter per point: a long spline stays smooth, so the closest-point searches have one basin per frame)"""
    rng = np.random.default_rng(9100 + seed)
    n = n_seg + 1
    t = np.linspace(0.0, len(path) - 1.0, n)
    pts = np.stack([np.interp(t, np.arange(len(path)), path[:, d]) for d in range(3)], axis=1)
    amp, phase = rng.uniform(2.0, 5.0, 3), rng.uniform(0.0, 2.0 * np.pi, 3)
    return pts + amp * np.sin(0.7 * t[:, None] + phase)


def keyframes(n, seed, path):
    """n root position constraints near the path, at seeded times of the canonical span, the first at its end"""
    rng = np.random.default_rng(9200 + seed)
    out = []
    for i in range(n):
        t = float(F - 1) if i == 0 else float(np.round(rng.uniform(0.0, F - 1.0), 2))
        p = path[int(round(t))] + rng.uniform(-8.0, 8.0, 3)
        out.append({"type": "position", "t": t, "weight": float(np.round(rng.uniform(0.2, 1.5), 2)) if i else 1.0,
                    "target": [float(p[0]), None if i % 2 == 0 else float(p[1]), float(p[2])]})
    return out


def row_inputs(r, data=None):
    """(model, keyframe constraints, trajectory constraints in device form, leaves' latents (n_leaves, L))"""
    data = model(r["prim"]) if data is None else data
    path = mean_path(r["prim"], data)
    seed = sum(ord(ch) for ch in r["name"])
    kf = keyframes(r["n_keyframes"], seed, path)
    trajs = [{"type": "trajectory", "control_points": control_points(path, t["n_seg"], t["seed"]).tolist(), "min_u": t["min_u"], "weight": t["weight"],
              "granularity": t["granularity"]} for t in r["trajectories"]]
    latents = np.random.default_rng(9300 + seed).standard_normal((r["n_leaves"], PRIMS[r["prim"]][0]))
    return data, kf, trajs, latents


# ---- the oracle's objective and the bound it is compared under ---------------------------------------------------------------------------------
WALK_TOL = 1.0e-9      # tests/test_gpu_trajectory_shapes.py: the walk's distances, rtol and atol
D_TOL = 1.0e-6         # ... the reference's search: |dd| / max(1, d)
KEYFRAME_RTOL, KEYFRAME_ATOL = 1.0e-9, 1.0e-8      # the keyframe scorer's contract with the oracle (tests/test_gpu_kd_cluster_tree.py)


def _aligned_coeffs(op, s, align):
    coeffs = op.back_project_spatial_coeffs(s)
    if align == 1:
        return orc.align_coeffs_to_previous_frame(coeffs, PREV7, HIPS[0], HIPS[1], "Hips")
    if align == 2:
        return orc.align_coeffs_to_start_pose(coeffs, {"position": list(START_POSE["position"]), "orientation": list(START_POSE["orientation"])})
    return coeffs


def oracle_objectives(data, kf, trajs, latents, align, search):
    """Per leaf (objective, bound): the keyframe constraints' weighted errors plus weight x the average closest-point distance of every
    trajectory, by oracle.mg_oracle alone; the bound the device's value must lie within -- the keyframe scorer's contract plus, per
    trajectory, |weight| x the frame average of the bound tests/test_gpu_trajectory_shapes.py holds the root-path scorer's distances to
    (with its conditioning term: relative to max(1, d) for the reference's search, rtol + atol for the walk)."""
    op = orc.OraclePrimitive(data)
    times = canonical_times()
    values, bounds = [], []
    for s in latents:
        coeffs = _aligned_coeffs(op, s, align)
        kv = 0.0
        for c in kf:
            frame = orc.spline_frames(op.knots, coeffs, [c["t"]])[0]
            kv += c["weight"] * orc.point_distance(c["target"], frame[:3])
        path = orc.spline_frames(op.knots, coeffs, times)[:, :3]
        value, bound = kv, KEYFRAME_ATOL + KEYFRAME_RTOL * abs(kv)
        for t in trajs:
            cps = np.asarray(t["control_points"], dtype=np.float64)
            u, ds = float(t["min_u"]), []
            for p in path:
                if search == 1:
                    pt, u = orc.closest_point_walk(cps, p, u, granularity=int(t["granularity"]))
                else:
                    pt, u = orc.closest_point_lbfgsb(cps, p, u, formk_rule=True)
                ds.append(float(np.linalg.norm(p - pt)))
            ds = np.asarray(ds)
            value += t["weight"] * float(ds.mean())
            per_frame = WALK_TOL * (1.0 + ds) if search == 1 else D_TOL * np.maximum(1.0, ds)
            bound += abs(t["weight"]) * float(per_frame.mean())
        values.append(value)
        bounds.append(bound)
    return np.asarray(values), np.asarray(bounds)
