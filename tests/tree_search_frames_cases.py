"""mg_cluster_tree_search_frames (csrc/mg_cluster_tree.hip): the one-launch tree search with per-frame constraint lists.  The plan of
csrc/mg_tree_plan.h's further rungs restated, the table of shapes, their inputs, and an objective that calls nothing of the library.

Shared by tests/test_tree_search_frames_host.py (no device: the restatement against the header through
tests/native/tree_frames_plan_check, the routing, the conditioning of every row for the oracle) and tests/test_gpu_tree_search_frames.py
(the same rows on the device).

A row is one search: a tree, a primitive with its skeleton, an alignment mode and a constraint list.  Every child the descent scores
is given its objective by oracle.mg_oracle alone (keyframe errors, the chained closest-point search, per_frame_constraint_residuals),
and the descent is replayed on those values; a row is conditioned when, at every level, the kept and the dropped children and the
two best children are further apart than 1000 x the tolerance the device's values are compared under.
"""
import heapq

import numpy as np

import tree_search_cases as sc
from morphablegraphs_amd import synthetic
from oracle import mg_oracle as orc

# ---- csrc/mg_tree_plan.h, the per-frame part, restated (held to the header by tests/test_tree_search_frames_host.py) ------------------
TRACK_GROUP = 4                       # MG_TREE_TRACK_GROUP
SCRATCH_MAX = 256 << 20               # MG_TREE_SCRATCH_MAX
FC_LDS_MAX = 150 * 1024               # MG_FC_LDS_MAX: tables beyond it stay in memory whatever the rung
LIST_MAX = 4                          # MG_FRAME_LIST_MAX


def frames_carve(plan_bytes, ncp, group, table_bytes):
    """mg_tree_frames_carve: (group, tables_lds, bytes) behind a kernel plan of plan_bytes"""
    group = group if ncp > 0 else 0
    table_bytes = table_bytes if ncp > 0 else 0
    o = plan_bytes + group * ncp * 8 + group * 64 + table_bytes
    return group, int(table_bytes > 0), (o + 15) & ~15


def frames_fit(kind, c, ncp, table_bytes):
    """mg_tree_frames_fit on a call's maxima c (tree_search_cases.call_shape): what mg_cluster_tree_search_frames_plan reports"""
    traj = c["traj"] > 0
    st = [c["wrows"], c["cp_rows"] if traj else 0, c["poly_doubles"] if traj else 0]
    state = dict(group=TRACK_GROUP, tables=table_bytes)

    def carve():
        return frames_carve(sc.plan_bytes(kind, c, st[0], st[1], st[2]), ncp, state["group"], state["tables"])
    g, t, b = carve()
    if b > sc.LDS_MAX and st[0] > 0:
        st[0] = 0
        g, t, b = carve()
    if traj:
        if b > sc.LDS_MAX and st[2] > 0:
            st[2] = 0
            g, t, b = carve()
        if b > sc.LDS_MAX and st[1] > 0:
            st[1] = 0
            g, t, b = carve()
    if b > sc.LDS_MAX and state["tables"] > 0:
        state["tables"] = 0
        g, t, b = carve()
    while b > sc.LDS_MAX and ncp > 0 and state["group"] > 1:
        state["group"] //= 2
        g, t, b = carve()
    return dict(lds_bytes=b, w_rows=st[0], root_rows=st[1], poly_doubles=st[2], trajectory_slots=c["traj"], lds_opt_in=b > sc.KB64, refused=b > sc.LDS_MAX,
                track_group=g, control_points=ncp, tables_lds=bool(t), table_bytes=state["tables"] if ncp > 0 else 0)


def scratch_bytes(requests, n_rotations, D):
    """mg_tree_frames_scratch: requests = [(T, joints)]"""
    doubles = sum(sc.CHUNK * T * J * 3 for T, J in requests) + sc.CHUNK * n_rotations * D
    return (doubles * 8 + 255) & ~255


def table_bytes(tables):
    """mg_fc_place_tables for one list: tables = [(key, n_seg, G, with_arcs)]; a table two trajectories share is placed once; 0 beyond
    MG_FC_LDS_MAX"""
    seen, doubles = set(), 0
    for key, n_seg, G, arcs in tables:
        for k, count in ((("p", key), n_seg * 12 + 3),) + (((("a", key), G + 1),) if arcs else ()):
            if k not in seen:
                seen.add(k)
                doubles += (count + 1) & ~1
    return 0 if doubles * 8 > FC_LDS_MAX else doubles * 8


# ---- the primitives and their skeletons ---------------------------------------------------------------------------------------------------
F = sc.F
CHAIN = ([("Hips", None, (0.0, 0.0, 0.0)), ("Spine", "Hips", (0.0, 10.0, 1.0)), ("Hand", "Spine", (3.0, 8.0, -1.0))], ["Hips", "Spine", "Hand"])
SKELETONS = {"tiny": sc.HIPS, "chain3": CHAIN}
PRIMS = {"tiny": (3, 7, 7), "chain3": (4, 7, 15)}     # name: (L, NB, D)
PREV = {"tiny": sc.PREV7, "chain3": np.concatenate([sc.PREV7, [0.95, 0.1, -0.2, 0.05], [0.9, -0.3, 0.1, 0.2]])}
for _p in PREV.values():
    for _j in range((len(_p) - 3) // 4):
        _p[3 + 4 * _j:7 + 4 * _j] /= np.linalg.norm(_p[3 + 4 * _j:7 + 4 * _j])
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = sc.model("tiny") if name == "tiny" else synthetic.make_primitive(seed=7415, n_components=4, n_frames=F, n_basis=7, n_dim=15, n_gmm=1,
                                                                                         name="chain3")
    return _MODELS[name]


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------
def _row(name, kind, tree, n_cand, prim, align, build, n_chan, requests, n_rot=0, tables=(), rtol=1.0e-8):
    """n_chan: the pose channels the track plan keeps -- the root's three, the root's quaternion (the aligning chain) and the quaternions
    ABOVE each joint on its chain (a joint's own rotation does not move it); requests: the plan's [(T, joints)] in the order the list
    first asks for them; n_rot: joint rotations (a frame row each); tables: what mg_fc_place_tables places"""
    return dict(name=name, kind=kind, tree=tree, n_cand=n_cand, prim=prim, align=align, build=build, n_chan=n_chan, requests=requests, n_rot=n_rot,
                tables=list(tables), rtol=rtol)


def _g_for(limit, kind, n_leaves, n_cand, under):
    """The granularity of a tiny-primitive local trajectory (3 segments) whose whole plan is the last under / first over `limit`"""
    c = call_of(dict(kind=kind, tree=("flat", n_leaves), n_cand=n_cand, prim="tiny", align=0), 0, [])
    G = 100
    while frames_fit(kind, c, 7 * 7, table_bytes([("a", 3, G + 1, True)]))["lds_bytes"] <= limit:
        G += 1
    return G if under else G + 1


def tree_counts(tree):
    """child counts in breadth-first order"""
    if tree[0] == "flat":
        return [tree[1]] + [0] * tree[1]
    inner, leaves = tree[1], tree[2]       # ("two_level", inner nodes, leaves each)
    return [inner] + [leaves] * inner + [0] * (inner * leaves)


def call_of(r, n_keyframes, n_segs):
    """The call's maxima as mg_tree_gather sees one search of row r"""
    L, NB, _ = PRIMS[r["prim"]]
    counts = tree_counts(r["tree"])
    depth = 1 if r["tree"][0] == "flat" else 2
    rows = sc.ROOT_CHANNELS * n_keyframes + sc.ALIGN_ROWS[r["align"]]
    return sc.call_shape([dict(L=L, nc=n_keyframes, n_cand=r["n_cand"], children=max(counts), depth=depth, kd_children=1, kd_depth=0, traj=len(n_segs), wrows=rows,
                               rows_known=rows > 0, cp_rows=(3 * NB + 4) if n_segs else 0, poly_doubles=max([12 * s + 3 for s in n_segs] + [0]))])


def _rows():
    T = F
    rows = [
        # flat feature trees on both sides of the chunk; n_frames = 1 and n_frames < T; each type alone; the three alignment modes
        _row("flat3-ca-one_frame", "feature", ("flat", 3), 2, "tiny", 0, ["ca:Hips:1"], 7, [(1, 1)]),
        _row("flat64-discrete", "feature", ("flat", 64), 2, "tiny", 1, ["discrete:Hips"], 7, [(T, 1)]),
        _row("flat65-local-short", "feature", ("flat", 65), 2, "tiny", 2, ["local:Hips:5:1000"], 7, [(5, 1)], tables=[("a", 3, 1000, True)]),
        # two levels at n_candidates 1 and 2; a joint at the end of a 3-joint chain
        _row("two_level-n1-set", "feature", ("two_level", 4, 5), 1, "chain3", 0, ["set:Hand,Hips"], 11, [(T, 2)],
             tables=[("a", 3, 1000, True), ("b", 3, 1000, True)]),
        _row("two_level-n2-rotation", "feature", ("two_level", 4, 5), 2, "chain3", 1, ["rotation:2:4.0"], 7, [(1, 1)], n_rot=1),
        _row("kd-ca-hand", "kd", ("flat", 12), 2, "chain3", 0, ["ca:Hand:12"], 11, [(T, 1)]),
        # a list at the cap; a keyframe, a root trajectory and a per-frame constraint
        _row("list_at_cap", "feature", ("flat", 24), 2, "chain3", 2, ["ca:Hand:7", "discrete:Spine", "rotation:0:9.0", "local:Hips:12:1000"], 11,
             [(7, 1), (T, 1), (T, 1)], n_rot=1, tables=[("a", 3, 1000, True)]),
        _row("mixed_list", "feature", ("flat", 12), 2, "tiny", 1, ["keyframe", "trajectory", "local:Hips:6:1000"], 7, [(6, 1)], tables=[("a", 3, 1000, True)],
             rtol=2.0e-6),
        # the lists' tables in memory: an arc table beyond the scorers' own bound
        _row("tables_memory", "feature", ("flat", 10), 2, "tiny", 0, ["local:Hips:12:20000"], 7, [(T, 1)], tables=[("a", 3, 20000, True)]),
    ]
    # the large-LDS opt-in, to the table entry
    for under in (True, False):
        G = _g_for(sc.KB64, "feature", 10, 2, under)
        rows.append(_row("last_under_64k" if under else "first_over_64k", "feature", ("flat", 10), 2, "tiny", 0, ["local:Hips:12:%d" % G], 7, [(T, 1)],
                         tables=[("a", 3, G, True)]))
    return rows


ROWS = _rows()
BY_NAME = {r["name"]: r for r in ROWS}
ROW_IDS = [r["name"] for r in ROWS]


def row_plan(r, cons=None):
    """What the plan query must report for row r alone"""
    cons = constraints_of(r) if cons is None else cons
    kf = [c for c in cons if c["type"] == "position"]
    segs = [len(c["control_points"]) - 1 for c in cons if c["type"] == "trajectory"]
    L, NB, D = PRIMS[r["prim"]]
    p = frames_fit(r["kind"], call_of(r, len(kf), segs), NB * r["n_chan"], table_bytes(r["tables"]))
    p["scratch_bytes"] = scratch_bytes(r["requests"], r["n_rot"], D)
    return p


# ---- the inputs of a row -------------------------------------------------------------------------------------------------------------------
def _mean_tracks(prim):
    """(op, joint -> (F, 3) positions of the zero latent on the canonical frames, local coordinates)"""
    op = orc.OraclePrimitive(model(prim))
    frames = orc.spline_frames(op.knots, op.back_project_spatial_coeffs(np.zeros(op.n_components)), np.linspace(0, F, F))
    joints, animated = SKELETONS[prim]
    return op, {j: np.array([orc.joint_global_position(f, joints, animated, j) for f in frames]) for j in animated}


def constraints_of(r):
    """The row's constraint list in device form, near the mean motion"""
    _, tracks = _mean_tracks(r["prim"])
    seed = sum(ord(ch) for ch in r["name"])
    rng = np.random.default_rng(4100 + seed)
    out = []
    for spec in r["build"]:
        kind, _, rest = spec.partition(":")
        a = rest.split(":")
        if kind == "keyframe":
            out += sc.keyframes(1, seed, tracks["Hips"])
        elif kind == "trajectory":
            out.append({"type": "trajectory", "control_points": sc.control_points(tracks["Hips"], 5, seed).tolist(), "min_u": 0.05, "weight": 0.8, "granularity": 1000})
        elif kind == "ca":
            tr, nf = tracks[a[0]], int(a[1])
            p = tr[nf // 2] + rng.uniform(2.0, 6.0, 3)
            out.append({"type": "frame_ca_position", "joint": a[0], "target": [float(p[0]), None, float(p[2])], "n_frames": nf, "weight": 2.0})
        elif kind == "discrete":
            out.append({"type": "frame_discrete_trajectory", "joint": a[0], "points": (tracks[a[0]][:8] + rng.uniform(-1.0, 1.0, 3)).tolist(), "unconstrained": [1],
                        "weight": 0.8})
        elif kind == "local":
            cps = tracks[a[0]][::3][:4] + np.array([0.5, 0.0, -0.5])
            out.append({"type": "frame_local_trajectory", "joint": a[0], "control_points": cps.tolist(), "granularity": int(a[2]), "start_t": 3.0,
                        "n_frames": int(a[1]), "weight": 0.01})
        elif kind == "set":
            names = a[0].split(",")
            out.append({"type": "frame_trajectory_set", "joints": names, "weight": 1.1, "arc_lengths": [4.0, 1.0][:len(names)], "n_frames": F,
                        "trajectories": [{"control_points": (tracks[j][::3][:4] + rng.uniform(-2.0, 2.0, 3)).tolist(), "granularity": 1000,
                                          "range_start": 0.0 if i == 0 else None, "range_end": 1500.0 if i == 0 else None} for i, j in enumerate(names)]})
        elif kind == "rotation":
            q = rng.standard_normal(4)
            out.append({"type": "frame_joint_rotation", "joint_index": int(a[0]), "quaternion": (q / np.linalg.norm(q)).tolist(), "frame_idx": float(a[1]), "weight": 0.6})
        else:
            raise ValueError(spec)
    return out


def tree_means(r):
    """The nodes' means (n_nodes, L) in breadth-first order (node 0 the root), seeded by the row"""
    L = PRIMS[r["prim"]][0]
    n = len(tree_counts(r["tree"]))
    means = np.random.default_rng(4300 + sum(ord(ch) for ch in r["name"])).standard_normal((n, L))
    means[0] = 0.0
    return means


def host_tree(r):
    """The row's tree as a HipFeatureClusterTree (a KD row's flat tree scores the same rows: its leaves hold no KD trees)"""
    from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree
    counts, means = np.array(tree_counts(r["tree"])), tree_means(r)
    first = np.where(counts == 0, np.arange(len(counts)), -1)
    return HipFeatureClusterTree(means, means, np.concatenate([[0], np.cumsum(counts)]), np.arange(1, len(counts)), first, n_spatial=means.shape[1])


# ---- the oracle's objective ----------------------------------------------------------------------------------------------------------------
ATOL = 1.0e-8      # tests/test_gpu_frame_constraints.py: assert_allclose(total, oracle, rtol=1e-8, atol=1e-8); rtol 2e-6 where a trajectory search is in the list


def tolerance(r, value):
    return ATOL + r["rtol"] * abs(value)


def _aligned(op, r, s):
    coeffs = op.back_project_spatial_coeffs(s)
    joints, animated = SKELETONS[r["prim"]]
    if r["align"] == 1:
        return orc.align_coeffs_to_previous_frame(coeffs, PREV[r["prim"]], joints, animated, "Hips")
    if r["align"] == 2:
        return orc.align_coeffs_to_start_pose(coeffs, {"position": list(sc.START_POSE["position"]), "orientation": list(sc.START_POSE["orientation"])})
    return coeffs


def oracle_values(r, cons, means):
    """The objective of every row of `means`, by oracle.mg_oracle alone: the additions of MotionPrimitiveConstraints.evaluate in list order"""
    op = orc.OraclePrimitive(model(r["prim"]))
    joints, animated = SKELETONS[r["prim"]]
    out = []
    for s in means:
        coeffs = _aligned(op, r, s)
        v = 0.0
        for c in cons:
            if c["type"] == "position":
                v += c["weight"] * orc.point_distance(c["target"], orc.spline_frames(op.knots, coeffs, [c["t"]])[0][:3])
            elif c["type"] == "trajectory":
                path = orc.spline_frames(op.knots, coeffs, sc.canonical_times())[:, :3]
                u, ds = float(c["min_u"]), []
                for p in path:
                    pt, u = orc.closest_point_lbfgsb(np.asarray(c["control_points"]), p, u, formk_rule=True)
                    ds.append(float(np.linalg.norm(p - pt)))
                v += c["weight"] * float(np.mean(ds))
            else:
                v += c.get("weight", 1.0) * orc.per_frame_constraint_residuals(c, op.knots, coeffs, F, joints, animated)[1]
        out.append(v)
    return np.asarray(out)


def replay(tree, values, n):
    """HipFeatureClusterTree.descend on given per-node values, with the gaps the comparison needs: (value, leaf, evaluations, gaps) where
    gaps = [(level, kept-to-dropped distance, best-to-second distance, the level's largest |value|)]"""
    gaps, level = [], [0]

    def score(ids):
        level[0] += 1
        return [values[i] for i in ids]
    cb, ch = tree.child_begin, tree.children
    frontier = [0]
    value, _, leaf, n_eval = tree.descend(score, n)
    # the levels again, for the gaps: the frontier's children, which of them the heaps' lists kept
    while frontier:
        nxt_heap, ids_level = [], []
        for node in frontier:
            kids = [int(c) for c in ch[cb[node]:cb[node + 1]]]
            if not kids:
                continue
            q = []
            for k in kids:
                heapq.heappush(q, (values[k], k))
            kept = [k for _, k in q[:n]]
            dropped = [k for k in kids if k not in kept]
            ids_level.append((kids, kept, dropped))
            for e in q[:n]:
                heapq.heappush(nxt_heap, e)
        if not ids_level:
            break
        nxt = [k for _, k in nxt_heap[:n]]
        allk = [k for kids, _, _ in ids_level for k in kids]
        out = [k for k in allk if k not in nxt]
        kd = min([abs(values[a] - values[b]) for a in nxt for b in out] + [np.inf])
        srt = sorted(values[k] for k in allk)
        gaps.append((len(gaps) + 1, kd, srt[1] - srt[0] if len(srt) > 1 else np.inf, max(abs(values[k]) for k in allk)))
        frontier = nxt
    return value, leaf, n_eval, gaps
