"""mg_cluster_tree_search_frames (csrc/mg_cluster_tree.hip): the one-launch tree search with per-frame constraint lists.  The plan of
csrc/mg_tree_plan.h's further rungs restated, the table of shapes, their inputs, and an objective that calls nothing of the library.

Shared by tests/test_tree_search_frames_host.py (no device: the restatement against the header through
tests/native/tree_frames_plan_check, the routing, the ledger, the conditioning of every row for the oracle), tests/test_gpu_tree_search_frames.py
(ROWS on the device) and tests/test_gpu_tree_search_frames_shapes.py (SWEEP_ROWS: the ladder's further rungs, halved groups, KD descents).

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
FAMILIES = {"hips": ("tiny", 7), "chain": ("chain3", 11)}     # a wide primitive's family: (the primitive whose skeleton it has, the channels an end joint's track keeps)


def wide(family, L):
    """The name of family's primitive with L latents (hips310: the Hips skeleton, D = 7; chain306: the 3-joint chain, D = 15), entered
    into PRIMS, SKELETONS and PREV; synthetic.make_primitive builds it with F frames"""
    like = FAMILIES[family][0]
    name = "%s%d" % (family, L)
    PRIMS[name], SKELETONS[name], PREV[name] = (L,) + PRIMS[like][1:], SKELETONS[like], PREV[like]
    return name


def model(name):
    if name not in _MODELS:
        L, NB, D = PRIMS[name]
        if name == "tiny":
            _MODELS[name] = sc.model("tiny")
        elif name == "chain3":
            _MODELS[name] = synthetic.make_primitive(seed=7415, n_components=4, n_frames=F, n_basis=7, n_dim=15, n_gmm=1, name="chain3")
        else:
            _MODELS[name] = synthetic.make_primitive(seed=7400 + L + D, n_components=L, n_frames=F, n_basis=NB, n_dim=D, n_gmm=1, name=name)
    return _MODELS[name]


# Rows whose seed is not 0, chosen on the CPU from oracle_of: lists_push_polynomials-feature because seed 0 leaves the kept and the
# dropped children 0.9 of the needed distance apart; the rows on a halved track group so that the score that decides for the winner stands
# in a slot of its chunk that only a group of that size reaches (in_later_group): the first seed that does it and keeps the row conditioned.
_SEEDS = {"lists_push_polynomials-feature": 2, "group2_65_children-hips-feature": 1, "group2_first-chain-feature": 2, "group2_first-hips-kd": 1,
          "group2_65_children-hips-kd": 2, "kd_descents-33-1-halved": 3, "kd_descents-33-2-halved": 3}


def in_later_group(slot, group):
    """Whether chunk slot `slot` is formed by a later group than the first of its stride of MG_TREE_TRACK_GROUP children: on group 2 the
    second pair of every four, on group 1 all but the first.  A group loop that strode by four would never form its tracks."""
    return slot % TRACK_GROUP >= group


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------
def _row(name, kind, tree, n_cand, prim, align, build, n_chan, requests, n_rot=0, tables=(), rtol=1.0e-8, kd=(0, 0), family=None, refused=False, seed=None):
    """n_chan: the pose channels the track plan keeps -- the root's three, the root's quaternion (the aligning chain) and the quaternions
    ABOVE each joint on its chain (a joint's own rotation does not move it); requests: the plan's [(T, joints)] in the order the list
    first asks for them; n_rot: joint rotations (a frame row each); tables: what mg_fc_place_tables places; kd: (KD trees per leaf, inner
    levels of each) of a KD row's leaves as test_gpu_kd_cluster_tree._kd_tree builds them; family: the ledger's name for the row (both tree
    kinds share it); refused: no rung takes the row -- only its plan and the launch's status are checked; seed: moves the tree's means (chosen where seed 0 leaves the row unconditioned).
    yardstick: "batched" where the host-driven descent through candidate_scoring.errors_of_samples can score the row, "oracle" where
    mg_score_constraints refuses its shape (scorer_refuses) and the oracle's replayed descent alone is what the launch is held to."""
    r = dict(name=name, kind=kind, tree=tree, n_cand=n_cand, prim=prim, align=align, build=build, n_chan=n_chan, requests=requests, n_rot=n_rot,
             tables=list(tables), rtol=rtol, kd=tuple(kd), family=family or name, refused=refused, seed=_SEEDS.get(name, 0) if seed is None else seed)
    r["yardstick"] = "oracle" if scorer_refuses(PRIMS[prim][0], n_keyframes_of(build)) else "batched"
    return r


def n_keyframes_of(build):
    return sum(int(b.partition(":")[2] or 1) for b in build if b.split(":")[0] in ("keyframe", "keyframes"))


def segments_of(build):
    return [int(b.partition(":")[2] or 5) for b in build if b.split(":")[0] == "trajectory"]


def scorer_refuses(L, n_keyframes):
    """Whether mg_score_constraints refuses a set of n root keyframe constraints on L latents, by tests/score_shape_cases.score_route --
    mg_score_route_of restated, held to csrc/mg_score_route.h by tests/test_score_shapes_host.py: the matrix-pipe kernels' row tiles end
    early, and the VALU kernel keeps 64 candidates' latents and residual rows in LDS and refuses beyond 150 KiB.  (errors_of_samples
    scores the keyframe set first, an empty one too, so the host-driven descent cannot score such a row.)"""
    import score_shape_cases as ssc
    try:
        ssc.score_route(L, 0 if L > 64 else sc.ROOT_CHANNELS * n_keyframes, n_keyframes, sc.CHUNK)
    except ssc.Refused:
        return True
    return False


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
    L, NB, _ = r.get("dims") or PRIMS[r["prim"]]      # (dims: a shape tried while a row is sized, before its primitive has a name)
    counts = tree_counts(r["tree"])
    depth = 1 if r["tree"][0] == "flat" else 2
    rows = 0 if L > 64 else sc.ROOT_CHANNELS * n_keyframes + sc.ALIGN_ROWS[r["align"]]     # (mg_constraint_set::rows: not known beyond 64 latents)
    kd_per_leaf, kd_levels = r.get("kd", (0, 0))
    return sc.call_shape([dict(L=L, nc=n_keyframes, n_cand=r["n_cand"], children=max(counts), depth=depth, kd_children=max(kd_per_leaf, 1), kd_depth=kd_levels,
                               traj=len(n_segs), wrows=rows,
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
ROW_IDS = [r["name"] for r in ROWS]


# ---- the sweep: the ladder's further rungs, the halved groups, KD descents with a list (tests/test_gpu_tree_search_frames_shapes.py) ---------
# Every size below is computed from the restated plan: the smallest (or the last) shape on its rung.
BIG_TABLE = [("a", 3, 18000, True)]      # a local trajectory's tables of 144336 bytes: under MG_FC_LDS_MAX, most of a workgroup's LDS
SMALL_TABLE = [("a", 3, 1000, True)]


def _shape(kind, tree, n_cand, prim, align=0, kd=(0, 0), dims=None):
    return dict(kind=kind, tree=tree, n_cand=n_cand, prim=prim, align=align, kd=kd, dims=dims)


def _fit(shape, n_keyframes, segs, n_chan, tables):
    NB = (shape.get("dims") or PRIMS[shape["prim"]])[1]
    return frames_fit(shape["kind"], call_of(shape, n_keyframes, segs), NB * n_chan, table_bytes(tables))


def _first(pred, start, stop):
    for v in range(start, stop):
        if pred(v):
            return v
    raise AssertionError("no shape in [%d, %d) lands there" % (start, stop))


def _group(p):
    """The rung of a fitted plan among the groups: 4, 2, 1, or 0 where it is refused"""
    return 0 if p["refused"] else p["track_group"]


def _ladder_rows(kind):
    """tiny, ten leaves: the lists' regions move W, the polynomials, the root rows and at last their own tables out of LDS"""
    rows, flat = [], ("flat", 10)
    sh = _shape(kind, flat, 2, "tiny")
    # by the keyframe: W leaves, then (nothing else to drop without trajectories) the tables
    fit = lambda n: _fit(sh, n, [], 7, BIG_TABLE)
    n_w = _first(lambda n: fit(n)["w_rows"] == 0, 2, 400)
    n_t = _first(lambda n: not fit(n)["tables_lds"], 2, 400)
    for name, n in (("lists_keep_w", n_w - 1), ("lists_push_w", n_w), ("tables_stay", n_t - 1), ("tables_leave", n_t)):
        rows.append(_row("%s-%s" % (name, kind), kind, flat, 2, "tiny", 0, ["keyframes:%d" % n, "local:Hips:12:18000"], 7, [(F, 1)], tables=BIG_TABLE, family=name))
    # by the table entry: one and two root trajectories, the list's table grown until the polynomials / the root rows leave
    for what, segs, key in (("polynomials", [5], "poly_doubles"), ("root_rows", [5, 7], "root_rows")):
        fit_g = lambda G: _fit(sh, 2, segs, 7, [("a", 3, G, True)])
        G = _first(lambda G: fit_g(G)[key] == 0, 1000, 19000)
        for name, g in (("lists_keep_" + what, G - 1), ("lists_push_" + what, G)):
            rows.append(_row("%s-%s" % (name, kind), kind, flat, 2, "tiny", 0, ["keyframes:2"] + ["trajectory:%d" % s for s in segs] + ["local:Hips:12:%d" % g], 7,
                             [(F, 1)], tables=[("a", 3, g, True)], rtol=2.0e-6, family=name, seed=None))
    # every rung in one search: root trajectories, a list with tables, and keyframes until the group is halved as well
    sh = _shape(kind, ("flat", 7), 2, "tiny", 1)
    n = _first(lambda n: _group(_fit(sh, n, [5, 7], 7, SMALL_TABLE)) < 4, 2, 600)
    rows.append(_row("everything_left-%s" % kind, kind, ("flat", 7), 2, "tiny", 1, ["keyframes:%d" % n, "trajectory:5", "trajectory:7", "local:Hips:12:1000"], 7,
                     [(F, 1)], tables=SMALL_TABLE, rtol=2.0e-6, family="everything_left"))
    return rows


def _group_rows(kind):
    """Wide primitives (64 rows of latents are most of the LDS): the track group 4 -> 2 by the latent, 2 -> 1 -> refused by the child (a
    latent's 512 bytes are wider than the window of group 1).  Once with the Hips skeleton (49 control points), once with the chain (77)."""
    rows = []
    for fam, (like, n_chan) in FAMILIES.items():
        _, NB, D = PRIMS[like]
        build = ["keyframes:3", "ca:%s:12" % SKELETONS[like][1][-1]]          # the list: a collision-avoidance position on the end joint
        grp = lambda L, c: _group(_fit(_shape(kind, ("flat", c), 2, None, dims=(L, NB, D)), 3, [], n_chan, []))
        L4 = _first(lambda L: grp(L + 1, 7) != 4, 100, 400)                  # the last L on group 4 with 7 children
        assert grp(L4, 7) == 4 and grp(L4 + 1, 7) == 2, (fam, kind, L4)

        def edges(L):
            on1 = [c for c in range(2, 120) if grp(L, c) == 1]
            return (on1[0], on1[-1]) if on1 and grp(L, on1[0] - 1) == 2 and grp(L, on1[-1] + 1) == 0 else None
        L1 = _first(lambda L: edges(L) is not None, L4 + 1, L4 + 8)
        c_first, c_last = edges(L1)
        specs = [("group4_last", L4, 7, 0), ("group2_first", L4 + 1, 7, 1), ("group1_first", L1, c_first, 2), ("group1_last", L1, c_last, 0)]
        if fam == "hips":
            L65 = _first(lambda L: grp(L, 65) == 2, L4 - 8, L4 + 8)          # 65 children on group 2: the second chunk holds one child
            specs += [("group2_65_children", L65, 65, 0), ("refused_by_group", L1, c_last + 1, 0)]
        for name, L, c, align in specs:
            rows.append(_row("%s-%s-%s" % (name, fam, kind), kind, ("flat", c), 2, wide(fam, L), align, build, n_chan, [(F, 1)], family=name,
                             refused=name == "refused_by_group"))
    return rows


def _kd_descent_rows():
    """KD leaves with real descents under a list of two: one group of descents and one more, one and two inner levels; on group 4 (the
    chain's own primitive) and on a halved group (the chain's skeleton over the fewest latents that halve it)"""
    rows = []
    build, requests = ["ca:Hand:12", "local:Hips:12:1000"], [(F, 1), (F, 1)]
    _, NB, D = PRIMS["chain3"]
    for per_leaf in (1, 32, 33):
        for levels in (1, 2):
            align = (per_leaf + levels) % 3
            rows.append(_row("kd_descents-%d-%d-group4" % (per_leaf, levels), "kd", ("flat", 2), 2, "chain3", align, build, 11, requests, tables=SMALL_TABLE,
                             kd=(per_leaf, levels), family="kd_descents_group4"))
            L = _first(lambda L: _group(_fit(_shape("kd", ("flat", 2), 2, None, align, (per_leaf, levels), (L, NB, D)), 0, [], 11, SMALL_TABLE)) in (1, 2), 100, 400)
            rows.append(_row("kd_descents-%d-%d-halved" % (per_leaf, levels), "kd", ("flat", 2), 2, wide("chain", L), align, build, 11, requests, tables=SMALL_TABLE,
                             kd=(per_leaf, levels), family="kd_descents_halved"))
    return rows


SWEEP_ROWS = [r for kind in sc.KINDS for r in _ladder_rows(kind) + _group_rows(kind)] + _kd_descent_rows()
SWEEP_IDS = [r["name"] for r in SWEEP_ROWS]
BY_NAME = {r["name"]: r for r in ROWS + SWEEP_ROWS}


# ---- the ledger: every comparison of mg_tree_frames_fit and the 64 KiB test with lists, with the families on each side ------------------------
# (comparison: ladder_trace's name for it; a row lies "above" where the comparison was made and held, "below" where it was made and did
# not hold; step: what the shapes move the plan by there, in bytes -- the distance from the boundary is at most that)
LEDGER = [
    dict(boundary="bytes > 64 KiB (the opt-in) on the rung taken", comparison="64k", below=["last_under_64k", "tables_leave"], above=["first_over_64k", "tables_stay"], step=None),
    # (step None: the feature kernel's two rows there lie 16 bytes apart, test_the_rows_stand_where_the_table_says; the KD rows straddle it widely)
    dict(boundary="bytes > MG_TREE_LDS_MAX with everything staged and st.wrows > 0 (W leaves)", comparison="w", below=["lists_keep_w"],
         above=["lists_push_w", "tables_leave", "everything_left"], step=7 * 4 * 8 + 512),
    dict(boundary="bytes > MG_TREE_LDS_MAX without W and st.poly_doubles > 0 (the polynomials leave)", comparison="poly", below=["lists_keep_polynomials"],
         above=["lists_push_polynomials", "everything_left"], step=16),
    dict(boundary="bytes > MG_TREE_LDS_MAX without the polynomials and st.cp_rows > 0 (the root rows leave)", comparison="cp", below=["lists_keep_root_rows"],
         above=["lists_push_root_rows", "everything_left"], step=16),
    dict(boundary="bytes > MG_TREE_LDS_MAX and tables > 0 (the lists' tables leave)", comparison="tables", below=["tables_stay", "lists_push_root_rows"],
         above=["tables_leave", "everything_left"], step=512),
    dict(boundary="bytes > MG_TREE_LDS_MAX on group 4 (the group is halved)", comparison="group4", below=["group4_last", "tables_leave"],
         above=["group2_first", "group2_65_children", "everything_left", "kd_descents_halved"], step=512),
    dict(boundary="bytes > MG_TREE_LDS_MAX on group 2 (down to one child)", comparison="group2", below=["group2_first", "group2_65_children"],
         above=["group1_first", "group1_last"], step=2 * (77 * 8 + 64)),      # (group 2's window is what halving it frees: its first row lies that far inside)
    dict(boundary="bytes > MG_TREE_LDS_MAX on group 1 (the refusal)", comparison="refused", below=["group1_last", "group1_first"], above=["refused_by_group"], step=sc.HENT),
]


def ladder_trace(kind, c, ncp, tables):
    """{comparison: (the bytes compared, whether they were beyond the limit)} for every comparison mg_tree_frames_fit makes on this call
    whose other condition holds (a rung that has nothing to drop compares nothing), and "64k" for the rung taken"""
    traj = c["traj"] > 0
    st = [c["wrows"], c["cp_rows"] if traj else 0, c["poly_doubles"] if traj else 0]
    state = dict(group=TRACK_GROUP, tables=tables)
    bytes_now = lambda: frames_carve(sc.plan_bytes(kind, c, st[0], st[1], st[2]), ncp, state["group"], state["tables"])[2]
    out = {}

    def compare(name, applies):
        b = bytes_now()
        if applies:
            out[name] = (b, b > sc.LDS_MAX)
        return applies and b > sc.LDS_MAX
    if compare("w", st[0] > 0):
        st[0] = 0
    if compare("poly", traj and st[2] > 0):
        st[2] = 0
    if compare("cp", traj and st[1] > 0):
        st[1] = 0
    if compare("tables", state["tables"] > 0):
        state["tables"] = 0
    if compare("group4", ncp > 0):
        state["group"] = 2
        if compare("group2", True):
            state["group"] = 1
            compare("refused", True)
    b = bytes_now()
    if b <= sc.LDS_MAX:
        out["64k"] = (b, b > sc.KB64)
    return out


def row_trace(r):
    return ladder_trace(r["kind"], call_of(r, n_keyframes_of(r["build"]), segments_of(r["build"])), PRIMS[r["prim"]][1] * r["n_chan"], table_bytes(r["tables"]))


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
_TRACKS = {}


def _mean_tracks(prim):
    """(op, joint -> (F, 3) positions of the zero latent on the canonical frames, local coordinates)"""
    if prim not in _TRACKS:
        _TRACKS[prim] = _mean_tracks_of(prim)
    return _TRACKS[prim]


def _mean_tracks_of(prim):
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
        if kind in ("keyframe", "keyframes"):
            out += sc.keyframes(int(rest or 1), seed, tracks["Hips"])
        elif kind == "trajectory":       # "trajectory:n_seg": further root trajectories of one list differ in length, path and start
            n_seg = int(rest or 5)
            out.append({"type": "trajectory", "control_points": sc.control_points(tracks["Hips"], n_seg, seed + (n_seg - 5)).tolist(),
                        "min_u": 0.05 if n_seg == 5 else 0.0, "weight": 0.8 if n_seg == 5 else 1.3, "granularity": 1000})
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
    means = np.random.default_rng(4300 + sum(ord(ch) for ch in r["name"]) + 100000 * r.get("seed", 0)).standard_normal((n, L))
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


# ---- KD rows: the tree with its descents, and the descent replayed with every comparison it makes ---------------------------------------------
def kd_tree(r):
    """Row r's tree as a HipClusterTree: the cluster nodes of tree_counts, every leaf with r["kd"] = (KD trees, inner levels of each) as
    test_gpu_kd_cluster_tree._kd_tree builds them (none: a leaf scores its mean)"""
    from test_gpu_kd_cluster_tree import _kd_tree
    counts = np.array(tree_counts(r["tree"]))
    return _kd_tree(counts, (counts == 0).astype(np.int32), tree_means(r), kd_per_leaf=r["kd"][0], kd_levels=r["kd"][1], seed=sum(ord(ch) for ch in r["name"]) % 997 + 1000 * r.get("seed", 0),
                    n_spatial=PRIMS[r["prim"]][0])


def table_of(r):
    """The latents the launch can score, in the order of its records' rows: a feature tree's means, a KD tree's points"""
    if r["kind"] == "kd":
        return kd_tree(r).points[:, :PRIMS[r["prim"]][0]]
    return host_tree(r).means


def kd_replay(tree, values, n, winner=None):
    """HipClusterTree.descend_rows on given per-row values, restated for trees whose leaves hang below the root or ARE the root's children,
    with every set of values the search compares among themselves: (value, row, leaf, evaluations, groups) -- a node's children, the
    level's kept candidates, right against left at every step of a descent, a descent's (cost, depth) heap, the descents of one leaf,
    the leaves' results.  Held to descend_rows itself by tests/test_tree_search_frames_host.py.  winner: a list that is given (e, depth) of the
    winning sample -- e its descent's place among its level's descents (the frontier's leaves in order, MG_KD_GROUP at a time), depth
    the step that scored it (0: the descent's start)."""
    cb, ch, kb, kr, nk = tree.child_begin, tree.children, tree.kd_begin, tree.kd_roots, tree.n_kd
    kl, krt, kin = tree.kd_left, tree.kd_right, tree.kd_inner
    groups, results, evaluations, frontier = [], [], 0, [0]
    while frontier:
        level, e = [], 0
        for c_idx, node in enumerate(frontier):
            if not tree.leaf[node]:
                kids = [int(k) for k in ch[cb[node]:cb[node + 1]]]
                evaluations += len(kids)
                groups.append([values[nk + k] for k in kids])
                level += sorted((values[nk + k], k) for k in kids)[:n]
                continue
            starts = [int(x) for x in kr[kb[node]:kb[node + 1]]] or [nk + node]
            evaluations += len(starts)
            ends = []
            for s in starts:
                heap, visited, cur = [values[s]], [s], (s if s < nk else -1)
                while cur >= 0 and kin[cur]:
                    rc, lc = int(krt[cur]), int(kl[cur])
                    evaluations += 2
                    groups.append([values[rc], values[lc]])
                    cur = lc if values[lc] < values[rc] else rc
                    heap.append(values[cur])
                    visited.append(cur)
                groups.append(heap)
                ends.append((min(heap), visited[int(np.argmin(heap))], e, int(np.argmin(heap))))
                e += 1
            groups.append([v for v, _, _, _ in ends])
            results.append(min(ends)[:2] + (node,) + min(ends)[2:])
        groups.append([v for v, _ in level])
        frontier = [k for _, k in sorted(level)[:n]]
    groups.append([x[0] for x in results])
    value, row, leaf, e, depth = min(results)
    if winner is not None:
        winner.append((e, depth))
    return value, row, leaf, evaluations, groups


def smallest_gap(groups):
    """(the smallest distance between two values the search compares, the largest |value| among them)"""
    gap, largest = np.inf, 0.0
    for g in groups:
        s = np.sort(np.asarray(g, dtype=np.float64))
        if len(s) > 1:
            gap = min(gap, float(np.min(np.diff(s))))
        if len(s):
            largest = max(largest, float(np.max(np.abs(s))))
    return gap, largest


# ---- a sweep row's oracle, once ------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_of(r):
    """Row r's objective of every row of table_of(r) by the oracle alone, and the descent replayed on it: dict(cons, values, value, row,
    leaf, evaluations, groups | gaps, slot).  slot: where in its chunk of 64 the score that decides for the winner stands (its place among the
    level's children; for KD descents the descent's start or the pair of its step).  groups: what a row with KD descents compares (kd_replay); gaps: replay's levels for every other row.  Computed once per process and never changed: the host file's conditioning and the GPU file share it."""
    if r["name"] not in _ORACLE:
        cons = constraints_of(r)
        values = oracle_values(r, cons, table_of(r))
        gaps = None
        if r["kd"] != (0, 0):
            won = []
            value, row, leaf, n_eval, groups = kd_replay(kd_tree(r), values, r["n_cand"], won)
            e, depth = won[0]
            slot = e % sc.KD_GROUP if depth == 0 else 2 * (e % sc.KD_GROUP)       # (a step scores descent t's children in slots 2t and 2t + 1)
        else:       # (a KD row without KD trees scores its leaves' means: the same rows, the same descent as the feature tree's)
            tree = host_tree(r)
            value, leaf, n_eval, gaps = replay(tree, values[kd_tree(r).n_kd:] if r["kind"] == "kd" else values, r["n_cand"])
            row, groups = int(tree.first_index[leaf]), None
            slot = (list(tree.children[tree.child_begin[0]:tree.child_begin[1]]).index(leaf)) % sc.CHUNK      # (the sweep's trees are flat)
            if r["kind"] == "kd":       # (... but the kept leaves then score their own means once more, and the record's row counts the tree's points)
                value, row, leaf, n_eval, _ = kd_replay(kd_tree(r), values, r["n_cand"])
        values.setflags(write=False)
        _ORACLE[r["name"]] = dict(cons=cons, values=values, value=float(value), row=int(row), leaf=int(leaf), evaluations=int(n_eval), groups=groups, gaps=gaps, slot=int(slot))
    return _ORACLE[r["name"]]


# ---- calls of several searches -------------------------------------------------------------------------------------------------------------------
def merged_fit(kind, rows, lists=None):
    """What the plan query reports for ONE call of these rows' searches (lists[i] False: search i goes without its per-frame list):
    mg_tree_gather's maxima, the most control points and the most table bytes over the searches with a list (no tables in LDS where one
    search's tables are beyond MG_FC_LDS_MAX)"""
    lists = [True] * len(rows) if lists is None else lists
    calls = [call_of(r, n_keyframes_of(r["build"]), segments_of(r["build"])) for r in rows]
    c = {k: max(x[k] for x in calls) for k in calls[0]}
    if any(x["wrows"] == 0 for x in calls):
        c["wrows"] = 0
    with_list = [r for r, on in zip(rows, lists) if on]
    ncp = max([(r.get("dims") or PRIMS[r["prim"]])[1] * r["n_chan"] for r in with_list] + [0])
    tabs = [table_bytes(r["tables"]) for r in with_list]
    fits = all(t > 0 or not r["tables"] for r, t in zip(with_list, tabs))
    return frames_fit(kind, c, ncp, max(tabs + [0]) if fits else 0)


def neighbour(kind, rows, group, lists=None):
    """A search on a wide Hips primitive (three keyframes, a collision-avoidance position) beside which the call of `rows` stands on track
    group `group`: the fewest latents, then the fewest children, by the restated plan"""
    build = ["keyframes:3", "ca:Hips:12"]
    for L in range(150, 400):
        for c in range(7, 121):
            cand = dict(_shape(kind, ("flat", c), 2, None, dims=(L, 7, 7)), build=build, n_chan=7, tables=[])
            if _group(merged_fit(kind, list(rows) + [cand], None if lists is None else list(lists) + [True])) == group:
                return _row("neighbour-%s-%d-%d" % (kind, L, c), kind, ("flat", c), 2, wide("hips", L), 0, build, 7, [(F, 1)])
    raise AssertionError("no neighbour puts the call on group %d" % group)
