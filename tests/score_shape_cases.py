"""The keyframe scorers' route restated, and the table of shapes on both sides of every one of its comparisons.

Shared by tests/test_score_shapes_host.py (no device: the restatement against the C text, the table against the restatement, the
reference-only conditions on the oracle alone) and tests/test_gpu_score_shapes.py (the same rows on the device, with a ledger of the
routes they took).

score_route restates mg_score_route_of (csrc/mg_score_route.h), set_rows the row counts of csrc/mg_constraint_image.h.  ROWS is the
table: every row names the kernels it exists for (`claims`), and the CPU companion asserts from the restatement that it takes them.
"""
import numpy as np

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
from oracle import c_oracle
from oracle import mg_oracle as orc

MG_ERR_INVALID_ARGUMENT = _capi.MG_ERR_INVALID_ARGUMENT
MG_ERR_UNSUPPORTED = _capi.MG_ERR_UNSUPPORTED

# ---- constants of mg_score_route.h, mg_score.hip and the C ABI (pinned by test_restatement_matches_the_source) ------------------------
MG_SCORE_WIDE_MIN_B = 49152
MG_SET_PARAMS_MAX = 496
MG_MAX_CHAIN = 32
MG_MAX_POSE_POINTS = 64
MG_MAX_KK = 16
KB64, KB150 = 64 * 1024, 150 * 1024
WORKGROUP_BOUND = 0x7fffffff


def k_steps(width):
    """mg_primitive_create: the even number of 4-wide k-steps that hold `width` columns, 0 past 64."""
    return (((width + 3) // 4 + 1) // 2) * 2 if width <= 4 * MG_MAX_KK else 0


class Refused(Exception):
    def __init__(self, status, why):
        Exception.__init__(self, why)
        self.status = status


def score_route(L, rows, n, B, kernel_opt=0, force_valu=0):
    """mg_score_route_of for a primitive of L components and a set of n constraints owning `rows` rows: dict(kernel, lds_bytes,
    lds_opt_in, workgroups, rows, row_tiles) as Primitive.score_plan reports it.  Raises Refused as the library does."""
    KK = k_steps(L)
    has_wpack = KK > 0 and rows > 0                      # mg_constraint_image_build: `if (KK > 0 && rows_total > 0)`
    RT = (rows + 15) // 16 if has_wpack else 0
    shown = dict(rows=rows if has_wpack else 0, row_tiles=RT)
    if has_wpack and not force_valu and KK in range(2, 17, 2):
        wide = kernel_opt == 2 or (kernel_opt == 0 and B >= MG_SCORE_WIDE_MIN_B)
        wide_lds = 4 * 64 * (RT * 16 + 1) * 8
        fits = True
        if wide and wide_lds <= 64 * 1024:
            grid = (B + 255) // 256
            if grid <= WORKGROUP_BOUND:
                return dict(kernel="wide", lds_bytes=wide_lds, lds_opt_in=False, workgroups=grid, **shown)
            fits = False
        lds = 4 * (16 * (RT * 16 + 1) + max(n, 1) * 16) * 8
        grid = (B + 63) // 64
        if fits and lds <= 150 * 1024 and grid <= WORKGROUP_BOUND:
            return dict(kernel="tile", lds_bytes=lds, lds_opt_in=lds > 64 * 1024, workgroups=grid, **shown)
    lds = (64 * (L + 1) + max(n, 1) * 64) * 8
    grid = (B + 63) // 64
    if lds > 150 * 1024:
        raise Refused(MG_ERR_UNSUPPORTED, "mg_score_constraints: n_components %d x %d constraints too large for LDS" % (L, n))
    if grid > WORKGROUP_BOUND:
        raise Refused(MG_ERR_UNSUPPORTED, "mg_score_constraints: too many samples")
    return dict(kernel="valu", lds_bytes=lds, lds_opt_in=lds > 64 * 1024, workgroups=grid, **shown)


def chain_links(skel, joint):
    """Links of the chain root .. joint: its joints less one."""
    joints = skel[0]
    parent = {j[0]: j[1] for j in joints}
    m, j = 0, joint
    while parent[j] is not None:
        m, j = m + 1, parent[j]
    return m


def set_rows(cons, D, skel=None, align=None, align_joint=None):
    """Rows of the fused keyframe matrices a set owns (mg_constraint_image.h): a root constraint min(7, n_dim); an FK constraint
    [3 +] 4 max(m, 1) [+ 4 max(m2, 1)]; a pose one or two blocks of 3 + 4 animated joints; the alignment 3 (start pose) or 3 + 4 len."""
    rows = 0
    for c in cons:
        t = c["type"]
        if t in ("position", "direction", "value_position"):
            rows += min(7, D)
        elif t == "pose":
            rows += (3 + 4 * len(skel[1])) * (2 if c.get("velocity") is not None else 1)
        else:
            links = chain_links(skel, c["joint"]) if skel is not None else 0
            own = t in ("joint_orientation", "look_at", "value_heading") or (t == "joint_position" and c.get("offset") is not None)
            rows += (3 if t in ("joint_position", "joint_midpoint", "look_at") else 0) + 4 * max(links + (1 if own else 0), 1)
            if t == "joint_midpoint":
                rows += 4 * max(chain_links(skel, c["joint2"]), 1)
    if align == "start_pose":
        rows += 3
    elif align == "previous":
        rows += 3 + 4 * ((chain_links(skel, align_joint) if skel is not None else 0) + 1)
    return rows


# ---- the table --------------------------------------------------------------------------------------------------------------------
F, NB = 12, 7
TL = float(F - 1)
WIDE_B = (1, 15, 16, 17, 48, 49, 63, 64, 65, 255, 256, 257)
TILE_B = (1, 15, 16, 17, 63, 64, 65, 257)
CHAINED_B = (17, 65)
START_POSE = {"position": [55.0, 7.5, -80.0], "orientation": [0.0, 37.5, 0.0]}
ROOT_SKEL = ([("Hips", None, (0.0, 0.0, 0.0))], ["Hips"])
LINE_JOINTS, LINE_FIXED = 33, (5, 17)                    # one line of 33 joints; joints 5 and 17 are not animated: identity rows


def line_skeleton(n=LINE_JOINTS):
    joints = [("j%d" % i, None if i == 0 else "j%d" % (i - 1), (0.0, 0.0, 0.0) if i == 0 else (0.5 * (i % 3), 3.0, 0.25 * ((i + 1) % 2))) for i in range(n)]
    return joints, [j[0] for i, j in enumerate(joints) if i not in LINE_FIXED]


LINE_D = 3 + 4 * (LINE_JOINTS - len(LINE_FIXED))


def _pos(i, t=None, axes=3):
    target = [20.0 + 7.0 * i, (35.0 - 3.0 * i) if i % 3 else None, -15.0 + 4.0 * i]
    return {"type": "position", "t": TL * (i % 5 + 1) / 5.0 if t is None else t, "weight": 0.5 + 0.125 * (i % 4), "target": target}


def _dir(i, t=None):
    return {"type": "direction", "t": TL * (i % 4 + 1) / 4.0 if t is None else t, "weight": 0.25 + 0.25 * (i % 3), "target": [0.3 + 0.2 * i, -1.0 + 0.4 * i]}


def _orient(i):
    q = np.array([1.0, 0.3 * (i + 1), -0.2 * i, 0.15 * (i - 1)])
    return {"type": "joint_orientation", "joint": "Hips", "t": TL * (i + 1) / 4.0, "weight": 1.0 + 0.5 * i, "orientation": list(q / np.linalg.norm(q)),
            "ref_dir": (0.0, 0.0, 1.0)}


def _mixed(n):
    return [(_dir(i) if i % 2 else _pos(i)) for i in range(n)]


def _pose(n_points, velocity):
    rng = np.random.default_rng(700 + n_points)
    joints = ["j%d" % ((7 * i + 32) % LINE_JOINTS) for i in range(n_points)]
    return {"type": "pose", "t": 4.25, "weight": 1.5, "joints": joints, "points": (40.0 * rng.standard_normal((n_points, 3))).tolist(),
            "weights": (0.5 + rng.random(n_points)).tolist(), "velocity": [1.5, -0.5, 2.0] if velocity else None}


def _row(name, L, D, cons, claims, batches=(17,), skel=None, align=None, oracle="root", ld_extra=0, chained=False, expect=None, seed=None):
    return dict(name=name, L=L, D=D, cons=cons, claims=set(claims), batches=tuple(batches), skel=skel, align=align, oracle=oracle, ld_extra=ld_extra,
                chained=chained, expect=expect, seed=seed)


def _rows():
    R = []
    ALL = ("wide", "tile", "valu")
    # sets of at most 16 rows: the wide kernel's
    R.append(_row("wide14", 8, 7, [_pos(0, TL), _dir(0, TL)], ALL, WIDE_B))
    R.append(_row("wide16", 8, 7, [_orient(i) for i in range(4)], ALL, (1, 17, 64, 65, 257), skel=ROOT_SKEL, oracle="skeleton"))
    R.append(_row("tile17", 8, 7, [_pos(1, TL), _dir(1, TL / 2.0)], ("tile", "valu"), TILE_B, align="start_pose", oracle="start_pose", skel=ROOT_SKEL))
    R.append(_row("wide15", 6, 7, [{"type": "look_at", "joint": "Hips", "t": 3.5, "weight": 0.7, "target": [100.0, 150.0, 30.0], "ref_dir": (0.0, 0.0, 1.0)}, _orient(1),
                                   {"type": "value_heading", "t": TL, "weight": 1.0, "axis": 2, "joint": "Hips", "ref_dir": (0.0, 0.0, 1.0)}], ALL, (17, 65),
                  skel=ROOT_SKEL, oracle="skeleton"))
    R.append(_row("wide14_aligned", 8, 7, [_pos(2, TL)], ALL, CHAINED_B, skel=ROOT_SKEL, align="previous", oracle="aligned", chained=True))
    R.append(_row("wide14_aligned_dir", 12, 7, [_dir(2, TL)], ALL, CHAINED_B, skel=ROOT_SKEL, align="previous", oracle="aligned", chained=True))
    R.append(_row("wide15_d3", 5, 3, [_pos(i) for i in range(5)], ALL, (16, 17, 65)))
    # the number of constraints against the 64 lanes of a tile wave and the four waves of a VALU workgroup
    R.append(_row("n0", 8, 7, [], ("valu",), (1, 65), oracle="zero"))
    R.append(_row("n1", 8, 7, _mixed(1), ALL, (17, 65)))
    R.append(_row("n3", 8, 7, _mixed(3), ("tile", "valu"), TILE_B))
    R.append(_row("n4", 9, 7, _mixed(4), ("tile", "valu"), (17, 65)))
    R.append(_row("n5", 8, 7, _mixed(5), ("tile", "valu"), (17, 65)))
    # the tile kernel's LDS, 512 (16 RT + 1 + n): three-row position constraints on n_dim = 3
    for n, claims in ((TILE_64K_N, ("tile", "valu")), (TILE_64K_N + 1, ("tile:opt_in", "valu")), (TILE_150K_N, ("tile:opt_in", "valu")),
                      (TILE_150K_N + 1, ("valu:fallthrough", "valu"))):
        R.append(_row("tile_lds_n%d" % n, 8, 3, [_pos(i) for i in range(n)], claims))
    # the VALU kernel's LDS, 512 (L + 1 + n), at L = 65 where it is the only route
    for n, claims in ((VALU_64K_N, ("valu",)), (VALU_64K_N + 1, ("valu:opt_in",)), (VALU_150K_N, ("valu:opt_in",)), (VALU_150K_N + 1, ("refused:lds",))):
        R.append(_row("valu_lds_n%d" % n, 65, 3, [_pos(i) for i in range(n)], claims, expect=MG_ERR_UNSUPPORTED if n > VALU_150K_N else None))
    R.append(_row("L65", 65, 7, _mixed(3), ("valu",), TILE_B))
    # rows wider than the primitive, NaN in the extra columns
    R.append(_row("wide_ld", 5, 7, [_pos(3, TL), _dir(3, TL)], ALL, (17, 65), ld_extra=4))
    R.append(_row("wide_ld_L65", 65, 7, _mixed(2), ("valu",), (17,), ld_extra=3))
    # chains of MG_MAX_CHAIN links on the device
    line = line_skeleton()
    last, fk = "j%d" % (LINE_JOINTS - 1), ("tile:opt_in", "valu")   # (a chain of 32 links alone is nine row tiles: past 64 KiB)
    R.append(_row("chain32", 8, LINE_D, [{"type": "joint_position", "joint": last, "t": 6.5, "weight": 2.0, "target": [30.0, 80.0, None]}], fk, skel=line, oracle="skeleton"))
    R.append(_row("chain32_midpoint", 8, LINE_D, [{"type": "joint_midpoint", "joint": last, "joint2": "j3", "t": 2.75, "weight": 1.25, "target": [10.0, 50.0, -5.0]}], fk,
                  skel=line, oracle="skeleton"))
    R.append(_row("chain31_relative", 8, LINE_D, [{"type": "joint_position", "joint": "j%d" % (LINE_JOINTS - 2), "t": 9.0, "weight": 0.5, "target": [5.0, 90.0, 12.0],
                                                  "offset": [1.5, -2.0, 0.75]}], fk, skel=line, oracle="skeleton"))
    for n_points in (1, MG_MAX_POSE_POINTS):
        for velocity in (False, True):
            R.append(_row("pose%d%s" % (n_points, "_velocity" if velocity else ""), 8, LINE_D, [_pose(n_points, velocity)], fk, skel=line, oracle="skeleton"))
    R.append(_row("chain33", 8, LINE_D + 4, [{"type": "joint_position", "joint": "j%d" % LINE_JOINTS, "t": 6.5, "weight": 2.0, "target": [30.0, 80.0, None]}],
                  ("refused:chain",), skel=line_skeleton(LINE_JOINTS + 1), oracle=None, expect=MG_ERR_INVALID_ARGUMENT))
    for k, r in enumerate(R):
        if r["seed"] is None:
            r["seed"] = 5100 + 10 * k                    # the primitive; its latents seed + 1; its previous frame / per-candidate alignments seed + 2
    return R


def _first_n(lds_of, limit):
    n = 1
    while lds_of(n + 1) <= limit:
        n += 1
    return n


# the exact n at the thresholds, from the restatement's own arithmetic
TILE_64K_N = _first_n(lambda n: 512 * (16 * ((3 * n + 15) // 16) + 1 + n), KB64)
TILE_150K_N = _first_n(lambda n: 512 * (16 * ((3 * n + 15) // 16) + 1 + n), KB150)
VALU_64K_N = _first_n(lambda n: 512 * (65 + 1 + n), KB64)
VALU_150K_N = _first_n(lambda n: 512 * (65 + 1 + n), KB150)
UPDATE_N = MG_SET_PARAMS_MAX // 8                        # the largest set without an alignment whose values travel as kernel arguments

ROWS = _rows()
IDS = [r["name"] for r in ROWS]
BY_NAME = {r["name"]: r for r in ROWS}
AUTO_B = (MG_SCORE_WIDE_MIN_B - 1, MG_SCORE_WIDE_MIN_B)   # the automatic switch under option 0
AUTO_SCALE = 0.2                                         # of its latents: 49 152 headings that all stay well away from the target and its opposite


def _auto_row():
    """The 14-row set for the automatic switch: position + direction, the direction's target square to the mean motion's heading at the
    keyframe, so that none of 49 152 candidates comes within 1e-6 of cosine +-1 (among as many headings drawn freely some would)."""
    row = _row("auto14", 8, 7, [_pos(0, TL), _dir(0, TL)], ("auto:tile", "auto:wide"), AUTO_B, seed=6900)
    op = orc.OraclePrimitive(model(row))
    frame = orc.spline_frames(op.knots, op.back_project_spatial_coeffs(np.zeros(8)), [TL])[0]
    p = orc.quaternion_rotate(frame[3:7], (0.0, 0.0, 1.0))
    row["cons"][1]["target"] = [float(np.round(-p[2], 3)), float(np.round(p[0], 3))]
    return row


def auto_latents(B):
    return (AUTO_SCALE * np.random.default_rng(6901).standard_normal((B, 8))).astype(np.float32).astype(np.float64)

# every (kernel, latent dtype, what is written) the dispatch can select
COMBOS = {(k, lat, out) for k in ("wide", "tile", "valu") for lat in ("float32", "float64") for out in ("out_f64", "out_f32", "res", "res_align_cand")}
SPECIALS = {"tile:opt_in", "valu:opt_in", "valu:fallthrough", "refused:lds", "refused:chain", "auto:tile", "auto:wide"}


def row_rows(row):
    return set_rows(row["cons"], row["D"], row["skel"], row["align"], "Hips" if row["align"] == "previous" else None)


def routes_of(row):
    """(label, option, value) the device test drives the row through: the tile kernel, the wide one where the set fits it, the VALU one."""
    out = [("tile", _capi.MG_OPT_SCORE_KERNEL, 1)]
    if 0 < row_rows(row) <= 16 and k_steps(row["L"]) > 0:
        out.append(("wide", _capi.MG_OPT_SCORE_KERNEL, 2))
    out.append(("valu", _capi.MG_OPT_FORCE_VALU_SCORE, 1))
    return out


def row_plan(row, B, label):
    """The restated plan of a row under one of routes_of's options (label "auto": option 0)."""
    kw = {"tile": dict(kernel_opt=1), "wide": dict(kernel_opt=2), "valu": dict(force_valu=1), "auto": {}}[label]
    return score_route(row["L"], row_rows(row), len(row["cons"]), B, **kw)


def claimed_combos(row):
    """The COMBOS a row claims: the kernels its routes select x both latent dtypes x what its calls write."""
    outs = ["out_f64", "out_f32", "res"] + (["res_align_cand"] if row["chained"] else [])
    if row["expect"] is not None:
        return set()
    kernels = {row_plan(row, max(row["batches"]), label)["kernel"] for label, _, _ in routes_of(row)}
    return {(k, lat, o) for k in kernels for lat in ("float32", "float64") for o in outs}


def model(row):
    return synthetic.make_primitive(seed=row["seed"], n_components=row["L"], n_frames=F, n_basis=NB, n_dim=row["D"], n_gmm=1, name=row["name"])


def latents(row, B=None):
    """(B, L) float64 holding float32 values, so that both latent dtypes score the same numbers."""
    B = max(row["batches"]) if B is None else B
    return (0.7 * np.random.default_rng(row["seed"] + 1).standard_normal((B, row["L"]))).astype(np.float32).astype(np.float64)


def previous_frame(row):
    prev = np.zeros(row["D"])
    rng = np.random.default_rng(row["seed"] + 2)
    prev[:3] = [120.0, 3.0, -40.0]
    prev[3:7] = [0.8, 0.1, 0.55, -0.2] + 0.05 * rng.standard_normal(4)
    return prev


def alignment_of(row):
    """The ConstraintSet `alignment` of a row, or None."""
    if row["align"] == "start_pose":
        return alignment_from_start_pose(dict(START_POSE, position=list(START_POSE["position"])))
    if row["align"] == "previous":
        return _capi.Skeleton(*ROOT_SKEL).alignment_to(previous_frame(row), "Hips")
    return None


def unit_headings(n, seed):
    """n distinct (x, z) whose norm, computed as mg_alignment_record computes it, is exactly 1: the record divides by it, the per-candidate
    table is taken as it stands, and the two must be the same numbers."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        a = rng.uniform(0.0, 2.0 * np.pi)
        x, z = float(np.cos(a)), float(np.sin(a))
        if np.sqrt(x * x + z * z) == 1.0:
            out.append((x, z))
    return np.array(out)


def align_cand_of(row, B):
    """(B, 4): previous unit heading (x, z) and previous root position (x, z), different for every candidate."""
    rng = np.random.default_rng(row["seed"] + 2)
    return np.hstack([unit_headings(B, row["seed"] + 3), 60.0 * rng.standard_normal((B, 2))])


def root_cons_matrix(cons):
    """The C oracle's rows {type, t, weight, a, b, c | rx, ry, rz} of position and direction constraints."""
    out = []
    for c in cons:
        if c["type"] == "position":
            out.append([0, c["t"], c["weight"]] + [np.nan if v is None else v for v in c["target"]] + [0.0, 0.0])
        else:
            out.append([1, c["t"], c["weight"], c["target"][0], c["target"][1], 0.0, 0.0, 1.0])
    return np.array(out, dtype=np.float64).reshape(len(cons), 8)


def oracle_of(row, S):
    """("errors", (B,)) or ("residuals", (B, n)) of the row's oracle on latents S, and the bounds the suite holds this scorer to."""
    data = model(row)
    kind = row["oracle"]
    if kind == "zero":
        return "errors", np.zeros(len(S)), (0.0, 0.0)
    if kind == "root":
        return "errors", c_oracle.COraclePrimitive(data).keyframe_errors_f64(S, root_cons_matrix(row["cons"])), (1e-10, 1e-9)
    op = orc.OraclePrimitive(data)
    joints, animated = row["skel"]
    if kind == "start_pose":
        return "residuals", op.start_pose_residuals(S, row["cons"], dict(START_POSE, position=list(START_POSE["position"])), joints, animated), (1e-9, 1e-8)
    if kind == "aligned":
        return "residuals", op.aligned_residuals(S, row["cons"], previous_frame(row), joints, animated, "Hips"), (1e-9, 1e-8)
    plain = [c for c in row["cons"] if c["type"] != "value_heading"]
    res = np.zeros((len(S), len(row["cons"])))
    cols = [i for i, c in enumerate(row["cons"]) if c["type"] != "value_heading"]
    res[:, cols] = op.skeleton_residuals(S, plain, joints, animated)
    for i, c in enumerate(row["cons"]):
        if c["type"] == "value_heading":                 # the unit heading's component: the oracle's node_heading on the oracle's frame
            for b in range(len(S)):
                frame = orc.spline_frames(op.knots, op.back_project_spatial_coeffs(S[b]), [c["t"]])[0]
                res[b, i] = c["weight"] * orc.node_heading(frame, joints, animated, c["joint"], c["ref_dir"])[{0: 0, 2: 1}[c["axis"]]]
    return "residuals", res, (1e-10, 1e-8)


def conditioning(row, S):
    """On the oracle alone: (the largest |cosine| any acos of the row is fed, the smallest heading / direction norm before it is made unit)
    over the candidates S."""
    if row["oracle"] in ("zero", None):
        return 0.0, np.inf
    op = orc.OraclePrimitive(model(row))
    joints, animated = row["skel"] if row["skel"] is not None else ROOT_SKEL
    worst_cos, least = 0.0, np.inf
    times = sorted({c["t"] for c in row["cons"]})
    basis = {t: orc.spline_frames(op.knots, np.eye(op.n_basis), [t])[0] for t in times}
    coeffs = (op.mean_vector[None, :] + S[:, :op.n_components] @ op.eigen_vectors.T).reshape(len(S), op.n_basis, op.n_dim)
    assert np.allclose(coeffs[0], op.back_project_spatial_coeffs(S[0]), rtol=1e-12, atol=1e-12)
    start = dict(START_POSE, position=list(START_POSE["position"]))
    for b in range(len(S)):
        cp = coeffs[b]
        if row["align"] == "previous":
            least = min(least, float(np.hypot(*(orc.joint_global_orientation(cp[0], joints, animated, "Hips") @ np.array([0.0, 0.0, 1.0]))[[0, 2]])))
            cp = orc.align_coeffs_to_previous_frame(cp, previous_frame(row), joints, animated, "Hips")
        elif row["align"] == "start_pose":
            cp = orc.align_coeffs_to_start_pose(cp, start)
        for c in row["cons"]:
            frame = basis[c["t"]] @ cp
            t = c["type"]
            if t == "direction":
                p = orc.quaternion_rotate(frame[3:7], c.get("ref_dir", (0.0, 0.0, 1.0)))
                m, tg = np.array([p[0], p[2]]), np.asarray(c["target"], dtype=np.float64)
                least = min(least, float(np.linalg.norm(m)), float(np.linalg.norm(tg)))
                worst_cos = max(worst_cos, abs(float(np.dot(m, tg) / (np.linalg.norm(m) * np.linalg.norm(tg)))))
            elif t in ("joint_orientation", "look_at", "value_heading"):
                v = orc.joint_global_orientation(frame, joints, animated, c["joint"]) @ np.asarray(c.get("ref_dir", (0.0, 0.0, 1.0)), dtype=np.float64)
                if t == "value_heading":
                    least = min(least, float(np.hypot(v[0], v[2])))
                    continue
                if t == "look_at":
                    w = np.asarray(c["target"], dtype=np.float64) - orc.joint_global_position(frame, joints, animated, c["joint"])
                else:
                    w = orc.quaternion_matrix3(c["orientation"]) @ np.asarray(c.get("ref_dir", (0.0, 0.0, 1.0)), dtype=np.float64)
                least = min(least, float(np.linalg.norm(v)), float(np.linalg.norm(w)))
                worst_cos = max(worst_cos, abs(float(np.dot(v, w) / (np.linalg.norm(v) * np.linalg.norm(w)))))
    return worst_cos, least


# ---- argmin and the winner copy -----------------------------------------------------------------------------------------------------
ARGMIN_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def argmin_cases():
    """name -> (values float64 that float32 holds exactly, tie on purpose)."""
    cases = {}
    for n in ARGMIN_SIZES:
        base = np.random.default_rng(8000 + n).permutation(n).astype(np.float64) + 10.0      # distinct whole numbers
        cases["distinct_%d" % n] = (base, False)
        for where, i in (("first", 0), ("last", n - 1), ("at1024", 1024)):
            if i < n:
                v = base.copy()
                v[i] = 1.0
                cases["min_%s_%d" % (where, n)] = (v, False)
        if n > 1:
            v = base.copy()
            v[0] = v[n - 1] = 2.0
            cases["tie_ends_%d" % n] = (v, True)
    big = np.random.default_rng(8999).permutation(2049).astype(np.float64) + 10.0
    for name, (i, j) in (("tie_one_thread", (7, 7 + 1024)), ("tie_across_lanes", (9, 10)), ("tie_across_waves", (5, 69)), ("tie_late_thread_first", (1030, 2047))):
        v = big.copy()
        v[i] = v[j] = 3.0
        cases[name] = (v, True)
    cases["negative_zero_first"] = (np.array([-0.0, 0.0, 5.0]), True)
    cases["positive_zero_first"] = (np.array([0.0, -0.0, 5.0]), True)
    cases["all_nan"] = (np.full(65, np.nan), True)
    cases["all_inf"] = (np.full(65, np.inf), True)
    v = big.copy()
    v[1500] = -np.inf
    cases["one_negative_inf"] = (v, False)
    v = big.copy()
    v[::2] = np.nan
    cases["nan_every_other"] = (v, False)
    return cases


ARGMIN_CASES = argmin_cases()
AUTO_ROW = _auto_row()
WINNER_WIDTHS = (1, 64, 65)
