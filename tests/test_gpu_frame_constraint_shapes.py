"""The per-frame constraint scorers, the joint tracks and the options-list kernel (csrc/mg_frame_constraints.hip) across their shape
edges, against the Python oracle.

tests/test_gpu_frame_constraints.py holds these kernels to the oracle at one shape (the 'walk' model, granularity 1000, tables of 8 KB,
n_frames = T, even T).  This module walks the branches that shape never takes:

* the host decisions restated -- place_tables (mg_fc_place_tables: one place per table, counts rounded up to even, arc tables only for
  the two types that walk by arc length, 150 KB), list_launches (mg_score_frame_constraints' groups of MG_FC_LIST_MAX, a joint trajectory
  up to 65 536 candidates a launch of its own) and track_lds (mg_joint_tracks' LDS bytes) -- and pinned to the C source line by line;
  TABLE_CASES / LIST_SIZES say, for every GPU case, which route it claims to take, and a CPU test holds the claim to the restatement;
* the six scorers on synthetic float64 tracks through mg_score_frame_constraint / mg_score_frame_constraints, against
  oracle.mg_oracle.per_frame_track_residuals times the weight at |device - oracle| <= 1e-9 max(1, max |oracle|) (the bound of
  test_gpu_frame_constraints._check), with NaN-payload guards round every output;
* mg_joint_tracks against the chain mg_back_project_frames_f64 -> mg_align_frames -> mg_joint_positions (bit for bit) and against the
  oracle's frames, alignment and forward kinematics (1e-9), over D in {3, 6, 7, 11, 79}, NB in {4, 7}, L in {1, 3, 40}, every B mod 4;
* mg_options_frame_lists: the first minimum over errors the test wrote (ties, NaN, +-inf, 129 workgroups per option, the counters'
  place moving between calls) and real lists on three primitives against the per-option launches, bit for bit.

LEDGER records the classes of route the GPU tests ran; test_the_ledger_covers_every_route (last) fails when one stops being reached.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
from oracle import mg_oracle as orc
from test_gpu_trajectory_shapes import FILL, Guarded, _bits64

TOL = 1.0e-9          # test_gpu_frame_constraints._check: float64 end to end

# ---- the host decisions, restated (kept in step with mg_frame_constraints.hip by test_restatement_matches_the_source) -------------
MG_FC_BLOCK = 64
MG_FC_LIST_MAX = 4
MG_FC_LDS_MAX = 150 * 1024
MG_FC_TRAJ_ALONE_MAX_B = 65536
MG_TRACK_CANDS = 4
MG_TRACK_BLOCK = 128
MG_OPT_LISTS_MAX = 24
MG_TRACK_LDS_MAX = 160 * 1024 - 64
KB64 = 64 * 1024           # dynamic LDS a kernel gets without the large-LDS opt-in
CA, DISCRETE, LOCAL, SET, ROTATION, JOINT_TRAJ = (_capi.MG_FRAME_CA_POSITION, _capi.MG_FRAME_DISCRETE_TRAJECTORY, _capi.MG_FRAME_LOCAL_TRAJECTORY,
                                                  _capi.MG_FRAME_TRAJECTORY_SET, _capi.MG_FRAME_JOINT_ROTATION, _capi.MG_FRAME_JOINT_TRAJECTORY)


def place_tables(constraints, dedup=True):
    """mg_fc_place_tables.  constraints: [(type, [(handle tag, n_seg, G), ...])]; returns (LDS bytes or 0, route) with route one of
    'none' (no tables), 'lds' (<= 64 KB), 'optin' (64 KB .. 150 KB: needs the large-LDS opt-in), 'global' (past 150 KB)."""
    seen, doubles = set(), 0

    def place(key, count):
        nonlocal doubles
        if dedup and key in seen:
            return
        seen.add(key)
        doubles += (count + 1) & ~1
    for kind, trajs in constraints:
        arcs = kind in (LOCAL, SET)
        for tag, n_seg, G in trajs:
            place((tag, "poly"), n_seg * 12 + 3)
            if arcs:
                place((tag, "arc"), G + 1)
    if doubles == 0:
        return 0, "none"
    if doubles * 8 > MG_FC_LDS_MAX:
        return 0, "global"
    return doubles * 8, "lds" if doubles * 8 <= KB64 else "optin"


def list_launches(types, B):
    """mg_score_frame_constraints' grouping loop: [('points' | 'list', [indices])] in launch order."""
    out, k0, n = [], 0, len(types)
    while k0 < n:
        if types[k0] == JOINT_TRAJ and B <= MG_FC_TRAJ_ALONE_MAX_B:
            out.append(("points", [k0]))
            k0 += 1
            continue
        group = []
        while len(group) < MG_FC_LIST_MAX and k0 + len(group) < n:
            i = k0 + len(group)
            if group and types[i] == JOINT_TRAJ and B <= MG_FC_TRAJ_ALONE_MAX_B:
                break
            group.append(i)
        out.append(("list", group))
        k0 += len(group)
    return out


def track_lds(NB, n_chan, L, D):
    """mg_track_fill_args' LDS bytes; None where the entry reports MG_ERR_UNSUPPORTED."""
    lds = MG_TRACK_CANDS * (NB * n_chan + L + 8) * 8 + D * 4 + 16
    return None if lds > MG_TRACK_LDS_MAX else lds


def effective_frames(n_frames, T):
    """mg_fc_args_from_desc / mg_frame_constraint_width: 0 and anything from T on mean T."""
    return n_frames if 0 < n_frames < T else T


def _source(name="mg_frame_constraints.hip"):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "morphablegraphs_amd", "csrc", name)).read()


def test_restatement_matches_the_source():
    """Every constant and every comparison restated above, pinned to its line in mg_frame_constraints.hip."""
    src = _source()
    for name, value in (("MG_FC_BLOCK", MG_FC_BLOCK), ("MG_FC_LIST_MAX", MG_FC_LIST_MAX), ("MG_TRACK_CANDS", MG_TRACK_CANDS),
                        ("MG_TRACK_BLOCK", MG_TRACK_BLOCK), ("MG_OPT_LISTS_MAX", MG_OPT_LISTS_MAX)):
        m = re.search(r"#define %s (\d+)\b" % name, src)
        assert m and int(m.group(1)) == value, name
    m = re.search(r"#define MG_FC_LDS_MAX \((\d+) \* 1024\)", src)
    assert m and int(m.group(1)) * 1024 == MG_FC_LDS_MAX
    assert _capi.MG_FRAME_LIST_MAX == MG_FC_LIST_MAX
    assert set(re.findall(r"B <= (\d+)\b", src)) == {str(MG_FC_TRAJ_ALONE_MAX_B)} and len(re.findall(r"B <= 65536\b", src)) == 2
    m = re.search(r"if \(lds > (\d+) \* 1024 - (\d+)\) \{ mg_set_error\(\"%s: %d basis functions", src)
    assert m and int(m.group(1)) * 1024 - int(m.group(2)) == MG_TRACK_LDS_MAX
    place = src[src.index("static size_t mg_fc_place_tables("):src.index("static int mg_fc_attributes(")]
    for line in ("for (int i = 0; i < n_seen; i++) if (seen[i].ptr == ptr) return seen[i].off;",
                 "doubles += (count + 1) & ~(size_t)1;",
                 "const bool arcs = c[i].type == MG_FRAME_LOCAL_TRAJECTORY || c[i].type == MG_FRAME_TRAJECTORY_SET;",
                 "if (!t.poly) continue;",
                 "t.poly_off = place(t.poly, (size_t)t.n_seg * 12 + 3);",
                 "t.arc_off = arcs ? place(t.arc, (size_t)t.G + 1) : -1;",
                 "if (doubles == 0 || doubles * 8 > MG_FC_LDS_MAX) {",
                 "return doubles * 8;"):
        assert line in place, line
    lists = src[src.index('extern "C" int mg_score_frame_constraints('):src.index("// mg_joint_tracks: the joints' global positions")]
    for line in ("bool any = accumulate != 0;",
                 "if (c0 && c0->type == MG_FRAME_JOINT_TRAJECTORY && B <= 65536 && n_joints[k0] == 1 && c0->trajectories[0] && tracks_dev[k0]) {",
                 "errors_dev, any ? 1 : 0,",
                 "L.accumulate = any ? 1 : 0;",
                 "while (L.n < MG_FC_LIST_MAX && k0 + L.n < n_constraints) {",
                 "if (L.n > 0 && c && c->type == MG_FRAME_JOINT_TRAJECTORY && B <= 65536) break;",
                 "const size_t lds = mg_fc_place_tables(L.c, L.n);",
                 "const dim3 grid((unsigned)((B + MG_FC_BLOCK - 1) / MG_FC_BLOCK));",
                 "k0 += L.n;"):
        assert line in lists, line
    for line in ("a.nf = c->n_frames > 0 && c->n_frames < T ? c->n_frames : T;",
                 "case MG_FRAME_LOCAL_TRAJECTORY: case MG_FRAME_TRAJECTORY_SET: return c->n_frames > 0 && c->n_frames < n_times ? c->n_frames : n_times;",
                 "const size_t lds = (size_t)MG_TRACK_CANDS * ((size_t)p->NB * pl->n_chan + p->L + 8) * 8 + (size_t)p->D * 4 + 16;",
                 "if ((((size_t)tr) & 15) == 0) {",
                 "const int64_t bb = b0 + c < a.B ? b0 + c : a.B - 1;",
                 "const int n_here = a.B - b0 < MG_TRACK_CANDS ? (int)(a.B - b0) : MG_TRACK_CANDS;",
                 "for (int q = lane; q < nwg; q += 64) {",
                 "if (lds_l == 0 && has_tables) tables_ok = false;",
                 "const int wg_per = (int)((B + MG_FC_BLOCK - 1) / MG_FC_BLOCK), twg_per = (int)((B + MG_TRACK_CANDS - 1) / MG_TRACK_CANDS);"):
        assert line in src, line
    # the large-LDS opt-in covers the three kernels that stage tables, up to the 160 KB the restated bounds stay under
    assert ("mg_lds_opt_in_once(ctx, MG_LDS_FRAME_CONSTRAINTS, 160 * 1024, mg_frame_constraint_kernel<true>, mg_frame_constraint_list_kernel<true>,"
            in src) and MG_FC_LDS_MAX <= 160 * 1024


# ---- the cases --------------------------------------------------------------------------------------------------------------------
CPS = np.array([[0.0, 0.0, 0.0], [30.0, 2.0, 10.0], [60.0, -1.0, 35.0], [95.0, 3.0, 40.0], [130.0, 0.0, 70.0]])
CPS_B = CPS[:, [2, 1, 0]] * np.array([1.0, -1.0, 0.8]) + np.array([5.0, 1.0, -3.0])
CPS_3 = np.array([[0.0, 1.0, 0.0], [20.0, 0.0, 8.0], [45.0, 2.0, 9.0]])
N_SEG = len(CPS) - 1
G_LDS, G_OPTIN, G_GLOBAL, G_QUARTER, G_SHARED = 1000, 10000, 20000, 6000, 12000
# name -> (constraints as place_tables takes them, the route the GPU case claims); B <= 65 536 everywhere
TABLE_CASES = {
    "local_G1000": ([(LOCAL, [("a", N_SEG, G_LDS)])], "lds"),
    "local_optin_band": ([(LOCAL, [("a", N_SEG, G_OPTIN)])], "optin"),
    "local_global": ([(LOCAL, [("a", N_SEG, G_GLOBAL)])], "global"),
    "set_global_by_sum": ([(SET, [("a", N_SEG, G_OPTIN), ("b", N_SEG, G_OPTIN)])], "global"),
    "set_shared_handle": ([(SET, [("a", N_SEG, G_LDS), ("a", N_SEG, G_LDS), ("b", N_SEG, G_LDS)])], "lds"),
    "four_quarters_list": ([(LOCAL, [(t, N_SEG, G_QUARTER)]) for t in "abcd"], "global"),
    "one_quarter_single": ([(LOCAL, [("a", N_SEG, G_QUARTER)])], "lds"),
    "shared_large_table": ([(LOCAL, [("a", N_SEG, G_SHARED)]), (LOCAL, [("a", N_SEG, G_SHARED)])], "optin"),
    "ca_no_tables": ([(CA, [])], "none"),
    "joint_trajectory_poly_only": ([(JOINT_TRAJ, [("a", 2, G_GLOBAL)])], "lds"),
}
LIST_SIZES = (1, 4, 5, 8, 9)
JT_PLACES = ("first", "middle", "last")
SHAPES = ((1, 1), (63, 2), (64, 3), (65, 7), (130, 8))       # (B, T): every value of both axes
NF_KINDS = ("zero", "one", "t_minus_1", "t", "t_plus_3")


def _nf_of(kind, T):
    return {"zero": 0, "one": 1, "t_minus_1": T - 1, "t": T, "t_plus_3": T + 3}[kind]


def _list_order(n, place):
    """Types of a mixed list of n constraints with the joint trajectory at `place` (the pool of test_lists...)."""
    others = [CA, DISCRETE, LOCAL, SET, ROTATION, CA, LOCAL, DISCRETE][:n - 1]
    at = {"first": 0, "middle": (n - 1) // 2, "last": n - 1}[place]
    return others[:at] + [JOINT_TRAJ] + others[at:]


def test_the_cases_take_the_routes_they_claim():
    """Every GPU case's restated route is the one it is there for; both sides of every comparison appear."""
    routes = {}
    for name, (cons, claim) in TABLE_CASES.items():
        nbytes, route = place_tables(cons)
        assert route == claim, (name, nbytes, route)
        routes[name] = nbytes
    one = (N_SEG * 12 + 3 + 1) * 8
    assert routes["local_G1000"] == one + (G_LDS + 2) * 8 <= KB64
    assert KB64 < routes["local_optin_band"] == one + (G_OPTIN + 2) * 8 <= MG_FC_LDS_MAX
    assert one + (G_GLOBAL + 2) * 8 > MG_FC_LDS_MAX and 2 * (one + (G_OPTIN + 2) * 8) > MG_FC_LDS_MAX
    # a list of four whose own tables each fit (without the opt-in, even) and whose sum does not
    assert 0 < routes["one_quarter_single"] <= KB64 and 4 * routes["one_quarter_single"] > MG_FC_LDS_MAX
    # placed once the shared table fits, placed twice it would not
    assert place_tables(TABLE_CASES["shared_large_table"][0], dedup=False)[1] == "global"
    assert routes["shared_large_table"] == place_tables(TABLE_CASES["shared_large_table"][0][:1])[0]
    assert place_tables(TABLE_CASES["set_shared_handle"][0])[0] == 2 * (one + (G_LDS + 2) * 8)
    # only the two arc-length walkers place arc tables
    assert place_tables([(JOINT_TRAJ, [("a", N_SEG, G_GLOBAL)])]) == (one, "lds") and place_tables([(DISCRETE, [])])[1] == "none"
    # odd counts round up to even, even ones stay
    assert place_tables([(LOCAL, [("a", 1, 2)])])[0] == (16 + 4) * 8 and place_tables([(LOCAL, [("a", 1, 3)])])[0] == (16 + 4) * 8
    # the 150 KB comparison, both sides, at the smallest G on each
    g = MG_FC_LDS_MAX // 8 - (N_SEG * 12 + 4) - 2
    assert place_tables([(LOCAL, [("a", N_SEG, g)])])[1] == "optin" and place_tables([(LOCAL, [("a", N_SEG, g + 2)])])[1] == "global"
    g = KB64 // 8 - (N_SEG * 12 + 4) - 2
    assert place_tables([(LOCAL, [("a", N_SEG, g)])])[1] == "lds" and place_tables([(LOCAL, [("a", N_SEG, g + 2)])])[1] == "optin"
    assert {c for _, c in TABLE_CASES.values()} == {"none", "lds", "optin", "global"}
    # the list grouping: launches per list, with the joint trajectory first, in the middle and last; above 65 536 it stays in its group
    launches = {(n, p): list_launches(_list_order(n, p), 65) for n in LIST_SIZES for p in JT_PLACES}
    assert launches[(1, "first")] == [("points", [0])]
    assert launches[(4, "first")] == [("points", [0]), ("list", [1, 2, 3])]
    assert launches[(4, "last")] == [("list", [0, 1, 2]), ("points", [3])]
    assert launches[(5, "middle")] == [("list", [0, 1]), ("points", [2]), ("list", [3, 4])]
    assert launches[(5, "last")] == [("list", [0, 1, 2, 3]), ("points", [4])]
    assert launches[(8, "first")] == [("points", [0]), ("list", [1, 2, 3, 4]), ("list", [5, 6, 7])]
    assert launches[(9, "last")] == [("list", [0, 1, 2, 3]), ("list", [4, 5, 6, 7]), ("points", [8])]
    assert launches[(9, "middle")] == [("list", [0, 1, 2, 3]), ("points", [4]), ("list", [5, 6, 7, 8])]
    assert [len(v) for v in launches.values()].count(3) >= 4
    assert list_launches(_list_order(9, "middle"), 65537) == [("list", [0, 1, 2, 3]), ("list", [4, 5, 6, 7]), ("list", [8])]
    assert list_launches([JOINT_TRAJ], 65536) == [("points", [0])] and list_launches([JOINT_TRAJ], 65537) == [("list", [0])]
    assert list_launches([CA] * 4, 9) == [("list", [0, 1, 2, 3])] and list_launches([CA] * 5, 9) == [("list", [0, 1, 2, 3]), ("list", [4])]
    # n_frames: 0 and T + 3 mean T; every kind of value on some shape
    for B, T in SHAPES:
        assert [effective_frames(_nf_of(k, T), T) for k in NF_KINDS] == [T, 1 if T > 1 else T, T - 1 if T > 1 else T, T, T]
    assert {B for B, _ in SHAPES} == {1, 63, 64, 65, 130} and {T for _, T in SHAPES} == {1, 2, 3, 7, 8}
    # the tracks kernel: the models' LDS sizes differ, the workload's large shape needs the opt-in, none is refused
    sizes = [track_lds(m["NB"], 3 + 4 * min(m["n_animated"], 7), m["L"], m["D"]) for m in TRACK_MODELS]
    assert all(s is not None and s <= 48 * 1024 for s in sizes) and len(set(sizes)) == len(sizes)
    assert 48 * 1024 < track_lds(104, 31, 40, 79) <= MG_TRACK_LDS_MAX       # (the workload's 104 x 79 model with a hand's 31 channels)
    assert track_lds(104, 79, 40, 79) is None and MG_TRACK_LDS_MAX == 163776
    # the options kernel: workgroups per option round 64; 8193 candidates make the second-stage loop run three times
    assert [(B + MG_FC_BLOCK - 1) // MG_FC_BLOCK for B in MIN_BATCHES] == [1, 1, 1, 2, 64, 65, 129]
    assert {b % MG_TRACK_CANDS for b in TRACK_BATCHES} == {0, 1, 2, 3} and 4 in TRACK_BATCHES


# ---- GPU plumbing -------------------------------------------------------------------------------------------------------------------
LEDGER = set()
LEDGER_WANT = {"route:lds", "route:optin", "route:global", "ca:vector", "ca:scalar", "nf<T:ca", "nf<T:local", "nf<T:set",
               "tracks:B%4=0", "tracks:B%4=1", "tracks:B%4=2", "tracks:B%4=3", "D<7", "nwg>64", "inlist_joint_trajectory"}
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def env(ctx):
    e = Env(ctx)
    yield e
    e.close()


_TABLES = {}


@pytest.fixture(autouse=True)
def _one_table_per_spline(monkeypatch):
    """The oracle builds a spline's arc-length table on every call (once per candidate here): the same function, its result kept per
    (control points, granularity)."""
    plain, kept = orc.arc_length_table, _TABLES

    def table(control_points, granularity=1000):
        key = (np.asarray(control_points, dtype=np.float64).tobytes(), int(granularity))
        if key not in kept:
            kept[key] = plain(control_points, granularity)
        return kept[key]
    monkeypatch.setattr(orc, "arc_length_table", table)
    yield


class Env(object):
    """One tiny primitive as the constraints' owner, its trajectories per (tag, control points, granularity), uploads to free."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.prim = _capi.Primitive(ctx, synthetic.make_tiny_primitive())
        self.lib = self.prim.lib
        self.trajs, self.bufs = {}, []

    def traj(self, cps, G, tag="a"):
        key = (tag, np.asarray(cps, dtype=np.float64).tobytes(), int(G))
        if key not in self.trajs:
            self.trajs[key] = _capi.Trajectory(self.prim, cps, granularity=G)
        return self.trajs[key]

    def upload(self, arr, offset_words=0):
        """The array on the device, `offset_words` doubles into its buffer: the address."""
        host = np.zeros(arr.size + offset_words, dtype=np.uint64)
        host[offset_words:] = np.ascontiguousarray(arr, dtype=np.float64).view(np.uint64).reshape(-1)
        buf = self.ctx.upload(host)
        assert buf.address % 16 == 0
        self.bufs.append(buf)
        return buf.address + 8 * offset_words

    def release(self):
        self.ctx.synchronize()
        for b in self.bufs:
            b.free()
        self.bufs = []

    def close(self):
        self.release()
        for t in self.trajs.values():
            t.close()
        self.prim.close()


class Con(object):
    """One constraint in the oracle's form, its tracks, the device record made of them."""

    def __init__(self, env, c, tracks, n_frames=0):
        self.c, self.tracks, self.keep = c, np.ascontiguousarray(tracks, dtype=np.float64), []
        kind = c["type"]
        self.B, self.T = self.tracks.shape[:2]
        self.J = self.tracks.shape[2]
        self.nf = effective_frames(n_frames, self.T)
        d = self.desc = _capi.FrameConstraintDesc()
        d.weight, d.n_joints, d.n_frames = float(c["weight"]), 1, int(n_frames)
        self.specs = []
        if kind == "frame_ca_position":
            d.type = CA
            for a in range(3):
                d.axis_on[a], d.target[a] = (0, 0.0) if c["target"][a] is None else (1, float(c["target"][a]))
            self.width = 1
        elif kind == "frame_discrete_trajectory":
            pts = np.asarray(c["points"], dtype=np.float64).reshape(-1, 3)
            d.type, d.n_points = DISCRETE, len(pts)
            d.points_dev = env.upload(pts) if len(pts) else None
            free = set(c.get("unconstrained") or ())
            for a in range(3):
                d.axis_on[a] = 0 if a in free else 1
            self.width = self.T
        elif kind == "frame_local_trajectory":
            t = env.traj(c["control_points"], c["granularity"], c.get("tag", "a"))
            d.type, d.start_arc = LOCAL, float(c["start_t"])
            d.trajectories[0] = t.handle.value
            self.specs = [(t.handle.value, len(c["control_points"]) - 1, c["granularity"])]
            self.width = self.nf
        elif kind == "frame_trajectory_set":
            d.type, d.n_joints = SET, self.J
            for j, t in enumerate(c["trajectories"]):
                tr = env.traj(t["control_points"], t["granularity"], t.get("tag", "a"))
                d.trajectories[j] = tr.handle.value
                d.arc0[j] = float(c["arc_lengths"][j])
                d.has_range[j] = 0 if t["range_start"] is None else 1
                if t["range_start"] is not None:
                    d.range_start[j], d.range_end[j] = float(t["range_start"]), float(t["range_end"])
                self.specs.append((tr.handle.value, len(t["control_points"]) - 1, t["granularity"]))
            self.width = self.nf
        elif kind == "frame_joint_rotation":
            d.type, d.quat_channel = ROTATION, int(c["quat_channel"])
            for e in range(4):
                d.quaternion[e] = float(c["quaternion"][e])
            self.width = 1
        elif kind == "frame_joint_trajectory":
            t = env.traj(c["control_points"], c["granularity"], c.get("tag", "a"))
            d.type, d.start_arc = JOINT_TRAJ, float(c["min_u"])
            d.trajectories[0] = t.handle.value
            self.specs = [(t.handle.value, len(c["control_points"]) - 1, c["granularity"])]
            self.width = self.T
        else:
            raise ValueError(kind)
        assert env.lib.mg_frame_constraint_width(C.byref(d), self.T) == self.width, (kind, self.T, n_frames)

    def placed(self):
        return (self.desc.type, self.specs)

    def oracle(self, b):
        """(weighted residual vector, weighted error) of candidate b."""
        c, tr, w = self.c, self.tracks[b], float(self.c["weight"])
        kind = c["type"]
        if kind == "frame_joint_rotation":
            # per_frame_constraint_residuals' statement for the class that reads a frame, on the first frame of the track
            q = np.array(tr[0, c["quat_channel"]:c["quat_channel"] + 4])
            q /= np.linalg.norm(q)
            t = np.asarray(c["quaternion"], dtype=np.float64)
            err = float(np.linalg.norm(np.ravel(orc.quaternion_matrix3(t / np.linalg.norm(t)) - orc.quaternion_matrix3(q))))
            return w * np.array([err]), w * err
        if kind == "frame_trajectory_set":
            names = ["j%d" % j for j in range(self.J)]
            res, err = orc.per_frame_track_residuals(dict(c, joints=names, n_frames=self.nf), {n: tr[:, j] for j, n in enumerate(names)})
        elif kind in ("frame_ca_position", "frame_local_trajectory"):
            res, err = orc.per_frame_track_residuals(dict(c, joint="j"), {"j": tr[:self.nf, 0]})
        else:
            res, err = orc.per_frame_track_residuals(dict(c, joint="j"), {"j": tr[:, 0]})
        return w * np.asarray(res), w * err


def _run_single(env, con, tracks_ptr=None, prefill=None, residuals=True, tag=""):
    """mg_score_frame_constraint on guarded buffers: (errors (B,), residuals (B, width) | None)."""
    B = con.B
    ptr = tracks_ptr if tracks_ptr is not None else env.upload(con.tracks)
    e = Guarded(env.ctx, B * 8, prefill)
    r = Guarded(env.ctx, B * con.width * 8) if residuals else None
    try:
        _capi._check(env.lib.mg_score_frame_constraint(env.prim.handle, C.byref(con.desc), ptr, B, con.T, con.J, e.ptr, 1 if prefill is not None else 0,
                                                       r.ptr if r is not None else None))
        err = e.read((B,), np.float64, tag)
        res = r.read((B, con.width), np.float64, tag) if r is not None else None
        for a in (err, res):
            if a is not None:
                assert not (_bits64(a) == np.uint64(FILL)).any(), ("elements the kernel never wrote", tag)
        return err, res
    finally:
        e.free()
        if r is not None:
            r.free()


def _run_list(env, cons, ptrs, prefill=None, with_res=None, tag=""):
    """mg_score_frame_constraints on guarded buffers: (errors, [residuals | None per constraint])."""
    n, B, vp = len(cons), cons[0].B, C.c_void_p
    with_res = [True] * n if with_res is None else with_res
    e = Guarded(env.ctx, B * 8, prefill)
    rs = [Guarded(env.ctx, B * c.width * 8) if w else None for c, w in zip(cons, with_res)]
    try:
        dptr = (vp * n)(*[C.addressof(c.desc) for c in cons])
        tptr = (vp * n)(*ptrs)
        tT, tJ = (C.c_int32 * n)(*[c.T for c in cons]), (C.c_int32 * n)(*[c.J for c in cons])
        rptr = (vp * n)(*[(r.ptr if r is not None else None) for r in rs])
        _capi._check(env.lib.mg_score_frame_constraints(env.prim.handle, n, dptr, tptr, tT, tJ, B, e.ptr, 1 if prefill is not None else 0, rptr))
        err = e.read((B,), np.float64, tag)
        return err, [r.read((B, c.width), np.float64, tag) if r is not None else None for c, r in zip(cons, rs)]
    finally:
        for b in [e] + [r for r in rs if r is not None]:
            b.free()


def _hold(con, err, res, cands=None, tag=""):
    """Errors and residual vectors against the oracle, at 1e-9 max(1, max |oracle|)."""
    for b in (range(con.B) if cands is None else cands):
        r_ref, e_ref = con.oracle(b)
        assert r_ref.shape == (con.width,), (tag, r_ref.shape, con.width)
        scale = max(1.0, float(np.abs(r_ref).max()), abs(e_ref))
        dev = max(float(np.abs(res[b] - r_ref).max()), abs(err[b] - e_ref)) / scale
        WORST[con.c["type"]] = max(WORST.get(con.c["type"], 0.0), dev)
        assert dev <= TOL, (tag, b, dev, err[b], e_ref)


def _walk_tracks(rng, B, T, J, cps=CPS, step=0.12, noise=1.5):
    """Tracks that wander along the polyline of cps: a few units beside it, 2 .. 12 % of it per frame."""
    u = rng.uniform(0.0, 0.3, (B, 1, J)) + np.cumsum(rng.uniform(0.02, step, (B, T, J)), axis=1)
    k = np.linspace(0.0, 1.0, len(cps))
    pts = np.stack([np.interp(u, k, cps[:, d]) for d in range(3)], axis=-1)
    return pts + rng.normal(0.0, noise, (B, T, J, 3))


def _walked(tracks, arc0, inclusive):
    """The arc length each scorer holds when it looks frame f up: (B, T, J).  inclusive: frame f's own step is in (the local
    trajectory); not inclusive: steps are added after the look-up, from the second frame on (the trajectory set)."""
    steps = np.linalg.norm(np.diff(tracks, axis=1), axis=-1)
    out = np.zeros(tracks.shape[:3]) + np.asarray(arc0, dtype=np.float64)
    if inclusive:
        out[:, 1:] += np.cumsum(steps, axis=1)
    else:
        out[:, 2:] += np.cumsum(steps, axis=1)[:, :-1]
    return out


# ---- 2. the scorers on given tracks ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
def test_ca_position_on_both_load_paths(env, B, T):
    """Every axis mask and every kind of n_frames; the same bytes at a 16-byte-aligned address (candidates whose track is aligned load
    frames in pairs) and 8 bytes further (the others do): the oracle's numbers, the same bits from both."""
    rng = np.random.default_rng(100 + B + T)
    tracks = _walk_tracks(rng, B, T, 1)
    p0, p8 = env.upload(tracks), env.upload(tracks, 1)
    aligned0 = (p0 + np.arange(B) * T * 24) % 16 == 0
    assert aligned0[0] and (T % 2 == 0 or B == 1 or not aligned0[1]) and p8 % 16 == 8
    for mi, mask in enumerate([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]):
        for kind in NF_KINDS if mi in (5, 7) else (NF_KINDS[mi % 5],):
            target = [float(v) if on else None for v, on in zip((40.0, 1.0, 20.0), mask)]
            con = Con(env, {"type": "frame_ca_position", "target": target, "weight": 1.0 + 0.25 * mi}, tracks, _nf_of(kind, T))
            tag = ("ca", B, T, mask, kind)
            e0, r0 = _run_single(env, con, p0, tag=tag)
            e8, r8 = _run_single(env, con, p8, tag=tag)
            np.testing.assert_array_equal(_bits64(e0), _bits64(e8), err_msg=str(tag))
            np.testing.assert_array_equal(_bits64(r0), _bits64(r8), err_msg=str(tag))
            np.testing.assert_array_equal(_bits64(e0), _bits64(r0[:, 0]), err_msg=str(tag))
            _hold(con, e0, r0, tag=tag)
            if not any(mask):
                assert not e0.any()
            if con.nf >= 2:
                LEDGER.update(["ca:vector", "ca:scalar"])          # (offset 0 and offset 8 between them put every candidate on both)
            if con.nf < T:
                LEDGER.add("nf<T:ca")
    env.release()


@pytest.mark.gpu
def test_ca_position_ignores_frames_from_n_frames_on(env):
    """Every candidate's closest frame is its last one; n_frames = T - 1 must not see it (odd T: both load paths in one launch)."""
    rng = np.random.default_rng(7)
    B, T = 65, 7
    tracks = _walk_tracks(rng, B, T, 1)
    target = [40.0, 30.0, 20.0]          # 29 above the path the tracks follow
    tracks[:, T - 1, 0] = np.array(target) + rng.normal(0.0, 1e-3, (B, 3))
    for nf in (T - 1, T - 2, 1):
        con = Con(env, {"type": "frame_ca_position", "target": target, "weight": 2.0}, tracks, nf)
        err, res = _run_single(env, con, tag=("ca beyond", nf))
        _hold(con, err, res, tag=("ca beyond", nf))
        assert (err > 2.0 * 0.5).all()            # nowhere near the 1e-3 of the frame it must not read
    whole = Con(env, {"type": "frame_ca_position", "target": target, "weight": 2.0}, tracks, T)
    assert (_run_single(env, whole)[0] < 2.0 * 1e-2).all()
    LEDGER.update(["nf<T:ca", "ca:vector", "ca:scalar"])
    env.release()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
def test_discrete_trajectory(env, B, T):
    rng = np.random.default_rng(200 + B + T)
    tracks = _walk_tracks(rng, B, T, 1)
    for i, n_points in enumerate(sorted({0, 1, max(T - 1, 0), T, T + 5})):
        for free in ([], [1], [0, 2]) if n_points in (T, T + 5) else ([[], [1], [0, 2]][i % 3],):
            pts = _walk_tracks(rng, 1, max(n_points, 1), 1)[0, :n_points, 0]
            con = Con(env, {"type": "frame_discrete_trajectory", "points": pts.tolist(), "unconstrained": free, "weight": 0.8}, tracks)
            tag = ("discrete", B, T, n_points, free)
            err, res = _run_single(env, con, tag=tag)
            _hold(con, err, res, tag=tag)
            assert not res[:, n_points:].any() and (n_points == 0 or res[:, :min(n_points, T)].all())
    env.release()


def _local(G, start_t, tag="a", cps=CPS, weight=1.2):
    return {"type": "frame_local_trajectory", "control_points": cps.tolist(), "granularity": G, "start_t": start_t, "weight": weight, "tag": tag}


def _clear_of(arcs, marks, what):
    """The scorers' tests against a spline's full arc length and a range's ends are step functions: the cases keep 1e-6 away."""
    for m in marks:
        gap = float(np.abs(arcs - m).min())
        assert gap >= 1e-6, (what, m, gap)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
def test_local_trajectory(env, B, T):
    """The walked arc length crossing the spline's full arc length in mid-track, starting beyond it, a track that does not move,
    n_frames < T (residual rows of n_frames entries)."""
    rng = np.random.default_rng(300 + B + T)
    tracks = _walk_tracks(rng, B, T, 1)
    full = orc.arc_length_table(CPS.tolist(), G_LDS)[1]
    steps = float(np.linalg.norm(np.diff(tracks, axis=1), axis=-1).sum(axis=1).mean()) if T > 1 else 0.0
    still = np.repeat(tracks[:, :1], T, axis=1)
    kinds = NF_KINDS if (B, T) == (65, 7) else (NF_KINDS[(B + T) % 5], "t_minus_1")
    crossed = 0
    for kind in kinds:
        for name, trk, start in (("from 3", tracks, 3.0), ("crossing", tracks, full - 0.25 - 0.5 * steps),("beyond", tracks, full + 1.0), ("still", still, 17.0)):
            con = Con(env, _local(G_LDS, start), trk, _nf_of(kind, T))
            arcs = _walked(trk, start, True)[:, :con.nf]
            _clear_of(arcs, [full], name)
            crossed += int(name == "crossing" and (arcs[:, 0] < full).any() and (arcs[:, -1] > full).any())
            tag = ("local", B, T, kind, name)
            err, res = _run_single(env, con, tag=tag)
            _hold(con, err, res, tag=tag)
            np.testing.assert_allclose(err, res.sum(axis=1), rtol=1e-13, atol=0.0)
            if name == "still":
                assert (res == res[:, :1]).all()
            if con.nf < T:
                LEDGER.add("nf<T:local")
    assert crossed or T == 1
    LEDGER.add("route:lds")
    env.release()


def _set(J, ranges, arc0, G=G_LDS, shared=False, weight=1.1):
    """A trajectory set over J joints; ranges: per joint (start, end) or None; shared: joints 0 and 1 read one handle."""
    trajs = []
    for j in range(J):
        cps = CPS if (j % 2 == 0 or (shared and j == 1)) else CPS_B
        tag = "a" if (j == 0 or (shared and j == 1)) else "set%d" % j
        rg = ranges[j]
        trajs.append({"control_points": cps.tolist(), "granularity": G, "tag": tag, "range_start": None if rg is None else rg[0],
                      "range_end": None if rg is None else rg[1]})
    return {"type": "frame_trajectory_set", "trajectories": trajs, "arc_lengths": list(arc0), "weight": weight}


@pytest.mark.gpu
@pytest.mark.parametrize("J", [1, 2, 3, 8])
def test_trajectory_set(env, J):
    """No range (all residuals 0), one joint's range entered only in mid-track, every range active; two joints on one handle;
    n_frames < T."""
    rng = np.random.default_rng(400 + J)
    shapes = {1: (65, 7), 2: (130, 8), 3: (63, 2), 8: (64, 3)}
    for B, T in [shapes[J], (1, 1)]:
        tracks = _walk_tracks(rng, B, T, J)
        arc0 = [4.0 + 2.5 * j for j in range(J)]
        walked = _walked(tracks, arc0, False)
        # a range of the last joint that opens between the least and the most any candidate has walked at the middle frame
        mid = walked[:, max(2, T // 2) if T > 2 else 0, J - 1]      # (the first step is in from the third frame on)
        opens = 0.5 * (float(mid.min()) + float(mid.max())) if T > 2 else arc0[J - 1] + 1.0
        variants = [("none", [None] * J), ("all", [(0.0, 1.0e4)] * J), ("mid", [None] * (J - 1) + [(opens, opens + 25.0)])]
        fulls = [orc.arc_length_table(CPS.tolist(), G_LDS)[1], orc.arc_length_table(CPS_B.tolist(), G_LDS)[1]]
        for kind in NF_KINDS if (B, T) == (65, 7) else ("t", "t_minus_1"):
            for name, ranges in variants:
                for shared in ((False, True) if J >= 2 and name == "all" else (False,)):
                    con = Con(env, _set(J, ranges, arc0, shared=shared), tracks, _nf_of(kind, T))
                    marks = fulls + [v for rg in ranges if rg is not None for v in rg]
                    _clear_of(walked[:, :con.nf], marks, name)
                    tag = ("set", J, B, T, kind, name, shared)
                    if shared:
                        assert con.specs[0][0] == con.specs[1][0] and place_tables([con.placed()])[0] < place_tables([con.placed()], dedup=False)[0]
                    err, res = _run_single(env, con, tag=tag)
                    _hold(con, err, res, tag=tag)
                    if name == "none":
                        assert not res.any() and not err.any()
                    if name == "all":
                        assert res.all()
                    if name == "mid" and T > 2 and con.nf == T and B > 1:
                        live = res != 0.0
                        assert not live[:, 0].any() and live.any() and not live.all()
                    if con.nf < T:
                        LEDGER.add("nf<T:set")
    env.release()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(1, 2), (63, 2), (64, 3), (65, 7), (130, 8)])
def test_joint_rotation(env, B, T):
    """Frames (B, T, n_dim), the first one read; the quaternion at the first and at the last channel it can be at; frame and target
    quaternions that are not unit."""
    rng = np.random.default_rng(500 + B + T)
    n_dim = 11
    frames = rng.standard_normal((B, T, n_dim)) * 1.7
    for ch in (3, n_dim - 4):
        con = Con(env, {"type": "frame_joint_rotation", "quat_channel": ch, "quaternion": [1.8, 0.2, -0.6, 0.4], "weight": 0.6}, frames)
        assert con.J == n_dim
        err, res = _run_single(env, con, tag=("rotation", B, T, ch))
        _hold(con, err, res, tag=("rotation", B, T, ch))
        assert (err > 0.0).all()
    env.release()


def _jt(cps=CPS, min_u=0.05, G=G_LDS, weight=1.5, tag="a"):
    return {"type": "frame_joint_trajectory", "control_points": np.asarray(cps).tolist(), "min_u": min_u, "granularity": G, "weight": weight, "tag": tag}


@pytest.mark.gpu
def test_joint_trajectory_entries_give_the_same_bits(env):
    """mg_score_frame_constraint's one-lane branch, mg_score_frame_constraints (which hands a joint trajectory to
    mg_score_trajectory_points up to 65 536 candidates) and mg_score_trajectory_points itself: the same errors and residuals, under
    both searches.  (The search's own arithmetic is held to the reference by test_gpu_closest_point.py and the trajectory sweep.)"""
    rng = np.random.default_rng(61)
    B, T = 65, 7
    tracks = _walk_tracks(rng, B, T, 1)
    con = Con(env, _jt(), tracks)
    ptr = env.upload(tracks)
    pre = rng.standard_normal(B)
    try:
        for search in (0, 1):
            env.ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, search)
            e1, r1 = _run_single(env, con, ptr, tag=("jt single", search))
            eL, rL = _run_list(env, [con], [ptr], tag=("jt list", search))
            eP, rP = env.prim.score_trajectory_points(env.trajs[("a", CPS.tobytes(), G_LDS)], tracks[:, :, 0], 0.05, 1.5, residuals=True)
            for e, r, who in ((eL, rL[0], "list"), (eP, rP, "points")):
                np.testing.assert_array_equal(_bits64(r1), _bits64(r), err_msg="%s, search %d" % (who, search))
                np.testing.assert_array_equal(_bits64(e1), _bits64(e), err_msg="%s, search %d" % (who, search))
            ea, _ = _run_single(env, con, ptr, prefill=pre, tag=("jt single acc", search))
            eb, _ = _run_list(env, [con], [ptr], prefill=pre, tag=("jt list acc", search))
            np.testing.assert_array_equal(_bits64(ea), _bits64(pre + e1))
            np.testing.assert_array_equal(_bits64(eb), _bits64(pre + e1))
            assert (e1 > 0.0).all() and len(np.unique(e1)) == B
    finally:
        env.ctx.set_option(_capi.MG_OPT_TRAJECTORY_SEARCH, 0)
    env.release()


@pytest.mark.gpu
def test_joint_trajectory_inside_a_list_above_65536_candidates(env):
    """B = 65 537: mg_score_frame_constraints keeps the joint trajectory in its group (the list kernel's own branch); a CA constraint
    beside it; against the single launches, bit for bit."""
    rng = np.random.default_rng(62)
    B, T = MG_FC_TRAJ_ALONE_MAX_B + 1, 2
    tracks = _walk_tracks(rng, B, T, 1, cps=CPS_3)
    jt = Con(env, _jt(cps=CPS_3, min_u=0.0, tag="three"), tracks)
    ca = Con(env, {"type": "frame_ca_position", "target": [10.0, None, 4.0], "weight": 0.5}, tracks)
    assert list_launches([JOINT_TRAJ, CA], B) == [("list", [0, 1])] and list_launches([JOINT_TRAJ, CA], B - 1)[0][0] == "points"
    ptr = env.upload(tracks)
    e1, r1 = _run_single(env, jt, ptr, tag="jt 65537 single")
    e2, r2 = _run_single(env, ca, ptr, prefill=e1, tag="ca 65537 single")
    eL, rL = _run_list(env, [jt, ca], [ptr, ptr], tag="65537 list")
    np.testing.assert_array_equal(_bits64(eL), _bits64(e2))
    np.testing.assert_array_equal(_bits64(rL[0]), _bits64(r1))
    np.testing.assert_array_equal(_bits64(rL[1]), _bits64(r2))
    eO, rO = _run_list(env, [jt], [ptr], tag="65537 list of one")
    np.testing.assert_array_equal(_bits64(eO), _bits64(e1))
    np.testing.assert_array_equal(_bits64(rO[0]), _bits64(r1))
    # rows of the last workgroup and the first against a launch of those rows alone
    pick = [0, 63, 64, B - 2, B - 1]
    few = Con(env, _jt(cps=CPS_3, min_u=0.0, tag="three"), tracks[pick])
    e3, r3 = _run_single(env, few, tag="jt five rows")
    np.testing.assert_array_equal(_bits64(e1[pick]), _bits64(e3))
    np.testing.assert_array_equal(_bits64(r1[pick]), _bits64(r3))
    LEDGER.add("inlist_joint_trajectory")
    env.release()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["local_G1000", "local_optin_band", "local_global", "set_global_by_sum"])
def test_table_routes_against_the_oracle(env, case):
    """Tables in LDS, in LDS by the large-LDS opt-in, and in global memory: the oracle's numbers at the same granularity."""
    rng = np.random.default_rng(70)
    B, T = 65, 3
    spec, claim = TABLE_CASES[case]
    G = spec[0][1][0][2]
    if spec[0][0] == LOCAL:
        tracks = _walk_tracks(rng, B, T, 1)
        con = Con(env, _local(G, 11.0), tracks)
        _clear_of(_walked(tracks, 11.0, True), [orc.arc_length_table(CPS.tolist(), G)[1]], case)
    else:
        tracks = _walk_tracks(rng, B, T, 2)
        con = Con(env, _set(2, [(0.0, 1.0e4), None], [4.0, 6.5], G=G), tracks)
        _clear_of(_walked(tracks, [4.0, 6.5], False), [orc.arc_length_table(c.tolist(), G)[1] for c in (CPS, CPS_B)], case)
    # what the library built is what the restatement was told
    for (handle, n_seg, g), (_, n_seg_claim, g_claim) in zip(con.specs, spec[0][1]):
        got_seg, got_G = C.c_int32(), C.c_int32()
        _capi._check(env.lib.mg_trajectory_tables(handle, None, None, C.byref(got_seg), C.byref(got_G), None))
        assert (got_seg.value, got_G.value) == (n_seg, g) == (n_seg_claim, g_claim)
    assert place_tables([con.placed()])[1] == claim
    err, res = _run_single(env, con, tag=case)
    _hold(con, err, res, tag=case)
    eL, rL = _run_list(env, [con], [env.upload(tracks)], tag=case + " list")
    np.testing.assert_array_equal(_bits64(eL), _bits64(err))
    np.testing.assert_array_equal(_bits64(rL[0]), _bits64(res))
    LEDGER.add("route:" + claim)
    env.release()


@pytest.mark.gpu
def test_a_list_whose_tables_only_fit_one_by_one(env):
    """Four local trajectories of 48 KB of tables each: the list reads global memory, the single launches LDS -- the same bits.  Two
    constraints on one 96 KB table: placed once, in LDS by the opt-in."""
    rng = np.random.default_rng(71)
    B, T = 65, 8
    tracks = _walk_tracks(rng, B, T, 1)
    ptr = env.upload(tracks)
    cons = [Con(env, _local(G_QUARTER, 2.0 + 3.0 * i, tag=t, cps=CPS if i % 2 == 0 else CPS_B, weight=0.5 + i), tracks, (0, T - 1, 3, T)[i])
            for i, t in enumerate("abcd")]
    assert place_tables([c.placed() for c in cons])[1] == "global" and all(place_tables([c.placed()])[1] == "lds" for c in cons)
    assert len({c.specs[0][0] for c in cons}) == 4
    pre = rng.standard_normal(B)
    for prefill in (None, pre):
        total, singles = prefill, []
        for c in cons:
            total, r = _run_single(env, c, ptr, prefill=total, tag="quarter single")
            singles.append(r)
        eL, rL = _run_list(env, cons, [ptr] * 4, prefill=prefill, tag="quarters list")
        np.testing.assert_array_equal(_bits64(eL), _bits64(total))
        for a, b in zip(rL, singles):
            np.testing.assert_array_equal(_bits64(a), _bits64(b))
    _hold(cons[1], *_run_single(env, cons[1], ptr), cands=(0, 1, 63, 64), tag="quarter against the oracle")
    LEDGER.update(["route:global", "route:lds", "nf<T:local"])
    shared = [Con(env, _local(G_SHARED, 5.0, tag="big"), tracks), Con(env, _local(G_SHARED, 40.0, tag="big", weight=0.7), tracks, T - 2)]
    assert shared[0].specs[0][0] == shared[1].specs[0][0]
    assert place_tables([c.placed() for c in shared])[1] == "optin" and place_tables([c.placed() for c in shared], dedup=False)[1] == "global"
    e0, r0 = _run_single(env, shared[0], ptr, tag="shared single 0")
    e1, r1 = _run_single(env, shared[1], ptr, prefill=e0, tag="shared single 1")
    eL, rL = _run_list(env, shared, [ptr, ptr], tag="shared list")
    np.testing.assert_array_equal(_bits64(eL), _bits64(e1))
    np.testing.assert_array_equal(_bits64(rL[0]), _bits64(r0))
    np.testing.assert_array_equal(_bits64(rL[1]), _bits64(r1))
    _hold(shared[0], e0, r0, cands=(0, 64), tag="shared against the oracle")
    LEDGER.add("route:optin")
    env.release()


def _pool(env, rng, B, T):
    """Nine constraints of mixed types on their own tracks (the order _list_order's types name)."""
    one, two = _walk_tracks(rng, B, T, 1), _walk_tracks(rng, B, T, 2)
    frames = rng.standard_normal((B, 2, 11))
    pts = _walk_tracks(rng, 1, T, 1)[0, :, 0]
    by_type = {
        CA: [Con(env, {"type": "frame_ca_position", "target": [40.0, None, 20.0], "weight": 2.0}, one, T - 1),
             Con(env, {"type": "frame_ca_position", "target": [None, 2.0, None], "weight": 0.3}, one)],
        DISCRETE: [Con(env, {"type": "frame_discrete_trajectory", "points": pts[:T - 2].tolist(), "unconstrained": [1], "weight": 0.8}, one),
                   Con(env, {"type": "frame_discrete_trajectory", "points": pts.tolist(), "unconstrained": [], "weight": 0.1}, one)],
        LOCAL: [Con(env, _local(G_LDS, 3.0), one, T - 2), Con(env, _local(G_LDS, 30.0, tag="poolb", cps=CPS_B), one)],
        SET: [Con(env, _set(2, [(0.0, 1.0e4), None], [4.0, 1.0]), two)],
        ROTATION: [Con(env, {"type": "frame_joint_rotation", "quat_channel": 7, "quaternion": [0.9, 0.1, -0.3, 0.2], "weight": 0.6}, frames)],
        JOINT_TRAJ: [Con(env, _jt(), one)],
    }
    ptrs = {id(one): env.upload(one), id(two): env.upload(two), id(frames): env.upload(frames)}
    for cs in by_type.values():
        for c in cs:
            c.ptr = ptrs[id(one)] if c.J == 1 else ptrs[id(two)] if c.J == 2 else ptrs[id(frames)]
    return by_type


@pytest.mark.gpu
@pytest.mark.parametrize("n", LIST_SIZES)
def test_lists_are_the_single_launches_in_order(env, n):
    """Lists of 1, 4, 5, 8 and 9 constraints of mixed types, the joint trajectory first, in the middle and last, written and added to
    errors that are there, residuals asked for from every other constraint: the bits of the same constraints launched singly in
    order."""
    rng = np.random.default_rng(800 + n)
    B, T = 65, 7
    pool = _pool(env, rng, B, T)
    pre = rng.standard_normal(B)
    singles = {}
    for place in JT_PLACES if n > 1 else ("first", "none"):
        used = {k: 0 for k in pool}
        cons = []
        for kind in ([CA] if place == "none" else _list_order(n, place)):
            cons.append(pool[kind][used[kind] % len(pool[kind])])
            used[kind] += 1
        assert len(cons) == n
        for vi, (prefill, with_res) in enumerate(((None, [True] * n), (pre, [i % 2 == 0 for i in range(n)]), (None, [i % 2 == 1 for i in range(n)]))):
            total = prefill
            for c in cons:
                key = (id(c), None if total is None else total.tobytes())
                if key not in singles:
                    singles[key] = _run_single(env, c, c.ptr, prefill=total, tag=("single", n, place))
                total = singles[key][0]
            tag = ("list", n, place, vi)
            eL, rL = _run_list(env, cons, [c.ptr for c in cons], prefill=prefill, with_res=with_res, tag=tag)
            np.testing.assert_array_equal(_bits64(eL), _bits64(total), err_msg=str(tag))
            total = prefill
            for c, r in zip(cons, rL):
                key = (id(c), None if total is None else total.tobytes())
                total = singles[key][0]
                if r is not None:
                    np.testing.assert_array_equal(_bits64(r), _bits64(singles[key][1]), err_msg=str(tag))
    env.release()


# ---- 3. mg_align_frames, mg_joint_positions and mg_joint_tracks across model shapes ---------------------------------------------------
TRACK_MODELS = [dict(name="D3", D=3, NB=4, L=1, F=9, n_animated=0), dict(name="D6", D=6, NB=7, L=3, F=34, n_animated=0),
                dict(name="D7", D=7, NB=4, L=3, F=35, n_animated=1), dict(name="D11", D=11, NB=7, L=40, F=34, n_animated=2),
                dict(name="D79", D=79, NB=7, L=3, F=35, n_animated=19)]
TRACK_BATCHES = (1, 2, 3, 4, 5, 9)
HIPS = ([("Hips", None, (0.0, 0.0, 0.0))], ["Hips"])
EIGHT = ["Hips", "Head", "LeftHand", "RightHand_EndSite", "LeftFoot", "RightToeBase", "Spine1", "Neck"]
# requests per call: (grid: None = canonical | T of an integer grid, joints by count)
REQUEST_SETS = [[(None, 1)], [(1, 3), (None, 8)], [(2, 8), (33, 1), (None, 3)], [(33, 3), (1, 1), (2, 8), (None, 1)]]
START_POSE = {"position": [3.0, 2.0, 1.0], "orientation": [0.0, 25.0, 0.0]}


def _track_configs(m):
    """(B, dtype, ld padding, requests, mode) of one model: every B with every mode; dtype, padding and request set rotate."""
    modes = ["none", "previous_root", "start_pose"] + (["previous_node"] if m["D"] >= 11 else [])
    out = []
    for mi, mode in enumerate(modes):
        for bi, B in enumerate(TRACK_BATCHES):
            reqs = [(T if (T is None or T < m["F"]) else 2, J) for T, J in REQUEST_SETS[(bi + mi) % 4]]
            out.append((B, (np.float64, np.float32)[(bi + mi) % 2], (0, 3)[((bi + mi) // 2) % 2], reqs, mode))
    return out


def test_track_configs_cover_every_value():
    for m in TRACK_MODELS:
        cfg = _track_configs(m)
        assert {c[0] for c in cfg} == set(TRACK_BATCHES) and {c[1] for c in cfg} == {np.float32, np.float64} and {c[2] for c in cfg} == {0, 3}
        assert {len(c[3]) for c in cfg} == {1, 2, 3, 4} and {J for c in cfg for _, J in c[3]} == {1, 3, 8}
        assert {T for c in cfg for T, _ in c[3]} >= ({None, 1, 2, 33} if m["F"] > 33 else {None, 1, 2})
        assert {(c[0] % 4, c[4]) for c in cfg} >= {(r, "previous_root") for r in range(4)}
        assert (m["D"] - 3) // 4 == m["n_animated"] or m["D"] < 7
    assert {m["D"] for m in TRACK_MODELS} == {3, 6, 7, 11, 79} and {m["NB"] for m in TRACK_MODELS} == {4, 7}
    assert {m["L"] for m in TRACK_MODELS} == {1, 3, 40} and {m["F"] % 2 for m in TRACK_MODELS} == {0, 1}


def _skeletons(m):
    """(device skeleton, the oracle's (joints, animated), the node a 'previous_node' alignment goes through)"""
    if m["D"] < 7:
        return _capi.Skeleton(HIPS[0], []), HIPS, None
    joints, animated = synthetic.make_skeleton(m["n_animated"])
    return _capi.Skeleton(joints, animated), (joints, animated), ("Spine" if m["D"] == 11 else "Spine1" if m["D"] > 11 else None)


def _joint_names(m, J):
    if m["D"] < 7:
        return ["Hips"] * J
    return {1: ["LeftHand"], 3: ["Hips", "Head", "RightFoot"], 8: EIGHT}[J]


def _oracle_tracks(op, m, ojoints, oanimated, s, mode, prev, node, times, names):
    coeffs = op.back_project_spatial_coeffs(s)
    if m["D"] < 7:       # no root quaternion: the identity (what the trajectory sweep's oracle does)
        coeffs = np.concatenate([coeffs[:, :3], np.tile([1.0, 0.0, 0.0, 0.0], (len(coeffs), 1))], axis=1)
    if mode in ("previous_root", "previous_node"):
        coeffs = orc.align_coeffs_to_previous_frame(coeffs, prev, ojoints, oanimated, "Hips" if mode == "previous_root" else node)
    elif mode == "start_pose":
        coeffs = orc.align_coeffs_to_start_pose(coeffs, {"position": list(START_POSE["position"]), "orientation": list(START_POSE["orientation"])})
    frames = orc.spline_frames(op.knots, coeffs, times)
    return np.array([[orc.joint_global_position(f, ojoints, oanimated, n) for n in names] for f in frames])


def _chain_below_seven(ctx, prim, sk, S, alignment, names, grid):
    """mg_back_project_frames_f64 -> mg_align_frames -> mg_joint_positions for a primitive without a root quaternion.  The Python
    layer's chain (frame_constraints._Batch) reads the candidates' first root position through a keyframe constraint set, which wants
    D >= 7; mg_align_frames itself takes any D >= 3 with the values handed to it: the first control point's (x, z) from the float64
    coefficient kernel (the fma chain the tracks kernel states) and, for a previous frame, the heading of a node without a quaternion
    -- ref_dir's (x, z) = (0, 1).  Returns (tracks, frames before, frames after)."""
    B, T = len(S), prim._grid_size(grid)
    before = prim.back_project_frames_f64(S, grid)
    d_f = ctx.upload(before)
    idx = sk.indices(names)
    d_o = ctx.malloc(B * T * len(idx) * 24)
    d_v = None
    try:
        if alignment is not None:
            cp0 = prim.back_project_coeffs(S, np.float64)[:, 0]
            cols = [cp0[:, 0], cp0[:, 2]] + ([] if alignment.get("joint", 0) == _capi.MG_ALIGN_START_POSE else [np.zeros(B), np.ones(B)])
            vals = np.ascontiguousarray(np.stack(cols, axis=1))
            d_v = ctx.upload(vals)
            al = _capi.ConstraintSet._marshal_alignment(alignment, sk)
            _capi._check(prim.lib.mg_align_frames(prim.handle, d_f.ptr, B, T, d_v.ptr, vals.shape[1], C.byref(al)))
        after = ctx.download(d_f, before.shape, np.float64)
        ctx.joint_positions_dev(sk, idx, d_f, B * T, prim.n_dim, d_o)
        return ctx.download(d_o, (B, T, len(idx), 3), np.float64), before, after
    finally:
        for b in (d_f, d_o, d_v):
            if b is not None:
                b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("model", [m["name"] for m in TRACK_MODELS])
def test_joint_tracks_are_the_chain_and_the_oracle(ctx, model):
    """mg_joint_tracks against mg_back_project_frames_f64 -> mg_align_frames -> mg_joint_positions (bit for bit) and against the
    oracle (1e-9), guards behind each request's last candidate."""
    from morphablegraphs_amd.frame_constraints import _Batch
    m = {x["name"]: x for x in TRACK_MODELS}[model]
    data = synthetic.make_primitive(seed=4000 + m["D"], name=model, n_components=m["L"], n_frames=m["F"], n_basis=m["NB"], n_dim=m["D"], n_gmm=1)
    prim = _capi.Primitive(ctx, data)
    op = orc.OraclePrimitive(data)
    sk, (ojoints, oanimated), node = _skeletons(m)
    rng = np.random.default_rng(m["D"])
    prev = rng.standard_normal(max(m["D"], 7))
    prev[:3] = [25.0, 89.0, -12.0]
    for q in range(3, len(prev) - 3, 4):
        prev[q:q + 4] /= np.linalg.norm(prev[q:q + 4])
    if m["D"] < 7:
        prev[3:7] = [1.0, 0.0, 0.0, 0.0]      # no root quaternion: the identity on both sides
    grids = {T: prim.time_grid(np.arange(T, dtype=np.float64)) for T in (1, 2, 33) if T < m["F"]}
    plans, worst = {}, 0.0
    try:
        for B, dtype, pad, reqs, mode in _track_configs(m):
            S = np.zeros((B, m["L"] + pad), dtype=dtype)
            S[:, :m["L"]] = rng.standard_normal((B, m["L"]))
            S[:, m["L"]:] = 1.0e3          # columns beyond the components: never read
            if mode == "none":
                alignment = None
            elif mode == "start_pose":
                alignment = alignment_from_start_pose(START_POSE)
            else:
                al_joint = 0 if mode == "previous_root" else sk.index(node)
                al = sk.alignment_to(prev[:max(m["D"], 3)] if m["D"] >= 7 else prev[:3], al_joint)
                alignment = {"joint": al_joint, "position": al["position"], "heading": al["heading"]}
            names = [_joint_names(m, J) for _, J in reqs]
            al_joint = alignment["joint"] if mode.startswith("previous") else 0
            pkey = (tuple(tuple(n) for n in names), al_joint)
            if pkey not in plans:
                plans[pkey] = _capi.TrackPlan(prim, sk, names, al_joint)
            plan = plans[pkey]
            assert prim.canonical_grid.size == m["F"] and all(g.size == T for T, g in grids.items())
            Ts = [m["F"] if T is None else T for T, _ in reqs]
            batch = _Batch(prim, S, sk, alignment) if m["D"] >= 7 else None
            d_S = ctx.upload(S)
            outs = [Guarded(ctx, B * T * J * 24) for T, (_, J) in zip(Ts, reqs)]
            try:
                plan.tracks_dev(d_S, dtype, B, S.shape[1], [None if T is None else grids[T] for T, _ in reqs], [o.ptr for o in outs], alignment)
                for qi, ((Tq, J), T, o) in enumerate(zip(reqs, Ts, outs)):
                    tag = (model, B, np.dtype(dtype).name, pad, mode, qi, Tq, J)
                    got = o.read((B, T, J, 3), np.float64, tag)
                    assert not (_bits64(got) == np.uint64(FILL)).any(), ("positions the kernel never wrote", tag)
                    if batch is not None:
                        d_c, Tc = batch.tracks(names[qi], None if Tq is None else np.arange(Tq, dtype=np.float64))
                        chain = ctx.download(d_c, (B, T, J, 3), np.float64)
                        assert Tc == T
                    else:
                        chain, before, after = _chain_below_seven(ctx, prim, sk, S, alignment, names[qi], None if Tq is None else grids[Tq])
                        if m["D"] > 3:       # nothing behind the root's position moves
                            np.testing.assert_array_equal(_bits64(before[:, :, 3:]), _bits64(after[:, :, 3:]), err_msg=str(tag))
                        assert (alignment is None) == np.array_equal(before[:, :, :3], after[:, :, :3])
                    np.testing.assert_array_equal(_bits64(got), _bits64(chain), err_msg=str(tag))
                    times = op.canonical_time_function() if Tq is None else np.arange(Tq, dtype=np.float64)
                    for b in range(B):
                        ref = _oracle_tracks(op, m, ojoints, oanimated, S[b, :m["L"]].astype(np.float64), mode, prev[:max(m["D"], 7)], node, times, names[qi])
                        dev = float(np.abs(got[b] - ref).max()) / max(1.0, float(np.abs(ref).max()))
                        worst = max(worst, dev)
                        assert dev <= TOL, (tag, b, dev)
                LEDGER.add("tracks:B%%4=%d" % (B % 4))
                if m["D"] < 7:
                    LEDGER.add("D<7")
            finally:
                ctx.synchronize()
                if batch is not None:
                    batch.close()
                d_S.free()
                for o in outs:
                    o.free()
    finally:
        for h in list(plans.values()) + list(grids.values()) + [prim]:
            h.close()
    WORST["tracks " + model] = worst


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 6])
def test_align_frames_leaves_the_channels_behind_the_root_alone_below_seven(ctx, D):
    """A primitive without a root quaternion: mg_align_frames moves channels 0 .. 2 and nothing else, under both kinds of alignment."""
    m = [x for x in TRACK_MODELS if x["D"] == D][0]
    data = synthetic.make_primitive(seed=4000 + D, name="align%d" % D, n_components=m["L"], n_frames=m["F"], n_basis=m["NB"], n_dim=D, n_gmm=1)
    prim = _capi.Primitive(ctx, data)
    sk = _capi.Skeleton(HIPS[0], [])
    S = np.random.default_rng(D).standard_normal((5, m["L"]))
    try:
        for alignment in ({"joint": 0, "position": [25.0, 89.0, -12.0], "heading": [0.6, -0.8]}, alignment_from_start_pose(START_POSE)):
            _, before, after = _chain_below_seven(ctx, prim, sk, S, alignment, ["Hips"], None)
            assert not np.array_equal(before[:, :, [0, 2]], after[:, :, [0, 2]])
            if D > 3:
                np.testing.assert_array_equal(_bits64(before[:, :, 3:]), _bits64(after[:, :, 3:]))
            np.testing.assert_allclose(np.diff(after[:, :, 1], axis=1), np.diff(before[:, :, 1], axis=1), rtol=0, atol=1e-9)
            # every candidate's first frame sits on the wanted root position (x, z): the first frame of a clamped spline is its first
            # control point, which the transform was derived from
            np.testing.assert_allclose(after[:, 0, [0, 2]], np.tile(np.asarray(alignment["position"])[[0, 2]], (5, 1)), rtol=0, atol=1e-9)
        LEDGER.add("D<7")
    finally:
        prim.close()


# ---- 4. the options-list kernel --------------------------------------------------------------------------------------------------------
MIN_BATCHES = (1, 63, 64, 65, 4096, 4097, 8193)
SENTINEL = 0x7FF8ABCDEF012345


def _error_patterns(rng, B):
    """Errors whose first minimum is at a place the reduction can get wrong."""
    ties = rng.uniform(1.0, 2.0, B)
    for i in sorted({B // 3, min(B // 3 + 1, B - 1), (B // 3) + 64 if (B // 3) + 64 < B else B - 1, B - 1}):
        ties[i] = 0.25                               # equal minima within one wave and in different workgroups: the first wins
    last = rng.uniform(1.0, 2.0, B)
    last[::5], last[::7] = np.nan, np.inf
    last[B - 1] = -5.0                               # the last lane of the last workgroup
    nothing = np.where(np.arange(B) % 2 == 0, np.nan, np.inf)
    minus = rng.uniform(-1.0, 1.0, B)
    minus[::3] = np.nan
    minus[B // 2] = -np.inf
    if B > 1:
        minus[B - 1] = -np.inf                       # ... twice: the first wins
    plain = rng.standard_normal(B)
    return [ties, last, nothing, minus, plain]


def _records(raw, n_options, stride, Lw):
    out = []
    for k in range(n_options):
        rec = raw[k * stride:(k + 1) * stride]
        out.append((int(rec[:8].view(np.int64)[0]), rec[8:16].view(np.float64)[0], rec[16:16 + 8 * Lw].view(np.float64), rec[16 + 8 * Lw:].view(np.uint64)))
    return out


def _min_only(ctx, prim, n_options, B, dtype, rng):
    """mg_options_frame_lists over options without lists: every option's record against first_min_argmin of the errors it was given."""
    vp = C.c_void_p
    Lw = prim.n_gmm_dims
    ld = Lw + 5
    x = rng.standard_normal((B, ld)).astype(dtype)
    patterns = _error_patterns(rng, B)
    errs = np.stack([patterns[(k + B) % len(patterns)] for k in range(n_options)])
    stride = 16 + 8 * Lw + 24
    d_x, d_e = ctx.upload(x), ctx.upload(errs)
    res = Guarded(ctx, n_options * stride, np.full(n_options * stride // 8, SENTINEL, dtype=np.uint64))
    try:
        prims, lats, eptr = (vp * n_options)(*[prim.handle.value] * n_options), (vp * n_options)(*[d_x.address] * n_options), (vp * n_options)()
        for k in range(n_options):
            eptr[k] = d_e.address + k * B * 8
        _capi._check(ctx.lib.mg_options_frame_lists(n_options, prims, None, lats, _capi._dtype_code(x), B, (C.c_int64 * n_options)(*[ld] * n_options), None, None, None,
                                                    (C.c_int32 * n_options)(), None, None, eptr, res.ptr, stride, None))
        raw = res.read((n_options * stride,), np.uint8, ("min only", n_options, B))
        np.testing.assert_array_equal(_bits64(ctx.download(d_e, errs.shape, np.float64)), _bits64(errs))      # an empty list adds nothing
        for k, (idx, err, row, rest) in enumerate(_records(raw, n_options, stride, Lw)):
            want_i, want_e = orc.first_min_argmin(errs[k])
            tag = (n_options, B, k, (k + B) % len(patterns))
            assert idx == want_i, (tag, idx, want_i)
            assert _bits64(np.array([err]))[0] == _bits64(np.array([want_e]))[0], (tag, err, want_e)
            np.testing.assert_array_equal(_bits64(row), _bits64(x[want_i, :Lw].astype(np.float64)), err_msg=str(tag))
            assert (rest == np.uint64(SENTINEL)).all(), ("bytes behind the record", tag)
        if (B + MG_FC_BLOCK - 1) // MG_FC_BLOCK > 64:
            LEDGER.add("nwg>64")
    finally:
        for b in (d_x, d_e, res):
            b.free()


@pytest.mark.gpu
def test_first_minimum_of_options_without_lists():
    """n_constraints = 0 needs no plan: the first minimum over errors the test wrote.  Ties within a wave and across workgroups, NaN and
    +inf scattered with the minimum in the last lane of the last workgroup, nothing finite (index 0, +inf), -inf; 1, 2 and 24 options;
    up to 129 workgroups per option; float32 and float64 candidates with ld = Lw + 5; the calls (24, 8193), (1, 1), (24, 8193),
    (2, 65) first, on one context, so that the counters' place moves and comes back."""
    c = _capi.Context(0)
    prim = _capi.Primitive(c, synthetic.make_tiny_primitive())
    rng = np.random.default_rng(90)
    try:
        for n_options, B in ((24, 8193), (1, 1), (24, 8193), (2, 65)):
            _min_only(c, prim, n_options, B, np.float32 if B == 65 else np.float64, rng)
        for B in MIN_BATCHES:
            for n_options in (1, 2, 24):
                if (n_options, B) not in ((24, 8193), (1, 1), (2, 65)):
                    _min_only(c, prim, n_options, B, (np.float32, np.float64)[(B + n_options) % 2], rng)
    finally:
        prim.close()
        c.close()


OPTION_MODELS = [dict(D=7, NB=7, L=3, F=12, n_animated=1), dict(D=11, NB=4, L=5, F=9, n_animated=2), dict(D=79, NB=9, L=8, F=15, n_animated=19)]


class _Option(object):
    """One option of a step: its primitive, plan, grids and constraint records; tracks and errors per call."""

    def __init__(self, ctx, m, k, n_list, G):
        self.m, self.ctx = m, ctx
        data = synthetic.make_primitive(seed=4100 + k, name="option%d" % k, n_components=m["L"], n_frames=m["F"], n_basis=m["NB"], n_dim=m["D"], n_gmm=1)
        self.prim = _capi.Primitive(ctx, data)
        joints, animated = synthetic.make_skeleton(m["n_animated"])
        self.sk = _capi.Skeleton(joints, animated)
        F = m["F"]
        self.requests = [["LeftHand"], ["Hips", "RightFoot"]]
        self.plan = _capi.TrackPlan(self.prim, self.sk, self.requests, 0)
        self.grid = self.prim.time_grid(np.arange(F - 2, dtype=np.float64))
        self.grids, self.Ts = [self.grid, None], [self.grid.size, self.prim.canonical_grid.size]
        assert self.Ts == [F - 2, F]
        self.alignment = [None, {"joint": 0, "position": [25.0, 89.0, -12.0], "heading": [0.6, -0.8]}, alignment_from_start_pose(START_POSE)][k % 3]
        path = self.prim.back_project_frames_f64(np.zeros((1, m["L"])))[0][::3, :3]
        cps = (path + np.array([3.0, 60.0, -2.0])).tolist()
        self.trajs = [_capi.Trajectory(self.prim, cps, granularity=G), _capi.Trajectory(self.prim, cps[::-1], granularity=1000)]
        descs = (_capi.FrameConstraintDesc * 4)()
        d = descs[0]
        d.type, d.weight, d.n_joints, d.n_frames, d.start_arc = LOCAL, 0.01, 1, F - 3, 2.0
        d.trajectories[0] = self.trajs[0].handle.value
        d = descs[1]
        d.type, d.weight, d.n_joints, d.n_frames = SET, 0.7, 2, F - 1
        for j in range(2):
            d.trajectories[j], d.arc0[j], d.has_range[j], d.range_start[j], d.range_end[j] = self.trajs[j].handle.value, 1.0 + j, 1, 0.0, 1.0e5
        d = descs[2]
        d.type, d.weight, d.n_joints, d.n_frames = CA, 2.0, 1, F - 4
        d.axis_on[0], d.target[0], d.axis_on[2], d.target[2] = 1, 40.0, 1, -5.0
        d = descs[3]
        d.type, d.weight, d.n_joints, d.start_arc = JOINT_TRAJ, 0.5, 1, 0.1
        d.trajectories[0] = self.trajs[1].handle.value
        self.descs, self.request_of, self.n_list = descs, [0, 1, 0, 0], n_list
        self.tables = [(LOCAL, [(0, len(cps) - 1, G)]), (SET, [(0, len(cps) - 1, G), (1, len(cps) - 1, 1000)]), (CA, []), (JOINT_TRAJ, [(1, len(cps) - 1, 1000)])][:n_list]

    def close(self):
        for h in self.trajs + [self.plan, self.grid, self.prim]:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lds", "global"])
def test_options_with_lists_are_the_per_option_launches(variant):
    """Three options on three primitives (different L, NB, F and D: different LDS sizes in the multi tracks kernel) with lists of 0, 1 and
    4 constraints; in the second variant one option's tables pass 150 KB, so every option reads global memory.  Errors and records:
    mg_joint_tracks + mg_score_frame_constraints + the first minimum, per option, bit for bit."""
    vp = C.c_void_p
    ctx = _capi.Context(0)
    R, Q = _capi.MG_TRACK_MAX_REQUESTS, _capi.MG_FRAME_LIST_MAX
    rng = np.random.default_rng(95)
    for lists in ((4, 0, 1), (1, 4, 4)):
        options = [_Option(ctx, m, k, n, G_GLOBAL if (variant == "global" and n == 4 and k < 2) else 1000) for k, (m, n) in enumerate(zip(OPTION_MODELS, lists))]
        routes = [place_tables(o.tables)[1] for o in options]
        assert ("global" in routes) == (variant == "global") and (variant == "global" or "lds" in routes)
        try:
            for B, dtype in ((65, np.float64), (4097, np.float32)):
                n = len(options)
                xs = [rng.standard_normal((B, o.m["L"] + 2)).astype(dtype) for o in options]
                pre = [rng.uniform(0.0, 3.0, B) for _ in options]
                d_x = [ctx.upload(x) for x in xs]
                errs = [Guarded(ctx, B * 8, p) for p in pre]
                refs = [Guarded(ctx, B * 8, p) for p in pre]
                tracks = [[Guarded(ctx, B * T * len(r) * 24) for T, r in zip(o.Ts, o.requests)] for o in options]
                rtracks = [[Guarded(ctx, B * T * len(r) * 24) for T, r in zip(o.Ts, o.requests)] for o in options]
                stride = 16 + 8 * max(o.prim.n_gmm_dims for o in options) + 16
                res = Guarded(ctx, n * stride, np.full(n * stride // 8, SENTINEL, dtype=np.uint64))
                try:
                    prims, plans, lats, eptr, als = (vp * n)(), (vp * n)(), (vp * n)(), (vp * n)(), (vp * n)()
                    grids, tptr, cons, req_of = (vp * (n * R))(), (vp * (n * R))(), (vp * (n * Q))(), (C.c_int32 * (n * Q))()
                    keep = []
                    for k, o in enumerate(options):
                        prims[k], lats[k], eptr[k] = o.prim.handle.value, d_x[k].address, errs[k].ptr
                        if o.n_list:
                            plans[k] = o.plan.handle.value
                            for q in range(2):
                                grids[k * R + q] = o.grids[q].handle.value if o.grids[q] is not None else None
                                tptr[k * R + q] = tracks[k][q].ptr
                            for i in range(o.n_list):
                                cons[k * Q + i], req_of[k * Q + i] = C.addressof(o.descs[i]), o.request_of[i]
                            if o.alignment is not None:
                                keep.append(_capi.ConstraintSet._marshal_alignment(o.alignment, o.sk))
                                als[k] = C.addressof(keep[-1])
                    _capi._check(ctx.lib.mg_options_frame_lists(n, prims, plans, lats, _capi._dtype_code(xs[0]), B, (C.c_int64 * n)(*[x.shape[1] for x in xs]), als, grids,
                                                                tptr, (C.c_int32 * n)(*[o.n_list for o in options]), cons, req_of, eptr, res.ptr, stride, None))
                    raw = res.read((n * stride,), np.uint8, ("lists", variant, lists, B))
                    for k, o in enumerate(options):
                        tag = (variant, lists, B, k)
                        if o.n_list:
                            o.plan.tracks_dev(d_x[k], dtype, B, xs[k].shape[1], o.grids, [t.ptr for t in rtracks[k]], o.alignment)
                            m_ = o.n_list
                            _capi._check(ctx.lib.mg_score_frame_constraints(
                                o.prim.handle, m_, (vp * m_)(*[C.addressof(o.descs[i]) for i in range(m_)]), (vp * m_)(*[rtracks[k][o.request_of[i]].ptr for i in range(m_)]),
                                (C.c_int32 * m_)(*[o.Ts[o.request_of[i]] for i in range(m_)]), (C.c_int32 * m_)(*[len(o.requests[o.request_of[i]]) for i in range(m_)]),
                                B, refs[k].ptr, 1, None))
                            for q, (T, r) in enumerate(zip(o.Ts, o.requests)):
                                shape = (B, T, len(r), 3)
                                np.testing.assert_array_equal(_bits64(tracks[k][q].read(shape, np.float64, tag)), _bits64(rtracks[k][q].read(shape, np.float64, tag)))
                        want = refs[k].read((B,), np.float64, tag)
                        got = errs[k].read((B,), np.float64, tag)
                        np.testing.assert_array_equal(_bits64(got), _bits64(want), err_msg=str(tag))
                        assert (o.n_list == 0) == np.array_equal(got, pre[k]) and np.isfinite(got).all()
                        idx, err, row, rest = _records(raw, n, stride, o.prim.n_gmm_dims)[k]
                        want_i, want_e = orc.first_min_argmin(want)
                        assert (idx, err) == (want_i, want_e), (tag, idx, err, want_i, want_e)
                        np.testing.assert_array_equal(_bits64(row), _bits64(xs[k][want_i, :o.prim.n_gmm_dims].astype(np.float64)), err_msg=str(tag))
                        assert (rest == np.uint64(SENTINEL)).all(), ("bytes behind the record", tag)
                    if variant == "global":
                        LEDGER.add("route:global")
                    if B > 4096:
                        LEDGER.add("nwg>64")
                finally:
                    ctx.synchronize()
                    for b in d_x + errs + refs + [t for ts in tracks + rtracks for t in ts] + [res]:
                        b.free()
        finally:
            for o in options:
                o.close()
    ctx.close()


# ---- 5. the ledger ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_ledger_covers_every_route():
    """Runs last: both table routes, the opt-in band, both CA load paths, n_frames < T for the three types that have it, every B mod 4
    and D < 7 for the tracks, more than 64 workgroups per option and the in-list joint trajectory ran on the GPU."""
    missing = LEDGER_WANT - LEDGER
    assert not missing, sorted(missing)
    print("worst deviation from the oracle, relative to max(1, max |oracle|) (bound %.0e): %s" % (
        TOL, ", ".join("%s %.2e" % kv for kv in sorted(WORST.items()))))
