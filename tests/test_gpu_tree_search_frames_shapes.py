"""mg_cluster_tree_search_frames across its ladder's further rungs, halved track groups, KD descents and slabs: the GPU half of the
sweep rows of tests/tree_search_frames_cases.py (SWEEP_ROWS; tests/test_tree_search_frames_host.py holds their plans to the header and
conditions every one of them for the oracle).

Every row: the plan query equals the row's claim; (row, leaf, evaluations) equal the descent replayed on the oracle's values and, where
mg_score_constraints takes the shape (yardstick "batched"), the host-driven descent through candidate_scoring.errors_of_samples; the value
agrees with each of them under fc.tolerance -- tests/test_gpu_frame_constraints.py's, unchanged.  Then: one search's record is the same
bytes whichever rung a neighbour forces the call onto; primitives of different widths in one call; the slab stays inside scratch_bytes
and a slab too short or misaligned is refused; misuse of the lists' arguments returns status codes with the records untouched."""
import ctypes as C

import numpy as np
import pytest

import tree_search_frames_cases as fc
from morphablegraphs_amd import _capi, candidate_scoring, cluster_tree, frame_constraints
from morphablegraphs_amd.cluster_tree import frames_search_plan, search_on_device
from test_gpu_tree_search_frames import Search, close_to

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    candidate_scoring.clear_constraint_cache()
    c.close()


@pytest.fixture(scope="module")
def prims(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _capi.Primitive(ctx, fc.model(name))
        return made[name]
    yield get
    candidate_scoring.clear_constraint_cache()
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def worst():
    """row -> |device - oracle| / tolerance, filled by the rows that ran; the largest is printed when the module is done"""
    seen = {}
    yield seen
    if seen:
        name = max(seen, key=seen.get)
        print("\nworst |device - oracle| / tolerance over %d rows: %.3g (%s)" % (len(seen), seen[name], name))


def _search(ctx, triples, n_cand):
    """search_on_device for searches with lists, into a slab of this test's own, filled with NaNs (every byte 0xFF) and exactly as long as
    the plan query says: a track that the launch scores without having formed it cannot pass for a position"""
    head, tail = cluster_tree._frames_arguments(triples)
    nbytes = max(_capi.cluster_tree_frames_plan(*head, n_cand, *tail)["scratch_bytes"], 256)
    slab = ctx.malloc(nbytes)
    try:
        ctx.upload_into(slab, np.full(nbytes, 0xFF, dtype=np.uint8))
        return _capi.search_cluster_trees_frames(*head, n_cand, *tail, scratch_dev=slab)
    finally:
        slab.free()


def _closed(searches):
    for s in searches:
        s.close()


@pytest.mark.parametrize("name", fc.SWEEP_IDS)
def test_every_sweep_row_is_the_descent_and_the_oracles_value(ctx, prims, worst, name):
    r = fc.BY_NAME[name]
    s = Search(prims(r["prim"]), r)
    try:
        want = fc.row_plan(r, s.cons)
        got = frames_search_plan([s.triple()], r["n_cand"])
        assert got == want, (name, got, want)
        if r["refused"]:
            assert got["refused"] and got["track_group"] == 1
            with pytest.raises(_capi.MGError) as e:
                search_on_device([s.triple()], r["n_cand"])
            assert e.value.status == _capi.MG_ERR_UNSUPPORTED
            return
        o = fc.oracle_of(r)
        rec = _search(ctx, [s.triple()], r["n_cand"])[0]
        ratio = abs(rec["value"] - o["value"]) / fc.tolerance(r, o["value"])
        worst[name] = float(ratio)
        print("%s (%s): plan %d bytes, group %d, tables %s; row %d leaf %d evaluations %d value %.15g; oracle row %d leaf %d evaluations %d value %.15g; "
              "|device - oracle| / tolerance %.3g" % (name, r["yardstick"], got["lds_bytes"], got["track_group"], got["tables_lds"], rec["row"], rec["leaf"],
                                                      rec["evaluations"], rec["value"], o["row"], o["leaf"], o["evaluations"], o["value"], ratio))
        assert rec["flags"] == 0
        assert (rec["row"], rec["leaf"], rec["evaluations"]) == (o["row"], o["leaf"], o["evaluations"]), (name, rec, o["row"], o["leaf"], o["evaluations"])
        assert close_to(r, rec["value"], o["value"]), (name, rec["value"], o["value"], ratio)
        if r["yardstick"] == "batched":
            value, row, leaf, n_eval = s.descent(r["n_cand"])
            assert (rec["row"], rec["leaf"], rec["evaluations"]) == (row, leaf, n_eval), (name, rec, row, leaf, n_eval)
            again = s.errors(s.table()[int(rec["row"] if r["kind"] == "kd" else rec["leaf"])][None, :])[0]        # of the sample the launch returned
            print("%s: descent %.15g, errors_of_samples %.15g" % (name, value, again))
            assert close_to(r, rec["value"], value) and close_to(r, rec["value"], again), (name, rec["value"], value, again)
        else:       # the oracle alone is the yardstick only because the host-driven descent's scorer really refuses the shape
            with pytest.raises(_capi.MGError) as e:
                s.errors(s.table()[:1])
            assert e.value.status == _capi.MG_ERR_UNSUPPORTED
    finally:
        s.close()


def _as_kind(name, kind):
    return dict(fc.BY_NAME[name], kind=kind)


@pytest.mark.parametrize("kind,subject", [("feature", "flat65-local-short"), ("kd", "kd_descents-33-2-group4")])
def test_a_search_returns_the_same_bytes_on_every_rung_a_neighbour_forces(ctx, prims, kind, subject):
    r = fc.BY_NAME[subject]
    s = Search(prims(r["prim"]), r)
    try:
        plan = frames_search_plan([s.triple()], 2)
        assert plan["track_group"] == 4 and plan["tables_lds"]
        alone = _search(ctx, [s.triple()], 2)[0]
        assert alone["flags"] == 0
        others = [(fc.neighbour(kind, [r], 2), 2), (fc.neighbour(kind, [r], 1), 1), (_as_kind("tables_memory", kind), 4)]
        for q, group in others:
            other, tables = q["name"], False
            assert fc.merged_fit(kind, [r, q])["track_group"] == group
            b = Search(prims(q["prim"]), q)
            try:
                plan = frames_search_plan([s.triple(), b.triple()], 2)
                assert (plan["track_group"], plan["tables_lds"]) == (group, tables) and not plan["refused"], (other, plan)
                assert {k: v for k, v in plan.items() if k != "scratch_bytes"} == fc.merged_fit(kind, [r, q]), (other, plan)
                both = _search(ctx, [s.triple(), b.triple()], 2)
                assert both[0].tobytes() == alone.tobytes(), (subject, other, both[0], alone)
                assert both[1].tobytes() == _search(ctx, [b.triple()], 2)[0].tobytes(), (other, both[1])
            finally:
                b.close()
    finally:
        s.close()


@pytest.mark.parametrize("kind", ["feature", "kd"])
def test_primitives_of_different_widths_in_one_call(ctx, prims, kind):
    """49 and 77 control points and a search without a list in one call: each workgroup strides the control points by its own count"""
    rows = [_as_kind("flat64-discrete", kind), fc.BY_NAME["kd_descents-32-1-group4"] if kind == "kd" else fc.BY_NAME["list_at_cap"], _as_kind("mixed_list", kind)]
    searches = [Search(prims(r["prim"]), r, with_frames=(i != 2)) for i, r in enumerate(rows)]
    halving = fc.neighbour(kind, rows, 2, [True, True, False])
    searches.append(Search(prims(halving["prim"]), halving))
    try:
        assert searches[2].sset.frame_constraints is None
        alone = [search_on_device([s.triple()], 2)[0] for s in searches]
        for n, group in ((3, 4), (4, 2)):
            triples = [s.triple() for s in searches[:n]]
            plan = frames_search_plan(triples, 2)
            assert plan["track_group"] == group and plan["control_points"] == 77, plan
            assert {k: v for k, v in plan.items() if k != "scratch_bytes"} == fc.merged_fit(kind, (rows + [halving])[:n], [True, True, False, True][:n]), plan
            for s, rec, want in zip(searches, _search(ctx, triples, 2), alone):
                assert rec["flags"] == 0 and rec.tobytes() == want.tobytes(), (s.r["name"], n, rec, want)
    finally:
        _closed(searches)


def _raw_call(searches):
    """The arguments of mg_cluster_tree_search_frames_host as _capi marshals them: (lib, m, args, what they point to)"""
    head, tail = cluster_tree._frames_arguments([s.triple() for s in searches])
    m, args, keep = _capi._tree_frames_arguments(*head, *tail)
    return head[0][0].lib, m, args, keep


def _launch(lib, m, args, n_cand, ptr, nbytes, records):
    return lib.mg_cluster_tree_search_frames_host(m, *args, int(n_cand), C.c_void_p(ptr), int(nbytes), records.ctypes.data_as(C.c_void_p))


def test_the_slab_stays_inside_scratch_bytes_and_a_short_or_misaligned_one_is_refused(ctx, prims):
    rows = [fc.BY_NAME[n] for n in ("list_at_cap", "flat65-local-short", "two_level-n2-rotation")]      # three slabs one behind the other, two with rotation rows
    searches = [Search(prims(r["prim"]), r) for r in rows]
    buf = None
    try:
        plan = frames_search_plan([s.triple() for s in searches], 2)
        nb = plan["scratch_bytes"]
        assert nb == sum(fc.row_plan(r)["scratch_bytes"] for r in rows) and nb % 256 == 0
        tail = 4096
        buf = ctx.malloc(nb + tail)
        ctx.upload_into(buf, np.full(nb + tail, 0xA5, dtype=np.uint8))
        lib, m, args, keep = _raw_call(searches)
        rec = np.zeros(m, dtype=_capi.TREE_SEARCH_RECORD)
        assert _launch(lib, m, args, 2, buf.ptr.value, nb, rec) == 0
        after = ctx.download(buf, (nb + tail,), np.uint8)
        assert np.all(after[nb:] == 0xA5) and np.any(after[:nb] != 0xA5)
        for s, got in zip(searches, rec):
            assert got.tobytes() == search_on_device([s.triple()], 2)[0].tobytes(), s.r["name"]
        # one byte short; eight bytes off the boundary: refused, the records untouched
        for ptr, nbytes in ((buf.ptr.value, nb - 1), (buf.ptr.value + 8, nb)):
            untouched = np.full(m * _capi.TREE_SEARCH_RECORD.itemsize, 0x5A, dtype=np.uint8)
            assert _launch(lib, m, args, 2, ptr, nbytes, untouched) == _capi.MG_ERR_INVALID_ARGUMENT
            assert np.all(untouched == 0x5A)
        assert np.array_equal(ctx.download(buf, (nb + tail,), np.uint8), after)
    finally:
        if buf is not None:
            buf.free()
        _closed(searches)


class _Rotation6(object):
    """A search on a primitive of six channels (no quaternion) whose list is one hand-made joint-rotation descriptor: what
    frame_constraints.TreeFrameList refuses to build.  A one-joint skeleton without animated joints, its track plan, a one-sample grid."""

    def __init__(self, ctx):
        from morphablegraphs_amd import synthetic
        from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, TreeSearchSet
        import types
        self.prim = _capi.Primitive(ctx, synthetic.make_primitive(seed=306, n_components=2, n_frames=8, n_basis=5, n_dim=6, n_gmm=2))
        self.sk = _capi.Skeleton([("Hips", None, (0.0, 0.0, 0.0))], [])
        self.plan = _capi.TrackPlan(self.prim, self.sk, [[0]], 0)
        self.grid = self.prim.time_grid(np.asarray([3.0]))
        descs = (_capi.FrameConstraintDesc * 1)()
        descs[0].type, descs[0].weight, descs[0].n_joints, descs[0].quat_channel = _capi.MG_FRAME_JOINT_ROTATION, 1.0, 1, 3
        descs[0].quaternion[0] = 1.0
        flist = types.SimpleNamespace(plan=self.plan, grids=[None], descs=descs, req_of=[0], rotation_grids=[self.grid], skeleton=self.sk, release=lambda: None)
        self.cset = _capi.ConstraintSet(self.prim, [{"type": "position", "t": 7.0, "weight": 1.0, "target": [1.0, None, 2.0]}])
        means = np.concatenate([np.zeros((1, 2)), np.random.default_rng(6).standard_normal((3, 2))])
        self.tree = HipFeatureClusterTree(means, means, [0, 3, 3, 3, 3], np.arange(1, 4), [-1, 1, 2, 3], n_spatial=2)
        self.sset = TreeSearchSet(self.cset, [], None, flist)

    def triple(self):
        return (self.tree, self.prim, self.sset)

    def close(self):
        self.grid.close()
        for h in (self.cset, self.tree, self.prim):
            h.close()


def test_misuse_of_the_lists_returns_status_codes_and_launches_nothing(ctx, prims):
    """Through _capi's ctypes layer, where the wrappers cannot express the misuse"""
    r = fc.BY_NAME["two_level-n2-rotation"]       # one joint rotation: one constraint, its one-sample grid
    s = Search(prims("chain3"), r)
    t = Search(prims("tiny"), fc.BY_NAME["flat3-ca-one_frame"])
    six = _Rotation6(ctx)
    buf = ctx.malloc(1 << 20)
    try:
        def status(search, change, says=None):
            lib, m, args, keep = _raw_call([search])
            plans, grids, counts, cons, req, rot = keep[2]
            change(plans, counts, cons, req, rot)
            records = np.full(m * _capi.TREE_SEARCH_RECORD.itemsize, 0x5A, dtype=np.uint8)
            rc = _launch(lib, m, args, 2, buf.ptr.value, buf.nbytes, records)
            if rc != 0:
                assert np.all(records == 0x5A)
                assert says is None or says in lib.mg_last_error().decode(), lib.mg_last_error()
            return rc, records
        # the control: the same calls into the same buffer, nothing changed
        for search in (t, s):
            rc, records = status(search, lambda plans, counts, cons, req, rot: None)
            assert rc == 0 and records.tobytes() == search_on_device([search.triple()], 2).tobytes()
        bad = _capi.MG_ERR_INVALID_ARGUMENT

        def five(plans, counts, cons, req, rot):
            counts[0] = _capi.MG_FRAME_LIST_MAX + 1
        assert status(t, five, "per-frame constraints outside")[0] == bad

        def foreign_plan(plans, counts, cons, req, rot):
            plans[0] = s.sset.frame_constraints.plan.handle.value
        assert status(t, foreign_plan, "no track plan of its primitive")[0] == bad

        def request_out_of_range(plans, counts, cons, req, rot):
            req[0] = 1
        assert status(t, request_out_of_range, "reads request 1 of 1")[0] == bad

        def negative_request(plans, counts, cons, req, rot):
            req[0] = -1
        assert status(t, negative_request, "reads request -1 of 1")[0] == bad

        def rotation_without_grid(plans, counts, cons, req, rot):
            rot[0] = None
        assert status(s, rotation_without_grid, "needs a one-sample grid")[0] == bad
        # a joint rotation on a primitive without quaternions: its plan, its one-sample grid, and still refused
        assert status(six, lambda plans, counts, cons, req, rot: None, "on a primitive without quaternions")[0] == bad
    finally:
        buf.free()
        six.close()
        s.close()
        t.close()


def test_slabs_beyond_the_scratch_limit_are_refused_by_the_plan_query(ctx, prims):
    """MG_TREE_SCRATCH_MAX, by the plan query alone (nothing allocated, nothing launched): 32 searches of one request whose grid has T
    samples take 32 x 64 x T x 24 bytes -- the last T under 256 MiB is planned, the next is MG_ERR_UNSUPPORTED"""
    s = Search(prims("tiny"), fc.BY_NAME["flat3-ca-one_frame"])
    n = 32
    per_sample = n * 64 * 24
    T = fc.SCRATCH_MAX // per_sample          # (the slabs are rounded up to 256 bytes each: 64 x 24 x T already is a multiple)
    grids = [s.prim.time_grid(np.linspace(0.0, fc.F - 1.0, t)) for t in (T, T + 1)]
    try:
        assert n * fc.scratch_bytes([(T, 1)], 0, 7) <= fc.SCRATCH_MAX < n * fc.scratch_bytes([(T + 1, 1)], 0, 7)
        for g, want in zip(grids, (_capi.MG_OK, _capi.MG_ERR_UNSUPPORTED)):
            lib, m, args, keep = _raw_call([s] * n)
            request_grids = keep[2][1]
            for i in range(n):
                request_grids[i * _capi.MG_TRACK_MAX_REQUESTS] = g.handle.value
            info = _capi.TreeFramesPlanInfo()
            rc = lib.mg_cluster_tree_search_frames_plan(m, *args, 2, C.byref(info))
            assert rc == want, (g.size, rc, lib.mg_last_error())
            if want == _capi.MG_OK:
                assert info.scratch_bytes == n * fc.scratch_bytes([(T, 1)], 0, 7) and not info.refused
            else:
                assert "track slabs" in lib.mg_last_error().decode()
    finally:
        for g in grids:
            g.close()
        s.close()
