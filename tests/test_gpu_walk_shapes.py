"""The graph-walk kernels across their shape edges: mg_walk_chain_kernel / mg_walk_frames_kernel (FRAME_ROWS), mg_walk_time_kernel
(TIME_ROWS) and mg_walk_score_kernel (SCORE_ROWS) of tests/walk_shape_cases.py; the CPU half is tests/test_walk_shapes_host.py.

Time rows: the one-launch objective against the step-by-step chain (obj_time_error_sum over HipTimeConstraints) bit for bit, and against
oracle.time_constraints_error over the oracle's canonical time functions plus score_samples, at the bounds
tests/test_gpu_walk_time_objective.py uses against the reference's own class; outputs between guard words; the refused row writes nothing.
Score rows: HipGraphWalkObjective.blocks against objective_functions._global_blocks bit for bit, against
oracle.graph_walk_residual_blocks on every candidate of the batches up to 17 at 1e-9, and the table by hand for errors only, wider rows,
descending offsets and the refusal.

Every row runs mg_walk_frames once over a NaN sentinel that is three rows longer than the walk:
  * rows of n_dim 3, 4, 6 are one unaligned step: the frames are the bits of mg_back_project_frames_f64, the transform the identity
    (the chain kernel then reads the root translation alone: with the root's quaternion channels in its list it read up to four doubles
    past the primitive's mean vector and past the last row of its eigenvectors);
  * every other row is held to graph_walk.assemble_walk_host within tests/test_graph_walk_host.py's WALK_TOLERANCE of the largest |root
    coordinate| -- frames and transforms -- after the CPU half has held assemble_walk_host to the oracle on that very row;
  * every element the walk does not own still holds the sentinel;
  * a row that expects a refusal gets that status and both outputs come back untouched.
The library's answer is compared with walk_frames_plan first: a refusal where the row claims a launch fails the row.  LEDGER collects
the routes of the rows that ran and matched; test_the_ledger_covers_every_route fails when one named by the table is missing.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import walk_shape_cases as wc
from morphablegraphs_amd import _capi
from morphablegraphs_amd import graph_walk as gw
from test_graph_walk_host import WALK_TOLERANCE, root_scale

pytestmark = pytest.mark.gpu

LEDGER = set()
GUARD_ROWS = 3
X_FILL = -777.25                        # what the transforms hold before the call


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def _run(ctx, prims, row, S, alignment, skeleton, stride):
    """One mg_walk_frames call: (status, frames (n, stride, D) over the sentinel, transforms (n, n_steps, 4) over X_FILL)."""
    seq = [prims[k] for k in row["sequence"]]
    n, m, D = S.shape[0], len(seq), row["D"]
    latent_offset = np.concatenate(([0], np.cumsum([p.n_components for p in seq])[:-1]))
    with ctx.buffers() as bufs:
        d_S, d_f = bufs.upload(S), bufs.upload(np.full((n, stride, D), np.nan))
        d_x = bufs.upload(np.full((n, m, 4), X_FILL))
        status = _capi.MG_OK
        try:
            gw.walk_frames_dev(seq, latent_offset, d_S, S.dtype, n, S.shape[1], d_f, stride, None, None, 0,
                               None if row["offsets"] is None else np.asarray(row["offsets"], dtype=np.int64), alignment, skeleton, d_x)
        except _capi.MGError as e:
            status = e.status
        ctx.synchronize()
        return status, ctx.download(d_f, (n, stride, D), np.float64), ctx.download(d_x, (n, m, 4), np.float64)


@pytest.mark.parametrize("name", wc.FRAME_IDS)
def test_walk_frames_rows(ctx, name):
    row = wc.FRAME_BY_NAME[name]
    models = wc.frame_models(row)
    prims = [_capi.Primitive(ctx, m) for m in models]
    try:
        _, steps, S64, alignment, hip_sk, _, _ = wc.frame_case(row, models)
        S = S64.astype(row["dtype"])
        assert np.array_equal(S.astype(np.float64), S64)
        total = sum(d["n_canonical_frames"] for d in steps)
        stride = wc.PARITY_STRIDE if row["offsets"] is not None else total + GUARD_ROWS
        try:
            plan, want_status = wc.frame_plan(row), _capi.MG_OK
        except wc.Refused as e:
            plan, want_status = None, e.status
        assert want_status == (row["expect"] if row["expect"] is not None else _capi.MG_OK)
        status, got, got_x = _run(ctx, prims, row, S, alignment, hip_sk, stride)
        assert status == want_status, "row %s: the library answers %d, the restated plan %d" % (name, status, want_status)
        if plan is None:
            assert np.isnan(got).all() and np.all(got_x == X_FILL), "a refused call wrote to its outputs"
        elif row["D"] < 7:
            ref = prims[row["sequence"][0]].back_project_frames_f64(S)
            assert np.array_equal(got[:, :total], ref) and np.isnan(got[:, total:]).all()
            assert np.array_equal(got_x, np.tile([1.0, 0.0, 0.0, 0.0], (len(S), 1, 1)))
        else:
            frames, offsets, ref_x = gw.assemble_walk_host(steps, S64, alignment=alignment, skeleton=hip_sk)
            ref = wc.place(frames, offsets, row, stride)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), "the sentinel around the walk, or a row of the walk"
            assert np.isnan(ref).sum() == (stride - total) * len(S) * row["D"]
            scale = root_scale(ref)
            worst, worst_x = float(np.nanmax(np.abs(got - ref))) / scale, float(np.max(np.abs(got_x - ref_x))) / scale
            print("row %s: frames %.3g, transforms %.3g of the root scale %.4g (bound %.3g)" % (name, worst, worst_x, scale, WALK_TOLERANCE))
            assert worst <= WALK_TOLERANCE and worst_x <= WALK_TOLERANCE
        LEDGER.update(row["routes"])
    finally:
        for p in prims:
            p.close()


# ---- mg_walk_time_kernel --------------------------------------------------------------------------------------------------------------
# Bounds against the oracle: those tests/test_gpu_walk_time_objective.py holds the kernel to against the reference's own class.
TIME_ERR_TOL, TIME_LL_RTOL, TIME_LL_ATOL = 1e-9, 1e-9, 1e-8
TIME_SCALES = (2.0, 0.3)
TIME_GUARD = -12345.5


@pytest.fixture(scope="module")
def time_nodes(ctx):
    from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode
    nodes = {}
    for name in sorted(wc.TIME_SHAPES):
        node = HipMotionStateGraphNode(context=ctx)
        node.init_from_dict("walk", {"name": name, "mm": wc.time_model(name)})
        nodes[name] = node
    yield nodes
    from morphablegraphs_amd import objective_functions as of
    of.clear_walk_objectives()
    for node in nodes.values():
        node.motion_primitive._prim.close()


@pytest.mark.parametrize("row", wc.TIME_IDS)
def test_walk_time_rows(ctx, time_nodes, row):
    from morphablegraphs_amd import objective_functions as of
    from test_gpu_walk_time_objective import _Graph, _Step, _Walk
    window, n, params, S, clist = wc.time_case(row)
    names = (wc.FIRST_STEP,) + tuple(window)
    graph = _Graph({time_nodes[k].node_key: time_nodes[k] for k in set(names)}, wc.FRAME_TIME)
    walk = _Walk([_Step(time_nodes[k].node_key, p, wc.TIME_SHAPES[k][1], wc.TIME_SHAPES[k][2]) for k, p in zip(names, params)])
    tc = of.HipTimeConstraints(graph, walk, 1, len(names), clist)
    try:
        plan, want_status = wc.time_plan(row), _capi.MG_OK
    except wc.Refused as e:
        plan, want_status = None, e.status
    assert want_status == wc.TIME_REFUSED.get(row, _capi.MG_OK)
    objective = of.HipWalkTimeObjective(graph, walk, tc)
    try:
        es, qs = TIME_SCALES
        guarded = np.full(3 * n + 4, TIME_GUARD)
        status = _capi.MG_OK
        with ctx.buffers() as bufs:
            d_S, d_o = bufs.upload(np.ascontiguousarray(S if S.shape[1] else np.zeros((n, 1)))), bufs.upload(guarded)
            at = lambda i: d_o.address + 8 * i
            try:
                objective.table.score_dev(d_S, np.float64, n, S.shape[1], es, qs, at(1), at(n + 2), at(2 * n + 3))
            except _capi.MGError as e:
                status = e.status
            ctx.synchronize()
            out = ctx.download(d_o, (3 * n + 4,), np.float64)
        assert status == want_status, "row %s: the library answers %d, the restated plan %d" % (row, status, want_status)
        if plan is None:
            assert np.all(out == TIME_GUARD), "a refused call wrote to its outputs"
            LEDGER.add("time:refused")
            return
        assert np.all(out[[0, n + 1, 2 * n + 2, 3 * n + 3]] == TIME_GUARD), "a guard word between the outputs"
        obj, err, ll = out[1:n + 1], out[n + 2:2 * n + 2], out[2 * n + 3:3 * n + 3]
        # 1. the step-by-step chain, bit for bit
        want_obj = np.atleast_1d(of.obj_time_error_sum(S, (graph, walk, tc, es, qs)))
        want_err, want_ll = np.atleast_1d(tc.evaluate_graph_walk(S, graph, walk)), np.atleast_1d(tc.get_average_loglikelihood(S, graph, walk))
        assert np.array_equal(ll, want_ll) and np.array_equal(err, want_err) and np.array_equal(obj, want_obj)
        # 2. the oracle
        start, tfs, lps = wc.time_oracle_functions(row)
        o_err = np.array([orc_error([tf[b] for tf in tfs], clist, start) for b in range(n)])
        o_ll = sum(lps) / len(lps)
        print("row %s: |error - oracle| / max(1, error) %.3g, |log-likelihood - oracle| %.3g" %
              (row, float(np.max(np.abs(err - o_err) / np.maximum(1.0, np.abs(o_err)))), float(np.max(np.abs(ll - o_ll)))))
        np.testing.assert_allclose(tc.start_keyframe, start, rtol=1e-12)
        np.testing.assert_allclose(err, o_err, rtol=TIME_ERR_TOL, atol=TIME_ERR_TOL)
        np.testing.assert_allclose(ll, o_ll, rtol=TIME_LL_RTOL, atol=TIME_LL_ATOL)
        np.testing.assert_allclose(obj, es * o_err - qs * o_ll, rtol=TIME_LL_RTOL, atol=TIME_LL_ATOL)
        for s in plan["steps"]:
            LEDGER.update({"time:KKg_%d" % s["KKg"], "time:chunks_%d" % s["chunks"], "time:gamma_%s" % ("memory" if s["gamma_from_memory"] else "registers")})
        LEDGER.update({"time:wave_doubles_%s" % ("chunk" if plan["wave_doubles"] == 16 * wc.MG_WTIME_BS else "mixture"), "time:steps_%d" % len(window),
                       "time:batch_%d" % n, "time:opt_in" if plan["opt_in"] else "time:plain_lds"})
    finally:
        objective.close()


# ---- mg_walk_score_kernel ---------------------------------------------------------------------------------------------------------------
SCORE_ORACLE_TOL = 1e-9                 # tests/test_gpu_walk_objective.py::test_one_launch_against_the_oracle
SCORE_FILL = -4321.75


@pytest.fixture(scope="module")
def score_world(ctx):
    from morphablegraphs_amd import objective_functions as of
    from morphablegraphs_amd import synthetic
    from morphablegraphs_amd.candidate_scoring import clear_constraint_cache
    from morphablegraphs_amd.motion_state_graph import HipMotionStateGraphNode
    w = type("World", (), {})()
    w.joints, w.animated = synthetic.make_skeleton()
    w.hip_sk = _capi.Skeleton(w.joints, w.animated)
    w.nodes, w.ops = {}, {}
    for L in wc.SCORE_WIDTHS + (wc.SCORE_REFUSED_L,):
        data = wc.score_model(L)
        node = HipMotionStateGraphNode(context=ctx)
        node.init_from_dict("walk", {"name": "L%d" % L, "mm": data})
        w.nodes[L], w.ops[L] = node, wc.orc.OraclePrimitive(data)
    prev = w.ops[33].back_project_frames(np.random.default_rng(9).standard_normal(33))[-3:].copy()
    prev[:, 0] += 120.0
    prev[:, 2] -= 40.0
    w.prev = prev
    yield w
    of.clear_walk_objectives()
    clear_constraint_cache()
    for node in w.nodes.values():
        node.motion_primitive._prim.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("row", wc.SCORE_IDS)
def test_walk_score_rows(ctx, score_world, row):
    from morphablegraphs_amd import objective_functions as of
    from test_gpu_walk_objective import _Constraints, _Graph, _Skeleton, _Step
    w = score_world
    widths, n_cons, n, dtype, what = wc.SCORE_ROWS[row]
    node_name = "Spine" if "deep" in what or n_cons == 15 else "Hips"
    ref_sk = _Skeleton(node_name)
    cons = [wc.score_constraints(n_cons, i, "deep" in what) for i in range(len(widths))]
    rng = np.random.default_rng(5)
    steps = [_Step(w.nodes[L].node_key, rng.standard_normal(L), L, _Constraints(c, False, w.hip_sk, ref_sk)) for L, c in zip(widths, cons)]
    graph = _Graph({w.nodes[L].node_key: w.nodes[L] for L in widths}, ref_sk, w.hip_sk)
    S = wc.score_latents(row)
    obj = of.HipGraphWalkObjective(graph, steps, w.prev, "frames")
    try:
        if "refused" in what:
            with pytest.raises(_capi.MGError) as e:
                obj.table.score(S, obj.n_columns, fill=SCORE_FILL)
            assert e.value.status == _capi.MG_ERR_UNSUPPORTED and "LDS" in str(e.value)
            with ctx.buffers() as bufs:        # nothing is written
                d_S, d_r = bufs.upload(S), bufs.upload(np.full((n, obj.n_columns + 5), SCORE_FILL))
                with pytest.raises(_capi.MGError):
                    obj.table.score_dev(d_S, S.dtype, n, S.shape[1], d_r, obj.n_columns, d_r.address + 8 * n * obj.n_columns, d_r.address + 8 * n * (obj.n_columns + 1))
                ctx.synchronize()
                assert np.all(ctx.download(d_r, (n, obj.n_columns + 5), np.float64) == SCORE_FILL)
            LEDGER.add("score:refused")
            return
        if "force_valu" in what:
            ctx.set_option(_capi.MG_OPT_FORCE_VALU_SCORE, 1)
        try:
            got = obj.blocks(S)
            want = of._global_blocks(S, graph, steps, w.prev, "frames")[2]      # (the chain under the same option)
        finally:
            ctx.set_option(_capi.MG_OPT_FORCE_VALU_SCORE, 0)
        assert len(got) == len(want) == len(widths)
        for g, v in zip(got, want):
            assert g.shape == v.shape == (n, n_cons) and np.array_equal(_bits(g), _bits(v))
        if "force_valu" in what:          # ... and the packed route of the same walk, against its own chain
            got2 = obj.blocks(S)
            for g, v in zip(got2, of._global_blocks(S, graph, steps, w.prev, "frames")[2]):
                assert np.array_equal(_bits(g), _bits(v))
            LEDGER.add("score:force_valu")
        # the oracle, every candidate up to 17
        if n <= 17:
            worst = 0.0
            for b in range(n):
                alphas = np.split(S[b].astype(np.float64), np.cumsum(widths)[:-1])
                blocks = wc.orc.graph_walk_residual_blocks([w.ops[L] for L in widths], alphas, cons, w.prev[-1], w.joints, w.animated, node_name, exit_from="frames")
                for g, o in zip(got, blocks):
                    worst = max(worst, float(np.max(np.abs(g[b] - o) / np.maximum(1.0, np.abs(o)))))
                    np.testing.assert_allclose(g[b], o, rtol=SCORE_ORACLE_TOL, atol=SCORE_ORACLE_TOL)
            print("row %s: worst |residual - oracle| / max(1, |oracle|) %.3g" % (row, worst))
            LEDGER.add("score:oracle_every_candidate")
        # the table by hand: errors only; rows wider than the walk with its columns off 0; steps listed with descending offsets
        recs = obj.table.steps
        res, err, ex = obj.table.score(S, obj.n_columns)
        if "errors_only" in what:
            _, err_only, _ = obj.table.score(S, obj.n_columns, residuals=False, errors=True, exit_state=False)      # (the columns are still checked against ld_res)
            assert np.array_equal(_bits(err_only), _bits(err))
            np.testing.assert_allclose(err_only, res.sum(axis=1), rtol=1e-9, atol=1e-9)
            LEDGER.add("score:errors_only")
        if "wide_ld" in what or "descending" in what:
            order = list(range(len(recs)))[::-1] if "descending" in what else list(range(len(recs)))
            pad = 3 if "wide_ld" in what else 0
            lat_at, col_at, lo, co = {}, {}, pad and 2, pad and 1
            for i in order:                   # offsets handed out in listing order: descending in step order when the order is reversed
                lat_at[i], col_at[i] = lo, co
                lo, co = lo + widths[i], co + recs[i][4]
            S2 = np.full((n, lo + (pad and 1)), 99.0, dtype=S.dtype)
            off = 0
            for i, L in enumerate(widths):
                S2[:, lat_at[i]:lat_at[i] + L] = S[:, off:off + L]
                off += L
            table = _capi.WalkScoreTable([(recs[i][0], recs[i][1], recs[i][2], lat_at[i], recs[i][4], col_at[i]) for i in range(len(recs))])
            res2, err2, ex2 = table.score(S2, co + pad, fill=SCORE_FILL)
            for i in range(len(recs)):
                assert np.array_equal(_bits(res2[:, col_at[i]:col_at[i] + recs[i][4]]), _bits(res[:, recs[i][5]:recs[i][5] + recs[i][4]]))
            owned = np.zeros(co + pad, dtype=bool)
            for i in range(len(recs)):
                owned[col_at[i]:col_at[i] + recs[i][4]] = True
            assert np.all(res2[:, ~owned] == SCORE_FILL) and np.array_equal(_bits(err2), _bits(err)) and np.array_equal(_bits(ex2), _bits(ex))
            LEDGER.add("score:wide_ld" if pad else "score:descending")
        for L in widths:
            LEDGER.add("score:KK_%d" % wc.k_steps(L))
            LEDGER.add("score:staged" if L > 64 else "score:packed")
        LEDGER.update({"score:batch_%d" % n, "score:sets_%d" % n_cons, "score:lat_%s" % np.dtype(dtype).name})
        if "deep" in what:
            LEDGER.add("score:deep_chains_beside_a_staged_step")
    finally:
        obj.close()


SCORE_ROUTES = ({"score:KK_%d" % k for k in range(0, 17, 2)} | {"score:packed", "score:staged", "score:force_valu", "score:refused", "score:errors_only",
                "score:wide_ld", "score:descending", "score:deep_chains_beside_a_staged_step", "score:oracle_every_candidate", "score:lat_float32", "score:lat_float64"} |
                {"score:batch_%d" % n for n in (1, 16, 17, 64, 65)} | {"score:sets_%d" % c for c in (1, 2, 15, 16, 17)})


def orc_error(time_functions, clist, start):
    return wc.orc.time_constraints_error(time_functions, clist, start, wc.FRAME_TIME)


TIME_ROUTES = ({"time:KKg_%d" % k for k in range(2, 17, 2)} | {"time:chunks_%d" % c for c in (0, 1, 2, 3)} | {"time:gamma_memory", "time:gamma_registers"} |
               {"time:wave_doubles_chunk", "time:wave_doubles_mixture", "time:opt_in", "time:plain_lds", "time:refused"} |
               {"time:steps_%d" % m for m in (1, 2, 3, 4, 5, 8, 9)} | {"time:batch_%d" % n for n in (1, 15, 16, 17, 33)})


def test_the_ledger_covers_every_route():
    missing = (wc.FRAME_ROUTES | TIME_ROUTES | SCORE_ROUTES) - LEDGER
    assert not missing, "routes no row took and matched: %s" % sorted(missing)
