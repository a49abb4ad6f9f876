"""The mixed-population walk kernels across their shape edges: mg_walks_chain_kernel / mg_walks_frames_kernel, plain and WARPED
(MIXED_FRAME_ROWS), mg_walks_time_kernel, plain and SMOOTH (MIXED_TIME_ROWS), and mg_walks_sample_kernel (MIXED_SAMPLE_ROWS) of
tests/walks_mixed_shape_cases.py; the CPU half is tests/test_walks_mixed_shapes_host.py.

Every call's outputs lie over a sentinel -- frames over NaN with GUARD_ROWS more rows per walk than the walk needs, transforms, times,
lengths and components over fixed odd values -- and the library's status is compared with the restated plan first: a refusal where the
plan claims a launch fails the row, and a refused call leaves every output untouched.

Frame rows: every walk has the bits of graph_walk.walk_frames_dev for that walk alone (its latents packed, its own times for a warped
row), frames and transforms; at n_dim >= 7 both are also within tests/test_graph_walk_host.py's WALK_TOLERANCE of the walk's largest
|root coordinate| of random_walks.assemble_walks_mixed_host, which the CPU half holds to the oracle on the same rows; below 7 the frames
are mg_back_project_frames_f64's bits and the transforms the identity; what no step owns keeps its sentinel.
Time rows: the lengths are the host rule's; a timed step has the bits of the single-primitive call (mg_time_function_sample, or
mg_time_function_sample_smoothed for a flagged node) and, unsmoothed, lies within timewarp_cases' tolerance of the 50-digit twin; an
untimed step has numpy.linspace's bits; a flagged row below the window reports its length and is not written; a row that does not fit
reports -T and is not written; a step behind a walk's end has length 0.
Sample rows: the components are random_walk_cases.walk_components', every drawn row has the bits of Primitive.gmm_sample_dev for its
component and global row index, everything behind a node's width and behind a walk's end is 0, float32 is the rounded float64, a
NULL component pointer changes nothing else.
LEDGER collects the routes of the rows that ran and matched; test_the_ledger_covers_every_route fails when one of MIXED_ROUTES is missing.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
import walks_mixed_shape_cases as mc
from morphablegraphs_amd import _capi
from morphablegraphs_amd import graph_walk as gw
from morphablegraphs_amd import random_walks as rw
from morphablegraphs_amd.time_smoothing import WINDOW, smooth_time_row_host
from test_gpu_time_smoothing import sample as smoothed_sample
from test_gpu_timewarp_shapes import sample as plain_sample
from test_graph_walk_host import WALK_TOLERANCE, root_scale

pytestmark = pytest.mark.gpu

LEDGER = set()
X_FILL = -777.25                        # what the transforms hold before the call
T_FILL = -7777.25                       # ... the times
L_FILL, C_FILL = 77, 79                 # ... the lengths and the components
HOST_TWINS = ("D11_previous", "warped_pitches")     # the rows that also go through the _host entry points


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _padded(lists, shape, dtype, fill=0):
    out = np.full(shape, fill, dtype=dtype)
    for w, row in enumerate(lists):
        out[w, :len(row)] = row
    return out


def _arrays(row, layout):
    """(node_of, n_steps, lengths int32 or None, times (n, s_max, t_cap) or None, t_cap, frame offsets int64 or None, stride)."""
    node_of, n_steps = mc.frame_tables(row)
    lengths, times, offsets, stride = layout
    fo = None if offsets is None else _padded(offsets, node_of.shape, np.int64)
    if lengths is None:
        return node_of, n_steps, None, None, 0, fo, stride
    ln = _padded(lengths, node_of.shape, np.int32)
    t_cap = int(ln.max())
    tm = np.zeros(node_of.shape + (t_cap,))
    for w, rows in enumerate(times):
        for i, t in enumerate(rows):
            tm[w, i, :len(t)] = t
    return node_of, n_steps, ln, tm, t_cap, fo, stride


def _mixed(ctx, prims, row, P, alignment, skeleton, layout, host=False):
    """One mg_walks_frames / mg_walks_frames_at call: (status, frames (n, stride, D) over NaN, transforms (n, s_max, 4) over X_FILL)."""
    node_of, n_steps, ln, tm, t_cap, fo, stride = _arrays(row, layout)
    n, s_max = node_of.shape
    frames, x = np.full((n, stride, row["D"]), np.nan), np.full((n, s_max, 4), X_FILL)
    status = _capi.MG_OK
    if host:
        if ln is None:
            rw.walks_frames_host(prims, node_of, n_steps, P, frames, fo, alignment, skeleton, x)
        else:
            rw.walks_frames_at_host(prims, node_of, n_steps, P, tm, ln, fo, frames, alignment, skeleton, x)
        return status, frames, x
    with ctx.buffers() as bufs:
        d_P, d_f, d_x = bufs.upload(P), bufs.upload(frames), bufs.upload(x)
        try:
            if ln is None:
                rw.walks_frames_dev(prims, node_of, n_steps, d_P, P.dtype, P.shape[2], d_f, stride, fo, alignment, skeleton, d_x)
            else:
                rw.walks_frames_at_dev(prims, node_of, n_steps, d_P, P.dtype, P.shape[2], bufs.upload(tm), ln, t_cap, fo, d_f, stride, alignment, skeleton, d_x)
        except _capi.MGError as e:
            status = e.status
        ctx.synchronize()
        return status, ctx.download(d_f, frames.shape, np.float64), ctx.download(d_x, x.shape, np.float64)


def _solo(ctx, prims, row, P, w, alignment, skeleton, layout):
    """mg_walk_frames for walk w alone, at the walk's own offsets and times: (frames (stride, D) over NaN, transforms (n_steps, 4))."""
    _, _, ln, tm, t_cap, fo, stride = _arrays(row, layout)
    seq = row["walks"][w]
    m = len(seq)
    widths = [row["shapes"][k][0] for k in seq]
    S = mc.walk_latents(row, P, w)[None, :].astype(P.dtype)
    with ctx.buffers() as bufs:
        d_f, d_x = bufs.upload(np.full((stride, row["D"]), np.nan)), bufs.upload(np.full((m, 4), X_FILL))
        gw.walk_frames_dev([prims[k] for k in seq], np.concatenate(([0], np.cumsum(widths)[:-1])), bufs.upload(S), P.dtype, 1, S.shape[1], d_f, stride,
                           None if tm is None else bufs.upload(np.ascontiguousarray(tm[w, :m])), None if ln is None else ln[w:w + 1, :m], t_cap,
                           None if fo is None else fo[w:w + 1, :m], alignment, skeleton, d_x)
        ctx.synchronize()
        return ctx.download(d_f, (stride, row["D"]), np.float64), ctx.download(d_x, (m, 4), np.float64)


def _no_walks(ctx, prims):
    """Every entry point with 0 walks and NULL pointers: accepted, nothing to write."""
    lib, handles = prims[0].lib, rw._handles(prims)
    n = len(prims)
    assert lib.mg_walks_frames(n, handles, None, None, None, _capi.MG_F64, 0, 1, 8, None, None, None, None, 1, None) == _capi.MG_OK
    assert lib.mg_walks_frames_at(n, handles, None, None, None, _capi.MG_F64, 0, 1, 8, None, None, 1, None, None, None, None, 1, None) == _capi.MG_OK
    assert lib.mg_walks_time_functions(n, handles, None, None, None, _capi.MG_F64, 0, 1, 8, 1.0, None, None, 1) == _capi.MG_OK
    assert lib.mg_walks_sample_latents(n, handles, None, None, 0, 1, C.c_uint64(5), None, _capi.MG_F64, 8, None) == _capi.MG_OK
    ctx.synchronize()


@pytest.mark.parametrize("name", mc.FRAME_IDS)
def test_walk_frame_rows(ctx, name):
    row = mc.FRAME_BY_NAME[name]
    models = mc.frame_models(row)
    prims = [_capi.Primitive(ctx, m) for m in models]
    try:
        _, P64, alignment, hip_sk, _, _ = mc.frame_case(row, models)
        P = P64.astype(row["dtype"])
        assert np.array_equal(P.astype(np.float64), P64)
        layout = mc.frame_layout(row)
        try:
            plan, want_status = mc.frame_plan(row), _capi.MG_OK
        except mc.Refused as e:
            plan, want_status = None, e.status
        assert want_status == (row["expect"] if row["expect"] is not None else _capi.MG_OK)
        if not row["walks"]:
            assert not plan["launched"]
            _no_walks(ctx, prims)
            LEDGER.update(row["routes"])
            return
        status, got, got_x = _mixed(ctx, prims, row, P, alignment, hip_sk, layout)
        assert status == want_status, "row %s: the library answers %d, the restated plan %d" % (name, status, want_status)
        if plan is None:
            assert np.isnan(got).all() and np.all(got_x == X_FILL), "a refused call wrote to its outputs"
            LEDGER.update(row["routes"])
            return
        node_of, n_steps, ln, tm, _, fo, stride = _arrays(row, layout)
        assert stride == plan["walk_stride"] and plan["tiles"] == len(plan["per_tile"])
        # 1. every walk is its solo call, bit for bit; what no step owns keeps the sentinel
        for w, seq in enumerate(row["walks"]):
            fr, tr = _solo(ctx, prims, row, P, w, alignment, hip_sk, layout)
            assert _same(got[w], fr), "row %s, walk %d: the frames are not the solo call's" % (name, w)
            assert _same(got_x[w, :len(seq)], tr) and np.all(got_x[w, len(seq):] == X_FILL), "row %s, walk %d: transforms" % (name, w)
            owned = np.zeros(stride, dtype=bool)
            for i, k in enumerate(seq):
                owned[plan["offsets"][w][i]:plan["offsets"][w][i] + (ln[w, i] if ln is not None else row["shapes"][k][1])] = True
            assert np.isnan(got[w, ~owned]).all() and not np.isnan(got[w, owned]).any() and (~owned).sum() >= mc.GUARD_ROWS, (name, w)
        # 2. the statement
        if row["D"] < 7:
            for w, seq in enumerate(row["walks"]):
                L, F, _ = row["shapes"][seq[0]]
                assert _same(got[w, :F], prims[seq[0]].back_project_frames_f64(np.ascontiguousarray(P[w, 0, :L][None]))[0]), (name, w)
                assert np.array_equal(got_x[w, 0], [1.0, 0.0, 0.0, 0.0])
        else:
            frames, offsets, ref_x = rw.assemble_walks_mixed_host(models, node_of, n_steps, P64, alignment, hip_sk, times=layout[1])
            ref = mc.place_walks(frames, offsets, row, plan["offsets"] if fo is not None else None, stride)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), "the sentinel around the walks, or a row of a walk"
            bound = row["bound"] if row["bound"] is not None else WALK_TOLERANCE
            worst = worst_x = 0.0
            for w, seq in enumerate(row["walks"]):
                scale = root_scale(ref[w])
                worst = max(worst, float(np.nanmax(np.abs(got[w] - ref[w]))) / scale)
                worst_x = max(worst_x, float(np.max(np.abs(got_x[w, :len(seq)] - ref_x[w, :len(seq)]))) / scale)
            print("row %s: frames %.3g, transforms %.3g of the walk's root scale (bound %.3g)" % (name, worst, worst_x, bound))
            assert worst <= bound and worst_x <= bound
        # 3. the _host entry points give the device's bits
        if name in HOST_TWINS:
            _, host_f, host_x = _mixed(ctx, prims, row, P, alignment, hip_sk, layout, host=True)
            assert _same(host_f, got) and _same(host_x, got_x)
            LEDGER.add("host:frames_at" if row["warped"] else "host:frames")
        assert row["routes"] & mc.DERIVED <= mc.frame_routes(row, plan)
        LEDGER.update(row["routes"])
    finally:
        for p in prims:
            p.close()


# ---- mg_walks_time_kernel -------------------------------------------------------------------------------------------------------------
class _AsPrimitive(object):
    """What test_gpu_timewarp_shapes.sample reads of a HipMotionPrimitive."""

    def __init__(self, prim, F):
        self._prim, self.n_canonical_frames = prim, F


class _AsWorld(object):
    """What test_gpu_time_smoothing.sample reads of its world."""

    def __init__(self, ctx, prim):
        self.ctx, self.prims = ctx, [prim]


def _time_call(ctx, prims, row, node_of, n_steps, P, speed, t_cap):
    with ctx.buffers() as bufs:
        d_t, d_l = bufs.upload(np.full(node_of.shape + (t_cap,), T_FILL)), bufs.upload(np.full(node_of.shape, L_FILL, dtype=np.int32))
        status = _capi.MG_OK
        try:
            if row["smooth"]:
                rw.walks_time_functions_smoothed_dev(prims, node_of, n_steps, [nd in row["smooth"] for nd in row["nodes"]], bufs.upload(P), P.dtype, P.shape[2],
                                                     speed, d_t, d_l, t_cap)
            else:
                rw.walks_time_functions_dev(prims, node_of, n_steps, bufs.upload(P), P.dtype, P.shape[2], speed, d_t, d_l, t_cap)
        except _capi.MGError as e:
            status = e.status
        ctx.synchronize()
        return status, ctx.download(d_t, node_of.shape + (t_cap,), np.float64), ctx.download(d_l, node_of.shape, np.int32)


@pytest.mark.parametrize("name", mc.TIME_IDS)
def test_walk_time_rows(ctx, name):
    row = mc.TIME_BY_NAME[name]
    jsons, shapes, P, speed = mc.time_case(row)
    prims = [_capi.Primitive(ctx, j) for j in jsons]
    try:
        node_of, n_steps = rc.tables(row["walks"])
        want = mc.time_reference(name) if row["expect"] is None else {}
        longest = max(len(ref["row"]) for ref in want.values()) if want else 8
        t_cap = longest - 1 if row["short"] else longest
        try:
            plan, want_status = mc.time_plan(row, t_cap, speed), _capi.MG_OK
        except mc.Refused as e:
            plan, want_status = None, e.status
        assert want_status == (row["expect"] if row["expect"] is not None else _capi.MG_OK)
        status, times, lens = _time_call(ctx, prims, row, node_of, n_steps, P, speed, t_cap)
        assert status == want_status, "row %s: the library answers %d, the restated plan %d" % (name, status, want_status)
        if plan is None:
            assert np.all(times == T_FILL) and np.all(lens == L_FILL), "a refused call wrote to its outputs"
            LEDGER.update(mc.time_routes(row))
            return
        worst, too_long, below_window = 0.0, 0, 0
        for w in range(node_of.shape[0]):
            for i in range(node_of.shape[1]):
                if i >= n_steps[w]:
                    assert lens[w, i] == 0 and np.all(times[w, i] == T_FILL), (w, i)      # a step behind the walk's end
                    continue
                ref, k = want[(w, i)], node_of[w, i]
                T = len(ref["row"])
                if T > t_cap:
                    assert lens[w, i] == -T and np.all(times[w, i] == T_FILL), (w, i)
                    too_long += 1
                    continue
                assert lens[w, i] == T, "row %s, step %s: %d samples, the host rule gives %d" % (name, (w, i), lens[w, i], T)
                assert np.all(times[w, i, T:] == T_FILL), (w, i)
                if not ref["timed"]:
                    assert plan["counts"][k] == T and _same(times[w, i, :T], ref["row"]), (w, i)
                    continue
                F, L, Lt = shapes[k]
                G = np.ascontiguousarray(P[w, i, L:L + Lt][None])
                if row["smooth"] and row["nodes"][k] in row["smooth"]:
                    solo_t, solo_l = smoothed_sample(_AsWorld(ctx, prims[k]), G, speed, t_cap, smoothed=True)
                    assert solo_l[0] == T
                    if T >= WINDOW:
                        plain_t, _ = plain_sample(_AsPrimitive(prims[k], F), G, speed, t_cap)
                        assert _same(times[w, i, :T], solo_t[0, :T]) and _same(times[w, i, :T], smooth_time_row_host(plain_t[0, :T])), (w, i)
                    else:                      # no smoothed form: the length is reported, the row is not written (the single-primitive call's rule)
                        assert np.isnan(solo_t[0]).all() and np.all(times[w, i] == T_FILL), (w, i)
                        below_window += 1
                    continue
                solo_t, solo_l = plain_sample(_AsPrimitive(prims[k], F), G, speed, t_cap)
                assert solo_l[0] == T and _same(times[w, i, :T], solo_t[0, :T]), "row %s, step %s: not the single-primitive call's bits" % (name, (w, i))
                deviation = float(np.max(np.abs(times[w, i, :T] - ref["twin"])))
                worst = max(worst, deviation / ref["tol"])
                assert deviation <= ref["tol"], (name, (w, i), deviation, ref["tol"])
        print("row %s: worst |device - twin| / tolerance %.3g; %d rows too long, %d below the window" % (name, worst, too_long, below_window))
        if row["short"]:
            assert 0 < too_long < int(n_steps.sum())
        else:
            assert too_long == 0 and int(np.max(lens)) == t_cap          # t_cap equal to the longest row: it is written
        if row["sized"] is not None:
            assert lens[0, 0] == row["sized"] and (below_window > 0) == (row["sized"] < WINDOW)
        LEDGER.update(mc.time_routes(row))
    finally:
        for p in prims:
            p.close()


# ---- mg_walks_sample_kernel -----------------------------------------------------------------------------------------------------------
def _sample_call(ctx, prims, node_of, n_steps, seed, dtype, ld, with_comp):
    with ctx.buffers() as bufs:
        d_x = bufs.upload(np.full(node_of.shape + (ld,), T_FILL, dtype=dtype))
        d_c = bufs.upload(np.full(node_of.shape, C_FILL, dtype=np.int32))
        status = _capi.MG_OK
        try:
            rw.sample_walk_latents_dev(prims, node_of, n_steps, seed, d_x, dtype, ld, d_c if with_comp else None)
        except _capi.MGError as e:
            status = e.status
        ctx.synchronize()
        return status, ctx.download(d_x, node_of.shape + (ld,), dtype), ctx.download(d_c, node_of.shape, np.int32)


@pytest.mark.parametrize("name", mc.SAMPLE_IDS)
def test_walk_sample_rows(ctx, name):
    mixtures, walks, ld, seed = mc.MIXED_SAMPLE_ROWS[name]
    jsons = [mc.sample_model(K, Lg) for K, Lg in mixtures]
    prims = [_capi.Primitive(ctx, j) for j in jsons]
    try:
        node_of, n_steps = rc.tables(walks)
        n, s_max = node_of.shape
        try:
            plan, want_status = mc.sample_plan(name), _capi.MG_OK
        except mc.Refused as e:
            plan, want_status = None, e.status
        assert want_status == mc.SAMPLE_REFUSED.get(name, _capi.MG_OK)
        status, x, comp = _sample_call(ctx, prims, node_of, n_steps, seed, np.float64, ld, True)
        assert status == want_status, "row %s: the library answers %d, the restated plan %d" % (name, status, want_status)
        if plan is None:
            assert np.all(x == T_FILL) and np.all(comp == C_FILL), "a refused call wrote to its outputs"
            status32, x32, comp32 = _sample_call(ctx, prims, node_of, n_steps, seed, np.float32, ld, True)
            assert status32 == want_status and np.all(x32 == np.float32(T_FILL)) and np.all(comp32 == C_FILL)
            LEDGER.update(mc.sample_routes(name))
            return
        assert plan["rows"] == n * s_max
        assert np.array_equal(comp, rc.walk_components([j["gmm_weights"] for j in jsons], node_of, n_steps, seed))
        for w in range(n):
            for i in range(s_max):
                if i >= n_steps[w]:
                    assert np.all(x[w, i] == 0.0) and comp[w, i] == -1, (w, i)
                    continue
                prim = prims[node_of[w, i]]
                K, Lg = mixtures[node_of[w, i]]
                counts = np.zeros(K, dtype=np.int64)
                counts[comp[w, i]] = n * s_max                            # all rows of the draw in the row's component
                with ctx.buffers() as bufs:
                    d_row = bufs.malloc(8 * Lg)
                    prim.gmm_sample_dev(counts, seed, d_row, np.float64, Lg, rows=(w * s_max + i, 1))
                    want = ctx.download(d_row, (Lg,), np.float64)
                assert _same(x[w, i, :Lg], want), "row %s, step %s: not the sampler's bits" % (name, (w, i))
                assert np.all(x[w, i, Lg:] == 0.0), (w, i)
        status32, x32, comp32 = _sample_call(ctx, prims, node_of, n_steps, seed, np.float32, ld, True)
        assert status32 == _capi.MG_OK and _same(x32, x.astype(np.float32)) and np.array_equal(comp32, comp)
        _, x_null, comp_null = _sample_call(ctx, prims, node_of, n_steps, seed, np.float64, ld, False)
        assert _same(x_null, x) and np.all(comp_null == C_FILL)
        LEDGER.update(mc.sample_routes(name))
    finally:
        for p in prims:
            p.close()


def test_the_ledger_covers_every_route():
    missing = (mc.MIXED_ROUTES | {"host:frames", "host:frames_at"}) - LEDGER
    assert not missing, "routes no row took and matched: %s" % sorted(missing)
