"""The keyframe scorers across every kernel route and shape edge: mg_score_kernel (VALU), mg_score_mfma_kernel (tile) and
mg_score_mfma64_kernel (wide) behind mg_score_constraints, mg_score_constraint_residuals[_chained] and mg_best_candidate, the argmin
and winner-copy kernels, and mg_constraint_set_update; rows of tests/score_shape_cases.py, CPU half tests/test_score_shapes_host.py.

Every row, for both latent dtypes and every batch size it lists:
  1. Primitive.score_plan (mg_score_plan) equals the restated route under every option the row is driven through -- a row that
     claims the wide kernel and is planned on the tile kernel FAILS here --, and the kernel goes into the ledger;
  2. every route gives the same bits: errors in float64, errors in float32 (= the float64 errors rounded once), the residual matrix;
     the residual rows sum to the errors within rtol 1e-13, atol 1e-12;
  3. the values against the oracle, at the bounds the suite already holds this scorer to (score_shape_cases.oracle_of);
  4. the device-pointer entry points write exactly their B (or B n) elements between 64 poisoned elements in front and behind; a
     refused call writes none;
  5. chained rows: with another alignment for every candidate, candidate b's residuals are the bits of the set updated to b's
     alignment and scored alone.
The last test asserts that the ledger holds every combination the CPU half says the table claims.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import score_shape_cases as sc
from morphablegraphs_amd import _capi
from oracle import c_oracle

pytestmark = pytest.mark.gpu

LEDGER = set()
GUARD = 64
POISON = -777.25


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def _reset(ctx):
    ctx.set_option(_capi.MG_OPT_SCORE_KERNEL, 0)
    ctx.set_option(_capi.MG_OPT_FORCE_VALU_SCORE, 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _guarded(ctx, bufs, count, dtype, call):
    """call(address) on `count` elements of dtype between GUARD poisoned ones: (status, the elements).  Asserts the guards hold and,
    after a launch, that every element in between was written."""
    host = np.full(count + 2 * GUARD, POISON, dtype=dtype)
    d = bufs.upload(host)
    status = _capi.MG_OK
    try:
        call(d.address + GUARD * host.itemsize)
    except _capi.MGError as e:
        status = e.status
    ctx.synchronize()
    got = ctx.download(d, host.shape, dtype)
    assert np.all(got[:GUARD] == POISON) and np.all(got[GUARD + count:] == POISON), "a write outside the output"
    return status, got[GUARD:GUARD + count]


def _score_all(ctx, prim, cset, X, B, ld, n, align_cand=None):
    """(status, errors float64, errors float32, residuals (B, n)) through the device-pointer entry points over poisoned buffers."""
    with ctx.buffers() as bufs:
        d_X = bufs.upload(X)
        d_A = bufs.upload(align_cand) if align_cand is not None else None
        s1, e64 = _guarded(ctx, bufs, B, np.float64, lambda at: prim.score_constraints_dev(cset, d_X, X.dtype, B, ld, at, np.float64))
        s2, e32 = _guarded(ctx, bufs, B, np.float32, lambda at: prim.score_constraints_dev(cset, d_X, X.dtype, B, ld, at, np.float32))
        s3, res = _guarded(ctx, bufs, B * n, np.float64, lambda at: prim.score_constraint_residuals_dev(cset, d_X, X.dtype, B, ld, at, d_A))
    assert s1 == s2 and (s1 == s3 or n == 0)
    return s1, e64, e32, res.reshape(B, n)


def _padded(S, B, dtype, ld_extra):
    """The first B latent rows as the dtype, NaN in ld_extra more columns."""
    X = np.full((B, S.shape[1] + ld_extra), np.nan, dtype=dtype)
    X[:, :S.shape[1]] = S[:B]
    return np.ascontiguousarray(X)


@pytest.mark.parametrize("name", sc.IDS)
def test_score_rows(ctx, name):
    row = sc.BY_NAME[name]
    n, L = len(row["cons"]), row["L"]
    _reset(ctx)
    prim = _capi.Primitive(ctx, sc.model(row))
    sk = _capi.Skeleton(*row["skel"]) if row["skel"] is not None else None
    if "refused:chain" in row["claims"]:
        try:
            with pytest.raises(_capi.MGError, match="chain of %d joints exceeds %d" % (sc.MG_MAX_CHAIN + 1, sc.MG_MAX_CHAIN)) as e:
                _capi.ConstraintSet(prim, row["cons"], sk)
            assert e.value.status == row["expect"] == sc.MG_ERR_INVALID_ARGUMENT
            LEDGER.add("refused:chain")
        finally:
            prim.close()
        return
    cset = _capi.ConstraintSet(prim, row["cons"], sk, alignment=sc.alignment_of(row))
    try:
        S = sc.latents(row)
        kind, ref, (rtol, atol) = sc.oracle_of(row, S)
        for dtype in (np.float32, np.float64):
            lat = np.dtype(dtype).name
            for B in row["batches"]:
                X = _padded(S, B, dtype, row["ld_extra"])
                seen = {}
                for label, opt, val in sc.routes_of(row):
                    _reset(ctx)
                    ctx.set_option(opt, val)
                    tag = "row %s %s B %d route %s" % (name, lat, B, label)
                    # 1. the plan
                    try:
                        want, want_status = sc.row_plan(row, B, label), _capi.MG_OK
                    except sc.Refused as e:
                        want, want_status, want_text = None, e.status, str(e)
                    if want is None:
                        with pytest.raises(_capi.MGError) as e:
                            prim.score_plan(cset, B)
                        assert e.value.status == want_status == row["expect"] and want_text in str(e.value), tag
                    else:
                        assert prim.score_plan(cset, B) == want, tag
                        if label == "wide":
                            assert want["kernel"] == "wide", tag
                    status, e64, e32, res = _score_all(ctx, prim, cset, X, B, X.shape[1], n)
                    assert status == want_status, tag
                    if want is None:                 # 4. a refused call writes nothing
                        assert np.all(e64 == POISON) and np.all(e32 == POISON) and np.all(res == POISON), tag
                        LEDGER.add("refused:lds")
                        continue
                    assert not np.any(e64 == POISON) and not np.any(e32 == POISON) and not np.any(res == POISON), tag + ": an element was not written"
                    assert np.array_equal(_bits(e32), _bits(e64.astype(np.float32))), tag
                    np.testing.assert_allclose(res.sum(axis=1) if n else np.zeros(B), e64, rtol=1e-13, atol=1e-12, err_msg=tag)
                    seen[label] = (want, e64, e32, res)
                    LEDGER.update({(want["kernel"], lat, o) for o in ("out_f64", "out_f32", "res")})
                    if want["lds_opt_in"]:
                        LEDGER.add(want["kernel"] + ":opt_in")
                    if label == "tile" and want["kernel"] == "valu" and n > 0 and L <= 64:
                        LEDGER.add("valu:fallthrough")
                _reset(ctx)
                if not seen:
                    continue
                # 2. every route the same bits
                first = next(iter(seen))
                for label, (_, e64, e32, res) in seen.items():
                    for a, b in zip((e64, e32, res), seen[first][1:]):
                        assert np.array_equal(_bits(a), _bits(b)), "row %s %s B %d: %s against %s" % (name, lat, B, label, first)
                # 3. the oracle
                _, e64, _, res = seen[first]
                got = e64 if kind == "errors" else res
                worst = float(np.max(np.abs(got - ref[:B]) / (atol + rtol * np.abs(ref[:B])))) if atol else float(np.max(np.abs(got - ref[:B])))
                print("row %s %s B %d: worst |device - oracle| / bound %.3g" % (name, lat, B, worst))
                np.testing.assert_allclose(got, ref[:B], rtol=rtol, atol=atol, err_msg="row %s %s B %d" % (name, lat, B))
    finally:
        _reset(ctx)
        cset.close()
        prim.close()


@pytest.mark.parametrize("name", [r["name"] for r in sc.ROWS if r["chained"]])
def test_chained_rows_are_the_updated_set_scored_alone(ctx, name):
    """5. align_cand differs for every candidate; candidate b under every kernel = the set updated to b's alignment, candidate b alone."""
    row = sc.BY_NAME[name]
    n = len(row["cons"])
    _reset(ctx)
    prim = _capi.Primitive(ctx, sc.model(row))
    sk = _capi.Skeleton(*row["skel"])
    base = sc.alignment_of(row)
    cset, single = _capi.ConstraintSet(prim, row["cons"], sk, alignment=base), _capi.ConstraintSet(prim, row["cons"], sk, alignment=base)
    try:
        S = sc.latents(row)
        for dtype in (np.float32, np.float64):
            lat = np.dtype(dtype).name
            for B in row["batches"]:
                X, A = _padded(S, B, dtype, 0), sc.align_cand_of(row, B)
                alone = np.empty((B, n))
                for b in range(B):
                    single.update(row["cons"], alignment=dict(base, heading=[A[b, 0], A[b, 1]], position=[A[b, 2], base["position"][1], A[b, 3]]))
                    alone[b] = prim.score_constraint_residuals(single, X[b:b + 1])[0]
                assert len({tuple(r) for r in alone}) == B                   # the alignments matter
                for label, opt, val in sc.routes_of(row):
                    _reset(ctx)
                    ctx.set_option(opt, val)
                    want = sc.row_plan(row, B, label)
                    assert prim.score_plan(cset, B) == want
                    with ctx.buffers() as bufs:
                        d_X, d_A = bufs.upload(X), bufs.upload(A)
                        status, res = _guarded(ctx, bufs, B * n, np.float64, lambda at: prim.score_constraint_residuals_dev(cset, d_X, X.dtype, B, X.shape[1], at, d_A))
                    assert status == _capi.MG_OK and np.array_equal(_bits(res.reshape(B, n)), _bits(alone)), "row %s %s B %d route %s" % (name, lat, B, label)
                    LEDGER.add((want["kernel"], lat, "res_align_cand"))
    finally:
        _reset(ctx)
        cset.close()
        single.close()
        prim.close()


def test_the_automatic_switch(ctx):
    """Option 0: 49 151 candidates take the tile kernel, 49 152 the wide one; the two kernels bit for bit on the whole batch, and the
    whole batch against the C oracle."""
    row = sc.AUTO_ROW
    _reset(ctx)
    prim = _capi.Primitive(ctx, sc.model(row))
    cset = _capi.ConstraintSet(prim, row["cons"])
    try:
        S = sc.auto_latents(sc.AUTO_B[1])
        ref = c_oracle.COraclePrimitive(sc.model(row)).keyframe_errors_f64(S, sc.root_cons_matrix(row["cons"]))
        for dtype in (np.float32, np.float64):
            X = S.astype(dtype)
            got = {}
            for B, kernel in zip(sc.AUTO_B, ("tile", "wide")):
                plan = prim.score_plan(cset, B)
                assert plan == sc.row_plan(row, B, "auto") and plan["kernel"] == kernel
                status, e64, e32, res = _score_all(ctx, prim, cset, np.ascontiguousarray(X[:B]), B, 8, 2)
                assert status == _capi.MG_OK and np.array_equal(_bits(e32), _bits(e64.astype(np.float32)))
                np.testing.assert_allclose(res.sum(axis=1), e64, rtol=1e-13, atol=1e-12)
                np.testing.assert_allclose(e64, ref[:B], rtol=1e-10, atol=1e-9)
                got[kernel] = (e64, e32, res)
                LEDGER.add("auto:" + kernel)
            ctx.set_option(_capi.MG_OPT_SCORE_KERNEL, 1)                     # the other kernel on the larger batch
            assert prim.score_plan(cset, sc.AUTO_B[1])["kernel"] == "tile"
            _, e64, e32, res = _score_all(ctx, prim, cset, X, sc.AUTO_B[1], 8, 2)
            _reset(ctx)
            for a, b in zip((e64, e32, res), got["wide"]):
                assert np.array_equal(_bits(a), _bits(b))
            for a, b in zip(got["tile"], got["wide"]):
                assert np.array_equal(_bits(a), _bits(b[:sc.AUTO_B[0]]))
    finally:
        _reset(ctx)
        cset.close()
        prim.close()


@pytest.mark.parametrize("n", (sc.UPDATE_N, sc.UPDATE_N + 1))
def test_an_updated_set_scores_like_a_fresh_one(ctx, n):
    """mg_constraint_set_update with the values as kernel arguments (n_par + n_align <= 496 doubles: 62 constraints) and one constraint
    more, through the synchronised copies: the scores of the updated set are the bits of a set created with the new values."""
    row = sc.BY_NAME["tile_lds_n%d" % sc.TILE_150K_N]
    _reset(ctx)
    prim = _capi.Primitive(ctx, sc.model(row))
    old = row["cons"][:n]
    new = [dict(c, weight=c["weight"] + 0.25, target=[None if v is None else v * 1.5 - 3.0 for v in c["target"]]) for c in old]
    assert n * 8 <= sc.MG_SET_PARAMS_MAX if n == sc.UPDATE_N else n * 8 > sc.MG_SET_PARAMS_MAX
    updated, fresh = _capi.ConstraintSet(prim, old), _capi.ConstraintSet(prim, new)
    try:
        S = sc.latents(row)
        before = prim.score_constraint_residuals(updated, S)
        updated.update(new)
        a, b = prim.score_constraint_residuals(updated, S), prim.score_constraint_residuals(fresh, S)
        assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(before))
        assert np.array_equal(_bits(prim.score_constraints(updated, S)), _bits(prim.score_constraints(fresh, S)))
        np.testing.assert_allclose(prim.score_constraints(updated, S), c_oracle.COraclePrimitive(sc.model(row)).keyframe_errors_f64(S, sc.root_cons_matrix(new)),
                                   rtol=1e-10, atol=1e-9)
        LEDGER.add("update:kernel_arguments" if n == sc.UPDATE_N else "update:copies")
    finally:
        updated.close()
        fresh.close()
        prim.close()


# ---- argmin and the winner copy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_argmin_first_cases(ctx, dtype):
    for name, (v, _) in sc.ARGMIN_CASES.items():
        vals = v.astype(dtype)
        want_i, want_m = c_oracle.first_min_argmin(vals)
        with ctx.buffers() as bufs:
            d_v, d_o = bufs.upload(vals), bufs.upload(np.full(2 + 2 * GUARD, POISON))
            got_i, got_m = ctx.argmin_first(d_v, len(vals), dtype)
            _capi._check(ctx.lib.mg_argmin_first_dev(ctx.handle, d_v.ptr, _capi.MG_F64 if dtype == np.float64 else _capi.MG_F32, len(vals),
                                                     _capi.C.c_void_p(d_o.address + 8 * GUARD)))
            ctx.synchronize()
            out = ctx.download(d_o, (2 + 2 * GUARD,), np.float64)
        assert (got_i, got_m) == (want_i, want_m) or (got_i == want_i and np.isinf(got_m) and np.isinf(want_m)), (name, got_i, got_m, want_i, want_m)
        assert int(out[GUARD:GUARD + 1].view(np.int64)[0]) == want_i and out[GUARD + 1] == want_m, name
        assert np.all(out[:GUARD] == POISON) and np.all(out[GUARD + 2:] == POISON), name
    LEDGER.add("argmin:" + np.dtype(dtype).name)


def test_best_candidate_on_the_empty_set_and_on_a_tie(ctx):
    _reset(ctx)
    for name in ("n0", "wide14", "L65"):
        row = sc.BY_NAME[name]
        prim = _capi.Primitive(ctx, sc.model(row))
        cset = _capi.ConstraintSet(prim, row["cons"])
        try:
            S = sc.latents(row, 65)
            if name == "n0":                             # every error 0.0: the first candidate
                assert prim.best_candidate(cset, S) == (0, 0.0)
                continue
            err = prim.score_constraints(cset, S)
            assert prim.best_candidate(cset, S) == c_oracle.first_min_argmin(err)
            best = int(np.argmin(err))
            T = S.copy()                                 # the tie row: the best candidate twice, the later copy further on or in front
            other = 64 if best < 64 else 3
            T[other] = S[best]
            with ctx.buffers() as bufs:
                got = prim.best_candidate_dev(cset, bufs.upload(T), np.float64, 65, T.shape[1])
            assert got == (min(best, other), float(err[best])) == c_oracle.first_min_argmin(prim.score_constraints(cset, T))
        finally:
            cset.close()
            prim.close()
    LEDGER.add("best_candidate")


@pytest.mark.parametrize("L", sc.WINNER_WIDTHS)
def test_the_winner_row_is_copied(ctx, L):
    """mg_option_step: the argmin and the winner's latent row (L = 1, 64, 65 columns) in one record, through mg_argmin_gather_kernel."""
    data = sc.synthetic.make_primitive(seed=6000 + L, n_components=L, n_frames=sc.F, n_basis=sc.NB, n_dim=7, n_gmm=2, name="winner%d" % L)
    prim = _capi.Primitive(ctx, data)
    cset = _capi.ConstraintSet(prim, [sc._pos(0, sc.TL), sc._dir(0, sc.TL)])
    n, ld = 1025, L + 2
    try:
        counts = np.array([600, 425], dtype=np.int64)
        with ctx.buffers() as bufs:
            d_x, d_e = bufs.upload(np.full((n, ld), POISON)), bufs.upload(np.full(n, POISON))
            d_r = bufs.upload(np.full(2 + L + GUARD, POISON))
            _capi._check(ctx.lib.mg_option_step(prim.handle, cset.handle, n, counts.ctypes.data_as(_capi.C.c_void_p), _capi.C.c_uint64(77), d_x.ptr, _capi.MG_F64, ld,
                                                d_e.ptr, d_r.ptr))
            ctx.synchronize()
            X, err, rec = ctx.download(d_x, (n, ld), np.float64), ctx.download(d_e, (n,), np.float64), ctx.download(d_r, (2 + L + GUARD,), np.float64)
        want_i, want_m = c_oracle.first_min_argmin(err)
        assert int(rec[:1].view(np.int64)[0]) == want_i and rec[1] == want_m
        assert np.array_equal(_bits(rec[2:2 + L]), _bits(X[want_i, :L])) and np.all(rec[2 + L:] == POISON)
        assert np.array_equal(_bits(err), _bits(prim.score_constraints(cset, np.ascontiguousarray(X[:, :L]))))
        LEDGER.add("winner:L%d" % L)
    finally:
        cset.close()
        prim.close()


def test_the_ledger_covers_every_claim():
    claimed = set().union(*[sc.claimed_combos(r) for r in sc.ROWS])
    want = claimed | sc.SPECIALS | {"update:kernel_arguments", "update:copies", "argmin:float32", "argmin:float64", "best_candidate"}
    want |= {"winner:L%d" % L for L in sc.WINNER_WIDTHS}
    assert claimed == sc.COMBOS
    missing = want - LEDGER
    assert not missing, "routes no row took and matched: %s" % sorted(map(str, missing))
