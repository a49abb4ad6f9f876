"""mg_step_length_kernel across its shape edges: the rows of tests/step_length_cases.py on the device; the CPU half is
tests/test_step_length_shapes_host.py, which holds the reference used here to the reference project's own frames.

Every row that launches:
  * against reference_step_lengths (extended precision, nothing of the library), under the bounds tests/test_gpu_step_lengths.py holds
    the kernel to against reference frames: (F - 1) 2 sqrt(2) 4e-12 scale for the arc length, 2 sqrt(3) 4e-12 scale for the distance;
    the largest ratio to the bound is printed per row and, by the last test, for the table;
  * bit for bit: float32 latents against their float64 values, the device-pointer entry point against the host-pointer one (between
    guard words), a second call, each method alone against "both";
  * the analytic rows: arc length = distance within _device_bound for every candidate.
The refused row gets MG_ERR_UNSUPPORTED from both entry points before anything is launched or written, and the context goes on.
The tables: five items over three models (16, 1, 0, 17, 15 candidates) and the item over 64 KiB beside a tiny one in both orders and
both latent dtypes, on the module's context and as the first call of a fresh one; every item gives the bits it gives alone.

Observed on an MI355X: the largest ratio to the bound over the table 1.71e-05 (arc length, row F2_NB4) and 7.45e-05 (distance, row
L64); the analytic rows' |arc length - distance| 3.6e-15 (F = 13, bound 1.95e-12) and 6.8e-13 (F = 257, bound 6.86e-11).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_length_cases as sc
from morphablegraphs_amd import _capi

pytestmark = pytest.mark.gpu

LEDGER = set()
WORST = {"arc": (0.0, None), "dist": (0.0, None)}
GUARD = -4242.5
_REFERENCE = {}


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def _reference(name):
    """(arc, dist, scale) of a row's model over its 2 TILE + 1 latents: computed once, read by every test that needs a prefix."""
    if name not in _REFERENCE:
        r = sc.BY_NAME[name]
        out = sc.reference_step_lengths(sc.model_of(r), sc.latents_of(r, 2 * sc.TILE + 1), with_scale=True)
        for a in out[:2]:
            a.setflags(write=False)
        _REFERENCE[name] = out
    return _REFERENCE[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _device_call(ctx, prim, S):
    """mg_step_lengths on device pointers: (status, the output block (2, n + 2): arc and distance, a guard word on either side)."""
    n = len(S)
    with ctx.buffers() as bufs:
        d_S, d_o = bufs.upload(S), bufs.upload(np.full((2, n + 2), GUARD))
        table = (_capi.StepLengthItem * 1)()
        rec = table[0]
        rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = prim.handle.value, d_S.address, 0, n, S.shape[1]
        rec.arc_length, rec.distance = d_o.address + 8, d_o.address + 8 * (n + 2) + 8
        status = _capi.MG_OK
        try:
            _capi.step_lengths_table(prim.lib, 1, table, S.dtype, host=False)
        except _capi.MGError as e:
            status = e.status
        ctx.synchronize()
        return status, ctx.download(d_o, (2, n + 2), np.float64)


@pytest.mark.parametrize("name", sc.IDS)
def test_step_length_rows(ctx, name):
    r = sc.BY_NAME[name]
    S = sc.latents_of(r)
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S) and len(S) == r["n"]
    prim = _capi.Primitive(ctx, sc.model_of(r))
    try:
        if r["expect"] is not None:
            # refused by the host-pointer form with nothing written, by the device-pointer form with nothing launched
            table = (_capi.StepLengthItem * 1)()
            arc, dist = np.full(len(S), GUARD), np.full(len(S), GUARD)
            rec = table[0]
            rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = prim.handle.value, S.ctypes.data, 0, len(S), S.shape[1]
            rec.arc_length, rec.distance = arc.ctypes.data, dist.ctypes.data
            with pytest.raises(_capi.MGError) as e:
                _capi.step_lengths_table(prim.lib, 1, table, np.float64)
            assert e.value.status == r["expect"] and "LDS" in str(e.value)
            assert np.all(arc == GUARD) and np.all(dist == GUARD)
            status, block = _device_call(ctx, prim, S)
            assert status == r["expect"] and np.all(block == GUARD), "a refused call wrote to its outputs"
            # ... and the context goes on: the same shape one frame shorter, on the same context
            fits = sc.BY_NAME["lds_at_max"]
            other = _capi.Primitive(ctx, sc.model_of(fits))
            try:
                got = other.step_lengths(sc.latents_of(fits, 2), "both")
                want = _reference("lds_at_max")
                assert np.abs(got[0] - want[0][:2]).max() <= sc.arc_bound(fits["F"], want[2]) and np.abs(got[1] - want[1][:2]).max() <= sc.dist_bound(want[2])
            finally:
                other.close()
            LEDGER.add(name)
            return
        arc, dist = prim.step_lengths(S, "both")
        assert arc.shape == dist.shape == (r["n"],) and arc.dtype == dist.dtype == np.float64
        # 1. the independent reference
        ref_arc, ref_dist, scale = _reference(name)
        ref_arc, ref_dist = ref_arc[:r["n"]], ref_dist[:r["n"]]
        ra = float(np.abs(arc - ref_arc).max()) / sc.arc_bound(r["F"], scale)
        rd = float(np.abs(dist - ref_dist).max()) / sc.dist_bound(scale)
        print("row %s: arc %.3g of its bound %.3g, distance %.3g of its bound %.3g (scale %.4g)" % (
            name, ra, sc.arc_bound(r["F"], scale), rd, sc.dist_bound(scale), scale))
        assert np.isfinite(arc).all() and np.isfinite(dist).all() and (arc > 0).all() and (dist > 0).all()
        assert ra <= 1.0 and rd <= 1.0
        # 2. bit for bit
        _same(prim.step_lengths(S32, "both"), (arc, dist))
        _same(prim.step_lengths(S, "both"), (arc, dist))
        assert np.array_equal(_bits(prim.step_lengths(S, "arc_length")), _bits(arc)) and np.array_equal(_bits(prim.step_lengths(S, "distance")), _bits(dist))
        for lat in (S, S32):
            status, block = _device_call(ctx, prim, lat)
            assert status == _capi.MG_OK and np.all(block[:, [0, -1]] == GUARD), "a guard word beside the outputs"
            _same((block[0, 1:-1], block[1, 1:-1]), (arc, dist))
        # 3. the analytic rows: a straight, level, monotone path whatever the latents
        if r["kind"] == "analytic":
            bound = sc.device_bound(r["F"], scale)
            print("row %s: |arc - distance| %.3g (bound %.3g)" % (name, float(np.abs(arc - dist).max()), bound))
            assert np.abs(arc - dist).max() <= bound
            assert np.array_equal(_bits(arc), _bits(np.repeat(arc[:1], r["n"]))) and abs(arc[0] - sc.analytic_length(r)) <= sc.arc_bound(r["F"], scale)
        for key, ratio in (("arc", ra), ("dist", rd)):
            if ratio > WORST[key][0]:
                WORST[key] = (ratio, name)
        LEDGER.add(name)
    finally:
        prim.close()


def test_a_batch_is_the_prefix_of_a_longer_one(ctx):
    """n = 1, 15, 16, 17, 32 of one model: the first n candidates of the 33"""
    rows = [r for r in sc.ROWS if r["name"].startswith("batch_n")]
    prim = _capi.Primitive(ctx, sc.model_of(rows[-1]))
    try:
        full = prim.step_lengths(sc.latents_of(rows[-1]), "both")
        for r in rows[:-1]:
            _same(prim.step_lengths(sc.latents_of(r), "both"), (full[0][:r["n"]], full[1][:r["n"]]))
    finally:
        prim.close()


def _table_case(ctx, items, dtype):
    """One host-pointer call over `items` ((row, candidates), ...), each item's latents its own array: [(arc, dist)] per item."""
    prims = {name: _capi.Primitive(ctx, sc.model_of(name)) for name in {name for name, _ in items}}
    try:
        return _capi.step_lengths([(prims[name], sc.latents_of(name, n).astype(dtype)) for name, n in items], "both")
    finally:
        for p in prims.values():
            p.close()


def _alone(ctx, items, dtype):
    out = []
    for name, n in items:
        if n == 0:
            out.append((np.empty(0), np.empty(0)))
        else:
            out.append(_table_case(ctx, [(name, n)], dtype)[0])
    return out


def test_an_item_of_a_mixed_table_gives_the_bits_it_gives_alone(ctx):
    for dtype in (np.float64, np.float32):
        got, want = _table_case(ctx, sc.MIXED_TABLE, dtype), _alone(ctx, sc.MIXED_TABLE, dtype)
        for (name, n), g, w in zip(sc.MIXED_TABLE, got, want):
            assert g[0].shape == g[1].shape == (n,)
            _same(g, w)
            if n:
                ref = _reference(name)
                assert np.abs(g[0] - ref[0][:n]).max() <= sc.arc_bound(sc.BY_NAME[name]["F"], ref[2]) and np.abs(g[1] - ref[1][:n]).max() <= sc.dist_bound(ref[2])
    LEDGER.add("table:mixed")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("order", sorted(sc.LDS_TABLES))
def test_a_small_item_beside_one_over_64_kib(ctx, order, dtype):
    """The launch takes the larger item's LDS, so the small item's workgroup runs under it, and the opt-in must not depend on which
    comes first; on a fresh context the table is the very first call, so no earlier one has made the opt-in."""
    items = sc.LDS_TABLES[order]
    want = _alone(ctx, items, dtype)
    fresh = _capi.Context(0)
    try:
        first = _table_case(fresh, items, dtype)
    finally:
        fresh.close()
    for tag, got in (("", _table_case(ctx, items, dtype)), (":fresh", first)):
        for (name, n), g, w in zip(items, got, want):
            _same(g, w)
            ref = _reference(name)
            assert np.abs(g[0] - ref[0][:n]).max() <= sc.arc_bound(sc.BY_NAME[name]["F"], ref[2]) and np.abs(g[1] - ref[1][:n]).max() <= sc.dist_bound(ref[2])
        LEDGER.add("table:%s:%s%s" % (order, np.dtype(dtype).name, tag))


def test_the_ledger_covers_every_row():
    print("the table's largest ratio to the bound: arc length %.3g (row %s), distance %.3g (row %s)" % (WORST["arc"] + WORST["dist"]))
    missing = sc.LEDGER_WANT - LEDGER
    assert not missing, "rows and tables that did not run and match: %s" % sorted(missing)
