"""The per-call descriptor tables a context keeps on the device (mg_device_table, csrc/mg_host.hip): rewritten only when a call's
table differs from the last call's.  For each of the five tables Python reaches -- cluster-tree search, mg_walk_frames,
mg_score_walk_residuals, mg_score_walk_time, mg_step_lengths -- one context sees a call X, X again (a hit: the counter of
Context.table_uploads stays), a smaller call Y, a call Z larger than anything before (the table grows, for mg_score_walk_time and
mg_step_lengths past what they reserve: 16 KiB and 32 KiB), and X again; every answer is, bit for bit, the answer of the same call
on a context that never saw another table.  The planner step's table: tests/test_gpu_adaptors.py."""
import ctypes as C

import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd import objective_functions as of
from morphablegraphs_amd.cluster_tree import HipFeatureClusterTree, search_on_device
from morphablegraphs_amd.graph_walk import walk_frames_dev

pytestmark = pytest.mark.gpu

SHAPES = {"a": dict(n_components=5, n_frames=12, n_basis=7, n_gmm=2, n_time_components=2),
          "b": dict(n_components=7, n_frames=20, n_basis=6, n_gmm=2, n_time_components=1),
          "c": dict(n_components=6, n_frames=17, n_basis=5, n_gmm=3, n_time_components=2)}
PIN_CONS = [[{"type": "position", "t": 11.0, "weight": 1.0, "target": [40.0, None, -25.0]},
             {"type": "position", "t": 5.5, "weight": 0.5, "target": [10.0, 3.0, 20.0]}],
            [{"type": "position", "t": 3.0, "weight": 1.0, "target": [-15.0, None, 30.0]}]]
ALIGNMENT = {"joint": 0, "position": (0.0, 0.0, 0.0), "heading": (0.0, 1.0), "ref_dir": (0.0, 0.0, 1.0)}


class _World(object):
    """Three primitives on a context of their own, and what the calls below need beside them, each made on first use and kept:
    a table only repeats while the device addresses in it do."""

    def __init__(self):
        self.ctx = _capi.Context(0)
        self.prims = {name: _capi.Primitive(self.ctx, synthetic.make_primitive(seed=700 + i, name=name, **kw))
                      for i, (name, kw) in enumerate(sorted(SHAPES.items()))}
        joints, animated = synthetic.make_skeleton()
        self.skeleton = _capi.Skeleton(joints, animated)
        self.kept, self.buffers = {}, []

    def keep(self, key, make):
        if key not in self.kept:
            self.kept[key] = make()
        return self.kept[key]

    def upload(self, arr):
        self.buffers.append(self.ctx.upload(np.ascontiguousarray(arr)))
        return self.buffers[-1]

    def malloc(self, nbytes):
        self.buffers.append(self.ctx.malloc(nbytes))
        return self.buffers[-1]

    def close(self):
        self.ctx.synchronize()
        for obj in self.kept.values():
            if hasattr(obj, "close"):
                obj.close()
        for buf in self.buffers:
            buf.free()
        for prim in self.prims.values():
            prim.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _latents(seed, n, ld):
    return 0.5 * np.random.default_rng(seed).standard_normal((n, ld))


# ---- the five calls: run(world, case) -> tuple of arrays ----------------------------------------------------------------
def _tree(w, case):
    """case: which constraint set each search of the call scores with."""
    prim = w.prims["a"]
    means = np.random.default_rng(21).standard_normal((8, prim.n_components))
    tree = w.keep("tree", lambda: HipFeatureClusterTree(means, means, [0, 3, 5, 7, 7, 7, 7, 7, 7], np.arange(1, 8), [-1, -1, -1, 3, 4, 5, 6, 7],
                                                       n_spatial=prim.n_components))
    sets = [w.keep(("pin", k), lambda k=k: _capi.ConstraintSet(prim, PIN_CONS[k])) for k in range(2)]
    rec = search_on_device([(tree, prim, sets[k]) for k in case], 2)
    assert not rec["flags"].any()
    return (rec,)


def _walk(w, case):
    """case: (the steps' primitives, walks)."""
    sequence, n = case
    prims = [w.prims[name] for name in sequence]
    widths = [p.n_components for p in prims]
    rows, D, m = sum(p.n_canonical_frames for p in prims), prims[0].n_dim, len(prims)
    S = _latents(31 + n, n, sum(widths))
    with w.ctx.buffers() as bufs:
        d_frames, d_xf = bufs.malloc(8 * n * rows * D), bufs.malloc(8 * n * m * 4)
        walk_frames_dev(prims, np.concatenate(([0], np.cumsum(widths)[:-1])), bufs.upload(S), np.float64, n, S.shape[1], d_frames, rows, d_transforms=d_xf)
        return w.ctx.download(d_frames, (n, rows, D), np.float64), w.ctx.download(d_xf, (n, m, 4), np.float64)


def _walk_score(w, case):
    """case: the steps' primitives; every step scores two constraints of its own and the four exit values, aligned to the step before."""
    records, lat_off = [], 0
    for i, name in enumerate(case):
        prim = w.prims[name]
        tl = float(prim.n_canonical_frames - 1)
        clist = [{"type": "position", "t": tl, "weight": 1.0, "target": [30.0 * (i + 1), None, -20.0 * i]},
                 {"type": "direction", "t": tl / 2.0, "weight": 0.5, "target": [0.3, 1.0]}]
        clist = clist + of._exit_constraints(float(prim.n_canonical_frames), 0, (0.0, 0.0, 1.0))
        cset = w.keep(("scored", name, i), lambda: _capi.ConstraintSet(prim, clist, w.skeleton, ALIGNMENT))
        records.append((prim, cset, None, lat_off, 2, 2 * i))
        lat_off += prim.n_components
    return _capi.WalkScoreTable(records).score(_latents(41, 17, lat_off), 2 * len(case))


def _walk_time(w, case):
    """case: (the window's primitives, constraints).  The table object is kept: its steps name its own copy of the spatial latents."""
    sequence, n_cons = case
    prims = [w.prims[name] for name in sequence]
    n = 17

    def make():
        rng = np.random.default_rng(51 + n_cons)
        steps, off = [], 0
        for p in prims:
            steps.append((p, off, 0.5 * rng.standard_normal(p.n_components)))
            off += p.n_time_components
        cons = [(c % len(prims), (7 * c) % prims[c % len(prims)].n_canonical_frames, float(rng.uniform(0.1, 3.0))) for c in range(n_cons)]
        table = _capi.WalkTimeTable(steps, cons, 0.0, 0.02)
        table.d_S, table.d_out = w.upload(0.3 * rng.standard_normal((n, off))), [w.malloc(8 * n) for _ in range(3)]
        return table
    table = w.keep(("time", case), make)
    table.score_dev(table.d_S, np.float64, n, table.n_latents, 2.0, 0.3, *table.d_out)
    return tuple(w.ctx.download(d, (n,), np.float64) for d in table.d_out)


def _step_lengths(w, case):
    """case: (primitive, candidates) per item, on device buffers that stay (mg_step_lengths; the host entry point's live in a block of the call)."""
    def make():
        table = (_capi.StepLengthItem * len(case))()
        outs, lat = [], {}
        for rec, (name, n) in zip(table, case):
            prim = w.prims[name]
            if (name, n) not in lat:
                lat[(name, n)] = w.upload(_latents(61 + n, n, prim.n_components))
            arc, dist = w.malloc(8 * n), w.malloc(8 * n)
            rec.prim, rec.latents, rec.latent_offset, rec.n_samples, rec.ld = prim.handle.value, lat[(name, n)].address, 0, n, prim.n_components
            rec.arc_length, rec.distance = arc.address, dist.address
            outs.append((arc, dist, n))
        return table, outs
    table, outs = w.keep(("lengths", case), make)
    _capi.step_lengths_table(w.prims["a"].lib, len(case), table, np.float64, host=False)
    return tuple(w.ctx.download(d, (n,), np.float64) for arc, dist, n in outs for d in (arc, dist))


# X (two steps or items), Y (one: a strict prefix-sized table), Z (the most, and past the table's reserve), then further calls
CALLS = {
    "tree": (_tree, (0, 1), (1,), (0, 1, 1, 0, 1), ()),
    # (the last one: X's steps for more walks -- the transforms' scratch behind the table grows)
    "walk": (_walk, (("a", "b"), 3), (("a",), 3), (("a", "b", "c", "b"), 3), ((("a", "b"), 40),)),
    "walk_score": (_walk_score, ("a", "b"), ("a",), ("a", "b", "c"), ()),
    # Z: 8 steps of 96 bytes and 800 constraints of 20 bytes are 16 768 bytes > 16 KiB
    "walk_time": (_walk_time, (("a", "b"), 4), (("a",), 2), (("a", "b", "c", "b", "a", "c", "b", "a"), 800), ()),
    # Z: 400 one-candidate items of 96 bytes are 38 400 bytes > 32 KiB, in two launches of at most 256 items
    "step_length": (_step_lengths, (("a", 16), ("b", 40)), (("a", 16),), tuple((("a", "b", "c")[i % 3], 1) for i in range(400)), ()),
}


def _assert_same_bits(got, want):
    assert len(got) == len(want)
    for g, e in zip(got, want):
        assert g.shape == e.shape and g.dtype == e.dtype
        np.testing.assert_array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(e).view(np.uint8))


def _fresh(run, case):
    other = _World()
    try:
        return run(other, case)
    finally:
        other.close()


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_table_is_uploaded_when_it_differs_and_only_then(world, name):
    run, X, Y, Z, more = CALLS[name]
    uploads = lambda: world.ctx.table_uploads(name)
    others = [n for n in _capi.DEVICE_TABLES if n != name]
    before, u0 = {n: world.ctx.table_uploads(n) for n in others}, uploads()
    first = run(world, X)
    assert uploads() == u0 + 1
    assert all(np.isfinite(a).all() for a in first if a.dtype == np.float64)
    _assert_same_bits(run(world, X), first)
    assert uploads() == u0 + 1                                  # the hit
    for k, case in enumerate((Y, Z) + more):
        got = run(world, case)
        assert uploads() == u0 + 2 + k
        _assert_same_bits(got, _fresh(run, case))
    _assert_same_bits(run(world, X), first)
    assert uploads() == u0 + 4 + len(more)
    assert {n: world.ctx.table_uploads(n) for n in others} == before   # every table counts for itself


def test_the_general_counter_is_the_walk_time_counter_and_refuses_other_tables(world):
    lib, n = world.prims["a"].lib, C.c_int64()
    _capi._check(lib.mg_walk_time_table_uploads(world.ctx.handle, C.byref(n)))
    assert n.value == world.ctx.table_uploads("walk_time")
    for which in (-1, len(_capi.DEVICE_TABLES)):
        assert lib.mg_context_table_uploads(world.ctx.handle, which, C.byref(n)) == _capi.MG_ERR_INVALID_ARGUMENT
