"""mg_mixture_scores on the device against mg_mixture_scores_host, the same statements on the host: the weighted log-probabilities
bit for bit, log p within the tolerance mg_gmm_log_prob is held to against its host statement, the reachable flags identical;
across the kernel's shape edges (one wave of 64 targets per workgroup; the target in registers up to 4 and up to 8 dimensions, in
LDS above; the large-LDS opt-in past 64 KB), the item table's edges, and HipReachabilityIndex against the sklearn fixture."""
import types

import numpy as np
import pytest

import reachability_cases as rc
from morphablegraphs_amd import _capi
from morphablegraphs_amd import feature_point_model as fpm

pytestmark = pytest.mark.gpu

CASES, REACHABLE_MARGIN = rc.fixture_cases()
IDS = ["K%d_dim%d" % c["means"].shape for c in CASES]
TILE = _capi.MG_MIXTURE_SCORES_TILE
ALL = ("logp", "wlp", "reachable")


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def _pair(ctx, weights, means, covars, threshold=-np.inf):
    """The same mixture with and without a device copy."""
    return _capi.FeatureMixture(ctx, weights, means, covars, threshold), _capi.FeatureMixture(None, weights, means, covars, threshold, host=True)


def _assert_device_is_host(got, want, threshold=None):
    for g, w in zip(got, want):
        assert rc.same_bits(g["wlp"], w["wlp"])
        assert g["logp"].shape == w["logp"].shape and np.array_equal(np.isnan(g["logp"]), np.isnan(w["logp"]))
        np.testing.assert_allclose(g["logp"], w["logp"], rtol=rc.LOGP_RTOL, atol=rc.LOGP_ATOL)
        if threshold is None:
            assert np.array_equal(g["reachable"], w["reachable"])
        else:
            clear = ~(np.abs(w["logp"] - threshold) <= rc.LOGP_ATOL + rc.LOGP_RTOL * np.abs(w["logp"]))
            assert np.array_equal(g["reachable"][clear], w["reachable"][clear])
            assert np.array_equal(g["reachable"], ~(g["logp"] < threshold))


def _check(ctx, specs):
    """specs: [(weights, means, covars, X, offset)]: one device call and one host call over all of them; returns the device's."""
    pairs = [_pair(ctx, w, mu, cov, -8.0 - 2.0 * mu.shape[1]) for w, mu, cov, _, _ in specs]
    got = _capi.mixture_scores([(p[0], s[3], s[4]) for p, s in zip(pairs, specs)], ALL, ctx=ctx)
    want = _capi.mixture_scores_host([(p[1], s[3], s[4]) for p, s in zip(pairs, specs)], ALL)
    for s, g, w in zip(specs, got, want):
        _assert_device_is_host([g], [w], -8.0 - 2.0 * s[1].shape[1])
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_device_is_the_host_twin_on_the_fixture(ctx, case):
    dev, host = _pair(ctx, case["weights"], case["means"], case["covars"], case["threshold"])
    got = _capi.mixture_scores([(dev, case["X"])], ALL, ctx=ctx)
    _assert_device_is_host(got, _capi.mixture_scores_host([(host, case["X"])], ALL))
    assert np.array_equal(got[0]["reachable"], ~(case["logp"] < case["threshold"]))      # no score within REACHABLE_MARGIN of the threshold
    rc.assert_within_fixture_tolerance(got[0]["wlp"], case["wlp"], "device wlp")
    rc.assert_within_fixture_tolerance(got[0]["logp"], case["logp"], "device logp")


# the register routes end at 4 and at 8 dimensions; 16 | 17: a factor column past one 128-byte line's worth of doubles
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 6, 8, 9, 16, 17, 96])
@pytest.mark.parametrize("K", [1, 2, 40, 64])
def test_dimensions_and_component_counts(ctx, K, dim):
    if dim == 96 and K > 2:
        K = {40: 30, 64: 31}[K]          # at 96 dimensions: both sides of the 64 KB past which the kernel takes the large-LDS opt-in
        assert _capi.mixture_lds_bytes(30, 96) <= 64 * 1024 < _capi.mixture_lds_bytes(31, 96)
    weights, means, covars = rc.seeded_mixture(K, dim)
    _check(ctx, [(weights, means, covars, rc.seeded_targets(means, TILE + 1), 0)])


def test_the_largest_mixture_the_caps_allow(ctx):
    weights, means, covars = rc.seeded_mixture(64, 96)
    assert _capi.mixture_lds_bytes(64, 96) == (96 * 65 + 64 * 64) * 8 <= 160 * 1024
    _check(ctx, [(weights, means, covars, rc.seeded_targets(means, 3), 0)])


@pytest.mark.parametrize("dim", [3, 6, 17])
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_target_counts_around_the_tile(ctx, n, dim):
    weights, means, covars = rc.seeded_mixture(3, dim)
    got = _check(ctx, [(weights, means, covars, rc.seeded_targets(means, n), 0)])
    assert got[0]["logp"].shape == (n,) and got[0]["wlp"].shape == (n, 3)


@pytest.mark.parametrize("dim", [4, 7, 12])
def test_items_share_a_wide_target_matrix(ctx, dim):
    rng = np.random.default_rng(dim)
    wide = rng.standard_normal((TILE + 7, 2 * dim + 3))                    # ld > dim; the items read columns 0, 3 and dim + 3 on
    mixtures = [rc.seeded_mixture(2 + k, dim, seed=k) for k in range(3)]
    specs = [(m + (wide, off)) for m, off in zip(mixtures, (0, 3, dim + 3))]
    two = _check(ctx, specs[:2])
    # five items over the one matrix, a mixture repeated, empty items among the others
    empty = np.zeros((0, dim))
    five = _check(ctx, [specs[0], mixtures[1] + (empty, 0), specs[1], specs[2], specs[0], mixtures[2] + (empty, 0), specs[1][:3] + (wide, 1)])
    for a, b in ((two[0], five[0]), (two[1], five[2]), (five[0], five[4])):
        for key in ALL:
            assert rc.same_bits(a[key], b[key])                               # neither the batch nor the other items show
    assert five[1]["logp"].shape == (0,)


def test_one_more_item_than_a_launch_holds(ctx):
    mixtures = [rc.seeded_mixture(1 + k % 3, (3, 6, 10)[k % 3], seed=k % 3) for k in range(3)]
    pairs = [_pair(ctx, *m, threshold=-12.0) for m in mixtures]
    n_items = _capi.MG_MIXTURE_SCORES_MAX_ITEMS + 1
    targets = [rc.seeded_targets(mixtures[i % 3][1], 1 + i % 2, seed=i) for i in range(n_items)]
    ctx.profile_reset()
    ctx.profile_enable(True)
    got = _capi.mixture_scores([(pairs[i % 3][0], targets[i]) for i in range(n_items)], ALL, ctx=ctx)
    ctx.synchronize()
    ctx.profile_enable(False)
    assert ctx.profile_get("mixture_scores")[1] == 2                        # two slices, and the slot counts them
    want = _capi.mixture_scores_host([(pairs[i % 3][1], targets[i]) for i in range(n_items)], ALL)
    _assert_device_is_host(got, want, -12.0)


def test_a_target_that_is_not_finite_poisons_its_own_row_only(ctx):
    for dim in (3, 8, 11):
        weights, means, covars = rc.seeded_mixture(4, dim)
        X = rc.seeded_targets(means, TILE + 3)
        clean = _check(ctx, [(weights, means, covars, X, 0)])[0]
        Y = X.copy()
        Y[5, dim - 1], Y[TILE, 0], Y[TILE + 2, dim // 2] = np.nan, np.inf, -np.inf
        got = _check(ctx, [(weights, means, covars, Y, 0)])[0]
        bad = np.zeros(len(X), bool)
        bad[[5, TILE, TILE + 2]] = True
        assert np.isnan(got["logp"][bad]).all() and np.isnan(got["wlp"][bad]).all() and got["reachable"][bad].all()     # NaN reads as reachable
        for key in ALL:
            assert rc.same_bits(got[key][~bad], clean[key][~bad])


def test_a_targets_values_do_not_depend_on_its_place_in_the_batch(ctx):
    for dim in (4, 6, 20):
        weights, means, covars = rc.seeded_mixture(5, dim)
        X = rc.seeded_targets(means, 2 * TILE + 9, seed=3)
        first = _check(ctx, [(weights, means, covars, X, 0)])[0]
        moved = _check(ctx, [(weights, means, covars, np.concatenate((X[1:], X[:1])), 0)])[0]
        alone = _check(ctx, [(weights, means, covars, X[:1], 0)])[0]
        for key in ALL:
            assert rc.same_bits(moved[key][-1], first[key][0]) and rc.same_bits(alone[key][0], first[key][0])
            assert rc.same_bits(moved[key][:-1], first[key][1:])


def test_a_second_identical_call_uploads_no_table(ctx):
    weights, means, covars = rc.seeded_mixture(3, 4)
    dev, host = _pair(ctx, weights, means, covars, -9.0)
    X = rc.seeded_targets(means, 70)
    with ctx.buffers() as bufs:
        d_x, d_logp, d_wlp = bufs.upload(X), bufs.malloc(8 * 70), bufs.malloc(8 * 70 * 3)
        table = (_capi.MixtureScoreItem * 2)()
        for rec, n in zip(table, (70, 40)):
            rec.mixture, rec.targets, rec.target_offset, rec.n_targets, rec.ld = dev.handle.value, d_x.address, 0, n, 4
        table[0].logp, table[1].wlp = d_logp.address, d_wlp.address
        u0 = ctx.table_uploads("mixture_scores")
        _capi.mixture_scores_table(ctx, 2, table)
        assert ctx.table_uploads("mixture_scores") == u0 + 1
        first = ctx.download(d_logp, (70,), np.float64)
        _capi.mixture_scores_table(ctx, 2, table)
        _capi.mixture_scores_table(ctx, 0, None)                            # nothing to do: no launch, no upload
        assert ctx.table_uploads("mixture_scores") == u0 + 1
        assert rc.same_bits(ctx.download(d_logp, (70,), np.float64), first)
        table[1].n_targets = 41
        _capi.mixture_scores_table(ctx, 2, table)
        assert ctx.table_uploads("mixture_scores") == u0 + 2
        want = _capi.mixture_scores_host([(host, X)], ("logp", "wlp"))[0]
        np.testing.assert_allclose(first, want["logp"], rtol=rc.LOGP_RTOL, atol=rc.LOGP_ATOL)
        assert rc.same_bits(ctx.download(d_wlp, (41, 3), np.float64), want["wlp"][:41])
        # a mixture without a device copy, or of another context, is refused before any launch
        table[0].mixture = host.handle.value
        with pytest.raises(_capi.MGError, match="no device copy"):
            _capi.mixture_scores_table(ctx, 2, table)
        assert ctx.table_uploads("mixture_scores") == u0 + 2


def _stub_model(ctx, name, case):
    model = fpm.HipFeaturePointModel(types.SimpleNamespace(name=name, has_time_parameters=False, t_pca={"n_components": 0}), None, ctx=ctx)
    model.feature_point_dist = fpm.FeatureMixture(case["weights"], case["means"], case["covars"])
    model.threshold = case["threshold"]
    model.root_feature_dist, model.root_threshold, model.root_feature_dist_type = model.feature_point_dist, case["threshold"], "angle"
    return model


def test_the_index_is_the_per_node_call_and_the_fixture(ctx):
    a, b = CASES[0], CASES[3]                                                # the fixture's two mixtures over 3 dimensions
    nodes = {"first": _stub_model(ctx, "first", a), "many": _stub_model(ctx, "many", b), "again": _stub_model(ctx, "again", a)}
    X = np.concatenate((a["X"], b["X"]))
    na = len(a["X"])
    for which in ("points", "root"):
        index = fpm.HipReachabilityIndex(nodes, which=which, ctx=ctx)
        u0 = ctx.table_uploads("mixture_scores")
        scores = index.scores(X)
        assert ctx.table_uploads("mixture_scores") == u0 + 1 and scores.shape == (3, len(X))
        for row, model in zip(scores, nodes.values()):
            per_node = model.score_targets(X, device=True) if which == "points" else model.score_trajectory_targets(X, device=True)
            assert rc.same_bits(row, per_node)
        rc.assert_within_fixture_tolerance(scores[0, :na], a["logp"], "index, node 0")
        rc.assert_within_fixture_tolerance(scores[1, na:], b["logp"], "index, node 1")
        rc.assert_within_fixture_tolerance(scores[2, :na], a["logp"], "index, node 2")
        reach = index.reachable(X)
        assert np.array_equal(reach[0, :na], ~(a["logp"] < a["threshold"])) and np.array_equal(reach[1, na:], ~(b["logp"] < b["threshold"]))
        assert np.array_equal(reach[1], nodes["many"].check_reachability_batch(X, device=True))
        host = fpm.HipReachabilityIndex(nodes, which=which, host=True)
        assert index.best_nodes(X) == host.best_nodes(X) and index.reachable_nodes(X[0]) == host.reachable_nodes(X[0])
        assert index.best_nodes(a["X"][:1]) == ["first"]                     # "again" scores the same bits; the first in key order wins
        each = index.scores_each({"many": b["X"], "first": a["X"]})
        assert rc.same_bits(each["many"], scores[1, na:]) and rc.same_bits(each["first"], scores[0, :na])
    # the model keeps its device mixture until it is retrained or reloaded; the default path never makes one
    model = nodes["first"]
    kept = model.device_mixture("points")
    model.score_targets(X, device=True)
    assert model.device_mixture("points") is kept
    model.threshold = a["threshold"] - 1.0
    assert model.device_mixture("points") is not kept
    assert rc.same_bits(model.score_targets(X), model.feature_point_dist.score_samples(X))
