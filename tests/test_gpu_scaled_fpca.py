"""The device's scaled functional PCA (mg_sfpca_create / mg_sfpca_errors / mg_sfpca_projector, morphablegraphs_amd.scaled_fpca)
against the host statement sfpca_errors_host and sklearn's values recorded in tests/golden/scaled_fpca.npz, on the cases of
tests/scaled_fpca_cases.py.  The rule: |ours - reference| <= 10 * max(spread, 1e-13 * |reference|), spread
the host statement's largest difference over 3 reruns on permuted sample rows, recorded in the fixture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_fpca_cases as sc  # noqa: E402
from test_scaled_fpca_host import EPS, load_case, within_rule  # noqa: E402
from conftest import load_golden  # noqa: E402

from morphablegraphs_amd import _capi  # noqa: E402
from morphablegraphs_amd import scaled_fpca as sf  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("scaled_fpca")


def device_object(ctx, c, coeffs, sk, joints, npc=None):
    return sf.HipScaledFunctionalPCA(coeffs, c["npc"] if npc is None else npc, sk, sc.knots_of(c), sc.N_JOINTS, joints=joints, step=c["step"], ctx=ctx)


@pytest.mark.parametrize("name", sc.NAMES)
def test_errors_reproduce_the_host_statement_and_sklearn(ctx, golden, name):
    """Measured on an MI355X: every case within 0.16 of the bound; the worst is npc_n_minus_1 (0.155 against the host statement and
    against sklearn), where the reconstruction is exact in exact arithmetic and what is compared are rounding-level zeros of 1e-26."""
    c, coeffs, weights, sk, design, joints = load_case(golden, name)
    obj = device_object(ctx, c, coeffs, sk, joints)
    try:
        ours = obj.errors(weights)
        assert ours.shape == (c["m"],) and np.all(obj.pca_statuses_ == _capi.MG_PCA_CONVERGED)
        host = sf.sfpca_errors_host(coeffs, weights, c["npc"], sk, design, joints)
        within_rule(name + " device vs host", ours, host, golden[name + "_spread"])
        within_rule(name + " device vs sklearn", ours, golden[name + "_sk_errors"], golden[name + "_spread"])
    finally:
        obj.close()


def test_independent_device_route(ctx, golden):
    """The same errors from pieces the project already had: mg_pca_fit of the weighted matrix, mg_pca_project / mg_pca_backproject,
    the spline evaluated on the host, mg_joint_positions."""
    name = sc.DEVICE_ROUTE_CASE
    c, coeffs, weights, sk, design, joints = load_case(golden, name)
    n, nb, D = coeffs.shape
    p, k = nb * D, c["npc"]
    original = ctx.joint_positions(sk, joints, np.einsum("fb,nbd->nfd", design, coeffs).reshape(-1, D))
    route = []
    for w in weights:
        ext = sf.spread_weights(w, D)[0]
        with ctx.buffers() as bufs:
            a_dev, c_dev = bufs.upload((coeffs * ext).reshape(n, p)), bufs.malloc(8 * n * p)
            fit = _capi.pca_fit(ctx, a_dev, n, p, c_dev)
            assert fit["status"] == _capi.MG_PCA_CONVERGED
            v_dev, m_dev = bufs.upload(np.ascontiguousarray(fit["vt"][:k])), bufs.upload(fit["mean"])
            low_dev, high_dev = bufs.malloc(8 * n * k), bufs.malloc(8 * n * p)
            _capi.pca_project(ctx, c_dev, v_dev, n, p, k, low_dev)
            _capi.pca_backproject(ctx, low_dev, v_dev, m_dev, n, p, k, high_dev)
            recon = ctx.download(high_dev, (n, p), np.float64).reshape(n, nb, D) / ext
        d = ctx.joint_positions(sk, joints, np.einsum("fb,nbd->nfd", design, recon).reshape(-1, D)) - original
        route.append(np.mean(np.sum(d * d, axis=2)))
    obj = device_object(ctx, c, coeffs, sk, joints)
    try:
        within_rule(name + " device vs the mg_pca_fit route", obj.errors(weights), np.array(route), golden[name + "_spread"])
    finally:
        obj.close()


@pytest.mark.parametrize("name", ["base", "n17", "m65", "npc5"])
def test_errors_are_reproducible_and_batch_independent(ctx, golden, name):
    c, coeffs, weights, sk, _, joints = load_case(golden, name)
    obj = device_object(ctx, c, coeffs, sk, joints)
    try:
        a, b = obj.errors(weights), obj.errors(weights)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        for j in sorted({0, len(weights) // 2, len(weights) - 1}):
            alone = obj.errors(weights[j])
            assert np.array_equal(alone.view(np.uint64), a[j:j + 1].view(np.uint64)), "weight vector %d alone differs from the batch" % j
    finally:
        obj.close()


@pytest.mark.parametrize("name", ["base", "n17", "weight_bounds", "constant_joint"])
def test_projector_and_fit_reproduce_the_reconstruction(ctx, golden, name):
    """U_k from mg_sfpca_projector spans the subspace of the host's (the bound of tests/test_scaled_fpca_host.py on the projector itself),
    follows the sign rule, and fit / transform / inverse_transform give the host's reconstruction under that test's bound."""
    c, coeffs, weights, sk, _, joints = load_case(golden, name)
    w = weights[min(1, len(weights) - 1)]
    n, npc = len(coeffs), c["npc"]
    ext = sf.spread_weights(w, sc.N_DIMS)[0]
    xc = (coeffs - coeffs.mean(axis=0)).reshape(n, -1)
    s = np.linalg.svd((xc.reshape(coeffs.shape) * ext).reshape(n, -1), compute_uv=False)
    gap = (s[npc - 1] - s[npc]) / s[npc - 1]
    turn = 8.0 * xc.shape[1] * EPS * (s[0] / s[npc - 1]) ** 2 / gap
    obj = device_object(ctx, c, coeffs, sk, joints)
    try:
        obj.fit(w)
        U, status = obj._handle.projector(w, npc)
        assert status == _capi.MG_PCA_CONVERGED and U.shape == (n, npc)
        Uh = sf.projector_host(coeffs, w, npc)
        dP = np.max(np.abs(U @ U.T - Uh @ Uh.T))
        print("%s: |P - P_host| %.3g, bound %.3g" % (name, dP, turn))
        assert dP <= turn
        for col in U.T:
            assert col[np.argmax(np.abs(col))] > 0
        assert np.max(np.abs(U.T @ U - np.eye(npc))) <= 64 * n * EPS
        low = obj.transform()
        assert low.shape == (n, npc)
        recon = obj.inverse_transform(low) / ext
        bound = turn * np.linalg.norm(xc, 2) + 8.0 * n * EPS * s[0] / np.min(ext)
        d = np.max(np.abs(recon - sf.sfpca_reconstruct_host(coeffs, w, npc)))
        print("%s: |reconstruction - host| %.3g, bound %.3g" % (name, d, bound))
        assert d <= bound
    finally:
        obj.close()


def test_heuristic_initialization_keeps_the_better_start(ctx, golden):
    c, coeffs, _, sk, design, joints = load_case(golden, "base")
    obj = device_object(ctx, c, coeffs, sk, joints)
    try:
        obj.heuristic_initialization()
        assert obj.n_objective_calls_ == 1
        ones = np.ones(sc.N_WEIGHTS)
        scaled = ones.copy()
        scaled[:3] = 1.0 / sf.scale_root_channels(coeffs)[1]
        e = sf.sfpca_errors_host(coeffs, np.stack([ones, scaled]), c["npc"], sk, design, joints)
        assert np.array_equal(obj.weight_vec, scaled if e[0] > e[1] else ones)
    finally:
        obj.close()


def test_optimiser_follows_scipys_run_on_the_host_statement(ctx, golden):
    """optimize_weights against the recorded SLSQP run of scipy on the host statement (jac=None): the same number of iterations; the
    first iterate under the rule scaled by 1 / epsilon (a forward-difference gradient amplifies a value's error by that); the final
    error not above the recorded one by more than the rule's bound.  Later iterates are printed, not compared."""
    name = "optimiser"
    c, coeffs, _, sk, _, joints = load_case(golden, name)
    spread = float(golden[name + "_spread"])
    obj = device_object(ctx, c, coeffs, sk, joints)
    try:
        obj.initialize_weights(np.ones(sc.N_WEIGHTS))
        ours = []
        x = obj.optimize_weights(callback=lambda xk: ours.append(np.array(xk)))
        recorded = golden[name + "_iterates"]
        print("iterations: ours %d, recorded %d; values: ours %d calls" % (obj.result_.nit, int(golden[name + "_nit"]), obj.n_objective_calls_))
        for i, (a, b) in enumerate(zip(ours, recorded)):
            print("iterate %d: largest |ours - recorded| %.3g" % (i + 1, np.max(np.abs(a - b))))
        print("final error: ours %.15g, recorded %.15g" % (obj.result_.fun, float(golden[name + "_fun"])))
        assert obj.result_.nit == int(golden[name + "_nit"]) and len(ours) == len(recorded)
        bound = 10.0 * max(spread, 1e-13 * abs(float(golden[name + "_start_fun"])))
        d1 = np.max(np.abs(ours[0] - recorded[0]))
        print("first iterate: %.3g, bound %.3g" % (d1, bound / sf.SLSQP_EPSILON))
        assert d1 <= bound / sf.SLSQP_EPSILON
        assert obj.result_.fun <= float(golden[name + "_fun"]) + 10.0 * max(spread, 1e-13 * abs(float(golden[name + "_fun"])))
        assert np.all(x >= sf.WEIGHT_LOWER_BOUND)
    finally:
        obj.close()


def test_misuse_is_refused_before_any_launch(ctx, golden):
    c, coeffs, weights, sk, design, joints = load_case(golden, "base")
    nb, D = coeffs.shape[1:]
    idx = sk.indices(joints)

    def status_of(call):
        with pytest.raises(_capi.MGError) as e:
            call()
        return e.value.status

    def create(data):
        with ctx.buffers() as bufs:
            _capi.ScaledFPCA(ctx, bufs.upload(np.ascontiguousarray(data)), len(data), nb, D, sk, idx, design).close()
    assert status_of(lambda: create(coeffs[:1])) == _capi.MG_ERR_UNSUPPORTED                                 # n = 1
    assert status_of(lambda: create(np.resize(coeffs, (1025, nb, D)))) == _capi.MG_ERR_UNSUPPORTED          # n = 1025
    bad = coeffs.copy()
    bad[3, 2, 5] = np.nan
    assert status_of(lambda: create(bad)) == _capi.MG_ERR_INVALID_ARGUMENT                                   # NaN data
    with ctx.buffers() as bufs:
        h = _capi.ScaledFPCA(ctx, bufs.upload(coeffs), len(coeffs), nb, D, sk, idx, design)
    try:
        assert status_of(lambda: h.errors(weights, len(coeffs))) == _capi.MG_ERR_INVALID_ARGUMENT           # npc = n
        assert status_of(lambda: h.errors(weights, 0)) == _capi.MG_ERR_INVALID_ARGUMENT
        for value in (0.0, -1.0, np.nan, np.inf):
            w = weights.copy()
            w[-1, 4] = value
            assert status_of(lambda: h.errors(w, c["npc"])) == _capi.MG_ERR_INVALID_ARGUMENT                 # a zero, negative or non-finite weight
            assert status_of(lambda: h.projector(w[-1], c["npc"])) == _capi.MG_ERR_INVALID_ARGUMENT
        assert status_of(lambda: h.errors(weights[:, :-1], c["npc"])) == _capi.MG_ERR_INVALID_ARGUMENT      # weights of the wrong width
        assert status_of(lambda: h.errors(np.ones((2, sc.N_WEIGHTS + 1)), c["npc"])) == _capi.MG_ERR_INVALID_ARGUMENT
        e, st = h.errors(weights, c["npc"])                                                                  # and the handle still works
        assert np.all(np.isfinite(e)) and np.all(st == _capi.MG_PCA_CONVERGED)
    finally:
        h.close()
