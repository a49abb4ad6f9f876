"""The NumPy statements of morphablegraphs_amd.scaled_fpca against sklearn's own PCA as recorded in tests/golden/scaled_fpca.npz
(tools/gen_scaled_fpca_golden.py), the identity the device route rests on, and the points of SLSQP's forward differences.
No GPU, no library.

The rule for an error value: |ours - reference| <= 10 * max(spread, 1e-13 * |reference|), spread the
host statement's largest difference over 3 reruns on permuted sample rows, recorded in the fixture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_fpca_cases as sc  # noqa: E402
from conftest import load_golden  # noqa: E402

from morphablegraphs_amd import feature_point_model as fpm  # noqa: E402
from morphablegraphs_amd import scaled_fpca as sf  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return load_golden("scaled_fpca")


def load_case(golden, name):
    """(case, coeffs, weights, skeleton, design, joints) drawn again from the recorded seed and held to the recorded digest."""
    c = sc.case(name)
    coeffs, weights = sc.draw(c, int(golden[name + "_seed"]))
    assert sc.digest(coeffs, weights) == str(golden[name + "_digest"]), "the drawn data of case %s drifted from the fixture" % name
    return c, coeffs, weights, sc.skeleton(), sf.sampled_design(sc.knots_of(c), c["F"], c["step"]), sc.joints_of(c)


def within_rule(what, ours, reference, spread, scale=1.0):
    ours, reference = np.asarray(ours, dtype=np.float64), np.asarray(reference, dtype=np.float64)
    bound = 10.0 * np.maximum(float(spread), 1e-13 * np.abs(reference)) * scale
    diff = np.abs(ours - reference)
    ratio = float(np.max(diff / bound))
    print("%s: worst |difference| %.3g, %.3g of the bound" % (what, float(np.max(diff)), ratio))
    assert np.all(diff <= bound), "%s: %.3g of the bound" % (what, ratio)
    return ratio


@pytest.mark.parametrize("name", sc.NAMES + ["optimiser"])
def test_host_statement_reproduces_sklearn(golden, name):
    c, coeffs, weights, sk, design, joints = load_case(golden, name)
    assert np.all(sc.relative_gaps(coeffs, weights, c["npc"]) >= sc.MIN_GAP)
    host = sf.sfpca_errors_host(coeffs, weights, c["npc"], sk, design, joints)
    within_rule(name + " host vs recorded host", host, golden[name + "_host_errors"], golden[name + "_spread"])
    within_rule(name + " host vs sklearn", host, golden[name + "_sk_errors"], golden[name + "_spread"])


@pytest.mark.parametrize("name", ["base", "n2_npc1", "weight_bounds", "constant_joint"])
def test_reconstruction_is_sklearns_and_the_gram_routes(golden, name):
    """Steps 1 to 3 equal mean + U_k U_k^T Xc with U_k from sum_g w_g^2 G_g.  Bound: the Gram matrix A = Xw Xw^T (Xw the weighted centred
    rows, p columns) is formed to about p eps |A| = p eps s_1^2; by Davis-Kahan the leading-k invariant subspace of A turns by at most
    |E| / (lambda_k - lambda_{k+1}) <= p eps s_1^2 / (s_k^2 gap), gap = (s_k - s_{k+1}) / s_k (lambda_k - lambda_{k+1} = s_k^2 gap (2 - gap));
    the SVD route's own subspace turns by eps s_1 / (s_k gap), less.  The projector moves by at most twice the sine, and an entry of
    (P' - P) Xc by at most that times |Xc|_2.  A factor 8 covers both routes and the products' rounding.  The SVD route (ours and
    sklearn's) also divides its weighted reconstruction U_k S_k Vt_k + mean, whose entries carry an absolute error of about n eps s_1, by
    the weights again: n eps s_1 / min(weight) in a lightly weighted channel, which the Gram route (it never weights the data) does not
    have.  The second term of the bound is that, under the same factor."""
    c, coeffs, weights, _, _, _ = load_case(golden, name)
    w = weights[min(1, len(weights) - 1)]
    n, npc = len(coeffs), c["npc"]
    ours = sf.sfpca_reconstruct_host(coeffs, w, npc)
    sklearns = golden[name + "_sk_reconstruction"]
    ext = sf.spread_weights(w, coeffs.shape[2])[0]
    xc = (coeffs - coeffs.mean(axis=0)).reshape(n, -1)
    s = np.linalg.svd((xc.reshape(coeffs.shape) * ext).reshape(n, -1), compute_uv=False)
    gap = 1.0 if npc >= len(s) else (s[npc - 1] - s[npc]) / s[npc - 1]
    bound = 8.0 * xc.shape[1] * EPS * (s[0] / s[npc - 1]) ** 2 / gap * np.linalg.norm(xc, 2) + 8.0 * n * EPS * s[0] / np.min(ext)
    d_sk, d_gram = np.max(np.abs(ours - sklearns)), np.max(np.abs(ours - sf.gram_reconstruct_host(coeffs, w, npc)))
    print("%s: gap %.3g, bound %.3g, |host - sklearn| %.3g, |host - Gram route| %.3g" % (name, gap, bound, d_sk, d_gram))
    assert d_sk <= bound and d_gram <= bound


def test_group_grams_add_up_to_the_weighted_gram(golden):
    _, coeffs, weights, _, _, _ = load_case(golden, "base")
    n = len(coeffs)
    grams = sf.group_grams_host(coeffs)
    assert grams.shape == (sc.N_WEIGHTS, n, n)
    for w in weights:
        xw = ((coeffs - coeffs.mean(axis=0)) * sf.spread_weights(w, sc.N_DIMS)[0]).reshape(n, -1)
        full = xw @ xw.T
        assert np.max(np.abs(np.tensordot(w * w, grams, axes=1) - full)) <= 64 * xw.shape[1] * EPS * np.max(np.abs(full))


@pytest.mark.parametrize("name", ["base", "weight_bounds", "joint_subset"])
def test_error_is_invariant_under_a_common_scale(golden, name):
    c, coeffs, weights, sk, design, joints = load_case(golden, name)
    a = sf.sfpca_errors_host(coeffs, weights, c["npc"], sk, design, joints)
    for scale in (2.5, 1.0 / 64.0):
        b = sf.sfpca_errors_host(coeffs, weights * scale, c["npc"], sk, design, joints)
        within_rule("%s x %g" % (name, scale), b, a, golden[name + "_spread"])


def test_constant_joint_has_no_gram(golden):
    c, coeffs, _, _, _, _ = load_case(golden, "constant_joint")
    g = 3 + c["constant_joint"]
    assert np.max(np.abs(sf.group_grams_host(coeffs)[g])) <= 1e-25      # (the mean of equal values rounds: not exactly 0)


def test_joint_positions_host_is_joint_position_host(golden):
    _, coeffs, _, sk, design, _ = load_case(golden, "base")
    frames = np.einsum("fb,nbd->nfd", design, coeffs).reshape(-1, sc.N_DIMS)[::37]
    joints = list(range(len(sk.names)))
    ours = sf.joint_positions_host(sk, frames, joints)
    for i, frame in enumerate(frames):
        for k, j in enumerate(joints):
            assert np.max(np.abs(ours[i, k] - fpm.joint_position_host(sk, frame, j))) <= 1e-13


def test_forward_difference_points_are_scipys():
    """scipy's SLSQP, left to its own gradient, evaluates x and then x + epsilon e_i: the calls recorded on a counting wrapper equal
    forward_difference_points bit for bit, and its gradient is (f_i - f_0) / dx."""
    from scipy.optimize import minimize
    calls = []

    def fun(x):
        calls.append(np.array(x))
        return float(np.sum((x - np.arange(1, len(x) + 1) * 0.3) ** 2) + 0.1 * np.prod(np.cos(x)))
    x0 = np.array([1.0, 0.75, 1.5, 1e-4, 2.0, 0.0001 * 3, 1.0, 1.25])
    G = len(x0)
    minimize(fun, x0, bounds=tuple((sf.WEIGHT_LOWER_BOUND, None) for _ in range(G)), method="SLSQP", options={"maxiter": 3})
    # every gradient is a run of G + 1 calls: the point (already evaluated or evaluated first), then the G steps
    i = found = 0
    while i + G < len(calls):
        pts, dx = sf.forward_difference_points(calls[i])
        block = np.array(calls[i + 1:i + 1 + G])
        if np.array_equal(block.view(np.uint64), pts[1:].view(np.uint64)):
            assert np.array_equal(pts[0].view(np.uint64), calls[i].view(np.uint64))
            assert np.all(dx > 0) and np.all(np.abs(dx - sf.SLSQP_EPSILON) <= EPS * np.maximum(calls[i], 1.0))
            found, i = found + 1, i + 1 + G
        else:
            i += 1
    assert found >= 2, "no forward-difference block of scipy's matched (%d calls)" % len(calls)


def test_spread_weights_and_misuse():
    w = np.arange(1.0, 9.0)
    ext = sf.spread_weights(w, sc.N_DIMS)[0]
    assert list(ext[:3]) == [1.0, 2.0, 3.0] and list(ext[3:7]) == [4.0] * 4 and list(ext[-4:]) == [8.0] * 4
    with pytest.raises(ValueError):
        sf.spread_weights(np.ones(7), sc.N_DIMS)
    with pytest.raises(ValueError):
        sf.spread_weights(np.ones(8), 22)
