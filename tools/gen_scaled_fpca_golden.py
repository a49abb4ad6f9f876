"""Writes tests/golden/scaled_fpca.npz: what steps 1 to 3 of the reference's sfpca_objective_func (construction/fpca/
objective_functions.py) give on the cases of tests/scaled_fpca_cases.py with sklearn's own PCA, and what scipy's SLSQP makes of
the host statement of the objective.

    python tools/gen_scaled_fpca_golden.py [--out tests/golden/scaled_fpca.npz]

Steps 1 to 3 are run as the reference writes them -- numpy.diag of the spread weights, sklearn.decomposition.PCA(n_components=
npc).fit_transform / inverse_transform on the weighted coefficients reshaped to (n, n_basis * D), numpy.linalg.inv of the weight
matrix -- and step 4 as morphablegraphs_amd.scaled_fpca restates it (the reference's step 4 is not in its tree).

Per case `<name>_`: seed, redraws (a case is drawn again with the next seed while the relative gap between singular values npc
and npc + 1 of the weighted centred matrix is below 1e-3 for any of its weight vectors), digest (SHA-256 of the drawn
coefficients and weights), gaps (m), sk_errors (m: the restated error of sklearn's reconstructions), host_errors (m:
sfpca_errors_host), spread (the largest difference of sfpca_errors_host from host_errors over 3 reruns on permuted sample rows),
and, for the cases in RECONSTRUCTIONS, sk_reconstruction (sklearn's reconstruction for weight vector 1 or the last, unweighted
again).  `optimiser_`: the SLSQP run of scipy.optimize.minimize (jac=None: scipy's own forward differences, bounds (1e-4, None),
maxiter 1000) on sfpca_errors_host from ones: iterates (nit, 3 + J) as the callback sees them, x, fun, nit, nfev, spread.
The archive is written with fixed timestamps: running the tool again gives the identical file.  At most a quarter of all draws may
be redraws, or the tool fails.
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scaled_fpca_cases as sc  # noqa: E402
from morphablegraphs_amd import scaled_fpca as sf  # noqa: E402

RECONSTRUCTIONS = ("base", "n2_npc1", "weight_bounds", "constant_joint")
FIRST_SEED = 20240


def reference_steps_1_to_3(quat_coeffs, weights, npc):
    """objective_functions.py:49-69, statement for statement."""
    from sklearn.decomposition import PCA
    dims = quat_coeffs.shape[2]
    n_joints = (dims - sf.LEN_CARTESIAN) // sf.LEN_QUAT
    extended_weights = np.zeros(dims)
    extended_weights[:sf.LEN_CARTESIAN] = weights[:sf.LEN_CARTESIAN]
    for i in range(n_joints):
        extended_weights[sf.LEN_CARTESIAN + i * sf.LEN_QUAT: sf.LEN_CARTESIAN + (i + 1) * sf.LEN_QUAT] = weights[sf.LEN_CARTESIAN + i]
    weight_mat = np.diag(extended_weights)
    weighted_quat_coeffs = np.dot(quat_coeffs, weight_mat)
    pca = PCA(n_components=npc)
    projection = pca.fit_transform(weighted_quat_coeffs.reshape(len(quat_coeffs), -1))
    backprojection = pca.inverse_transform(projection)
    inv_weight_mat = np.linalg.inv(weight_mat)
    return np.dot(backprojection.reshape(quat_coeffs.shape), inv_weight_mat)


def host_errors(c, coeffs, weights, perm=None):
    sk = sc.skeleton()
    design = sf.sampled_design(sc.knots_of(c), c["F"], c["step"])
    data = coeffs if perm is None else coeffs[perm]
    return sf.sfpca_errors_host(data, weights, c["npc"], sk, design, sc.joints_of(c))


def spread_of(c, coeffs, weights, recorded, seed):
    rng = np.random.default_rng(seed + 7919)
    worst = 0.0
    for _ in range(3):
        worst = max(worst, float(np.max(np.abs(host_errors(c, coeffs, weights, rng.permutation(len(coeffs))) - recorded))))
    return worst


def draw_with_gap(c, seed):
    redraws = 0
    while True:
        coeffs, weights = sc.draw(c, seed)
        gaps = sc.relative_gaps(coeffs, weights, c["npc"])
        if np.all(gaps >= sc.MIN_GAP):
            return coeffs, weights, gaps, seed, redraws
        seed, redraws = seed + 1000, redraws + 1


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scaled_fpca.npz"))
    args = ap.parse_args()
    out = {}
    draws = redraws_total = 0
    sk = sc.skeleton()
    for i, c in enumerate(sc.CASES + [sc.OPTIMISER_CASE]):
        coeffs, weights, gaps, seed, redraws = draw_with_gap(c, FIRST_SEED + i)
        draws, redraws_total = draws + 1 + redraws, redraws_total + redraws
        design = sf.sampled_design(sc.knots_of(c), c["F"], c["step"])
        joints = sc.joints_of(c)
        recorded = host_errors(c, coeffs, weights)
        recon = [reference_steps_1_to_3(coeffs, w, c["npc"]) for w in weights]
        sk_errors = np.array([sf.reconstruction_error_host(coeffs, r, sk, design, joints) for r in recon])
        pre = c["name"] + "_"
        out.update({pre + "seed": seed, pre + "redraws": redraws, pre + "digest": sc.digest(coeffs, weights), pre + "gaps": gaps,
                    pre + "sk_errors": sk_errors, pre + "host_errors": recorded, pre + "spread": spread_of(c, coeffs, weights, recorded, seed)})
        if c["name"] in RECONSTRUCTIONS:
            out[pre + "sk_reconstruction"] = recon[min(1, len(recon) - 1)]
        print("%-16s seed %d redraws %d  min gap %.3g  spread %.3g  |host - sklearn| %.3g" % (c["name"], seed, redraws, gaps.min(), out[pre + "spread"],
                                                                                         np.max(np.abs(recorded - sk_errors))))
        if c["name"] == "optimiser":
            from scipy.optimize import minimize
            iterates = []
            res = minimize(lambda w: float(sf.sfpca_errors_host(coeffs, w, c["npc"], sk, design, joints)[0]), np.ones(sc.N_WEIGHTS),
                           bounds=tuple((sf.WEIGHT_LOWER_BOUND, None) for _ in range(sc.N_WEIGHTS)), method="SLSQP",
                           options={"maxiter": sf.MAX_ITERATIONS}, callback=lambda x: iterates.append(np.array(x)))
            out.update({pre + "iterates": np.array(iterates), pre + "x": res.x, pre + "fun": float(res.fun), pre + "nit": int(res.nit),
                        pre + "nfev": int(res.nfev), pre + "start_fun": float(recorded[0])})
            print("  SLSQP: %d iterations, %d values, %.6g -> %.6g (%s)" % (res.nit, res.nfev, recorded[0], res.fun, res.message))
    assert 4 * redraws_total <= draws, "%d of %d draws were redraws" % (redraws_total, draws)
    write_npz(args.out, out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
