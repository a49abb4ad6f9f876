"""Writes tests/golden/fpca.npz: what the reference's functional PCA (construction/fpca: FunctionalData, PCAFunctionalData,
FPCASpatialData, FPCATimeSemantic, run_pca) and the dimension-reduction stages of MotionModelConstructor do on small
synthetic sets of aligned motions, with, per quantity, the reference's own sensitivity to the order of its rows and to
ARPACK's start vector.

    python tools/gen_fpca_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--out tests/golden/fpca.npz]

fpca/utils.py, functional_data.py, pca_functional_data.py, fpca_spatial_data.py, fpca_time_semantic.py and
construction/utils.py are imported unmodified under a synthetic parent package; `transformations` and `anim_utils` are
stubs, np.float is set to float in this process (fpca_time_semantic uses it), prints are discarded.  svds is wrapped (the
module's name, not its file) so that the singular values run_pca sees are recorded.

Cases (kind): spatial (PCAFunctionalData through FPCASpatialData), temporal (FPCATimeSemantic.functional_pca), construct
(normalize_root_translation, align_quaternion_frames, the spatial and temporal fits, scale_root_translation_in_fpca_data:
the stages of run_dimension_reduction, each recorded).  Per case `c<i>_`: name, kind, input, n_basis, fraction, n_pc (-1:
None), functional_data, mean, singular_values (the k = min - 1 that svds computes), npc, eigenvectors and low_vecs (signs
fixed by our rule: each row's entry of largest magnitude positive), backprojection (low_vecs . eigenvectors + mean),
resolved (per eigenvector: its relative gaps to both neighbours are at least 1e-6), seed, redraws, rows_rejected (warping
functions thrown away while the input was drawn: [frame-index rows with an increment below 4e-3, frame-index rows that needed
no repair, plain rows], see warping_functions); for every float quantity
spread_<q>: the largest difference from the recorded run (eigenvectors: over the resolved rows) over 3 reruns, each on another
row permutation and another seed of np.random (un-permuted, sign-fixed).  A case is drawn again with the next seed when
two of its first npc + 2 singular values lie within 1e-6 (relative to the largest), when the cumulated variance at npc lies within 1e-9 of the fraction, or
when a rerun's npc differs.  At most a quarter of all draws may be redraws, or the tool fails.
The archive is written with fixed timestamps, so running the tool again gives the identical file.
"""
import argparse
import collections
import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP, NPC_MARGIN = 1e-6, 1e-9
RECORD = {}


def load_reference(reference):
    np.float = float
    for name in ("transformations", "anim_utils", "anim_utils.animation_data", "anim_utils.animation_data.motion_distance"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["transformations"].quaternion_matrix = sys.modules["transformations"].quaternion_from_matrix = None
    sys.modules["anim_utils.animation_data.motion_distance"].convert_quat_frame_to_point_cloud = None
    base = os.path.join(reference, "morphablegraphs", "construction")
    for name in ("mgref", "mgref.construction", "mgref.construction.fpca"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    mods = {"cutils": load("mgref.construction.utils", os.path.join(base, "utils.py"))}
    for m in ("utils", "functional_data", "pca_functional_data", "fpca_spatial_data", "fpca_time_semantic"):
        mods[m] = load("mgref.construction.fpca." + m, os.path.join(base, "fpca", m + ".py"))
    svds = mods["utils"].svds

    def svds_and_record(A, k):
        U, D, Vt = svds(A, k)
        RECORD["D"] = np.sort(D)[::-1].copy()
        return U, D, Vt
    mods["utils"].svds = svds_and_record
    return mods


def sign_of_rows(Vt):
    return np.array([1.0 if row[np.argmax(np.abs(row))] >= 0 else -1.0 for row in Vt])


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


# ---- one run of the reference per kind; returns {quantity: array} with rows in the order of `data` -----------------------
def run_spatial(mods, data, n_basis, fraction, n_pc, perm):
    with quiet():
        fs = mods["fpca_spatial_data"].FPCASpatialData(n_basis, n_pc, fraction)
        fs.fit(data[perm])
    obj = fs.fpcaobj
    inv = np.argsort(perm)
    sg = sign_of_rows(obj.eigenvectors)
    D = RECORD["D"]
    sumvar = np.cumsum(D ** 2) / np.sum(D ** 2)
    npc = int(np.searchsorted(sumvar, fraction) + 1)
    low = np.asarray(obj.low_vecs)
    return {"functional_data": obj.functional_data[inv], "mean": obj.mean, "singular_values": D, "npc": npc,
            "eigenvectors": obj.eigenvectors * sg[:, None], "low_vecs": low[inv] * sg[None, :],
            "backprojection": obj.backproject_data(low)[inv], "_sumvar": sumvar}


def run_temporal(mods, data, n_basis, fraction, n_pc, perm):
    with quiet():
        ft = mods["fpca_time_semantic"].FPCATimeSemantic(n_basis, n_components_temporal=n_pc, precision_temporal=fraction)
        ft.temporal_semantic_data = np.array(data[perm])
        ft.semantic_annotation_list = []
        ft.functional_data_representation()
        fd = np.array(ft.fpca_data)
        ft.functional_pca()
    inv = np.argsort(perm)
    sg = sign_of_rows(ft.eigenvectors)
    D = RECORD["D"]
    sumvar = np.cumsum(D ** 2) / np.sum(D ** 2)
    low = np.asarray(ft.lowVs)
    return {"functional_data": fd[inv], "mean": ft.mean_vec, "singular_values": D, "npc": int(ft.npc),
            "eigenvectors": ft.eigenvectors * sg[:, None], "low_vecs": low[inv] * sg[None, :],
            "backprojection": (np.dot(low, ft.eigenvectors) + ft.mean_vec)[inv], "_sumvar": sumvar}


def run_construct(mods, case, perm):
    """The stages of run_dimension_reduction; the first motion (the quaternion reference frame) stays first."""
    frames, warps, cfg, n_joints = case["input"], case["warps"], case["config"], case["n_joints"]
    cu = mods["cutils"]
    keys = ["m%03d" % i for i in perm]
    aligned = collections.OrderedDict((k, frames[i].copy()) for k, i in zip(keys, perm))
    skeleton = types.SimpleNamespace(animated_joints=list(range(n_joints)))
    with quiet():
        scaled, scale_vec = cu.normalize_root_translation(aligned)
        smoothed = cu.align_quaternion_frames(skeleton, scaled)
    prepared = np.array(list(smoothed.values()))
    n_basis = int(frames.shape[1] * cfg["n_spatial_basis_factor"])
    identity = np.arange(len(perm))
    sp = run_spatial(mods, prepared, n_basis, cfg["fraction"], cfg["n_components"], identity)
    inv = np.argsort(perm)
    mean, eig = cu.scale_root_translation_in_fpca_data(sp["mean"].copy(), sp["eigenvectors"].copy(), scale_vec, n_basis, frames.shape[2])
    tp = run_temporal(mods, warps[perm], cfg["n_basis_functions_temporal"], cfg["precision_temporal"], cfg["npc_temporal"], identity)
    out = {"scale_vec": np.asarray(scale_vec, dtype=np.float64), "prepared": prepared[inv], "scaled_mean": mean, "scaled_eigenvectors": eig,
           "scaled_backprojection": (np.dot(sp["low_vecs"], eig) + mean)[inv],
           "motion_parameters": np.concatenate((sp["low_vecs"], tp["low_vecs"]), axis=1)[inv]}
    for k, v in sp.items():
        out[k] = v[inv] if k in ("functional_data", "low_vecs", "backprojection") else v
    for k, v in tp.items():
        out["t_" + k] = v[inv] if k in ("functional_data", "low_vecs", "backprojection") else v
    return out


# ---- synthetic aligned motions -----------------------------------------------------------------------------------------------
def smooth_motions(rng, n, n_frames, n_dims, n_modes=6, noise=0.02):
    t = np.linspace(0.0, 1.0, n_frames)
    modes = np.stack([np.sin((k + 1) * np.pi * t + rng.uniform(0, np.pi)) for k in range(n_modes)])      # (modes, F)
    mix = rng.standard_normal((n_modes, n_dims))
    latent = rng.standard_normal((n, n_modes)) * (0.6 ** np.arange(n_modes))
    base = rng.standard_normal(n_dims)[None, None, :] + np.cos(2 * np.pi * t)[None, :, None] * rng.standard_normal(n_dims)[None, None, :]
    data = base + np.einsum("nk,kf,kd->nfd", latent, modes, mix) + np.einsum("nk,kf,kd->nfd", latent ** 2, modes[::-1], mix * 0.3)
    return data + noise * rng.standard_normal((n, n_frames, n_dims))


MIN_INCREMENT = 4e-3


def warping_functions(rng, mods, n, n_frames, n_repaired, n_basis=8):
    """n warping functions, the first n_repaired of them frame indices with runs of repeated values whose control points the
    reference's monotonic repair has to break up.  The repair leaves increments anywhere in (0, 0.01], and log(increment)
    moves by delta / increment when a control point moves by delta: two correct least-squares solvers differ by a few ulp
    of the control points (up to F - 1 = 39: delta about 2e-14), and the rule's floor for this quantity is 1e-12 max|q| with
    max|q| = log(F) .. 8, about 6e-12.  So a row is kept only if its smallest increment is at least MIN_INCREMENT (4e-3 >
    2e-14 / 6e-12); a row that each run fits alone shows none of this in the spread over row permutations.  Rows thrown away
    are counted (they are outside the redraw accounting of whole cases) and recorded per case as rows_rejected."""
    w, rejected = [], [0, 0, 0]       # rows thrown away: frame-index rows below MIN_INCREMENT, frame-index rows that needed no repair, plain rows
    while len(w) < n:
        steps = np.exp(0.35 * np.cumsum(rng.standard_normal(n_frames - 1)) * 0.3 + 0.2 * rng.standard_normal(n_frames - 1))
        f = np.concatenate([[0.0], np.cumsum(steps)])
        f = f / f[-1] * (n_frames - 1) * rng.uniform(0.7, 1.3)
        repaired = len(w) < n_repaired
        if repaired:
            f = np.floor(f)
            f[:3] = 0.0
        with quiet():
            ft = mods["fpca_time_semantic"].FPCATimeSemantic(n_basis)
            ft.temporal_semantic_data = np.array([f])
            ft.functional_data_representation()
        smallest = float(np.exp(np.min(ft.fpca_data)))
        if (MIN_INCREMENT <= smallest <= 0.01 + 1e-9) if repaired else smallest >= 0.05:
            w.append(f)
        else:
            rejected[(0 if smallest < MIN_INCREMENT else 1) if repaired else 2] += 1
    return np.array(w)[rng.permutation(n)], rejected


def quaternion_motions(rng, n, n_frames, n_joints, root_scale):
    data = smooth_motions(rng, n, n_frames, 3 + 4 * n_joints, noise=0.01)
    data[:, :, :3] *= root_scale
    for j in range(n_joints):
        q = data[:, :, 3 + 4 * j:7 + 4 * j] * 0.2 + np.array([1.0, 0.0, 0.0, 0.0])
        q /= np.linalg.norm(q, axis=2, keepdims=True)
        flip = rng.random((n, n_frames)) < 0.3
        flip[0, 0] = False
        q[flip] *= -1
        data[:, :, 3 + 4 * j:7 + 4 * j] = q
    return data


def draw(mods, i, seed):
    rng = np.random.default_rng(7000 + 100 * i + seed)
    if i == 0:
        return {"name": "spatial_n60_f47_d11", "kind": "spatial", "input": smooth_motions(rng, 60, 47, 11), "n_basis": 9, "fraction": 0.95, "n_pc": None}
    if i == 1:
        return {"name": "spatial_tall_n120_f20_d3", "kind": "spatial", "input": smooth_motions(rng, 120, 20, 3, noise=0.05), "n_basis": 6,
                "fraction": 0.99, "n_pc": None}
    if i == 2:
        return {"name": "spatial_npc5_n40_f30_d7", "kind": "spatial", "input": smooth_motions(rng, 40, 30, 7), "n_basis": 7, "fraction": 0.95, "n_pc": 5}
    if i == 3:
        w, rejected = warping_functions(rng, mods, 50, 40, 0)
        return {"name": "temporal_n50_f40", "kind": "temporal", "input": w, "rows_rejected": rejected, "n_basis": 8, "fraction": 0.99, "n_pc": None}
    if i == 4:
        w, rejected = warping_functions(rng, mods, 30, 40, 6)
        return {"name": "temporal_repair_n30_f40", "kind": "temporal", "input": w, "rows_rejected": rejected, "n_basis": 8, "fraction": 0.95,
                "n_pc": None}
    frames = quaternion_motions(rng, 40, 30, 2, 1e2)
    w, rejected = warping_functions(rng, mods, 40, 30, 5)
    return {"name": "construct_n40_f30_j2", "kind": "construct", "input": frames, "warps": w, "rows_rejected": rejected, "n_joints": 2, "n_basis": 9, "fraction": 0.95, "n_pc": None,
            "config": {"n_spatial_basis_factor": 0.3, "n_components": None, "fraction": 0.95, "n_basis_functions_temporal": 8,
                       "npc_temporal": None, "precision_temporal": 0.99}}


N_CASES = 6


def run(mods, case, perm, seed):
    np.random.seed(seed)
    if case["kind"] == "construct":
        return run_construct(mods, case, perm)
    fn = run_spatial if case["kind"] == "spatial" else run_temporal
    return fn(mods, case["input"], case["n_basis"], case["fraction"], case["n_pc"], perm)


def resolved_rows(D, n_rows):
    """Per leading singular vector: both relative gaps (s_i - s_{i+1}) / s_1 to its neighbours are at least GAP (the last
    computed value has an uncomputed neighbour: not resolved)."""
    gaps = (D[:-1] - D[1:]) / D[0]
    ok = np.zeros(n_rows, dtype=bool)
    for r in range(n_rows):
        ok[r] = r < len(gaps) and gaps[r] >= GAP and (r == 0 or gaps[r - 1] >= GAP)
    return ok


def check_draw(res, fraction, prefix=""):
    D, npc, sumvar = res[prefix + "singular_values"], int(res[prefix + "npc"]), res[prefix + "_sumvar"]
    lead = D[:min(len(D), npc + 2)]
    if np.any((lead[:-1] - lead[1:]) / D[0] < GAP):
        return "close singular values among the first npc + 2"
    if abs(sumvar[npc - 1] - fraction) <= NPC_MARGIN or (npc >= 2 and abs(sumvar[npc - 2] - fraction) <= NPC_MARGIN):
        return "cumulated variance within %g of the fraction" % NPC_MARGIN
    return None


def _write_npz(path, arrays):
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
    ap.add_argument("--reference", required=True, help="a checkout of dfki-asr/morphablegraphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fpca.npz"))
    args = ap.parse_args()
    mods = load_reference(args.reference)
    out, names = {}, []
    draws = redraws_total = 0
    for i in range(N_CASES):
        redraws = 0
        for seed in range(10):
            draws += 1
            case = draw(mods, i, seed)
            n = len(case["input"])
            identity = np.arange(n)
            res = run(mods, case, identity, 100 + seed)
            why = check_draw(res, case["fraction"])
            if why is None and case["kind"] == "construct":
                why = check_draw(res, case["config"]["precision_temporal"], "t_")
            floats = [k for k, v in res.items() if "_sumvar" not in k and not k.endswith("npc")]
            spread = dict.fromkeys(floats, 0.0)
            prng = np.random.default_rng(900 + 10 * i + seed)
            for rerun in range(3):
                if why is not None:
                    break
                perm = prng.permutation(n)
                if case["kind"] == "construct":       # the first motion holds the frame every quaternion is aligned to
                    perm = np.concatenate([[0], 1 + prng.permutation(n - 1)])
                again = run(mods, case, perm, 200 + 10 * seed + rerun)
                if any(int(again[k]) != int(res[k]) for k in res if k.endswith("npc")):
                    why = "npc differs in a rerun"
                    break
                for k in floats:
                    diff = np.abs(again[k] - res[k])
                    if k.endswith("eigenvectors"):      # rows that ARPACK resolves only
                        D = res["t_singular_values" if k.startswith("t_") else "singular_values"]
                        diff = diff[resolved_rows(D, len(diff))]
                    spread[k] = max(spread[k], float(np.max(diff)) if diff.size else 0.0)
            if why is None:
                break
            print("%s: seed %d: %s; next seed" % (case["name"], seed, why))
            redraws += 1
            redraws_total += 1
        else:
            raise RuntimeError("case %d: no seed passes the redraw rules" % i)
        p = "c%d_" % i
        names.append(case["name"])
        out.update({p + "name": np.array(case["name"]), p + "kind": np.array(case["kind"]), p + "input": case["input"],
                    p + "n_basis": np.int64(case["n_basis"]), p + "fraction": np.float64(case["fraction"]),
                    p + "n_pc": np.int64(-1 if case["n_pc"] is None else case["n_pc"]), p + "seed": np.int64(seed), p + "redraws": np.int64(redraws)})
        out[p + "rows_rejected"] = np.array(case.get("rows_rejected", [0, 0, 0]), dtype=np.int64)
        if case["kind"] == "construct":
            out.update({p + "warps": case["warps"], p + "n_joints": np.int64(case["n_joints"]),
                        p + "config_keys": np.array(sorted(case["config"])),
                        p + "config_values": np.array([np.nan if case["config"][k] is None else case["config"][k] for k in sorted(case["config"])])})
        for k, v in res.items():
            if "_sumvar" in k:
                continue
            out[p + k] = np.int64(v) if k.endswith("npc") else np.asarray(v, dtype=np.float64)
            if k in spread:
                out[p + "spread_" + k] = np.float64(spread[k])
        out[p + "resolved"] = resolved_rows(res["singular_values"], len(res["eigenvectors"]))
        if case["kind"] == "construct":
            out[p + "t_resolved"] = resolved_rows(res["t_singular_values"], len(res["t_eigenvectors"]))
        print("%-28s seed %d redraws %d rows rejected %s npc %d rows %d  spread: eigenvectors %.2e low_vecs %.2e singular_values %.2e functional_data %.2e" % (
            case["name"], seed, redraws, case.get("rows_rejected", [0, 0, 0]), int(res["npc"]), len(res["eigenvectors"]), spread["eigenvectors"], spread["low_vecs"],
            spread["singular_values"], spread["functional_data"]))
    if 4 * redraws_total > draws:
        raise RuntimeError("%d of %d draws redrawn: more than a quarter" % (redraws_total, draws))
    out.update({"names": np.array(names), "draws": np.int64(draws), "redraws": np.int64(redraws_total)})
    _write_npz(args.out, out)
    print("draws %d, redraws %d" % (draws, redraws_total))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
