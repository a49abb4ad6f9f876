"""The model-construction kernels at their shape boundaries.

mg_fpca.hip (the f64 MFMA GEMM behind spline fit / project / back-project, the Jacobi PCA), mg_gmm_em.hip (the trainer's EM),
mg_kmeans.hip, mg_dtw.hip and mg_segment.hip are pinned to golden fixtures elsewhere; the tables below walk the kernels' own
boundaries instead -- every template instance, tile edge, k-tail, bye, grid.y split and LDS limit -- on seeded synthetic data
generated here, each family against a reference that is not the code under test, with tolerances taken from the project's
existing rules (close / check_grid / _inertia_ok) or from a derivable rounding bound.

LEDGER records the (family, boundary) entries that ran and matched; test_the_ledger_covers_every_boundary fails when a row
stops exercising what it was put in the table for (a kernel that declines a shape is a failure, not a skip).  The two CPU
tests restate every dispatch / limit formula next to the source line it restates, assert the tables straddle each boundary,
and assert the input-quality conditions (gaps, margins, iteration counts) on the references alone.

Two places where the tables differ from a literal reading of the sweep's brief, both forced by documented limits:
  * k-means: mg_kmeans_segments documents 2 <= k <= 64 (k = 1 is MG_ERR_UNSUPPORTED, asserted in
    test_gpu_cluster_tree_build.py), so the lower edge in the table is k = 2; the segment of 5 positions needs k <= 5.
  * PCA: "at least two resolved vectors" cannot hold where min(n, p) - 1 < 2 (the criterion never resolves the last value):
    the inputs test asserts min(2, min(n, p) - 1).
Nothing was shrunk: the 1024 x 1024 x 64 grid is compared with the host restatement in every cell (about 15 s of NumPy with
the three runs that measure its spread).
"""
import math
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dtw_host import FLOOR as GRID_FLOOR, MARGIN as GRID_MARGIN, same_bits  # noqa: E402
from test_fpca_host import FACTOR, FLOOR, close  # noqa: E402

from morphablegraphs_amd import _capi, dtw, fpca  # noqa: E402
from morphablegraphs_amd import gmm_trainer as gt  # noqa: E402
from morphablegraphs_amd import segmentation as seg  # noqa: E402

T0 = time.time()

# ---- the dispatch and limit formulas, restated (kept in step with the sources by test_tables_straddle_every_boundary) ------------
EM_BLOCK, EM_NSLOT, EM_TILE, EM_MAX_D, EM_MAX_K = 256, 16, 32, 64, 64
FP_BLOCK, FP_MAX_BASIS, FP_MAX_FRAMES, GRID_Y = 256, 64, 1024, 65535
MG_KM_BLOCK, MG_KM_ACC, MG_KM_MAX_DIM, MG_KM_MAX_K = 256, 8, 128, 64
DTW_TILE, DTW_CODE_LDS_BYTES, DTW_MAX_FRAMES, DTW_MAX_JOINTS = 16, 96 * 1024, 1024, 64
SEG_FRAMES, SEG_MAX_KEYFRAMES = 64, 8


def em_dp(d):
    """mg_gmm_em_fit: the em_estep_kernel instance."""
    return 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64


def jacobi_mp(m):
    """mg_pca_fit: players of the round-robin schedule (an odd m gets a bye)."""
    return m + (m & 1)


def gemm_launches(batch):
    return (batch + GRID_Y - 1) // GRID_Y


def paths_in_lds(fr, f_max):
    """mg_dtw_paths: the back-step codes (one 32-bit word per 16 cells of a row) stay in the LDS."""
    return fr * ((f_max + 15) // 16) * 4 <= DTW_CODE_LDS_BYTES


LEDGER = set()
RATIOS = {}
_DONE = set()       # families (or rows) attempted: the ledger test runs what is left, and nothing twice


def _note(family, what):
    LEDGER.add((family, what))


def _ratio(family, err, bound):
    """Records error / bound (0 / 0 counts as 0); returns it."""
    r = 0.0 if err == 0.0 else (float("inf") if bound == 0.0 else float(err) / float(bound))
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    return r


def _close(family, name, ours, ref, spread):
    """test_fpca_host.close, with the ratio recorded first."""
    ours, ref = np.asarray(ours, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size and ours.shape == ref.shape:
        _ratio(family, float(np.max(np.abs(ours - ref))), FACTOR * max(float(spread), FLOOR * float(np.max(np.abs(ref)))))
    close(name, ours, ref, spread)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# =================================================================================================================================
# 1. GEMM
# =================================================================================================================================
# (n_basis, F, D, motions)
SPLINE_SHAPES = [
    (1, 1, 1, 3), (1, 5, 3, 2), (4, 4, 15, 3), (4, 5, 1, 5), (4, 6, 3, 2), (4, 9, 16, 2), (4, 13, 17, 2), (16, 16, 3, 2), (16, 47, 79, 3),
    (17, 17, 1, 2), (17, 256, 16, 2), (17, 1023, 15, 1), (33, 33, 3, 2), (33, 47, 17, 2), (33, 1024, 79, 1), (64, 64, 15, 2), (64, 256, 1, 2),
    (64, 1023, 17, 1), (64, 1024, 79, 2),
]
SPLINE_BATCH = dict(n_basis=4, F=5, D=1, n=GRID_Y + GRID_Y + 3)
PROJECT_L, PROJECT_P, PROJECT_N = (1, 15, 16, 17), (None, 33, 257, 2449), (1, 16, 17, 300)      # p None: p = l
PROJECT_SHAPES = [(l, l if p is None else p, n) for l in PROJECT_L for p in PROJECT_P for n in PROJECT_N]


def spline_operator(n_basis, n_frames):
    """fpca.spline_fit_operator where the reference's cubic knot vector exists (n_basis >= 4); below that a seeded row
    operator (the kernel is a plain product either way)."""
    if n_basis >= 4:
        return fpca.spline_fit_operator(n_basis, n_frames)[0], True
    return np.random.default_rng(900 + n_basis * 7 + n_frames).standard_normal((n_basis, n_frames)), False


def spline_motions(n_basis, F, D, n):
    rng = np.random.default_rng(1000 + 31 * n_basis + 7 * F + D)
    return rng.standard_normal((n, F, D)) * np.exp(rng.uniform(-2.0, 2.0, (1, 1, D)))


def gemm_reference(A, B, bias=None):
    """(reference in numpy.longdouble rounded to float64, the bound K 2^-52 sum_k |a_ik| |b_kj| + 2^-53 |c|) of A . B (+ bias)."""
    c = np.matmul(A.astype(np.longdouble), B.astype(np.longdouble))
    if bias is not None:
        c = c + bias.astype(np.longdouble)
    c = c.astype(np.float64)
    mag = np.matmul(np.abs(A), np.abs(B)) + (0.0 if bias is None else np.abs(bias))
    return c, A.shape[-1] * 2.0 ** -52 * mag + 2.0 ** -53 * np.abs(c)


def project_inputs(l, p, n):
    rng = np.random.default_rng(5000 + 101 * l + 3 * p + n)
    return rng.standard_normal((n, p)), rng.standard_normal((l, p)) / math.sqrt(p), rng.standard_normal(p) * 3.0, rng.standard_normal((n, l))


# =================================================================================================================================
# 2. PCA
# =================================================================================================================================
GAP = 1e-6        # tools/gen_fpca_golden.py


def _pca(n, p, centre=True, kind="plain"):
    return dict(name="n%d_p%d%s%s" % (n, p, "" if centre else "_raw", "" if kind == "plain" else "_" + kind), n=n, p=p, centre=centre, kind=kind)


PCA_SHAPES = [
    _pca(1, 5), _pca(2, 9, centre=False), _pca(3, 3), _pca(5, 5), _pca(61, 300), _pca(7, 1000), _pca(33, 2449),
    _pca(300, 33, centre=False), _pca(1000, 7), _pca(257, 255), _pca(129, 129),
    _pca(12, 40, kind="duplicates"),         # rows 9, 10, 11 = row 0: with the centring four rows without a direction
    _pca(50, 6, kind="constant"),            # column 2 constant
]
PCA_IDS = [c["name"] for c in PCA_SHAPES]


def resolved_rows(s, n_rows):
    """tools/gen_fpca_golden.py: both relative gaps (s_i - s_{i+1}) / s_1 to the neighbours are at least GAP; the last
    computed value has an uncomputed neighbour and is not resolved."""
    ok = np.zeros(n_rows, dtype=bool)
    if len(s) < 2 or not s[0] > 0:
        return ok
    gaps = (s[:-1] - s[1:]) / s[0]
    for r in range(n_rows):
        ok[r] = r < len(gaps) and gaps[r] >= GAP and (r == 0 or gaps[r - 1] >= GAP)
    return ok


def pca_matrix(c):
    n, p = c["n"], c["p"]
    rng = np.random.default_rng(2000 + 13 * n + p)
    m = min(n, p)
    s = 10.0 / (1.0 + np.arange(m))
    U, V = np.linalg.qr(rng.standard_normal((n, m)))[0], np.linalg.qr(rng.standard_normal((p, m)))[0]
    A = (U * s) @ V.T + 3.0 * rng.standard_normal(p)
    if c["kind"] == "duplicates":
        A[-3:] = A[0]
    elif c["kind"] == "constant":
        A[:, 2] = 0.7
    return np.ascontiguousarray(A)


_PCA_REF = {}


def pca_reference(c):
    """LAPACK's fit (fpca.pca_fit_host), its change under three row permutations, its orthonormality, the resolved rows."""
    if c["name"] in _PCA_REF:
        return _PCA_REF[c["name"]]
    A = pca_matrix(c)
    host = fpca.pca_fit_host(A, centre=c["centre"])
    m = min(A.shape)
    ok = resolved_rows(host["singular_values"], m)
    rng = np.random.default_rng(77 + A.shape[0])
    spread_s = spread_v = 0.0
    for _ in range(3):
        again = fpca.pca_fit_host(A[rng.permutation(len(A))], centre=c["centre"])
        spread_s = max(spread_s, float(np.max(np.abs(again["singular_values"] - host["singular_values"]))))
        if ok.any():
            spread_v = max(spread_v, float(np.max(np.abs(again["vt"][ok] - host["vt"][ok]))))
    _, _, Vt = np.linalg.svd(host["centred"], full_matrices=False)
    ref = dict(A=A, host=host, resolved=ok, spread_s=spread_s, spread_v=spread_v, lapack_orth=float(np.max(np.abs(Vt @ Vt.T - np.eye(m)))))
    _PCA_REF[c["name"]] = ref
    return ref


# =================================================================================================================================
# 3. EM
# =================================================================================================================================
def _em(d, n, Ks, sep, long_run=False):
    return dict(name="d%d_n%d_K%s" % (d, n, "_".join(str(k) for k in Ks)), d=d, n=n, Ks=list(Ks), sep=sep, long_run=long_run)


# sep: the spread of the component centres in units of the noise; small = overlapping clusters (many iterations)
EM_SHAPES = [
    _em(1, 15, (1, 2), 6.0),
    _em(8, 16, (1,), 6.0),
    _em(8, 1000, (1, 2, 8), 0.8, long_run=True),
    _em(9, 255, (2,), 2.0),
    _em(16, 256, (1, 2), 2.0),
    _em(16, 1000, (2, 8), 0.6, long_run=True),
    _em(17, 257, (2,), 2.0),
    _em(24, 513, (2,), 1.0),
    _em(32, 1000, (1, 2, 8), 0.5, long_run=True),
    _em(33, 513, (2,), 2.0),
    _em(64, 255, (1,), 2.0),
    _em(64, 1000, (1, 2), 0.35, long_run=True),
    _em(2, 1300, (63, 64), 6.0),
]
EM_IDS = [c["name"] for c in EM_SHAPES]
EM_KEYS = ("weights", "means", "covariances", "precisions_cholesky", "lower_bounds", "score")
EM_TOL = 1e-3


def em_inputs(c):
    """X (n, d) and one initial label array per K: the nearest of the first K generating centres (every label in use)."""
    d, n, Ks = c["d"], c["n"], c["Ks"]
    rng = np.random.default_rng(3000 + 17 * d + n)
    kmax = max(Ks)
    if kmax >= 63:
        side = int(math.ceil(math.sqrt(kmax)))
        centres = np.zeros((kmax, d))
        centres[:, 0], centres[:, 1] = c["sep"] * (np.arange(kmax) % side), c["sep"] * (np.arange(kmax) // side)
    else:
        centres = c["sep"] * rng.standard_normal((kmax, d))
    comp = np.concatenate([np.arange(kmax), rng.integers(0, kmax, n - kmax)])
    X = centres[comp] + rng.standard_normal((n, d)) * np.exp(rng.uniform(-0.4, 0.4, d))
    labels = []
    for K in Ks:
        dist = ((X[:, None, :] - centres[None, :K, :]) ** 2).sum(axis=2)
        labels.append(np.argmin(dist, axis=1).astype(np.int32))
    return np.ascontiguousarray(X), labels


_EM_REF = {}


def em_reference(c):
    """Per K: the host EM's fit, its spread per quantity over three row permutations, the n_iter of the four runs."""
    if c["name"] in _EM_REF:
        return _EM_REF[c["name"]]
    X, labels = em_inputs(c)
    out = []
    rng = np.random.default_rng(5 + c["d"])
    for K, lab in zip(c["Ks"], labels):
        ref = gt.em_from_labels_host(X, lab, K)
        spread = dict.fromkeys(EM_KEYS, 0.0)
        iters = [ref["n_iter"]]
        for _ in range(3):
            p = rng.permutation(len(X))
            q = gt.em_from_labels_host(X[p], lab[p], K)
            iters.append(q["n_iter"])
            if q["n_iter"] == ref["n_iter"]:
                for key in spread:
                    spread[key] = max(spread[key], float(np.max(np.abs(np.asarray(q[key]) - np.asarray(ref[key])))))
        out.append(dict(ref=ref, spread=spread, iters=iters))
    _EM_REF[c["name"]] = (X, labels, out)
    return _EM_REF[c["name"]]


# =================================================================================================================================
# 4. k-means
# =================================================================================================================================
def _km(dim, k, n, kind="plain"):
    return dict(name="dim%d_k%d_n%d%s" % (dim, k, n, "" if kind == "plain" else "_" + kind), dim=dim, k=k, n=n, kind=kind)


KM_SEGMENTS = (5, 255, 256, 257, 1300)
KM_SHAPES = [
    _km(1, 2, 300), _km(43, 7, 600), _km(44, 8, 600), _km(127, 9, 700), _km(128, 16, 800), _km(43, 63, 2000), _km(1, 64, 1500),
    _km(128, 64, 2000),                      # the largest LDS case
    _km(44, 5, sum(KM_SEGMENTS), kind="segments"),
    _km(3, 5, 300, kind="empty"),
]
KM_IDS = [c["name"] for c in KM_SHAPES]
KM_GAP = 1e-9
KM_TOL, KM_MAX_ITER = 1e-4, 300


def km_inputs(c):
    """(X table, rows permutation, seg_begin, init (segments, k, dim))."""
    dim, k, n = c["dim"], c["k"], c["n"]
    rng = np.random.default_rng(4000 + 11 * dim + k)
    blobs = 3.0 * rng.standard_normal((max(k // 2, 2), dim))
    X = blobs[rng.integers(0, len(blobs), n)] + rng.standard_normal((n, dim))
    if c["kind"] == "segments":
        rows = rng.permutation(n).astype(np.int64)
        seg_begin = np.concatenate([[0], np.cumsum(KM_SEGMENTS)]).astype(np.int64)
    else:
        rows, seg_begin = np.arange(n, dtype=np.int64), np.array([0, n], dtype=np.int64)
    if c["kind"] == "empty":
        # one member far out, then two identical members at the next largest distance (positions 40 < 200): the two empty
        # clusters take the far one and the FIRST of the twins
        X[120] = X.mean(axis=0) + 40.0
        X[40] = X[200] = X.mean(axis=0) - 25.0
    init = np.stack([X[rows[a:b]][rng.permutation(b - a)[:k]] for a, b in zip(seg_begin[:-1], seg_begin[1:])])
    if c["kind"] == "empty":
        init[0, 1], init[0, 3] = 1e3 + np.arange(dim), -1e3 - np.arange(dim)        # nobody's nearest centre
    return np.ascontiguousarray(X), rows, seg_begin, np.ascontiguousarray(init)


def _sqdist(x, C):
    return np.stack([((x - cj) ** 2).sum(axis=1) for cj in C], axis=1)


def _gap(D):
    """Smallest relative difference between a row's two smallest squared distances."""
    if D.shape[1] < 2:
        return np.inf
    two = np.partition(D, 1, axis=1)[:, :2]
    return float(np.min((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)))


def lloyd_reference(x, init, max_iter=KM_MAX_ITER, tol=KM_TOL):
    """The statements of mg_kmeans.hip's header comment in float64 NumPy, for one segment x (n, dim) from the centres init.
    Returns labels, centres, inertia, n_iter and the margins the inputs test asserts: `gap` (assignments), `stop` (the
    relative distance of the summed squared shift from the tolerance, over the iterations), `reloc` (relative distance
    between the distinct values the relocation order compared), `relocated` (members moved to empty clusters)."""
    n, dim = x.shape
    k = len(init)
    C = np.array(init, dtype=np.float64)
    c0 = x - x[0]
    tol_abs = tol * float(np.mean((c0 * c0).sum(axis=0) / n - (c0.sum(axis=0) / n) ** 2))
    labels = np.full(n, -1)
    gap, stop, reloc, relocated = np.inf, np.inf, np.inf, 0
    strict = False
    for it in range(1, max_iter + 1):
        D = _sqdist(x, C)
        gap = min(gap, _gap(D))
        new = np.argmin(D, axis=1)                    # ties: the lowest centre
        dmin = D[np.arange(n), new]
        changed = int(np.count_nonzero(new != labels))
        labels = new
        cnt = np.bincount(labels, minlength=k).astype(np.float64)
        S = np.stack([x[labels == j].sum(axis=0) for j in range(k)])
        empty = np.flatnonzero(cnt == 0)
        if len(empty):
            order = np.lexsort((np.arange(n), -dmin))      # descending distance, the first position on ties
            top = np.unique(dmin[order[:len(empty) + 1]])
            if len(top) > 1:
                reloc = min(reloc, float(np.min(np.diff(top) / top[1:])))
            for e, j_new in enumerate(empty):              # ascending cluster order
                far = order[e]
                j_old = labels[far]
                S[j_old] = S[j_old] - x[far]
                S[j_new] = x[far]
                cnt[j_new], cnt[j_old] = 1.0, cnt[j_old] - 1.0
                relocated += 1
        new_c = np.where(cnt[:, None] > 0, S * (1.0 / np.maximum(cnt, 1.0))[:, None], S)
        shift = float(((new_c - C) ** 2).sum())
        C = new_c
        if changed == 0:
            strict = True
            break
        stop = min(stop, abs(shift - tol_abs) / tol_abs)
        if shift <= tol_abs or it >= max_iter:
            break
    if strict:
        inertia = float(((x - C[labels]) ** 2).sum())
    else:
        D = _sqdist(x, C)
        gap = min(gap, _gap(D))
        labels = np.argmin(D, axis=1)
        inertia = float(D[np.arange(n), labels].sum())
    return dict(labels=labels, centres=C, inertia=inertia, n_iter=it, gap=gap, stop=stop, reloc=reloc, relocated=relocated)


_KM_REF = {}


def km_reference(c):
    if c["name"] not in _KM_REF:
        X, rows, seg_begin, init = km_inputs(c)
        _KM_REF[c["name"]] = (X, rows, seg_begin, init,
                              [lloyd_reference(X[rows[a:b]], init[s]) for s, (a, b) in enumerate(zip(seg_begin[:-1], seg_begin[1:]))])
    return _KM_REF[c["name"]]


# =================================================================================================================================
# 5. DTW and keyframes
# =================================================================================================================================
GRID_J = (1, 2, 19, 63, 64)
GRID_FRAMES = (1, 15, 16, 17, 33)
# (J, weighted, Fr): every J with and without weights, every Fr twice; the motions of a row have every F of GRID_FRAMES
GRID_SHAPES = [(J, w, GRID_FRAMES[(i + 2 * w) % 5]) for i, J in enumerate(GRID_J) for w in (0, 1)]
BIG_GRID = (64, 1024, 1024)
KEY_J, KEY_K, KEY_FRAMES = (1, 19, 64), (1, 7, 8), (1, 63, 64, 65, 200)
PATH_GRIDS = [(768, 512), (768, 513), (1, 1), (1, 9), (9, 1), (16, 16), (17, 33), (64, 64)]
WARP_DIMS = (1, 79, 257)


def clouds_for(J, lengths, seed):
    """Seeded point clouds: a random skeleton pose drifting and turning over the frames."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((J, 3)) * np.array([30.0, 60.0, 30.0])
    out = []
    for F in lengths:
        t = np.linspace(0.0, 1.0, F)[:, None, None] if F > 1 else np.zeros((1, 1, 1))
        ang = rng.uniform(-1.5, 1.5) * t[:, :, 0] + rng.uniform(-3.0, 3.0)
        cloud = np.repeat(base[None], F, axis=0) + 8.0 * rng.standard_normal((F, J, 3)) + t * rng.standard_normal((1, 1, 3)) * 50.0
        x, z = cloud[:, :, 0].copy(), cloud[:, :, 2].copy()
        cloud[:, :, 0], cloud[:, :, 2] = x * np.cos(ang) + z * np.sin(ang), -x * np.sin(ang) + z * np.cos(ang)
        out.append(np.ascontiguousarray(cloud))
    return out


def joint_weights(J, weighted, seed):
    return np.random.default_rng(seed).uniform(0.2, 2.0, J) if weighted else None


def grid_spread(a, b, weights, S, rng):
    """tools/gen_dtw_golden.py spread_of_S on the host restatement: its largest change over 3 reruns with the joints permuted."""
    worst = 0.0
    for _ in range(3):
        perm = rng.permutation(a.shape[1])
        again = dtw.distance_grid_host(a[:, perm], b[:, perm], None if weights is None else weights[perm])
        worst = max(worst, float(np.max(np.abs(again - S))))
    return worst


def check_cells(family, what, ours, host, spread):
    """check_grid's rule: |ours - reference| <= 10 * max(spread, 1e-13 * max|S|); prints the figure before it asserts."""
    err, bound = float(np.max(np.abs(ours - host))), GRID_MARGIN * max(float(spread), GRID_FLOOR * float(np.max(np.abs(host))))
    r = _ratio(family, err, bound)
    print("%s: max |S - host| %.3g, bound %.3g, ratio %.3g" % (what, err, bound, r))
    assert ours.shape == host.shape and err <= bound, (what, err, bound)


def path_grid(fr, f):
    """Integer-valued cells: ties abound."""
    return np.floor(np.random.default_rng(6000 + 3 * fr + f).uniform(0.0, 4.0, (fr, f)))


# =================================================================================================================================
# CPU tests
# =================================================================================================================================
def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "morphablegraphs_amd", "csrc", name)) as f:
        return f.read()


def test_tables_straddle_every_boundary():
    """The formulas restated above match the sources, and the tables have a row on each side of every boundary."""
    em, fp, km, dt, sg = (_source(n) for n in ("mg_gmm_em.hip", "mg_fpca.hip", "mg_kmeans.hip", "mg_dtw.hip", "mg_segment.hip"))
    dev = _source("mg_dtw_device.h")
    # EM
    assert "d <= 8 ? em_estep_kernel<8> : d <= 16 ? em_estep_kernel<16> : d <= 32 ? em_estep_kernel<32> : em_estep_kernel<64>;" in em
    for name, value in (("EM_BLOCK", EM_BLOCK), ("EM_NSLOT", EM_NSLOT), ("EM_TILE", EM_TILE)):
        assert "#define %s %d " % (name, value) in em, name
    assert "#define EM_MAX_D %d\n" % EM_MAX_D in em and "#define EM_MAX_K %d\n" % EM_MAX_K in em
    assert (_capi.MG_GMM_EM_MAX_DIM, _capi.MG_GMM_EM_MAX_K) == (EM_MAX_D, EM_MAX_K)
    assert [em_dp(d) for d in (1, 8, 9, 16, 17, 32, 33, 64)] == [8, 8, 16, 16, 32, 32, 64, 64]
    ds, ns = {c["d"] for c in EM_SHAPES}, {c["n"] for c in EM_SHAPES}
    assert {1, 8, 9, 16, 17, 24, 32, 33, EM_MAX_D} <= ds
    assert {EM_NSLOT - 1, EM_NSLOT, EM_BLOCK - 1, EM_BLOCK, EM_BLOCK + 1, 2 * EM_BLOCK + 1, 1000} <= ns
    for dp in (8, 16, 32, 64):
        rows = [c for c in EM_SHAPES if em_dp(c["d"]) == dp]
        assert any(c["n"] % EM_TILE and c["n"] % EM_BLOCK for c in rows), "DP %d: no ragged n" % dp
        assert any(c["long_run"] for c in rows), "DP %d: no case meant to iterate" % dp
    for d in ds:
        assert any(c["n"] % EM_TILE for c in EM_SHAPES if c["d"] == d), "d = %d: no ragged n" % d
    ks = {k for c in EM_SHAPES for k in c["Ks"]}
    assert {1, 2, 8, EM_MAX_K - 1, EM_MAX_K} <= ks and any(len(c["Ks"]) > 1 for c in EM_SHAPES)
    assert all(c["n"] >= 20 * max(c["Ks"]) for c in EM_SHAPES if max(c["Ks"]) >= 63)
    assert all(c["d"] <= EM_MAX_D and max(c["Ks"]) <= EM_MAX_K and c["n"] >= max(c["Ks"]) for c in EM_SHAPES)
    # Jacobi PCA and the GEMM
    assert "#define FP_BLOCK %d\n" % FP_BLOCK in fp and "#define FP_MAX_BASIS %d\n" % FP_MAX_BASIS in fp and "#define FP_MAX_FRAMES %d\n" % FP_MAX_FRAMES in fp
    assert "const int32_t mp = (int32_t)(m + (m & 1));" in fp and "if (j >= m) return;" in fp
    assert "for (int64_t b0 = 0; b0 < batch; b0 += %d) {" % GRID_Y in fp and "std::min<int64_t>(%d, batch - b0)" % GRID_Y in fp
    assert "const bool wide = n <= p;" in fp
    assert "for (int k0 = 0; k0 < g.K; k0 += 4) {" in fp
    assert (_capi.MG_FPCA_MAX_BASIS, _capi.MG_FPCA_MAX_FRAMES) == (FP_MAX_BASIS, FP_MAX_FRAMES)
    assert [jacobi_mp(m) for m in (1, 2, 3, 4, 257)] == [2, 2, 4, 4, 258]
    short = {min(c["n"], c["p"]) for c in PCA_SHAPES}
    long_ = {max(c["n"], c["p"]) for c in PCA_SHAPES}
    assert {1, 2, 3} <= short and any(m % 2 for m in short if m > 3) and any(m % 2 == 0 for m in short if m > 3)
    assert any(L <= FP_BLOCK for L in long_) and any(L > FP_BLOCK for L in long_) and FP_BLOCK + 1 in long_ and any(L > 2 * FP_BLOCK for L in long_)
    for wide in (True, False):
        rows = [c for c in PCA_SHAPES if (c["n"] <= c["p"]) == wide]
        assert any(min(c["n"], c["p"]) % 2 for c in rows) and any(max(c["n"], c["p"]) > FP_BLOCK for c in rows), wide
    assert any(c["n"] == c["p"] for c in PCA_SHAPES) and sum(not c["centre"] for c in PCA_SHAPES) == 2
    assert any(not c["centre"] and c["n"] > c["p"] for c in PCA_SHAPES) and any(not c["centre"] and c["n"] <= c["p"] for c in PCA_SHAPES)
    assert any(c["kind"] == "duplicates" and c["n"] <= c["p"] for c in PCA_SHAPES) and any(c["kind"] == "constant" and c["n"] > c["p"] for c in PCA_SHAPES)
    nbs, fs, dims = ({s[i] for s in SPLINE_SHAPES} for i in range(3))
    assert {1, 4, 16, 17, 33, FP_MAX_BASIS} <= nbs and {1, 3, 15, 16, 17, 79} <= dims
    assert {5, 9, 13, 47, 256, FP_MAX_FRAMES - 1, FP_MAX_FRAMES} <= fs and {f % 4 for f in fs} == {0, 1, 2, 3}
    assert all(any(nb == f for nb, f, _, _ in SPLINE_SHAPES if nb == b) for b in nbs)             # F = n_basis
    assert {(nb + 15) // 16 for nb in nbs} == {1, 2, 3, 4}
    assert all(1 <= nb <= f <= FP_MAX_FRAMES and nb <= FP_MAX_BASIS for nb, f, _, _ in SPLINE_SHAPES)
    assert any(nb == FP_MAX_BASIS and f == FP_MAX_FRAMES for nb, f, _, _ in SPLINE_SHAPES)
    assert gemm_launches(SPLINE_BATCH["n"]) == 3 and gemm_launches(GRID_Y) == 1 and SPLINE_BATCH["F"] % 4 == 1
    assert {l for l, _, _ in PROJECT_SHAPES} == {1, 15, 16, 17} and {n for _, _, n in PROJECT_SHAPES} == {1, 16, 17, 300}
    assert {p for _, p, _ in PROJECT_SHAPES} >= {1, 15, 16, 17, 33, 257, 2449} and all(l <= p for l, p, _ in PROJECT_SHAPES)
    # k-means
    for name, value in (("MG_KM_BLOCK", MG_KM_BLOCK), ("MG_KM_ACC", MG_KM_ACC)):
        assert "#define %s %d " % (name, value) in km, name
    assert "#define MG_KM_MAX_DIM %d\n" % MG_KM_MAX_DIM in km and "#define MG_KM_MAX_K %d\n" % MG_KM_MAX_K in km
    assert "k >= 2 && k <= MG_KM_MAX_K" in km              # the documented lower limit: the table starts at k = 2
    assert (_capi.MG_KMEANS_MAX_DIM, _capi.MG_KMEANS_MAX_K) == (MG_KM_MAX_DIM, MG_KM_MAX_K)
    assert {1, 43, 44, MG_KM_MAX_DIM - 1, MG_KM_MAX_DIM} <= {c["dim"] for c in KM_SHAPES}
    assert {2, MG_KM_ACC - 1, MG_KM_ACC, MG_KM_ACC + 1, 2 * MG_KM_ACC, MG_KM_MAX_K - 1, MG_KM_MAX_K} <= {c["k"] for c in KM_SHAPES}
    assert any(c["k"] == MG_KM_MAX_K and c["dim"] == MG_KM_MAX_DIM for c in KM_SHAPES)
    assert {5, MG_KM_BLOCK - 1, MG_KM_BLOCK, MG_KM_BLOCK + 1} <= set(KM_SEGMENTS) and max(KM_SEGMENTS) > 4 * MG_KM_BLOCK
    assert any(c["kind"] == "segments" and c["k"] <= min(KM_SEGMENTS) for c in KM_SHAPES) and any(c["kind"] == "empty" for c in KM_SHAPES)
    assert all(2 <= c["k"] <= MG_KM_MAX_K and c["dim"] <= MG_KM_MAX_DIM for c in KM_SHAPES)
    # DTW and keyframes
    assert "#define DTW_TILE %d\n" % DTW_TILE in dt and "#define DTW_CODE_LDS_BYTES (96 * 1024)\n" in dt and "#define DTW_MAX_FRAMES %d\n" % DTW_MAX_FRAMES in dt
    assert "const size_t code_bytes = (size_t)n_ref_frames * wpr_max * 4;" in dt and "const int32_t wpr_max = (f_max + 15) / 16;" in dt
    assert "const bool in_lds = code_bytes <= DTW_CODE_LDS_BYTES;" in dt
    assert "#define DTW_MAX_JOINTS %d\n" % DTW_MAX_JOINTS in dev
    assert "#define SEG_FRAMES %d " % SEG_FRAMES in sg and "#define SEG_MAX_KEYFRAMES %d\n" % SEG_MAX_KEYFRAMES in sg
    assert (_capi.MG_DTW_MAX_FRAMES, _capi.MG_DTW_MAX_JOINTS, _capi.MG_SEGMENT_MAX_KEYFRAMES) == (DTW_MAX_FRAMES, DTW_MAX_JOINTS, SEG_MAX_KEYFRAMES)
    assert {1, 2, 19, DTW_MAX_JOINTS - 1, DTW_MAX_JOINTS} == {J for J, _, _ in GRID_SHAPES}
    for J in GRID_J:
        assert {w for j, w, _ in GRID_SHAPES if j == J} == {0, 1}
    assert {1, DTW_TILE - 1, DTW_TILE, DTW_TILE + 1, 2 * DTW_TILE + 1} == set(GRID_FRAMES) == {fr for _, _, fr in GRID_SHAPES}
    assert BIG_GRID == (DTW_MAX_JOINTS, DTW_MAX_FRAMES, DTW_MAX_FRAMES)
    assert {1, 19, DTW_MAX_JOINTS} == set(KEY_J) and {1, SEG_MAX_KEYFRAMES - 1, SEG_MAX_KEYFRAMES} == set(KEY_K)
    assert {1, SEG_FRAMES - 1, SEG_FRAMES, SEG_FRAMES + 1, 200} == set(KEY_FRAMES)
    assert 768 * 512 == 393216 and paths_in_lds(768, 512) and not paths_in_lds(768, 513) and 768 * ((512 + 15) // 16) * 4 == DTW_CODE_LDS_BYTES
    assert {(768, 512), (768, 513), (1, 1), (1, 9), (9, 1)} <= set(PATH_GRIDS) and any(1 < a <= 64 and 1 < b <= 64 for a, b in PATH_GRIDS)
    assert all(a <= DTW_MAX_FRAMES and b <= DTW_MAX_FRAMES for a, b in PATH_GRIDS) and set(WARP_DIMS) == {1, 79, 257}


def test_inputs_meet_their_conditions():
    """Every condition the GPU families rely on, computed from the references alone."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63          # the GEMM reference carries 11 more bits than the kernel
    for nb, F, D, n in SPLINE_SHAPES:
        P, _ = spline_operator(nb, F)
        assert P.shape == (nb, F) and np.all(np.isfinite(P)) and np.abs(P).max() < 1e6, (nb, F)
    # PCA: NumPy's mean(axis=0) is the row-order sum the kernel's comment promises; enough resolved vectors
    for c in PCA_SHAPES:
        r = pca_reference(c)
        A = r["A"]
        s = np.zeros(A.shape[1])
        for row in A:
            s = s + row
        assert np.array_equal(s / len(A), A.mean(axis=0)), c["name"]
        m = min(A.shape)
        assert int(r["resolved"].sum()) >= min(2, m - 1), (c["name"], int(r["resolved"].sum()))
        print("pca %-22s resolved %3d of %3d  spread s %.2e vt %.2e  LAPACK orth %.2e" % (c["name"], r["resolved"].sum(), m, r["spread_s"], r["spread_v"],
                                                                                        r["lapack_orth"]))
        null = int(np.sum(r["host"]["singular_values"] <= r["host"]["singular_values"][0] * np.finfo(float).eps * max(A.shape)))
        if c["kind"] == "duplicates":
            assert null >= 3 and A.shape[0] <= A.shape[1]
    # EM: n_iter stable under the permutations, a long run per instance, nothing ill-defined, no lower-bound step at the tolerance
    longest = {}
    for c in EM_SHAPES:
        X, labels, fits = em_reference(c)         # (a ValueError here is an ill-defined case)
        for K, lab, f in zip(c["Ks"], labels, fits):
            assert np.bincount(lab, minlength=K).min() >= 2, (c["name"], K)
            assert len(set(f["iters"])) == 1, (c["name"], K, f["iters"])
            lb = f["ref"]["lower_bounds"]
            steps = np.abs(np.diff(np.concatenate([[-np.inf], lb])))
            assert np.all(np.abs(steps - EM_TOL) > 1e-9), (c["name"], K)
            longest[em_dp(c["d"])] = max(longest.get(em_dp(c["d"]), 0), f["ref"]["n_iter"])
            print("em %-22s K %2d  n_iter %3d converged %s" % (c["name"], K, f["ref"]["n_iter"], f["ref"]["converged"]))
    assert all(longest[dp] >= 5 for dp in (8, 16, 32, 64)), longest
    # k-means: the gap condition at every assignment, the stop rule and the relocation order away from their thresholds
    for c in KM_SHAPES:
        _, _, _, _, refs = km_reference(c)
        for s, r in enumerate(refs):
            print("kmeans %-24s segment %d: n_iter %3d gap %.2e stop %.2e relocated %d" % (c["name"], s, r["n_iter"], r["gap"], r["stop"], r["relocated"]))
            assert r["gap"] > KM_GAP and r["stop"] > KM_GAP and r["reloc"] > KM_GAP and r["n_iter"] < KM_MAX_ITER, (c["name"], s)
        if c["kind"] == "empty":
            assert refs[0]["relocated"] == 2 and refs[0]["n_iter"] >= 2
    assert max(r["n_iter"] for c in KM_SHAPES for r in km_reference(c)[4]) >= 5
    # paths: the integer grids do tie
    S = path_grid(17, 33)
    D, _, _ = dtw.dtw_paths_host(S)
    assert np.any(D[:-1, 1:] == D[1:, :-1])


# =================================================================================================================================
# GPU families
# =================================================================================================================================
@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


class _Dev(object):
    """Device buffers freed together."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def up(self, a):
        self.bufs.append(self.ctx.upload(np.ascontiguousarray(a)))
        return self.bufs[-1]

    def new(self, nbytes):
        self.bufs.append(self.ctx.malloc(max(int(nbytes), 8)))
        return self.bufs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def _spline_fit(ctx, motions, P):
    n, F, D = motions.shape
    nb = len(P)
    with _Dev(ctx) as dev:
        m_dev, p_dev, c_dev = dev.up(motions), dev.up(P), dev.new(8 * n * nb * D)
        _capi.spline_fit_batch(ctx, m_dev, n, F, D, p_dev, nb, c_dev)
        return ctx.download(c_dev, (n, nb, D), np.float64)


def _within(family, what, got, ref, bound):
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(err > 0, err / bound, 0.0)))
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    assert got.shape == ref.shape and np.all(err <= bound), "%s: error / bound %.3g at %s" % (
        what, ratio, np.unravel_index(int(np.argmax(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))), err.shape))


def _gemm_spline(ctx, shape):
    nb, F, D, n = shape
    P, from_fpca = spline_operator(nb, F)
    Y = spline_motions(nb, F, D, n)
    got = _spline_fit(ctx, Y, P)
    ref, bound = gemm_reference(P[None], Y)
    _within("gemm", "spline fit %s" % (shape,), got, ref, bound)
    if from_fpca:
        _close("gemm_vs_host", "spline fit %s vs spline_fit_host" % (shape,), got, fpca.spline_fit_host(Y, nb), 0.0)
    assert _bits(_spline_fit(ctx, Y, P)) == _bits(got)
    assert _bits(_spline_fit(ctx, Y[n - 1:], P)[0]) == _bits(got[n - 1])
    _note("gemm", "F%%4=%d" % (F % 4))
    _note("gemm", "row_tiles=%d" % ((nb + 15) // 16))
    if F == nb:
        _note("gemm", "F=n_basis")
    if (nb, F) == (FP_MAX_BASIS, FP_MAX_FRAMES):
        _note("gemm", "n_basis=64,F=1024")


def _gemm_batch(ctx):
    """Three launches over grid.y: the motions next to each seam are the bits of the same motions fitted alone."""
    b = SPLINE_BATCH
    P, _ = spline_operator(b["n_basis"], b["F"])
    Y = spline_motions(b["n_basis"], b["F"], b["D"], b["n"])
    got = _spline_fit(ctx, Y, P)
    ref, bound = gemm_reference(P[None], Y)
    _within("gemm", "spline fit batch", got, ref, bound)
    for i in (0, GRID_Y - 1, GRID_Y, 2 * GRID_Y - 1, 2 * GRID_Y, b["n"] - 1):
        assert _bits(_spline_fit(ctx, Y[i:i + 1], P)[0]) == _bits(got[i]), "motion %d alone differs from the batch" % i
    _note("gemm", "batch>65535")


def _gemm_project(ctx, shape):
    l, p, n = shape
    X, Vt, mean, low = project_inputs(l, p, n)
    with _Dev(ctx) as dev:
        x_dev, v_dev, m_dev, l_dev = dev.up(X), dev.up(Vt), dev.up(mean), dev.up(low)
        lo_dev, hi_dev = dev.new(8 * n * l), dev.new(8 * n * p)
        _capi.pca_project(ctx, x_dev, v_dev, n, p, l, lo_dev)
        got = ctx.download(lo_dev, (n, l), np.float64)
        ref, bound = gemm_reference(X, Vt.T)
        _within("gemm", "project %s" % (shape,), got, ref, bound)
        for bias, b_dev in ((None, None), (mean, m_dev)):
            _capi.pca_backproject(ctx, l_dev, v_dev, b_dev, n, p, l, hi_dev)
            got = ctx.download(hi_dev, (n, p), np.float64)
            ref, bound = gemm_reference(low, Vt, bias)
            _within("gemm", "back-project %s mean %s" % (shape, bias is not None), got, ref, bound)
            _note("gemm", "backproject mean" if bias is not None else "backproject no mean")
    _note("gemm", "project l=%d" % l)
    _note("gemm", "project p=%d" % p)
    _note("gemm", "project n=%d" % n)


def _run_gemm(ctx):
    if "gemm" in _DONE:
        return
    _DONE.add("gemm")
    for shape in SPLINE_SHAPES:
        _gemm_spline(ctx, shape)
    _gemm_batch(ctx)
    for shape in PROJECT_SHAPES:
        _gemm_project(ctx, shape)


def _run_pca(ctx, c):
    if "pca " + c["name"] in _DONE:
        return
    _DONE.add("pca " + c["name"])
    from test_gpu_fpca import device_pca
    r = pca_reference(c)
    A, host, ok, name = r["A"], r["host"], r["resolved"], "pca " + c["name"]
    n, p = A.shape
    m = min(n, p)
    fit = device_pca(ctx, A, centre=c["centre"])
    assert fit["status"] == _capi.MG_PCA_CONVERGED and fit["n_sweeps"] <= _capi.MG_PCA_MAX_SWEEPS, (name, fit["status"], fit["n_sweeps"])
    print("%s: %d sweeps" % (name, fit["n_sweeps"]))
    mean = A.mean(axis=0) if c["centre"] else np.zeros(p)
    assert _bits(fit["mean"]) == _bits(mean), name + ": mean"
    assert _bits(fit["centred"]) == _bits(A - mean), name + ": centred"
    s, vt = fit["singular_values"], fit["vt"]
    assert s.shape == (m,) and vt.shape == (m, p)
    _close("pca", name + " singular values", s, host["singular_values"], r["spread_s"])
    ours = float(np.max(np.abs(vt @ vt.T - np.eye(m))))
    print("%s: max|Vt Vt^T - I| ours %.3e, LAPACK %.3e" % (name, ours, r["lapack_orth"]))
    _ratio("pca_orthonormality", ours, 10 * r["lapack_orth"])
    assert ours <= 10 * r["lapack_orth"], name
    _close("pca", name + " |centred . vt_i| = s_i", np.linalg.norm(fit["centred"] @ vt.T, axis=0), s, r["spread_s"])
    for row in vt:
        assert row[np.argmax(np.abs(row))] > 0, name + ": sign rule"
    assert np.all(np.diff(s) <= 0), name + ": order"
    _close("pca", name + " eigenvectors (resolved)", vt[ok], host["vt"][ok], r["spread_v"])
    _close("pca", name + " mean vs pca_fit_host", fit["mean"], host["mean"], 0.0)
    again = device_pca(ctx, A, centre=c["centre"])
    for key in ("mean", "singular_values", "vt", "centred"):
        assert _bits(again[key]) == _bits(fit[key]), (name, key)
    assert again["n_sweeps"] == fit["n_sweeps"]
    L = max(n, p)
    _note("pca", "odd m" if m % 2 else "even m")
    _note("pca", "L>256" if L > FP_BLOCK else "L<=256")
    _note("pca", "wide" if n <= p else "tall")
    if m <= 3:
        _note("pca", "m=%d" % m)
    if n == p:
        _note("pca", "n==p")
    if not c["centre"]:
        _note("pca", "centre=0")
    if c["kind"] != "plain":
        _note("pca", c["kind"])
    if m % 2 and L > FP_BLOCK:
        _note("pca", "odd m, wide" if n <= p else "odd m, tall")


def _em_dict(g):
    return {"weights": g.weights_, "means": g.means_, "covariances": g.covariances_, "precisions_cholesky": g.precisions_cholesky_,
            "lower_bounds": np.array(g.lower_bounds_), "score": g.train_score_}


def _em_bytes(g):
    return b"".join(_bits(a) for a in (g.weights_, g.means_, g.covariances_, g.precisions_cholesky_, np.array(g.lower_bounds_), g.labels_,
                                       np.array([g.train_score_, g.n_iter_])))


def _run_em(ctx, c):
    if "em " + c["name"] in _DONE:
        return
    _DONE.add("em " + c["name"])
    X, labels, refs = em_reference(c)
    fits = gt.fit_gaussian_mixtures(X, c["Ks"], init=labels, ctx=ctx)
    for K, lab, g, r in zip(c["Ks"], labels, fits, refs):
        ref, name = r["ref"], "em %s K=%d" % (c["name"], K)
        assert g.n_iter_ == ref["n_iter"] and g.converged_ == ref["converged"], (name, g.n_iter_, ref["n_iter"], g.converged_, ref["converged"])
        mine = _em_dict(g)
        for key in EM_KEYS:
            _close("em", "%s %s" % (name, key), mine[key], ref[key], r["spread"][key])
        assert np.array_equal(g.labels_, ref["labels"]), name + ": labels"
        if len(c["Ks"]) > 1:
            alone = gt.fit_gaussian_mixtures(X, [K], init=[lab], ctx=ctx)[0]
            assert _em_bytes(alone) == _em_bytes(g), name + ": alone differs from the batch"
            _note("em", "several K in one call")
        if ref["n_iter"] >= 5:
            _note("em_long", em_dp(c["d"]))
        if K >= EM_MAX_K - 1:
            _note("em", "K=%d" % K)
    n = c["n"]
    _note("em_estep", em_dp(c["d"]))
    _note("em", "d=%d" % c["d"])
    _note("em", "n=%d" % n)
    if n % EM_TILE:
        _note("em", "n%32!=0")


def _run_kmeans(ctx, c):
    if "kmeans " + c["name"] in _DONE:
        return
    _DONE.add("kmeans " + c["name"])
    from test_gpu_cluster_tree_build import _inertia_ok
    X, rows, seg_begin, init, refs = km_reference(c)
    k, dim = c["k"], c["dim"]
    with _Dev(ctx) as dev:
        d_x = dev.up(X)
        call = lambda sb, r, ini: _capi.kmeans_segments(ctx, d_x, len(X), dim, sb, r, k, 1, ini, None, 0, KM_MAX_ITER, KM_TOL)      # noqa: E731
        labels, centres, inertia, n_iter = call(seg_begin, rows, init)
        for s, ref in enumerate(refs):
            a, b = int(seg_begin[s]), int(seg_begin[s + 1])
            name = "kmeans %s segment %d" % (c["name"], s)
            x = X[rows[a:b]]
            assert n_iter[s] == ref["n_iter"], (name, n_iter[s], ref["n_iter"])
            np.testing.assert_array_equal(labels[a:b], ref["labels"], err_msg=name)
            count = np.maximum(np.bincount(ref["labels"], minlength=k), 1).astype(np.float64)
            bound = count[:, None] * 2.0 ** -52 * float(np.max(np.abs(x))) * np.ones((1, dim))
            _within("kmeans", name + " centres", centres[s], ref["centres"], bound)
            tss = float(((x - x.mean(axis=0)) ** 2).sum())
            _ratio("kmeans", abs(float(inertia[s]) - ref["inertia"]), 1e-12 * max(abs(ref["inertia"]), tss))
            assert _inertia_ok(inertia[s], ref["inertia"], x), (name, inertia[s], ref["inertia"])
            if len(refs) > 1:
                alone = call([0, b - a], rows[a:b], init[s:s + 1])
                assert _bits(alone[0]) == _bits(labels[a:b]) and _bits(alone[1][0]) == _bits(centres[s]), name + ": alone differs"
                assert alone[2][0] == inertia[s] and alone[3][0] == n_iter[s], name + ": alone differs"
        again = call(seg_begin, rows, init)
        assert all(_bits(x) == _bits(y) for x, y in zip(again, (labels, centres, inertia, n_iter)))
    _note("kmeans", "dim=%d" % dim)
    _note("kmeans", "k=%d" % k)
    if c["kind"] != "plain":
        _note("kmeans", c["kind"])
    if (k, dim) == (MG_KM_MAX_K, MG_KM_MAX_DIM):
        _note("kmeans", "lds 64x128")


def _run_grids(ctx):
    if "grids" in _DONE:
        return
    _DONE.add("grids")
    for J, weighted, fr in GRID_SHAPES:
        seed = 7000 + 10 * J + weighted
        clouds = clouds_for(J, (fr,) + GRID_FRAMES, seed)
        ref, motions = clouds[0], clouds[1:]
        w = joint_weights(J, weighted, seed)
        grids = dtw.distance_grids(ref, motions, w, ctx=ctx)
        rng = np.random.default_rng(seed)
        for b, S in zip(motions, grids):
            host = dtw.distance_grid_host(ref, b, w)
            check_cells("grids", "grid J=%d weights=%d %dx%d" % (J, weighted, fr, len(b)), S, host, grid_spread(ref, b, w, host, rng))
            assert same_bits(dtw.distance_grids(ref, [b], w, ctx=ctx)[0], S)
        _note("grids", "J=%d weights=%d" % (J, weighted))
        _note("grids", "Fr=%d" % fr)
    J, fr, f = BIG_GRID
    ref, b = clouds_for(J, (fr, f), 7777)
    S = dtw.distance_grids(ref, [b], None, ctx=ctx)[0]
    assert S.shape == (fr, f) and np.all(np.isfinite(S))
    host = dtw.distance_grid_host(ref, b)
    check_cells("grids", "grid J=64 1024x1024", S, host, grid_spread(ref, b, None, host, np.random.default_rng(1)))
    # and the same cells computed as grids of their own (a quarter of the columns each): the same bits
    for q in range(4):
        part = dtw.distance_grids(ref, [b[256 * q:256 * (q + 1)]], None, ctx=ctx)[0]
        assert same_bits(part, S[:, 256 * q:256 * (q + 1)]), "columns %d.. differ from the whole grid" % (256 * q)
    _note("grids", "1024x1024x64")


def _run_keyframes(ctx):
    if "keyframes" in _DONE:
        return
    _DONE.add("keyframes")
    for J in KEY_J:
        for K in KEY_K:
            for weighted in (0, 1):
                seed = 8000 + 10 * J + K
                clouds = clouds_for(J, KEY_FRAMES + (K,), seed + weighted)
                keys, clouds = clouds[-1], clouds[:-1]
                w = joint_weights(J, weighted, seed)
                dist = seg.keyframe_distances(clouds, keys, w, ctx=ctx)
                host = seg.keyframe_distances_host(clouds, keys, w)
                rng = np.random.default_rng(seed)
                for cl, d, h in zip(clouds, dist, host):
                    assert d.shape == (K, len(cl))
                    check_cells("keyframes", "keyframes J=%d K=%d weights=%d F=%d" % (J, K, weighted, len(cl)), d.T, h.T, grid_spread(cl, keys, w, h.T, rng))
                    for k in range(K):
                        grid = dtw.distance_grids(cl, [keys[k][None]], w, ctx=ctx)[0]
                        assert grid.shape == (len(cl), 1) and same_bits(d[k], grid[:, 0]), (J, K, k, len(cl))
                    assert same_bits(seg.keyframe_distances([cl], keys, w, ctx=ctx)[0], d)
                _note("keyframes", "J=%d K=%d" % (J, K))


def _run_paths(ctx):
    if "paths" in _DONE:
        return
    _DONE.add("paths")
    from test_gpu_dtw import brute_force_dp
    for fr, f in PATH_GRIDS:
        S = path_grid(fr, f)
        r = dtw.paths_from_grids([S], ctx=ctx)[0]
        D, path, warp = dtw.dtw_paths_host(S)
        name = "paths %dx%d" % (fr, f)
        assert same_bits(r["D"], D) and same_bits(r["total"], D[-1, -1]), name
        assert r["path"].dtype == np.int32 and [tuple(int(v) for v in p) for p in r["path"]] == path, name
        assert r["warping_function"].tolist() == warp, name
        if fr <= 64 and f <= 64:
            assert same_bits(r["D"], brute_force_dp(S)), name
            _note("paths", "brute force")
        skipped = dtw.paths_from_grids([S], accumulated=False, ctx=ctx)[0]
        assert skipped["D"] is None and np.array_equal(skipped["path"], r["path"]) and skipped["total"] == r["total"]
        _note("paths", "%dx%d %s" % (fr, f, "lds" if paths_in_lds(fr, f) else "device memory"))
    # the small grids of one Fr in one call with a longer one: the same bits
    small = [path_grid(9, 1), path_grid(9, 40), path_grid(9, 7)]
    for S, r in zip(small, dtw.paths_from_grids(small, ctx=ctx)):
        D, path, warp = dtw.dtw_paths_host(S)
        assert same_bits(r["D"], D) and [tuple(int(v) for v in p) for p in r["path"]] == path and r["warping_function"].tolist() == warp


def _run_warp(ctx):
    if "warp" in _DONE:
        return
    _DONE.add("warp")
    for n_dim in WARP_DIMS:
        rng = np.random.default_rng(9000 + n_dim)
        lengths, fr = (1, 17, 64, 5), 33
        frames = [rng.standard_normal((f, n_dim)) for f in lengths]
        w = np.stack([np.sort(rng.integers(0, f, fr)) for f in lengths]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        with _Dev(ctx) as dev:
            f_dev, w_dev, o_dev = dev.up(np.concatenate(frames)), dev.up(w), dev.new(8 * len(lengths) * fr * n_dim)
            _capi.warp_motions(ctx, f_dev, off, n_dim, w_dev, fr, o_dev)
            out = ctx.download(o_dev, (len(lengths), fr, n_dim), np.float64)
        for m, fm in enumerate(frames):
            assert same_bits(out[m], fm[w[m]]), ("warp", n_dim, m)
        _note("warp", "n_dim=%d" % n_dim)


@pytest.mark.gpu
def test_gemm_family(ctx):
    _run_gemm(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("c", PCA_SHAPES, ids=PCA_IDS)
def test_pca_family(ctx, c):
    """n257_p255 is the row that found the drift of the companion G (max|Vt Vt^T - I| 7.4e-14 after 13 sweeps, against the
    bound 10 x LAPACK's 2.2e-15 = 2.2e-14) that mg_pca_fit's Newton-Schulz step after the last sweep now removes."""
    _run_pca(ctx, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", EM_SHAPES, ids=EM_IDS)
def test_em_family(ctx, c):
    _run_em(ctx, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", KM_SHAPES, ids=KM_IDS)
def test_kmeans_family(ctx, c):
    _run_kmeans(ctx, c)


@pytest.mark.gpu
def test_distance_grids_family(ctx):
    _run_grids(ctx)


@pytest.mark.gpu
def test_keyframe_distances_family(ctx):
    _run_keyframes(ctx)


@pytest.mark.gpu
def test_paths_and_warp_family(ctx):
    _run_paths(ctx)
    _run_warp(ctx)


def wanted_ledger():
    want = {("gemm", "F%%4=%d" % r) for r in range(4)} | {("gemm", "row_tiles=%d" % t) for t in (1, 2, 3, 4)}
    want |= {("gemm", w) for w in ("F=n_basis", "n_basis=64,F=1024", "batch>65535", "backproject mean", "backproject no mean")}
    want |= {("gemm", "project l=%d" % l) for l in PROJECT_L} | {("gemm", "project p=%d" % p) for p in (1, 15, 16, 17, 33, 257, 2449)}
    want |= {("gemm", "project n=%d" % n) for n in PROJECT_N}
    want |= {("pca", w) for w in ("odd m", "even m", "L>256", "L<=256", "wide", "tall", "m=1", "m=2", "m=3", "n==p", "centre=0", "duplicates", "constant",
                                  "odd m, wide", "odd m, tall")}
    want |= {("em_estep", dp) for dp in (8, 16, 32, 64)} | {("em_long", dp) for dp in (8, 16, 32, 64)}
    want |= {("em", "d=%d" % d) for d in (1, 8, 9, 16, 17, 24, 32, 33, 64)} | {("em", "n=%d" % n) for n in (15, 16, 255, 256, 257, 513, 1000)}
    want |= {("em", "n%32!=0"), ("em", "K=63"), ("em", "K=64"), ("em", "several K in one call")}
    want |= {("kmeans", "dim=%d" % d) for d in (1, 43, 44, 127, 128)} | {("kmeans", "k=%d" % k) for k in (2, 7, 8, 9, 16, 63, 64)}
    want |= {("kmeans", "lds 64x128"), ("kmeans", "segments"), ("kmeans", "empty")}
    want |= {("grids", "J=%d weights=%d" % (J, w)) for J in GRID_J for w in (0, 1)} | {("grids", "Fr=%d" % f) for f in GRID_FRAMES}
    want |= {("grids", "1024x1024x64")} | {("keyframes", "J=%d K=%d" % (J, K)) for J in KEY_J for K in KEY_K}
    want |= {("paths", "768x512 lds"), ("paths", "768x513 device memory"), ("paths", "1x1 lds"), ("paths", "1x9 lds"), ("paths", "9x1 lds"),
             ("paths", "brute force")}
    want |= {("warp", "n_dim=%d" % d) for d in WARP_DIMS}
    return want


@pytest.mark.gpu
def test_the_ledger_covers_every_boundary(ctx):
    """Every (family, boundary) entry of the tables ran and matched.  (Families the run has not reached yet -- a selection
    with -k -- are run here; a kernel that declines a shape fails there.  A row that failed above is not run again: the
    entries only it holds are then missing here.)"""
    _run_gemm(ctx)
    for c in PCA_SHAPES:
        _run_pca(ctx, c)
    for c in EM_SHAPES:
        _run_em(ctx, c)
    for c in KM_SHAPES:
        _run_kmeans(ctx, c)
    _run_grids(ctx)
    _run_keyframes(ctx)
    _run_paths(ctx)
    _run_warp(ctx)
    table = {}
    for fam, what in sorted(LEDGER, key=lambda e: (e[0], str(e[1]))):
        table.setdefault(fam, []).append(str(what))
    print("\nledger (family: boundaries that ran and matched)")
    for fam, whats in sorted(table.items()):
        print("  %-10s %s" % (fam, ", ".join(whats)))
    print("worst error / bound per family")
    for fam, r in sorted(RATIOS.items()):
        print("  %-20s %.3g" % (fam, r))
    print("construction shapes: %.1f s since the module was imported" % (time.time() - T0))
    missing = sorted(wanted_ledger() - LEDGER, key=str)
    assert not missing, "rows of the tables no longer exercise: %s" % missing
