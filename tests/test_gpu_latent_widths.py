"""Every latent width against the oracle.

Almost every hot kernel is a template on KK, the number of 4-wide k-steps of the latent vector (the smallest even number
>= ceil(L / 4): L = 1 .. 64 -> KK in {2, 4, ..., 16}); each KK is its own code object with its own register budget, fragment
layout and tail.  SHAPES below is one table of synthetic primitives that puts every KK boundary (L = 4k, 4k + 1), both sides of
the mixture kernels' LDS limit, of the fusion limit (K = 16 / 17) and of the chunk-stationary kernel's window in front of the
kernels, and checks each family against the oracle with the contracts the rest of the suite uses.

LEDGER records which (family, KK, latent dtype) combinations ran and matched; test_the_ledger_covers_every_width fails when a
shape stops exercising what it was put in the table for (a kernel that declines a shape is not a skip).  The boundary check
(no GPU) recomputes the dispatch formulas of mg_host.hip / mg_frames.hip / mg_gmm.hip and asserts the table straddles each one.
"""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from oracle import c_oracle
from oracle import mg_oracle as orc
from test_gpu_parity import _bits, _fused_step, pose_tol

MG_ERR_UNSUPPORTED = -4
N_CU = 256                       # MI355X compute units (BIG_B: two chunk-stationary units per workgroup)
KKS = (2, 4, 6, 8, 10, 12, 14, 16)

# ---- the dispatch formulas, restated (kept in step with the C sources by test_table_straddles_every_dispatch_boundary) -------------
MG_MAX_KK = 16                   # mg_hostdefs.h
MG_FUSE_MAX_KK = 10              # mg_frames_common.h
MG_GMM_LDS_MIN_B = 20480         # mg_gmm.hip
LDS_BUDGET = 160 * 1024


def kk_of(L):
    """mg_primitive_create: p->KK (0 = no MFMA instance)."""
    return ((L + 3) // 4 + 1) // 2 * 2 if L <= 4 * MG_MAX_KK else 0


def jt_of(Lg):
    return (Lg + 15) // 16


def gmm_lds_nf(KK, JT):
    return sum(min(4 * (jt + 1), KK) for jt in range(JT))


def gmm_lds_fits(K, Lg):
    """mg_gmm_use_lds_kernel: the LDS-resident mixture kernel holds K components of Lg dimensions."""
    KK, JT = kk_of(Lg), jt_of(Lg)
    return KK > 0 and K * (gmm_lds_nf(KK, JT) * 64 + JT * 16 + 512) * 8 <= LDS_BUDGET - 64


def gmm_lds_max_k(Lg):
    K = 0
    while gmm_lds_fits(K + 1, Lg):
        K += 1
    return K


def jac_mfma_fits(K, Lg):
    """mg_launch_gmm_jac_mfma_kk: its LDS (else the VALU kernel)."""
    JTM = (kk_of(Lg) + 3) // 4
    return kk_of(Lg) > 0 and (K * 16 * (JTM * 16 + 1) + K * 16 + 16 + 4 * 16 * JTM * 16) * 8 <= 150 * 1024


def fuse_static(L, Lg, K):
    """mg_frames_can_fuse_gmm, the parts that do not depend on the batch or the grid's LDS."""
    return 0 < kk_of(L) <= MG_FUSE_MAX_KK and K <= 16 and Lg == L


def cs_spills(KK, lat_f64):
    """mg_frames_kernel_choice: instances the library's own choice keeps on the tile-major kernel."""
    return KK >= 16 or (lat_f64 and KK >= 14)


# ---- the table ------------------------------------------------------------------------------------------------------------------
# grid "short": F = 48, NB = 5 -- one chunk whose window (5 basis functions, 25 row tiles at D = 79) fits the chunk-stationary
# kernel's registers at every KK; "walk": F = 156, NB = 31, D = 79.  big: a batch of 16 * 512 + 5 candidates, where the library
# picks the chunk-stationary kernel by itself (units >= 2 x grid).
SHORT = dict(n_frames=48, n_basis=5)
WALK = dict(n_frames=156, n_basis=31, n_dim=79)
BIG_B = 16 * 2 * N_CU + 5


def _row(L, K, D=79, grid="short", Lt=0, big=False):
    kw = dict(SHORT if grid == "short" else WALK)
    kw.setdefault("n_dim", D)
    name = "L%d_K%d_D%d_%s%s" % (L, K, kw["n_dim"], grid, ("_t%d" % Lt) if Lt else "")
    return dict(name=name, L=L, K=K, Lt=Lt, big=big, grid=grid,
                model=dict(n_components=L, n_gmm=K, n_time_components=Lt, n_basis_time=6 if Lt else None, **kw))


SHAPES = [
    _row(1, 1),
    _row(4, 31, D=23),                 # KK 2: the LDS mixture kernel's largest K ...
    _row(5, 32, D=15),                 # ... and one more
    _row(8, 16, big=True),             # fusion at K = 16
    _row(9, 27),                       # KK 4: one past the LDS limit (26)
    _row(16, 26, D=23, big=True),      # KK 4: largest LDS K
    _row(17, 18),                      # KK 6: one past the LDS limit (17)
    _row(24, 17, big=True),            # KK 6: largest LDS K; K = 17: no fusion
    _row(25, 15, big=True),            # KK 8: largest LDS K, fused
    _row(32, 16, D=15),                # KK 8: one past the LDS limit, fused at K = 16
    _row(33, 10, big=True),            # KK 10: largest LDS K, fused
    _row(40, 11),                      # KK 10: one past
    _row(41, 9, big=True),             # KK 12: largest LDS K
    _row(48, 10),                      # KK 12: one past
    _row(49, 6, big=True),             # KK 14: largest LDS K; float64 latents stay tile-major from here (cs_spills)
    _row(52, 7, D=23),                 # KK 14: one past
    _row(53, 1, big=True),
    _row(56, 3, grid="walk"),
    _row(57, 6, big=True),             # KK 16: largest LDS K; spilling chunk-stationary instance: forced only
    _row(60, 7),                       # KK 16: one past
    _row(61, 2, grid="walk"),
    _row(64, 6),
    _row(64, 7, D=15),
    _row(65, 3, D=15),                 # the VALU fallback next to the last MFMA width
    _row(41, 4, grid="walk"),
    _row(49, 2, grid="walk"),
    _row(14, 4, Lt=5),                 # Lg = 19: the mixture in KK 6, the frames in KK 4
    _row(38, 5, Lt=6),                 # Lg = 44: the mixture in KK 12, the frames in KK 10
    _row(62, 3, D=15, Lt=4),           # Lg = 66: the mixture on the VALU kernels, the frames on KK 16
    _row(13, 5, D=22),                 # KK 4 and KK 12 at a channel count that is not 3 (mod 4): the sweep waves' last quad lane
    _row(45, 4, D=22),                 # stores three floats, the root lane three (no lane stores a borrowed float)
]
SHAPE_IDS = [s["name"] for s in SHAPES]

LEDGER = set()       # (family, KK, dtype name) that ran and matched
_DONE = {}           # shape name -> True once its sweep passed


def _note(family, KK, dtype):
    LEDGER.add((family, int(KK), np.dtype(dtype).name))


# ---- CPU checks -----------------------------------------------------------------------------------------------------------------
def _source(name):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "morphablegraphs_amd", "csrc", name)).read()


def test_table_straddles_every_dispatch_boundary():
    """The formulas restated above match the C sources, and the table has shapes on both sides of every boundary."""
    image, gmm, common, hostdefs, frames = (_source(n) for n in ("mg_primitive_image.h", "mg_gmm.hip", "mg_frames_common.h", "mg_hostdefs.h",
                                                                   "mg_frames.hip"))
    assert "p->KK = (L <= 4 * MG_MAX_KK) ? (((L + 3) / 4 + 1) / 2) * 2 : 0;" in image
    assert "#define MG_MAX_KK %d " % MG_MAX_KK in hostdefs
    assert "#define MG_FUSE_MAX_KK %d " % MG_FUSE_MAX_KK in common
    assert "#define MG_GMM_LDS_MIN_B %d" % MG_GMM_LDS_MIN_B in gmm
    assert "(size_t)p->K * mg_gmm_lds_nf(p->KKg, JT) * 64 + (size_t)p->K * JT * 16 + (size_t)16 * 2 * p->K * 16) * 8;" in gmm
    assert "if (lds > 160 * 1024 - 64) return false;" in gmm
    assert "for (int jt = 0; jt < JT; jt++) nf += std::min(4 * (jt + 1), KK);" in gmm
    assert "p->K <= 16 && p->KK <= MG_FUSE_MAX_KK && p->Lg == p->L" in frames
    assert "const bool cs_spills = p->KK >= 16 || (lat_f64 && p->KK >= 14);" in frames
    assert [kk_of(L) for L in (1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64, 65)] == \
        [2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14, 16, 16, 0]
    assert gmm_lds_max_k(64) == 6 and gmm_lds_max_k(40) == 10
    widths = {s["L"] for s in SHAPES}
    assert {1, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 52, 53, 56, 57, 60, 61, 64, 65} <= widths
    lg = lambda s: s["L"] + s["Lt"]
    for KK in KKS:
        rows = [s for s in SHAPES if kk_of(lg(s)) == KK]
        kmax = gmm_lds_max_k(4 * KK)
        assert any(s["K"] == kmax and gmm_lds_fits(s["K"], lg(s)) for s in rows), "KK %d: no shape at the LDS kernel's largest K" % KK
        assert any(not gmm_lds_fits(s["K"], lg(s)) for s in rows), "KK %d: no shape past the LDS kernel's limit" % KK
        assert all(jac_mfma_fits(s["K"], lg(s)) for s in rows), "KK %d: a shape the Jacobian's MFMA kernel does not hold" % KK
        assert any(s["grid"] == "short" for s in rows if kk_of(s["L"]) == KK)
        assert any(s["big"] for s in SHAPES if kk_of(s["L"]) == KK), "KK %d: no batch where the library picks its own kernel" % KK
    fused = [s for s in SHAPES if fuse_static(s["L"], lg(s), s["K"])]
    assert any(s["K"] == 16 for s in fused) and any(s["K"] == 17 and 0 < kk_of(s["L"]) <= MG_FUSE_MAX_KK for s in SHAPES)
    assert any(s["K"] == 1 for s in SHAPES)
    assert any(kk_of(s["L"]) > MG_FUSE_MAX_KK for s in SHAPES if s["big"])
    # mixtures over spatial + time latents: in a higher KK than the frames, and past 64 with the frames on MFMA
    assert any(s["Lt"] and kk_of(lg(s)) > kk_of(s["L"]) > 0 for s in SHAPES)
    assert any(s["Lt"] and kk_of(lg(s)) == 0 and kk_of(s["L"]) > 0 for s in SHAPES)
    # both sides of the spilling instances: chunk-stationary by choice at KK 14 for float32, not for float64
    assert not cs_spills(14, False) and cs_spills(14, True) and cs_spills(16, False) and not cs_spills(12, True)
    assert any(s["grid"] == "walk" for s in SHAPES) and {s["name"] for s in SHAPES} == set(SHAPE_IDS) and len(SHAPE_IDS) == len(SHAPES)
    assert any((d - 3) % 4 for d in (s["model"]["n_dim"] for s in SHAPES))     # a channel count whose last quad is partial


def test_device_sampler_restatement_draws_standard_normals_and_the_mixture():
    """oracle.device_gmm_sample: shape, grouping and moments of the restated device draw (the GPU tests pin the device to it)."""
    z = orc.device_normals(np.arange(60000), 99, 2)
    assert z.shape == (60000, 8)
    np.testing.assert_allclose(z.mean(axis=0), 0.0, atol=5 * 1 / np.sqrt(60000))
    np.testing.assert_allclose(z.std(axis=0), 1.0, atol=0.02)
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.02
    np.testing.assert_array_equal(orc.device_normals(np.arange(5, 9), 99, 2), z[5:9])       # counter = the row, not the position
    assert not np.array_equal(orc.device_normals(np.arange(4), 98, 2), z[:4])
    data = synthetic.make_primitive(seed=3, n_components=5, n_frames=20, n_dim=7, n_gmm=3)
    means, covars = np.array(data["gmm_means"]), np.array(data["gmm_covars"])
    counts = [30000, 0, 20000]
    x, comp, scale = orc.device_gmm_sample(counts, 5, means, covars)
    assert x.shape == (50000, 5) and scale.shape == x.shape and np.all(scale >= 1e-3)
    np.testing.assert_array_equal(comp, np.repeat([0, 1, 2], counts))
    for k in (0, 2):
        xs = x[comp == k]
        assert np.all(np.abs(xs.mean(axis=0) - means[k]) < 5 * np.sqrt(np.diag(covars[k]) / len(xs)))
        assert np.abs(np.cov(xs.T) - covars[k]).max() < 0.05 * np.abs(covars[k]).max()
    # the z of row b are the same whichever component b falls in
    x2, _, _ = orc.device_gmm_sample([50000, 0, 0], 5, means, covars)
    np.testing.assert_allclose(x2[:30000], x[:30000], rtol=0, atol=0)


# ---- GPU sweep ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def _reset(ctx):
    for option in range(_capi.MG_OPT_COUNT):
        ctx.set_option(option, 0)


@pytest.fixture(autouse=True)
def _default_options(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        if c.handle:
            _reset(c)


def _eval_times(F):
    """Fractional, repeated, backwards and out-of-range times."""
    return np.array([0.0, 0.25, 0.25, F / 3.0 + 0.5, F - 1.0, F - 1.5, 2.0, 1.0, -3.0, F + 4.0, 0.5 * (F - 1), 0.5 * (F - 1)])


def _far_rows(data, rng, n):
    """Rows 30 .. 300 standard deviations from every component: an unshifted log-sum-exp underflows to -inf in float64."""
    means, covars = np.array(data["gmm_means"]), np.array(data["gmm_covars"])
    sd = np.sqrt(max(np.diag(c).max() for c in covars))
    u = rng.standard_normal((n, means.shape[1]))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    reach = np.abs(means).max() + np.linspace(30.0, 300.0, n)[:, None] * sd
    return means.mean(axis=0) + reach * u


def _frames_family(ctx, data, s, S, cp):
    """Direct, tile-major, chunk-stationary (forced) and the library's choice; float32 / float64 latents; root modes 1 and 2;
    canonical and evaluation grid: bit for bit the oracle's float32 model."""
    L = s["L"]
    F = int(data["n_canonical_frames"])
    times = _eval_times(F)
    for mode in (1, 2):
        ctx.set_option(_capi.MG_OPT_ROOT_MODE, mode)
        prim = _capi.Primitive(ctx, data)
        split = mode == 2
        assert prim.root_split == split
        KK = prim.kk
        grid = prim.time_grid(times)
        try:
            for dtype in (np.float32, np.float64):
                X = S.astype(dtype)
                X64 = X[:, :L].astype(np.float64)
                model, model_t = cp.frames_f32model(X64, root_split=split), cp.frames_f32model(X64, tp=times, root_split=split)
                got = prim.back_project_frames(X, path=_capi.MG_PATH_DIRECT)
                np.testing.assert_array_equal(_bits(got), _bits(model), err_msg="%s direct %s mode %d" % (s["name"], dtype, mode))
                np.testing.assert_array_equal(_bits(prim.back_project_frames(X, grid=grid, path=_capi.MG_PATH_DIRECT)), _bits(model_t))
                if not split:
                    ref = cp.frames_f64(X64)
                    assert np.all(np.abs(got.astype(np.float64) - ref) <= pose_tol(ref)), s["name"]
                if not prim.mfma_supported:
                    with pytest.raises(_capi.MGError):
                        prim.back_project_frames(X, path=_capi.MG_PATH_MFMA)
                    continue
                for kern in (1, 2, 0):
                    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, kern)
                    for g, want in ((None, model), (grid, model_t)):
                        try:
                            out = prim.back_project_frames(X, grid=g, path=_capi.MG_PATH_MFMA)
                        except _capi.MGError as e:
                            assert kern == 2 and e.status == MG_ERR_UNSUPPORTED, e
                            continue
                        np.testing.assert_array_equal(_bits(out), _bits(want), err_msg="%s kernel %d %s mode %d grid %s" % (
                            s["name"], kern, np.dtype(dtype).name, mode, g is not None))
                        if kern == 1:
                            _note("frames_ws", KK, dtype)
                        elif kern == 2:
                            _note("frames_cs", KK, dtype)
                ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
        finally:
            grid.close()
            prim.close()
    ctx.set_option(_capi.MG_OPT_ROOT_MODE, 0)


def _float64_family(prim, s, S, cp):
    """back_project_frames_f64 / back_project_coeffs against the oracle's float64 frames and coefficients; the persistent
    large-batch coefficient path (a batch of 16 x) bit for bit the small-batch one."""
    L = s["L"]
    X64 = S[:, :L].astype(np.float64)
    ref = cp.frames_f64(X64)
    scale = max(1.0, np.abs(ref).max())
    np.testing.assert_allclose(prim.back_project_frames_f64(S), ref, rtol=0, atol=4e-12 * scale)
    cref = cp.coeffs_f64(X64)
    np.testing.assert_allclose(prim.back_project_coeffs(S), cref, rtol=0, atol=4e-12 * scale)
    c32 = prim.back_project_coeffs(S, dtype=np.float32)
    assert np.all(np.abs(c32 - cref) <= pose_tol(cref))
    big = np.tile(S, (16, 1))
    np.testing.assert_array_equal(_bits(prim.back_project_coeffs(big, dtype=np.float32)), _bits(np.tile(c32, (16, 1, 1))))
    np.testing.assert_allclose(prim.back_project_coeffs(big), np.tile(cref, (16, 1, 1)), rtol=0, atol=4e-12 * scale)


def _step_family(ctx, prim, s, S, cp):
    """mg_step_frames_and_logp (fused where allowed, two launches where not): frames the tile-major kernel's bits, log p the
    stand-alone float32 log-likelihood's bits and within float32 tolerance of the float64 oracle."""
    F, D = prim.n_canonical_frames, prim.n_dim
    for dtype in (np.float32, np.float64):
        X = S.astype(dtype)
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 1)
        tm = prim.back_project_frames(X, path=_capi.MG_PATH_MFMA if prim.mfma_supported else _capi.MG_PATH_AUTO)
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
        frames, logp = _fused_step(ctx, prim, X, F, D)
        np.testing.assert_array_equal(_bits(frames), _bits(tm), err_msg="%s step %s" % (s["name"], np.dtype(dtype).name))
        np.testing.assert_array_equal(_bits(logp), _bits(prim.gmm_log_prob(X, dtype=np.float32)))
        np.testing.assert_allclose(logp, cp.log_prob_f64(X.astype(np.float64)), rtol=3e-7, atol=1e-6)
        if prim.mfma_supported and prim.step_plan(len(X), dtype=dtype)["fused"]:
            _note("step_fused", prim.kk, dtype)


def _big_batch_family(ctx, prim, s, cp, rng):
    """A batch where the library picks the kernel by itself: step_plan names it; frames (stand-alone and in the step) are the
    tile-major kernel's bits, rows at both ends the oracle's model, log p the stand-alone kernel's bits."""
    B, L = BIG_B, s["L"]
    F, D = prim.n_canonical_frames, prim.n_dim
    S = rng.standard_normal((B, L + s["Lt"]))
    idx = np.concatenate([np.arange(150), np.arange(B - 69, B)])
    for dtype in (np.float32, np.float64):
        X = S.astype(dtype)
        plan = prim.step_plan(B, dtype=dtype)
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 1)
        tm = prim.back_project_frames(X, path=_capi.MG_PATH_MFMA)
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
        auto = prim.back_project_frames(X, path=_capi.MG_PATH_MFMA)
        np.testing.assert_array_equal(_bits(auto), _bits(tm), err_msg="%s big %s (%s)" % (s["name"], np.dtype(dtype).name, plan["kernel"]))
        np.testing.assert_array_equal(_bits(auto[idx]), _bits(cp.frames_f32model(X[idx, :L].astype(np.float64))))
        del auto
        frames, logp = _fused_step(ctx, prim, X, F, D)
        np.testing.assert_array_equal(_bits(frames), _bits(tm))
        del frames, tm
        np.testing.assert_array_equal(_bits(logp), _bits(prim.gmm_log_prob(X, dtype=np.float32)))
        np.testing.assert_allclose(logp[idx], cp.log_prob_f64(X[idx].astype(np.float64)), rtol=3e-7, atol=1e-6)
        want_cs = not cs_spills(prim.kk, dtype == np.float64)
        assert plan["kernel"] == ("mg_frames_cs_kernel" if want_cs else "mg_frames_ws_kernel"), (s["name"], np.dtype(dtype).name, plan)
        if want_cs:
            _note("frames_cs_chosen", prim.kk, dtype)


def _gmm_family(ctx, prim, data, s, S, cp, rng):
    """MG_OPT_GMM_KERNEL 1 / 2 (the LDS-resident kernel where it holds the mixture), the VALU kernel past 64 dimensions:
    float32 / float64 in and out, a leading dimension > n_gmm_dims, rows far from every component."""
    Lg = prim.n_gmm_dims
    far = _far_rows(data, rng, 8)
    X = np.concatenate([S, far])
    ref64 = cp.log_prob_f64(X)
    assert np.all(np.isfinite(ref64)) and ref64[-1] < -2000.0
    lds = gmm_lds_fits(prim.n_gmm, Lg) and prim.kk_gmm > 0
    for xdt in (np.float32, np.float64):
        Xd = X.astype(xdt)
        refd = cp.log_prob_f64(Xd.astype(np.float64))
        outs = {}
        for mode in (1, 2):
            ctx.set_option(_capi.MG_OPT_GMM_KERNEL, mode)
            lp64 = prim.gmm_log_prob(Xd, dtype=np.float64)
            lp32 = prim.gmm_log_prob(Xd, dtype=np.float32)
            np.testing.assert_allclose(lp64, refd, rtol=1e-9, atol=1e-7, err_msg="%s mode %d %s" % (s["name"], mode, np.dtype(xdt).name))
            np.testing.assert_allclose(lp32[:len(S)], refd[:len(S)], rtol=3e-7, atol=1e-6)
            # a leading dimension past n_gmm_dims, through the device entry point
            ld = Lg + 3
            pad = np.zeros((len(Xd), ld), dtype=xdt)
            pad[:, :Lg] = Xd
            d_x, d_o = ctx.upload(pad), ctx.malloc(8 * len(Xd))
            prim.gmm_log_prob_dev(d_x, xdt, len(Xd), ld, d_o, np.float64)
            ctx.synchronize()
            np.testing.assert_array_equal(ctx.download(d_o, (len(Xd),), np.float64).view(np.uint64), lp64.view(np.uint64))
            d_x.free()
            d_o.free()
            outs[mode] = (lp64, lp32)
            if prim.kk_gmm == 0:
                _note("gmm_valu", 0, xdt)
            elif mode == 1:
                _note("gmm_mfma", prim.kk_gmm, xdt)
            elif lds:
                _note("gmm_lds", prim.kk_gmm, xdt)
        np.testing.assert_array_equal(outs[1][0].view(np.uint64), outs[2][0].view(np.uint64), err_msg=s["name"])
        np.testing.assert_array_equal(outs[1][1].view(np.uint32), outs[2][1].view(np.uint32), err_msg=s["name"])
    ctx.set_option(_capi.MG_OPT_GMM_KERNEL, 0)
    # the Jacobian, far rows included (the reference returns ones where the density underflows)
    Xj = np.concatenate([S[:10], far[[0, 3, 7]]])
    jac = prim.gmm_log_prob_jac(Xj)
    ref = orc.OraclePrimitive(data).log_likelihood_jac(Xj)
    np.testing.assert_allclose(jac, ref, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(ref[:10]).max()), err_msg=s["name"])
    if prim.kk_gmm > 0 and jac_mfma_fits(prim.n_gmm, Lg):
        _note("jac_mfma", prim.kk_gmm, np.float64)


# |x - x_ref| <= SAMPLER_C 2^-20 sum_j |chol_ij| (1 + |z_j|): the float32 transcendentals of the normals (v_log_f32, v_sqrt_f32,
# v_sin_f32 / v_cos_f32).  The largest ratio |x - x_ref| / (2^-20 sum_j |chol_ij| (1 + |z_j|)) seen on an MI355X over the whole
# table, both kernels and both output types: 0.145.
SAMPLER_C = 1.0


def _sampler_family(ctx, prim, data, s, rng):
    """The device sampler (MFMA and lane-per-row VALU kernels) against oracle.device_gmm_sample -- the same Philox counters,
    Box-Muller, component grouping and x = mu + chol z -- within float32 resolution of the normals; rows of a sub-range of the
    draw equal the same rows of the whole draw bit for bit."""
    K, Lg = prim.n_gmm, prim.n_gmm_dims
    counts = rng.integers(0, 40, K)
    counts[rng.random(K) < 0.3] = 0
    counts[-1] += 21            # ragged: the last tile of the last component is short
    n = int(counts.sum())
    seed = 0x1234567 + 977 * K + Lg
    xr, comp_r, scale = orc.device_gmm_sample(counts, seed, data["gmm_means"], data["gmm_covars"])
    worst = 0.0
    for dtype in (np.float64, np.float32):
        got = {}
        for valu in (0, 1):
            ctx.set_option(_capi.MG_OPT_FORCE_VALU_SAMPLE, valu)
            X, comp = prim.gmm_sample(counts, seed, dtype=dtype)
            np.testing.assert_array_equal(comp, comp_r)
            err = np.abs(X.astype(np.float64) - xr)
            bound = SAMPLER_C * 2.0 ** -20 * scale + (2.0 ** -24 * np.abs(xr) if dtype == np.float32 else 0.0)
            worst = max(worst, float((err / (2.0 ** -20 * scale)).max()))
            assert np.all(err <= bound), (s["name"], np.dtype(dtype).name, valu, float((err / bound).max()))
            got[valu] = X
            # a sub-range of the draw: the same rows, bit for bit
            b0, cnt = n // 3, n - n // 3 - 5
            view = np.uint64 if dtype == np.float64 else np.uint32
            d_x = ctx.malloc(max(cnt, 1) * Lg * np.dtype(dtype).itemsize)
            prim.gmm_sample_dev(counts, seed, d_x, dtype, Lg, rows=(b0, cnt))
            ctx.synchronize()
            np.testing.assert_array_equal(ctx.download(d_x, (cnt, Lg), dtype).view(view), X[b0:b0 + cnt].view(view))
            d_x.free()
            if prim.kk_gmm > 0:
                _note("sample_valu" if valu else "sample_mfma", prim.kk_gmm, dtype)
        view = np.uint64 if dtype == np.float64 else np.uint32
        np.testing.assert_array_equal(got[0].view(view), got[1].view(view), err_msg=s["name"])
    ctx.set_option(_capi.MG_OPT_FORCE_VALU_SAMPLE, 0)
    SAMPLER_RATIOS.append(worst)


SAMPLER_RATIOS = []


def _score_family(ctx, prim, data, s, S):
    """Root position, 2-D direction and (D = 79) a joint_position constraint, local and aligned to a start pose:
    MG_OPT_SCORE_KERNEL 1 / 2 and the VALU scorer bit-identical, errors against the oracle; the one-launch objective equals the
    two separate calls where it carries the set.  Three root constraints own 21 rows, more than the 16 the wide kernel takes: option 2
    runs the tile kernel here, as the plan asserted per option states (the wide kernel: tests/test_gpu_score_shapes.py)."""
    from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
    L, F, D = s["L"], prim.n_canonical_frames, prim.n_dim
    op = orc.OraclePrimitive(data)
    cp = c_oracle.COraclePrimitive(data)
    tl = F - 1.0
    root = [{"type": "position", "t": tl, "weight": 1.0, "target": [30.0, None, -40.0]},
            {"type": "position", "t": tl / 2.0 + 0.5, "weight": 0.5, "target": [5.0, 90.0, 3.0]},
            {"type": "direction", "t": tl, "weight": 2.0, "target": [0.3, -1.0]}]
    nan = np.nan
    root_c = np.array([[0, tl, 1.0, 30.0, nan, -40.0, 0, 0], [0, tl / 2.0 + 0.5, 0.5, 5.0, 90.0, 3.0, 0, 0],
                       [1, tl, 2.0, 0.3, -1.0, 0.0, 0.0, 1.0]])
    sk, joints, animated = None, None, None
    cons = list(root)
    if D == 79:
        joints, animated = synthetic.make_skeleton(19)
        sk = _capi.Skeleton(joints, animated)
        cons.append({"type": "joint_position", "joint": "RightHand", "t": tl / 3.0, "weight": 2.0, "target": [12.0, 90.0, 4.0]})
    start_pose = {"position": [55.0, 7.5, -80.0], "orientation": [0.0, 37.5, 0.0]}
    for aligned in (False, True):
        al = alignment_from_start_pose(dict(start_pose, position=list(start_pose["position"]))) if aligned else None
        cset = _capi.ConstraintSet(prim, cons, sk, alignment=al)
        try:
            for dtype in (np.float32, np.float64):
                X = S.astype(dtype)
                Xo = X[:, :L].astype(np.float64)
                outs = []
                for opt, val in ((_capi.MG_OPT_SCORE_KERNEL, 1), (_capi.MG_OPT_SCORE_KERNEL, 2), (_capi.MG_OPT_FORCE_VALU_SCORE, 1)):
                    ctx.set_option(opt, val)
                    plan = prim.score_plan(cset, len(X))
                    assert plan["kernel"] == ("tile" if prim.mfma_supported and opt == _capi.MG_OPT_SCORE_KERNEL else "valu"), (s["name"], opt, val, plan)
                    assert not prim.mfma_supported or plan["rows"] >= 21
                    outs.append((prim.score_constraints(cset, X), prim.score_constraint_residuals(cset, X)))
                    ctx.set_option(opt, 0)
                for e, r in outs[1:]:
                    np.testing.assert_array_equal(e.view(np.uint64), outs[0][0].view(np.uint64), err_msg=s["name"])
                    np.testing.assert_array_equal(r.view(np.uint64), outs[0][1].view(np.uint64), err_msg=s["name"])
                err, res = outs[0]
                if aligned:
                    ref = op.start_pose_residuals(Xo, cons, {"position": [55.0, 7.5, -80.0], "orientation": [0.0, 37.5, 0.0]}, joints, animated)
                    np.testing.assert_allclose(res, ref, rtol=1e-9, atol=1e-8, err_msg=s["name"])
                else:
                    np.testing.assert_allclose(err if len(cons) == 3 else res[:, :3].sum(axis=1), cp.keyframe_errors_f64(Xo, root_c),
                                               rtol=1e-10, atol=1e-9, err_msg=s["name"])
                    if len(cons) > 3:
                        np.testing.assert_allclose(res[:, 3:], op.joint_position_residuals(Xo, cons[3:], joints, animated),
                                                   rtol=1e-10, atol=1e-8, err_msg=s["name"])
                np.testing.assert_allclose(res.sum(axis=1), err, rtol=1e-13, atol=1e-12)
                if prim.mfma_supported:
                    _note("score_mfma", prim.kk, dtype)
        finally:
            cset.close()
    # the optimiser's objective in one launch (root constraints, no alignment)
    cset = _capi.ConstraintSet(prim, root)
    try:
        for dtype in (np.float32, np.float64):
            X = S.astype(dtype)
            try:
                obj, err, lp = prim.objective(cset, X, 0.75, 1.25)
            except _capi.MGError as e:
                assert e.status == MG_ERR_UNSUPPORTED, (s["name"], e)      # mg_objective_can_fuse: not this mixture / set
                continue
            err2 = prim.score_constraints(cset, X)
            lp2 = prim.gmm_log_prob(X, dtype=np.float64)
            np.testing.assert_array_equal(err.view(np.uint64), err2.view(np.uint64), err_msg=s["name"])
            np.testing.assert_array_equal(lp.view(np.uint64), lp2.view(np.uint64), err_msg=s["name"])
            np.testing.assert_array_equal(obj.view(np.uint64), (0.75 * err2 + (-lp2) * 1.25).view(np.uint64))
            _note("objective", prim.kk, dtype)
    finally:
        cset.close()


def _sweep(ctx, s):
    if s["name"] in _DONE:
        return
    data = synthetic.make_primitive(seed=1000 + s["L"] * 7 + s["K"], name=s["name"], **s["model"])
    cp = c_oracle.COraclePrimitive(data)
    rng = np.random.default_rng(s["L"] * 100 + s["K"])
    Lg = s["L"] + s["Lt"]
    S = rng.standard_normal((16 * 4 + 5, Lg))           # 69 rows: a ragged last tile
    _reset(ctx)
    _frames_family(ctx, data, s, S, cp)
    prim = _capi.Primitive(ctx, data)
    try:
        assert prim.kk == kk_of(s["L"]) and prim.kk_gmm == kk_of(Lg) and prim.n_gmm_dims == Lg
        _float64_family(prim, s, S, cp)
        _step_family(ctx, prim, s, S, cp)
        if s["big"]:
            _big_batch_family(ctx, prim, s, cp, rng)
        _gmm_family(ctx, prim, data, s, S, cp, rng)
        _sampler_family(ctx, prim, data, s, rng)
        _score_family(ctx, prim, data, s, S)
    finally:
        prim.close()
        _reset(ctx)
    _DONE[s["name"]] = True


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_width_sweep_against_the_oracle(ctx, shape):
    _sweep(ctx, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [49, 53, 56, 57, 64])
def test_step_plan_names_the_kernel_float64_latents_run(ctx, L):
    """mg_step_plan_dtype: from 49 latents on, a step over float64 latents runs the tile-major kernel where float32 latents get
    the chunk-stationary one; the plan says so (same kernel, grid and LDS as with the tile-major kernel forced), and for float32
    latents it is mg_step_plan_for's plan unchanged."""
    import ctypes as C
    data = synthetic.make_primitive(seed=L, n_components=L, n_gmm=2, name="plan%d" % L, **SHORT)
    prim = _capi.Primitive(ctx, data)
    try:
        B = BIG_B
        auto64, auto32 = prim.step_plan(B, dtype=np.float64), prim.step_plan(B, dtype=np.float32)
        old = (C.c_int32 * 4)()
        assert prim.lib.mg_step_plan_for(prim.handle, B, None, old) == 0
        assert (auto32["kernel"], auto32["fused"], auto32["workgroups"], auto32["lds_bytes"]) == \
            (prim.FRAMES_KERNEL_NAMES[old[0]], bool(old[1]), old[2], old[3])
        assert prim.step_plan(B) == auto32
        assert auto32["kernel"] == ("mg_frames_ws_kernel" if prim.kk >= 16 else "mg_frames_cs_kernel")
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 1)
        assert auto64 == prim.step_plan(B, dtype=np.float64) == prim.step_plan(B, dtype=np.float32)
        assert auto64["kernel"] == "mg_frames_ws_kernel"
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
        # and that is what runs: the step over float64 latents equals the tile-major kernel's frames; forced, the
        # chunk-stationary kernel gives the same bits
        S = np.random.default_rng(L).standard_normal((B, L))
        frames, _ = _fused_step(ctx, prim, S, prim.n_canonical_frames, prim.n_dim)
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 1)
        np.testing.assert_array_equal(_bits(frames), _bits(prim.back_project_frames(S, path=_capi.MG_PATH_MFMA)))
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 2)
        np.testing.assert_array_equal(_bits(frames), _bits(prim.back_project_frames(S, path=_capi.MG_PATH_MFMA)))
    finally:
        prim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 8, 16, 24, 32, 40, 48, 56, 57, 64, 65])
def test_instantiations_the_sweep_leaves_out(ctx, L):
    """The (kernel, KK, flags) combinations the host dispatch can select and the table above does not launch, at the widest
    width of every KK (and the narrowest of the first and the last), 17 candidates -- a full tile of 16 and a tail of one -- and
    65 for the 64-candidate scorer: the fused step in BOTH frames kernels with both root modes and latent types (KK <= 10),
    the scorers' float32 output, the Jacobian over float32 latents, the objective in one launch, and the MFMA sampler with
    its prefix sums in device memory (more than 16 components); at L = 65 the VALU scorer and Jacobian in their place.  Each
    against what its neighbours in the sweep compare with."""
    KK = kk_of(L)
    data = synthetic.make_primitive(seed=2000 + L, n_components=L, n_gmm=3, n_dim=79, name="inst%d" % L, **SHORT)
    cp = c_oracle.COraclePrimitive(data)
    rng = np.random.default_rng(L)
    S = rng.standard_normal((65, L))
    _reset(ctx)
    if 0 < KK <= MG_FUSE_MAX_KK:
        for mode in (1, 2):
            ctx.set_option(_capi.MG_OPT_ROOT_MODE, mode)
            prim = _capi.Primitive(ctx, data)
            try:
                for dtype in (np.float32, np.float64):
                    X = S[:17].astype(dtype)
                    model = cp.frames_f32model(X.astype(np.float64), root_split=mode == 2)
                    lp_sep = prim.gmm_log_prob(X, dtype=np.float32)
                    for kern, name in ((1, "mg_frames_ws_kernel"), (2, "mg_frames_cs_kernel")):
                        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, kern)
                        plan = prim.step_plan(len(X), dtype=dtype)
                        assert plan["fused"] and plan["kernel"] == name, (L, mode, kern, plan)
                        frames, logp = _fused_step(ctx, prim, X, prim.n_canonical_frames, prim.n_dim)
                        tag = "L %d mode %d %s kernel %d" % (L, mode, np.dtype(dtype).name, kern)
                        np.testing.assert_array_equal(_bits(frames), _bits(model), err_msg=tag)
                        np.testing.assert_array_equal(_bits(logp), _bits(lp_sep), err_msg=tag)
                        np.testing.assert_allclose(logp, cp.log_prob_f64(X.astype(np.float64)), rtol=3e-7, atol=1e-6, err_msg=tag)
                    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
            finally:
                prim.close()
        ctx.set_option(_capi.MG_OPT_ROOT_MODE, 0)
    prim = _capi.Primitive(ctx, data)
    tl = prim.n_canonical_frames - 1.0
    root = [{"type": "position", "t": tl, "weight": 1.0, "target": [30.0, None, -40.0]},
            {"type": "direction", "t": tl, "weight": 2.0, "target": [0.3, -1.0]}]
    cset = _capi.ConstraintSet(prim, root)
    try:
        assert prim.kk == KK and prim.kk_gmm == KK
        for dtype in (np.float32, np.float64):
            # the scorers' float32 output is their float64 sum rounded once: MG_OPT_SCORE_KERNEL 1 (17 candidates), 2 (65), VALU
            for opt, val, B in ((_capi.MG_OPT_SCORE_KERNEL, 1, 17), (_capi.MG_OPT_SCORE_KERNEL, 2, 65), (_capi.MG_OPT_FORCE_VALU_SCORE, 1, 17)):
                ctx.set_option(opt, val)
                X = S[:B].astype(dtype)
                e64, e32 = prim.score_constraints(cset, X, dtype=np.float64), prim.score_constraints(cset, X, dtype=np.float32)
                ctx.set_option(opt, 0)
                assert e32.dtype == np.float32
                np.testing.assert_array_equal(_bits(e32), _bits(e64.astype(np.float32)), err_msg="L %d option %d = %d" % (L, opt, val))
            if KK == 0:
                continue
            # the objective in one launch: the two separate calls' bits (the sweep's comparison)
            X = S[:17].astype(dtype)
            obj, err, lp = prim.objective(cset, X, 0.75, 1.25)
            err2, lp2 = prim.score_constraints(cset, X), prim.gmm_log_prob(X, dtype=np.float64)
            np.testing.assert_array_equal(err.view(np.uint64), err2.view(np.uint64))
            np.testing.assert_array_equal(lp.view(np.uint64), lp2.view(np.uint64))
            np.testing.assert_array_equal(obj.view(np.uint64), (0.75 * err2 + (-lp2) * 1.25).view(np.uint64))
        # the Jacobian over float32 latents: the oracle's at the same (rounded) rows
        X32 = S[:17].astype(np.float32)
        ref = orc.OraclePrimitive(data).log_likelihood_jac(X32.astype(np.float64))
        np.testing.assert_allclose(prim.gmm_log_prob_jac(X32), ref, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(ref).max()))
    finally:
        cset.close()
        prim.close()
    # 17 components: the sampler reads its prefix sums from device memory (MG_SAMPLE_ARG_K = 16)
    many = synthetic.make_primitive(seed=3000 + L, n_components=L, n_gmm=17, n_dim=15, name="inst%d_K17" % L, **SHORT)
    prim = _capi.Primitive(ctx, many)
    ledger = set(LEDGER)
    try:
        _sampler_family(ctx, prim, many, dict(name=many["name"]), rng)
    finally:
        LEDGER.clear()
        LEDGER.update(ledger)       # (the ledger is the sweep's: what ran here must not stand in for a shape of the table)
        prim.close()
        _reset(ctx)


@pytest.mark.gpu
def test_planner_step_across_widths(ctx):
    """The planner's one-launch step over options of five widths (KK 2, 8, 12, 14, 16) against the per-option chains, bit for
    bit; each option's winner is the first minimum of the oracle's errors on the candidates the step left on the device."""
    from morphablegraphs_amd.motion_state_graph import HipPrimitiveSet
    from test_gpu_adaptors import _options_step_raw
    widths = (5, 29, 44, 53, 64)
    prims = [synthetic.make_primitive(seed=300 + L, n_components=L, n_gmm=3 + i, name="w%02d" % L, **SHORT)
             for i, L in enumerate(widths)]
    names = [p["name"] for p in prims]
    joints, animated = synthetic.make_skeleton(19)
    hip_sk = _capi.Skeleton(joints, animated)
    cons = {}
    for n, p in zip(names, prims):
        tl = float(p["n_canonical_frames"] - 1)
        cons[n] = [{"type": "position", "t": tl, "weight": 1.0, "target": [10.0, None, 5.0]},
                   {"type": "direction", "t": tl / 2.0, "weight": 0.5, "target": [0.3, 1.0]},
                   {"type": "joint_position", "joint": "RightHand", "t": tl, "weight": 2.0, "target": [12.0, 90.0, 4.0]}]
    pset = HipPrimitiveSet(prims)
    for dtype in (np.float32, np.float64):
        pset.ctx.set_option(_capi.MG_OPT_OPTIONS_STEP, 1)
        b1, r1 = _options_step_raw(pset, names, cons, 777, 43, dtype, skeleton=hip_sk)
        pset.ctx.set_option(_capi.MG_OPT_OPTIONS_STEP, 0)
        b2, r2 = _options_step_raw(pset, names, cons, 777, 43, dtype, skeleton=hip_sk)
        assert b1 == b2
        for name, data in zip(names, prims):
            np.testing.assert_array_equal(r1[name][3].view(np.uint8), r2[name][3].view(np.uint8))   # candidates
            np.testing.assert_array_equal(r1[name][2].view(np.uint64), r2[name][2].view(np.uint64))  # errors
            np.testing.assert_array_equal(r1[name][0].view(np.uint64), r2[name][0].view(np.uint64))  # winning latent
            X = r2[name][3].astype(np.float64)
            c = cons[name]
            ref = (c_oracle.COraclePrimitive(data).keyframe_errors_f64(X, np.array(
                       [[0, c[0]["t"], 1.0, 10.0, np.nan, 5.0, 0, 0], [1, c[1]["t"], 0.5, 0.3, 1.0, 0.0, 0.0, 1.0]]))
                   + orc.OraclePrimitive(data).joint_position_residuals(X, c[2:], joints, animated)[:, 0])
            np.testing.assert_allclose(r2[name][2], ref, rtol=1e-10, atol=1e-8, err_msg=name)
            w = int(np.argmin(ref))
            assert r2[name][1] == r2[name][2][w], (name, dtype)
            np.testing.assert_array_equal(np.asarray(r2[name][0], dtype=np.float64), X[w])
    pset.ctx.set_option(_capi.MG_OPT_OPTIONS_STEP, 0)


@pytest.mark.gpu
def test_the_ledger_covers_every_width(ctx):
    """Every KK of the tile-major kernel, the chunk-stationary kernel (spilling instances forced), the mixture kernels (MFMA,
    LDS-resident, Jacobian, sampler) and the scorer ran and matched in the sweep above, for both latent dtypes -- and the
    library chose the chunk-stationary kernel by itself wherever it may.  (Shapes the sweep has not run yet -- a selection
    with -k -- are run here.)"""
    for s in SHAPES:
        _sweep(ctx, s)
    f32, f64 = "float32", "float64"
    want = {(fam, KK, dt) for fam in ("frames_ws", "frames_cs", "gmm_mfma", "gmm_lds", "sample_mfma", "sample_valu", "score_mfma")
            for KK in KKS for dt in (f32, f64)}
    want |= {("jac_mfma", KK, f64) for KK in KKS}
    want |= {("frames_cs_chosen", KK, dt) for KK in KKS for dt in (f32, f64) if not cs_spills(KK, dt == f64)}
    want |= {("gmm_valu", 0, f32), ("gmm_valu", 0, f64), ("step_fused", 2, f32), ("step_fused", 10, f64)}
    table = {}
    for fam, KK, dt in sorted(LEDGER):
        table.setdefault((fam, dt), []).append(KK)
    print("\nledger (family, dtype: KK)")
    for (fam, dt), kks in sorted(table.items()):
        print("  %-18s %-8s %s" % (fam, dt, kks))
    print("sampler: largest |x - x_ref| / (2^-20 sum_j |chol_ij| (1 + |z_j|)) = %.3f" % max(SAMPLER_RATIOS))
    missing = sorted(want - LEDGER)
    assert not missing, "shapes of the table no longer exercise: %s" % missing
