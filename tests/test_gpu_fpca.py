"""The device functional PCA (mg_spline_fit_batch, mg_pca_fit, mg_pca_project / mg_pca_backproject and the classes of
morphablegraphs_amd.fpca) against the reference's construction/fpca as recorded in tests/golden/fpca.npz, under the rule
of tests/test_fpca_host.py: per quantity, |ours - reference| <= 10 * max(spread_q, 1e-13 * max|q_reference|)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fpca_host import CASES, CONSTRUCT, KIND, SPATIAL, TEMPORAL, _FakeTrainer, case, check_pca, close, sub  # noqa: E402

from morphablegraphs_amd import _capi, fpca  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def device_spline_fit(ctx, motions, n_basis):
    motions = np.ascontiguousarray(motions, dtype=np.float64)
    n, n_frames, n_dims = motions.shape
    P, _ = fpca.spline_fit_operator(n_basis, n_frames)
    m_dev, p_dev, c_dev = ctx.upload(motions), ctx.upload(P), ctx.malloc(8 * n * n_basis * n_dims)
    try:
        _capi.spline_fit_batch(ctx, m_dev, n, n_frames, n_dims, p_dev, n_basis, c_dev)
        return ctx.download(c_dev, (n, n_basis, n_dims), np.float64)
    finally:
        for b in (m_dev, p_dev, c_dev):
            b.free()


def device_pca(ctx, A, centre=True):
    A = np.ascontiguousarray(A, dtype=np.float64)
    a_dev, c_dev = ctx.upload(A), ctx.malloc(A.nbytes)
    try:
        fit = _capi.pca_fit(ctx, a_dev, A.shape[0], A.shape[1], c_dev, centre)
        fit["centred"] = ctx.download(c_dev, A.shape, np.float64)
        return fit
    finally:
        a_dev.free()
        c_dev.free()


def spatial_input(c, i):
    return c["prepared"] if KIND[i] == "construct" else c["input"]


def temporal_case(i):
    c = case(i)
    if KIND[i] == "construct":
        cfg = c["config"]
        return sub(c, "t_"), c["warps"], cfg["n_basis_functions_temporal"], cfg["precision_temporal"], cfg["npc_temporal"], "construct temporal"
    return c, c["input"], c["n_basis"], c["fraction"], c["n_pc"], c["name"]


@pytest.mark.parametrize("i", SPATIAL + CONSTRUCT)
def test_spline_fit_batch_reproduces_splrep(ctx, i):
    c = case(i)
    ours = device_spline_fit(ctx, spatial_input(c, i), c["n_basis"])
    close(c["name"] + " functional data", ours, c["functional_data"], c["spread_functional_data"])


@pytest.mark.parametrize("i", SPATIAL + CONSTRUCT)
def test_spline_fit_is_reproducible_and_batch_independent(ctx, i):
    c = case(i)
    data = spatial_input(c, i)
    a, b = device_spline_fit(ctx, data, c["n_basis"]), device_spline_fit(ctx, data, c["n_basis"])
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for r in (0, len(data) // 2, len(data) - 1):
        alone = device_spline_fit(ctx, data[r:r + 1], c["n_basis"])
        assert np.array_equal(alone[0].view(np.uint64), a[r].view(np.uint64)), "motion %d alone differs from the batch" % r


@pytest.mark.parametrize("i", TEMPORAL + CONSTRUCT)
def test_temporal_spline_fit_single_channel(ctx, i):
    c, w, n_basis, _, _, name = temporal_case(i)
    coeffs = device_spline_fit(ctx, w[:, :, None], n_basis)[:, :, 0]
    host = fpca.spline_fit_host(w[:, :, None], n_basis)[:, :, 0]
    close(name + " control points vs host", coeffs, host, 0.0)
    close(name + " z-t functional data", fpca.temporal_functional_data_host(coeffs, w), c["functional_data"], c["spread_functional_data"])


def pca_quantities(ctx, fit, A_shape, fraction, n_pc):
    k, npc = fpca.npc_from_singular_values(fit["singular_values"], A_shape, fraction)
    ev = np.ascontiguousarray(fit["vt"][:k][:npc if n_pc is None else n_pc])
    n, p = A_shape
    x_dev, v_dev, m_dev = ctx.upload(fit["centred"]), ctx.upload(ev), ctx.upload(fit["mean"])
    low_dev, high_dev = ctx.malloc(8 * n * len(ev)), ctx.malloc(8 * n * p)
    try:
        _capi.pca_project(ctx, x_dev, v_dev, n, p, len(ev), low_dev)
        _capi.pca_backproject(ctx, low_dev, v_dev, m_dev, n, p, len(ev), high_dev)
        low, high = ctx.download(low_dev, (n, len(ev)), np.float64), ctx.download(high_dev, (n, p), np.float64)
    finally:
        for b in (x_dev, v_dev, m_dev, low_dev, high_dev):
            b.free()
    return {"mean": fit["mean"], "singular_values": fit["singular_values"], "npc": npc, "eigenvectors": ev, "low_vecs": low, "backprojection": high}


@pytest.mark.parametrize("i", CASES)
def test_pca_fit_and_projection_reproduce_the_reference(ctx, i):
    if KIND[i] == "temporal":
        c, _, _, fraction, n_pc, name = temporal_case(i)
        runs = [(c, c["functional_data"], fraction, n_pc, name)]
    else:
        c = case(i)
        fd = c["functional_data"]
        runs = [(c, fd.reshape(len(fd), -1), c["fraction"], c["n_pc"], c["name"])]
        if KIND[i] == "construct":
            t, _, _, fraction, n_pc, name = temporal_case(i)
            runs.append((t, t["functional_data"], fraction, n_pc, name))
    for c, A, fraction, n_pc, name in runs:
        fit = device_pca(ctx, A)
        assert fit["status"] == _capi.MG_PCA_CONVERGED and 1 <= fit["n_sweeps"] <= _capi.MG_PCA_MAX_SWEEPS
        print("%s: %d sweeps" % (name, fit["n_sweeps"]))
        check_pca(name, c, pca_quantities(ctx, fit, A.shape, fraction, n_pc), min(A.shape))
        assert np.all(np.diff(fit["singular_values"]) <= 0)
        for row in fit["vt"]:
            assert row[np.argmax(np.abs(row))] > 0                       # the sign rule
        # orthonormality: at most 10 x what LAPACK's SVD of the same centred matrix shows
        m = min(A.shape)
        _, _, Vt = np.linalg.svd(fit["centred"], full_matrices=False)
        lapack = float(np.max(np.abs(Vt @ Vt.T - np.eye(m))))
        ours = float(np.max(np.abs(fit["vt"] @ fit["vt"].T - np.eye(m))))
        print("%s: max|Vt Vt^T - I| ours %.3e, LAPACK %.3e" % (name, ours, lapack))
        assert ours <= 10 * lapack
        again = device_pca(ctx, A)
        for key in ("mean", "singular_values", "vt", "centred"):
            assert np.array_equal(again[key].view(np.uint64), fit[key].view(np.uint64)), key
        assert again["n_sweeps"] == fit["n_sweeps"]


@pytest.mark.parametrize("i", SPATIAL + CONSTRUCT)
def test_pca_functional_data_class(ctx, i):
    c = case(i)
    obj = fpca.HipPCAFunctionalData(spatial_input(c, i), n_basis=c["n_basis"], fraction=c["fraction"], n_pc=c["n_pc"], ctx=ctx)
    close(c["name"] + " class functional data", obj.functional_data, c["functional_data"], c["spread_functional_data"])
    assert obj.origin_shape == c["functional_data"].shape and obj.reshaped_fd.shape == (len(c["input"]), c["mean"].size)
    ours = {"mean": obj.mean, "singular_values": obj.singular_values_, "npc": obj.npc_, "eigenvectors": obj.eigenvectors, "low_vecs": obj.low_vecs,
            "backprojection": obj.backproject_data(obj.low_vecs)}
    check_pca(c["name"] + " class", c, ours, min(obj.reshaped_fd.shape))
    assert np.array_equal(obj.project_data(obj.reshaped_fd).view(np.uint64), obj.low_vecs.view(np.uint64))
    back = obj.from_pca_to_data(ours["backprojection"], obj.origin_shape)
    assert back.shape == obj.origin_shape and back[2, 1, 0] == ours["backprojection"][2, c["functional_data"].shape[2]]
    sp = fpca.HipFPCASpatialData(c["n_basis"], c["n_pc"], c["fraction"], ctx=ctx)
    sp.fit_motion_dictionary({"m%d" % r: m for r, m in enumerate(spatial_input(c, i))})
    assert sp.fileorder[1] == "m1" and np.array_equal(sp.fpcaobj.low_vecs.view(np.uint64), obj.low_vecs.view(np.uint64))
    obj.close()
    sp.fpcaobj.close()


@pytest.mark.parametrize("i", TEMPORAL + CONSTRUCT)
def test_time_semantic_class(ctx, i):
    c, w, n_basis, fraction, n_pc, name = temporal_case(i)
    ft = fpca.HipFPCATimeSemantic(n_basis, n_components_temporal=n_pc, precision_temporal=fraction, ctx=ctx)
    ft.temporal_semantic_data = w
    ft.functional_pca()
    close(name + " class functional data", ft.fpca_data + ft.mean_vec, c["functional_data"], c["spread_functional_data"])
    ours = {"mean": ft.mean_vec, "singular_values": ft.singular_values_, "npc": ft.npc, "eigenvectors": ft.eigenvectors, "low_vecs": ft.lowVs,
            "backprojection": ft.lowVs @ ft.eigenvectors + ft.mean_vec}
    check_pca(name + " class", c, ours, min(ft.fpca_data.shape))


def test_run_pca_quirk_on_the_device(ctx):
    c = case([str(case(i)["name"]) for i in CASES].index("spatial_tall_n120_f20_d3"))
    fd = c["functional_data"]
    A = fd.reshape(len(fd), -1)
    A = A - A.mean(axis=0)
    Vt, npc = fpca.run_pca(A, c["fraction"], ctx=ctx)
    assert Vt.shape == (A.shape[1] - 1, A.shape[1]) and npc == int(c["npc"])
    ok = np.asarray(c["resolved"], dtype=bool)
    close("run_pca eigenvectors", Vt[:len(ok)][ok], c["eigenvectors"][ok], c["spread_eigenvectors"])


def _expect(status, call, *args):
    with pytest.raises(_capi.MGError) as e:
        call(*args)
    assert e.value.status == status, e.value


def test_limits_are_unsupported(ctx):
    """Every stated limit, one step past it, on buffers of the full size of those shapes: were a check ever lost, the
    kernels would run inside their buffers and the test would fail on the missing error."""
    uns = _capi.MG_ERR_UNSUPPORTED
    for n_basis, n_frames in ((_capi.MG_FPCA_MAX_BASIS + 1, 200), (8, _capi.MG_FPCA_MAX_FRAMES + 1)):
        bufs = [ctx.malloc(8 * n_frames * 2), ctx.malloc(8 * n_basis * n_frames), ctx.malloc(8 * n_basis * 2)]
        try:
            _expect(uns, _capi.spline_fit_batch, ctx, bufs[0], 1, n_frames, 2, bufs[1], n_basis, bufs[2])
        finally:
            for b in bufs:
                b.free()
    for n, p in ((_capi.MG_PCA_MAX_SHORT + 1, _capi.MG_PCA_MAX_SHORT + 1), (1, _capi.MG_PCA_MAX_LONG + 1), (_capi.MG_PCA_MAX_LONG + 1, 1)):
        a_dev, c_dev = ctx.malloc(8 * n * p), ctx.malloc(8 * n * p)
        try:
            _expect(uns, _capi.pca_fit, ctx, a_dev, n, p, c_dev)
        finally:
            a_dev.free()
            c_dev.free()
    big = _capi.MG_PCA_PROJECT_MAX_SIDE + 1
    wide, one = ctx.malloc(8 * big), ctx.malloc(8 * big)
    small = ctx.malloc(64)
    try:
        _expect(uns, _capi.pca_project, ctx, wide, one, 1, big, 1, small)            # p past the limit
        _expect(uns, _capi.pca_project, ctx, wide, small, big, 1, 1, one)            # n past the limit
        _expect(uns, _capi.pca_backproject, ctx, small, one, None, 1, big, 1, wide)
        _expect(uns, _capi.pca_backproject, ctx, wide, small, None, big, 1, 1, one)
    finally:
        for b in (wide, one, small):
            b.free()
    with pytest.raises(ValueError):
        fpca.run_pca(np.zeros((1, _capi.MG_PCA_MAX_LONG + 1)), ctx=ctx)               # the classes check before they allocate


def test_pca_fit_rejects_non_finite_input(ctx):
    A = np.random.default_rng(3).standard_normal((12, 7))
    A[5, 2] = np.nan
    a_dev, c_dev = ctx.upload(A), ctx.malloc(A.nbytes)
    try:
        _expect(_capi.MG_ERR_INVALID_ARGUMENT, _capi.pca_fit, ctx, a_dev, 12, 7, c_dev)
    finally:
        a_dev.free()
        c_dev.free()


def _construct(ctx, c, version):
    frames = {"m%03d" % r: m for r, m in enumerate(c["input"])}
    warps = {"m%03d" % r: w for r, w in enumerate(c["warps"])}
    return fpca.construct_motion_primitive_model(frames, warps, c["config"], n_animated_joints=int(c["n_joints"]), name="walk", version=version,
                                                 frame_time=1.0 / 30, gmm_trainer=_FakeTrainer(), ctx=ctx, return_stages=True)


@pytest.mark.parametrize("version", [1, 3])
@pytest.mark.parametrize("i", CONSTRUCT)
def test_constructed_model_back_projects_its_training_latents(ctx, i, version):
    """The dict as construct_motion_primitive_model returns it (v1 directly, v3 through model_io, as a model file is read),
    loaded into HipMotionPrimitive: back_project_spatial_coeffs of its own training latents against the golden file's
    back-projection with the root rescale applied.  Both loaders read the spatial model and the mixture over the
    concatenated spatial | temporal latents, and no time model."""
    from morphablegraphs_amd import model_io
    from morphablegraphs_amd.motion_primitive import HipMotionPrimitive
    c = case(i)
    data, stages = _construct(ctx, c, version)
    ok = np.asarray(c["resolved"], dtype=bool)
    close("construct motion parameters (resolved)", stages["motion_parameters"][:, :len(ok)][:, ok], c["motion_parameters"][:, :len(ok)][:, ok],
          c["spread_motion_parameters"])
    close("construct scaled mean", stages["spatial"]["mean"], c["scaled_mean"], c["spread_scaled_mean"])
    close("construct scaled eigenvectors (resolved)", stages["spatial"]["eigenvectors"][ok], c["scaled_eigenvectors"][ok], c["spread_scaled_eigenvectors"])
    prim = HipMotionPrimitive(context=ctx)
    prim._initialize_from_json(model_io.primitive_dict_from_json(data))
    n_s = prim.get_n_spatial_components()
    assert n_s == len(c["eigenvectors"]) and not prim.has_time_parameters
    assert prim.gaussian_mixture_model is not None and np.asarray(data["gmm"]["means"] if version == 3 else data["gmm_means"]).shape[1] == n_s + len(
        c["t_eigenvectors"])
    n, nb, d = c["functional_data"].shape
    ours = np.stack([prim.back_project_spatial_coeffs(s[:n_s]) for s in stages["motion_parameters"]])
    close("MotionPrimitive back-projection of the training latents", ours.reshape(n, nb * d), c["scaled_backprojection"],
          c["spread_scaled_backprojection"])


def test_v2_model_with_a_time_model_does_not_load_as_in_the_reference(ctx):
    """The v2 dict carries eigen_vectors_time as the reference's constructor writes it, (npc_temporal, n_basis_time); the
    loaders (the reference's and ours) read (n_basis_time, n_time_components), and npc < n_basis always (run_pca returns at
    most min - 1 rows): HipMotionPrimitive refuses the dict."""
    from morphablegraphs_amd.motion_primitive import HipMotionPrimitive
    c = case(CONSTRUCT[0])
    data, _ = _construct(ctx, c, 2)
    et = np.array(data["eigen_vectors_time"])
    assert et.shape == c["t_eigenvectors"].shape and et.shape[1] == data["n_basis_time"] and et.shape[0] < et.shape[1]
    with pytest.raises(ValueError):
        HipMotionPrimitive(context=ctx)._initialize_from_json(data)


def test_device_trainer_in_the_construct_leg(ctx):
    """The whole leg with HipGMMTrainer on the concatenated latents; the v3 dict loads through model_io."""
    from morphablegraphs_amd import model_io
    c = case(CONSTRUCT[0])
    frames = {"m%03d" % r: m for r, m in enumerate(c["input"])}
    warps = {"m%03d" % r: w for r, w in enumerate(c["warps"])}
    np.random.seed(5)
    data = fpca.construct_motion_primitive_model(frames, warps, c["config"], animated_joints=["Hips", "Spine"], name="walk", version=3,
                                                 frame_time=1.0 / 30, ctx=ctx)
    legacy = model_io.primitive_dict_from_json(data)
    d = c["motion_parameters"].shape[1]
    K = len(legacy["gmm_weights"])
    assert K >= 1 and np.array(legacy["gmm_means"]).shape == (K, d) and np.array(legacy["gmm_covars"]).shape == (K, d, d)
    assert abs(sum(legacy["gmm_weights"]) - 1.0) < 1e-12
