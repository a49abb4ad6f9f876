"""The error paths of the model-construction entry points (csrc/mg_construct.h states the rules): a call that is refused, before
or after it has allocated its device block, returns the documented status and leaves nothing behind, so the valid call that
follows at once returns MG_OK (the wrappers raise on anything else) with the host reference's result.  The refused calls
are invalid arguments; nothing here can fault, and the out-of-memory path is not exercised.

The valid calls use the smallest shapes.  k-means and the DTW / search results are exact (small dyadic rationals, integer
cells); EM and PCA are held to test_fpca_host.close's rule with no spread, 10 * 1e-13 * max|reference|."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dtw_host import same_bits  # noqa: E402
from test_fpca_host import close  # noqa: E402
from test_gpu_construction_shapes import lloyd_reference  # noqa: E402

from morphablegraphs_amd import _capi, dtw, fpca  # noqa: E402
from morphablegraphs_amd import gmm_trainer as gt  # noqa: E402
from morphablegraphs_amd import segmentation as seg  # noqa: E402

pytestmark = pytest.mark.gpu
BAD, UNS = _capi.MG_ERR_INVALID_ARGUMENT, _capi.MG_ERR_UNSUPPORTED
X4 = np.array([[0.0, 0.0], [0.0, 1.0], [10.0, 0.0], [10.0, 1.0]])      # n = 4, dim = 2: two pairs, k = 2
LABELS4 = np.array([0, 0, 1, 1], dtype=np.int32)


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def status_of(call, *args):
    with pytest.raises(_capi.MGError) as ei:
        call(*args)
    return ei.value.status


def test_kmeans_after_a_refused_call(ctx):
    init = np.array([[[0.0, 0.0], [10.0, 0.0]]])
    ref = lloyd_reference(X4, init[0])
    with ctx.buffers() as bufs:
        x_dev = bufs.upload(X4)
        call = lambda k, ini: _capi.kmeans_segments(ctx, x_dev, 4, 2, [0, 4], np.arange(4), k, 1, ini, None, 0, 300, 1e-4)      # noqa: E731
        assert status_of(call, _capi.MG_KMEANS_MAX_K + 1, None) == UNS
        assert status_of(call, 1, None) == UNS
        labels, centres, inertia, n_iter = call(2, init)
    assert labels.tolist() == ref["labels"].tolist() == [0, 0, 1, 1] and n_iter[0] == ref["n_iter"]
    assert same_bits(centres[0], ref["centres"]) and centres[0].tolist() == [[0.0, 0.5], [10.0, 0.5]]
    assert inertia[0] == ref["inertia"] == 1.0


def test_em_after_a_refused_call(ctx):
    ref = gt.em_from_labels_host(X4, LABELS4, 2)
    with ctx.buffers() as bufs:
        x_dev = bufs.upload(X4)
        assert status_of(_capi.gmm_em_fit, ctx, x_dev, 4, 2, [_capi.MG_GMM_EM_MAX_K + 1], np.zeros((1, 4), dtype=np.int32)) == UNS
        assert status_of(_capi.gmm_em_fit, ctx, x_dev, 4, 2, [2], np.array([[0, 0, 1, 2]], dtype=np.int32)) == BAD      # a label outside [0, K)
        fit = _capi.gmm_em_fit(ctx, x_dev, 4, 2, [2], LABELS4[None])[0]
    assert fit["status"] == _capi.MG_GMM_EM_CONVERGED and ref["converged"] and fit["n_iter"] == ref["n_iter"]
    assert fit["labels"].tolist() == ref["labels"].tolist() == [0, 0, 1, 1]
    for key in ("weights", "means", "covariances", "precisions_cholesky", "lower_bounds", "score"):
        close("EM n = 4 " + key, fit[key], ref[key], 0.0)


def test_pca_after_a_refused_call(ctx):
    A = np.array([[1.0, 2.0], [3.0, 5.0], [4.0, 1.0]])
    ref = fpca.pca_fit_host(A)
    long_side = _capi.MG_PCA_MAX_LONG + 1
    with ctx.buffers() as bufs:
        column, centred = bufs.malloc(8 * long_side), bufs.malloc(8 * long_side)      # the full size of the refused shape
        a_dev, c_dev = bufs.upload(A), bufs.malloc(A.nbytes)
        assert status_of(_capi.pca_fit, ctx, column, long_side, 1, centred) == UNS
        assert status_of(_capi.pca_fit, ctx, a_dev, 0, 2, c_dev) == BAD
        fit = _capi.pca_fit(ctx, a_dev, 3, 2, c_dev)
        assert same_bits(ctx.download(c_dev, A.shape, np.float64), ref["centred"])
    assert fit["status"] == _capi.MG_PCA_CONVERGED and same_bits(fit["mean"], ref["mean"])
    close("PCA 3 x 2 singular values", fit["singular_values"], ref["singular_values"], 0.0)
    close("PCA 3 x 2 eigenvectors", fit["vt"], ref["vt"], 0.0)


def test_dtw_paths_after_refused_calls(ctx):
    """Refused by the offsets check, then by the flag the non-finite kernel sets (after the allocation), then valid."""
    grids = [np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[3.0, 1.0, 2.0], [1.0, 2.0, 0.0]])]      # 2 and 3 frames, 2 reference frames
    with ctx.buffers() as bufs:
        s_dev = bufs.upload(np.concatenate([g.reshape(-1) for g in grids]))
        assert status_of(dtw._paths_on_device, ctx, bufs, s_dev, 2, np.array([0, 2, 2]), False) == BAD
    broken = [grids[0], grids[1].copy()]
    broken[1][1, 2] = np.nan
    assert status_of(dtw.paths_from_grids, broken, True, ctx) == BAD
    for S, r in zip(grids, dtw.paths_from_grids(grids, ctx=ctx)):
        D, path, warp = dtw.dtw_paths_host(S)
        assert same_bits(r["D"], D) and r["total"] == D[-1, -1]
        assert [tuple(int(v) for v in p) for p in r["path"]] == path and r["warping_function"].tolist() == warp


def test_segment_search_after_refused_calls(ctx):
    """Refused for its mode, then by the flag the non-finite kernel sets (after the allocation), then valid."""
    start, end = np.array([3.0, 1.0, 1.0, 2.0]), np.array([2.0, 4.0, 0.5, 0.5])      # one motion of 4 frames
    with ctx.buffers() as bufs:
        s_dev, e_dev, p_dev, c_dev = bufs.upload(start), bufs.upload(end), bufs.malloc(8), bufs.malloc(4)
        assert status_of(_capi.segment_search, ctx, s_dev, e_dev, [0, 4], 7, 1.0, 10, [0, 1], p_dev, c_dev) == BAD
    assert status_of(seg.segment_search, [np.array([3.0, np.inf, 1.0, 2.0])], [end], seg.SINGLE, 1.0, 10, ctx) == BAD
    pairs = seg.segment_search([start], [end], seg.SINGLE, ctx=ctx)[0]
    assert pairs.tolist() == [list(p) for p in seg.segment_search_host(start, end, seg.SINGLE)] == [[1, 2]]
    start = np.array([1.0, 3.0, 3.0, 1.0])      # two instances; the window of the first ends at the second
    pairs = seg.segment_search([start], [end], seg.MULTI, threshold=0.0, min_segment_size=0, ctx=ctx)[0]
    assert pairs.tolist() == [list(p) for p in seg.segment_search_host(start, end, seg.MULTI, 0.0, 0)] == [[0, 2]]
