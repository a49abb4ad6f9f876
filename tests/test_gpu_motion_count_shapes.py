"""The construction kernels past one launch's worth of motions (tests/motion_count_cases.py): the second launch of the loops
that step by 65535 motions, the second reference chunk of the pair costs, and the strided second legs of the reductions of
csrc/mg_spatial_align.hip.  Every comparison is exact (integers or bits) except the alignment's root channels and transforms,
which keep the project's 4 ulp against spatial_alignment.align_motions_spatially_host.  Every output is filled with a
sentinel first, and has slack behind it: a cell a launch did not reach, or one written past the end, shows.
tests/test_motion_count_shapes_host.py asserts on the host that every count used here lies on the side of its cut it names."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_count_cases as mc  # noqa: E402
from test_spatial_alignment_host import same_bits  # noqa: E402

from morphablegraphs_amd import _capi, dtw  # noqa: E402

pytestmark = pytest.mark.gpu
ULPS = 4            # tests/test_gpu_spatial_alignment.py
SLACK = 64          # sentinel values behind every output
S = mc.SENTINEL


@pytest.fixture(scope="module")
def ctx():
    from morphablegraphs_amd.motion_primitive import get_context
    return get_context(0)


def ulps_apart(a, b):
    """tests/test_gpu_spatial_alignment.py: the largest |a - b| in units of the spacing of the larger magnitude."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(np.float64).tiny))))


def filled(bufs, n, dtype=np.float64):
    """A device buffer of n + SLACK sentinels."""
    return bufs.upload(np.full(n + SLACK, S, dtype=dtype))


def fetch(ctx, buf, n, dtype=np.float64):
    """(the n values, True if the slack behind them still holds the sentinel)."""
    a = ctx.download(buf, (n + SLACK,), dtype)
    return a[:n], bool(np.all(a[n:] == dtype(S)))


# ---- mg_align_motions_spatially ------------------------------------------------------------------------------------------------
def _align(ctx, bufs, table, off, out, tr):
    _capi.align_motions_spatially(ctx, bufs.upload(table), off, mc.ALIGN_D, 0, mc.ALIGN_REF, out, tr)


@pytest.mark.parametrize("n_motions", mc.ALIGN_COUNTS)
def test_alignment_counts(ctx, n_motions):
    """sa_align_kernel's second launch (n0 = 65535: 65536 motions reach it with one motion, 65539 with four; 255 .. 65535 stay
    in one launch), with blocks_x = 3 from the 65-frame motion 65535 that opens it.  The 64 distinct motions and the long ones
    against the host at 4 ulp; every other motion n and its transform row in the bits of its twin n % 64."""
    motions, host, host_t = mc.align_distinct()
    lengths, off, table = mc.align_table(n_motions)
    total = int(off[-1]) * mc.ALIGN_D
    with ctx.buffers() as bufs:
        out_dev, t_dev = filled(bufs, total), filled(bufs, 5 * n_motions)
        _align(ctx, bufs, table, off, out_dev, t_dev)
        out, out_slack = fetch(ctx, out_dev, total)
        t, t_slack = fetch(ctx, t_dev, 5 * n_motions)
    assert out_slack and t_slack, "written past offsets[-1] * D or past 5 * n_motions"
    out, t = out.reshape(-1, mc.ALIGN_D), t.reshape(n_motions, 5)
    assert not np.any(out == S) and not np.any(t == S), "motions %s were never written" % np.flatnonzero(np.any(t == S, axis=1))[:5]
    # the distinct motions against the host
    firsts = sorted({mc.align_twin(n) for n in range(min(n_motions, 2 * mc.ALIGN_K))} | {n for n in mc.ALIGN_LONG if n < n_motions})
    assert len(firsts) == mc.ALIGN_K + sum(n < n_motions for n in mc.ALIGN_LONG)
    worst = 0.0
    for n in firsts:
        key = mc.align_key(n)
        worst = max(worst, ulps_apart(out[off[n]:off[n + 1]], host[key]), ulps_apart(t[n], host_t[key]))
        assert np.all(out[off[n], :3] == 0.0), n
    print("%d motions: the distinct motions at most %.3g ulp from the host" % (n_motions, worst))
    assert worst <= ULPS, worst
    # every motion in the bits of its twin
    ids = np.arange(n_motions)
    plain = np.ones(n_motions, dtype=bool)
    plain[[n for n in mc.ALIGN_LONG if n < n_motions]] = False
    for k in range(mc.ALIGN_K):
        idx = np.flatnonzero(plain & (ids % mc.ALIGN_K == k))
        first, f = int(idx[0]), int(lengths[idx[0]])
        rows = out[off[idx][:, None] + np.arange(f)[None, :]]
        same = np.all(rows.view(np.uint64) == out[off[first]:off[first + 1]].view(np.uint64)[None], axis=(1, 2))
        same &= np.all(t[idx].view(np.uint64) == t[first].view(np.uint64)[None], axis=1)
        assert same.all(), "motion %d differs from its twin %d" % (idx[np.argmin(same)], first)
    # the motions next to the seam and the last one, by name
    for n in (mc.GRID_Y - 1, mc.GRID_Y, mc.GRID_Y + 1, n_motions - 1):
        if n < n_motions:
            key = mc.align_key(n)
            assert ulps_apart(out[off[n]:off[n + 1]], host[key]) <= ULPS, "motion %d" % n
            assert same_bits(out[off[n]:off[n + 1]], out[off[mc.align_twin(n)]:off[mc.align_twin(n) + 1]]), "motion %d" % n
    for n in (mc.GRID_Y, n_motions - 1):
        if n < n_motions:
            assert ulps_apart(t[n], host_t[mc.align_key(n)]) <= ULPS and same_bits(t[n], t[mc.align_twin(n)]), "transform row %d" % n


@pytest.mark.parametrize("what,bad,n_motions,named", mc.ALIGN_REFUSALS, ids=["_".join(str(n) for n in r[1]) for r in mc.ALIGN_REFUSALS])
def test_alignment_refusals_name_the_first_motion(ctx, what, bad, n_motions, named):
    """sa_heading_check_kernel: a lane's second motion (n += SA_BLOCK: motions 261 and 700 are lane 5's second and lane 188's
    third; 256 is lane 0's second, 65536 its 257th) and the minimum over the lanes that names the first refused motion.  A
    refusal by the check kernel: nothing is written, and a good call succeeds afterwards."""
    lengths, off, table = mc.align_table(n_motions)
    total = int(off[-1]) * mc.ALIGN_D
    with ctx.buffers() as bufs:
        out_dev, t_dev = filled(bufs, total), filled(bufs, 5 * n_motions)
        with pytest.raises(_capi.MGError, match=r"motion %d:" % named) as ei:
            _align(ctx, bufs, mc.no_heading(table, off, bad), off, out_dev, t_dev)
        assert ei.value.status == _capi.MG_ERR_INVALID_ARGUMENT
        out, out_slack = fetch(ctx, out_dev, total)
        t, t_slack = fetch(ctx, t_dev, 5 * n_motions)
        assert np.all(out == S) and np.all(t == S) and out_slack and t_slack
        _align(ctx, bufs, table, off, out_dev, t_dev)
        out, out_slack = fetch(ctx, out_dev, total)
    assert out_slack and not np.any(out == S)
    _, host, _ = mc.align_distinct()
    n = n_motions - 1
    assert ulps_apart(out.reshape(-1, mc.ALIGN_D)[off[n]:off[n + 1]], host[mc.align_key(n)]) <= ULPS


# ---- mg_prepare_aligned_frames -------------------------------------------------------------------------------------------------
def _prepare(ctx, x):
    with ctx.buffers() as bufs:
        out_dev = filled(bufs, x.size)
        scale = _capi.prepare_aligned_frames(ctx, bufs.upload(x), x.shape[0], x.shape[1], x.shape[2], 1, out_dev)
        out, slack = fetch(ctx, out_dev, x.size)
    assert slack, "written past the table"
    return out.reshape(x.shape), scale


@pytest.mark.parametrize("shape", mc.PREPARE_SHAPES, ids=str)
def test_prepare_counts(ctx, shape):
    """pa_max_final_kernel's second visit (b += SA_BLOCK: 65537 rows make 257 partials, 65536 rows 256) and
    pa_max_partial_kernel's grid-stride leg (262145 rows against 1024 workgroups of 256; 262144 rows have none).  The three
    maxima stand where only those legs see them: channel 0 in row 65536 (partial 256), channel 1 in row 262144 (workgroup 0's
    second stride), channel 2, negative, in the last row.  Scale: the planted magnitudes; output: the host's bits."""
    x = mc.prepare_table(shape)
    want, want_scale = mc.prepare_reference(x)
    assert want_scale.tolist() == list(mc.PLANTED)
    out, scale = _prepare(ctx, x)
    assert scale.tolist() == list(mc.PLANTED), scale
    assert same_bits(out, want)
    rows = out.reshape(-1, shape[2])
    r0, r1, r2 = mc.planted_rows(len(rows))
    assert rows[r0, 0] == 1.0 and rows[r1, 1] == 1.0 and rows[r2, 2] == -1.0
    # a quaternion flip in the last row: the exact negative of frame 0 of motion 0 comes back as that quaternion
    y = np.array(x)
    y[-1, -1, 3:7] = -y[0, 0, 3:7]
    want, _ = mc.prepare_reference(y)
    out, scale = _prepare(ctx, y)
    assert scale.tolist() == list(mc.PLANTED) and same_bits(out, want) and same_bits(out[-1, -1, 3:7], y[0, 0, 3:7])


def test_prepare_zero_channel_at_262145_rows(ctx):
    """One root channel zero everywhere, past the grid stride: the scale is ones and nothing is scaled."""
    z = np.array(mc.prepare_table(mc.PREPARE_SHAPES[-1]))
    z[:, :, 1] = 0.0
    want, want_scale = mc.prepare_reference(z)
    out, scale = _prepare(ctx, z)
    assert np.all(want_scale == 1.0) and np.all(scale == 1.0)
    assert same_bits(out, want) and same_bits(out[:, :, :3], z[:, :, :3])


# ---- mg_dtw_distance_grids, mg_dtw_paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fr", mc.DTW_REF_FRAMES)
@pytest.mark.parametrize("n_motions", mc.DTW_COUNTS)
def test_dtw_counts(ctx, n_motions, fr):
    """dtw_distance_grids_kernel's and dtw_paths_kernel's second launch (n0 = 65535: 65536 motions reach it with one motion,
    65539 with four; 65535 stay in one), motions of 1, 2, 3 frames in turn against a reference motion of 1, 2, 3 frames.
    Grids, accumulated cost, totals, path lengths, paths and warping functions: the integer reference, exactly, in the
    layouts of include/mg_hip.h; what the kernels do not write keeps the sentinel."""
    c = mc.dtw_case(n_motions, fr)
    off, total = c["off"], int(c["off"][-1])
    with ctx.buffers() as bufs:
        a_dev, b_dev = bufs.upload(mc.clouds_of(c["ref"])), bufs.upload(mc.clouds_of(c["ys"]))
        s_dev, d_dev, t_dev = filled(bufs, fr * total), filled(bufs, fr * total), filled(bufs, n_motions)
        p_dev, l_dev, w_dev = filled(bufs, 2 * c["n_pairs"], np.int32), filled(bufs, n_motions, np.int32), filled(bufs, n_motions * fr, np.int32)
        _capi.dtw_distance_grids(ctx, a_dev, fr, b_dev, off, 1, None, s_dev)
        grids, slack = fetch(ctx, s_dev, fr * total)
        assert slack and same_bits(grids, c["grids"]), "grids: first wrong cell %d" % int(np.argmax(grids != c["grids"]))
        _capi.dtw_paths(ctx, s_dev, fr, off, d_dev, t_dev, p_dev, l_dev, w_dev)
        for name, buf, want in (("accumulated", d_dev, c["acc"]), ("totals", t_dev, c["totals"]), ("paths", p_dev, c["paths"].reshape(-1)),
                                ("path lengths", l_dev, c["path_len"]), ("warping", w_dev, c["warp"].reshape(-1))):
            got, slack = fetch(ctx, buf, want.size, want.dtype.type)
            assert slack, name + ": written past the end"
            assert got.tobytes() == want.tobytes(), "%s: first wrong entry %d of %d" % (name, int(np.argmax(got != want)), want.size)


# ---- mg_dtw_pair_costs ---------------------------------------------------------------------------------------------------------------
def _pair_costs(ctx, n_motions, refs):
    lengths, off, ys = mc.integer_motions(n_motions)
    n_refs = n_motions if refs is None else len(refs)
    want = mc.pair_costs_reference(lengths, off, ys, np.arange(n_motions) if refs is None else refs)
    with ctx.buffers() as bufs:
        c_dev, o_dev = bufs.upload(mc.clouds_of(ys)), filled(bufs, n_refs * n_motions)
        t0 = time.time()
        assert _capi.dtw_pair_costs(ctx, c_dev, off, 1, None, refs, o_dev) == n_refs
        seconds = time.time() - t0
        got, slack = fetch(ctx, o_dev, n_refs * n_motions)
    print("mg_dtw_pair_costs: %d x %d pairs in %.3f s" % (n_refs, n_motions, seconds))
    assert slack, "written past the matrix"
    got = got.reshape(n_refs, n_motions)
    wrong = np.argwhere(got != want)
    assert same_bits(got, want), "%d wrong entries, the first at (row, motion) %s" % (len(wrong), wrong[:1].tolist())


def test_pair_costs_second_motion_chunk(ctx):
    """mg_dtw_pair_costs' second n0 chunk: 65539 motions, reference motions 0, 65535, 65536 and the last; the second chunk has
    nb = 4, so chunk_r changes from 64 to 65535 between the chunks.  The whole matrix, exactly."""
    _pair_costs(ctx, mc.PAIRS_A["n"], np.array(mc.PAIRS_A["refs"], dtype=np.int64))


def test_pair_costs_second_reference_chunk(ctx):
    """mg_dtw_pair_costs' second r0 chunk: 65535 motions make chunk_r = 2^22 / 65535 = 64, and 66 reference indices (not in
    order, one repeated, 65534 among them) a second launch with r0 = 64.  4.3 M one-frame-scale pairs; the whole matrix, exactly."""
    _pair_costs(ctx, mc.PAIRS_B["n"], mc.pairs_b_refs())


def test_pair_costs_all_references_in_two_chunks(ctx):
    """ref_indices NULL at 2049 motions: chunk_r = 2^22 / 2049 = 2047 < n_refs = 2049, a second r0 launch of two rows."""
    _pair_costs(ctx, mc.PAIRS_C["n"], None)


def test_pair_costs_where_the_pass_halves(ctx):
    """pass_rows: 64 at J = 57, halved to 32 from J = 58 on when a reference motion has 1024 frames (derived in
    tests/test_motion_count_shapes_host.py).  Motions of 1024, 3 and 70 frames, all pairs, in the bits of the pairwise pin
    of tests/test_gpu_dtw_pairs.py; reference motion 1 alone (3 frames: the pass stays at 64 rows) gives the bits it gives
    beside motion 0 (the pass halves at J = 58)."""
    from test_gpu_dtw_pairs import pairwise, synthetic_clouds
    J0 = mc.first_halved_joint_count()
    for J in (J0 - 1, J0):
        table = synthetic_clouds(J, mc.PASS_LENGTHS, 300 + J)
        costs = dtw.all_pairs_costs(table, ctx=ctx)
        assert same_bits(costs, pairwise(ctx, table, None)), J
        alone = dtw.all_pairs_costs(table, references=[1], ctx=ctx)
        beside = dtw.all_pairs_costs(table, references=[1, 0], ctx=ctx)
        assert same_bits(alone[0], beside[0]) and same_bits(alone[0], costs[1]) and same_bits(beside[1], costs[0]), J
