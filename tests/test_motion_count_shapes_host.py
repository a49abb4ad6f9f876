"""The premises of tests/test_gpu_motion_count_shapes.py, on the host: the cut statements of the construction kernels still read
as tests/motion_count_cases.py restates them, every case's counts lie on both sides of the cut they name, the vectorised
integer DTW reference is dtw.dtw_paths_host, and each cut, dropped in a host model of the launch loop or reduction, would
change what the cases compare (so a case that passes has crossed its cut)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_count_cases as mc  # noqa: E402
from test_spatial_alignment_host import same_bits  # noqa: E402

from morphablegraphs_amd import dtw  # noqa: E402


def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "morphablegraphs_amd", "csrc", name)) as f:
        return f.read()


def test_the_cut_statements_read_as_the_cases_assume():
    sa_, dt, pr = _source("mg_spatial_align.hip"), _source("mg_dtw.hip"), _source("mg_dtw_pairs.hip")
    dev = _source("mg_dtw_device.h")
    # the three launch loops over the motions, and the offset each kernel adds
    assert "for (int64_t n0 = 0; n0 < n_motions; n0 += %d) {   // grid.y limit" % mc.GRID_Y in sa_
    assert "const int64_t nb = std::min<int64_t>(%d, n_motions - n0);" % mc.GRID_Y in sa_
    assert "const int64_t n = n0 + blockIdx.y, b0 = off[n], F = off[n + 1] - b0;" in sa_ and "double *tr = transforms + 5 * n;" in sa_
    assert "for (int64_t n0 = 0; n0 < n_motions; n0 += %d) {     // grid.y limit" % mc.GRID_Y in dt
    assert "const int64_t chunk = %d;" % mc.GRID_Y in dt and "for (int64_t n0 = 0; n0 < n_motions; n0 += chunk) {" in dt
    assert "const int64_t n = n0 + blockIdx.y, b0 = off[n];" in dt and "const int64_t n = n0 + blockIdx.x, b0 = off[n];" in dt
    assert "const int64_t chunk_n = %d;" % mc.GRID_Y in pr and "for (int64_t n0 = 0; n0 < n_motions; n0 += chunk_n) {" in pr
    assert "chunk_r = std::min<int64_t>(%d, ((int64_t)1 << 22) / nb);" % mc.GRID_Y in pr and mc.PAIRS_MAX_WORKGROUPS == 1 << 22
    assert "for (int64_t r0 = 0; r0 < n_refs; r0 += chunk_r) {" in pr
    assert "const int64_t n = n0 + blockIdx.x, r = r0 + blockIdx.y, m = refs ? refs[r] : r;" in pr
    # the strided legs
    assert "#define SA_BLOCK %d\n" % mc.SA_BLOCK in sa_ and "#define SA_FRAMES %d\n" % mc.SA_FRAMES in sa_
    assert "#define SA_MAX_PARTIALS %d\n" % mc.SA_MAX_PARTIALS in sa_
    assert "for (int64_t n = threadIdx.x; n < n_motions; n += SA_BLOCK) {" in sa_
    assert "for (int b = threadIdx.x; b < n_partials; b += SA_BLOCK)" in sa_
    assert "r < n_rows; r += (int64_t)gridDim.x * SA_BLOCK) {" in sa_
    assert "const int n_partials = (int)std::min<int64_t>(SA_MAX_PARTIALS, (n_rows + SA_BLOCK - 1) / SA_BLOCK);" in sa_
    assert "const unsigned blocks_x = (unsigned)((longest + SA_FRAMES - 1) / SA_FRAMES);" in sa_
    # the pass of the pair costs and its LDS
    assert "#define PAIRS_LDS_BYTES (152 * 1024)\n" in pr and mc.PAIRS_LDS_BYTES == 152 * 1024
    for name, value in (("PAIRS_MAX_FRAMES", mc.PAIRS_MAX_FRAMES), ("PAIRS_STRIP", mc.PAIRS_STRIP), ("PAIRS_SUB", mc.PAIRS_SUB),
                        ("PAIRS_PASS_ROWS", mc.PAIRS_PASS_ROWS)):
        assert "#define %s %d" % (name, value) in pr, name
    assert "#define DTW_MAX_JOINTS %d\n" % mc.DTW_MAX_JOINTS in dev
    assert "const size_t stride = (size_t)(3 * J) | 1;" in pr
    assert ("return (PAIRS_STRIP + PAIRS_SUB) * stride + DTW_MAX_JOINTS + 2 * PAIRS_STRIP + 2 * PAIRS_SUB + 1 + 2 * PAIRS_STRIP + (size_t)bnd + "
            "(size_t)rows * PAIRS_STRIP;") in pr
    assert "while (pairs_lds_doubles(n_joints, pass_rows, (int32_t)longest_ref) * 8 > PAIRS_LDS_BYTES) pass_rows /= 2;" in pr


def test_the_pass_halves_from_58_joints_on():
    """The smallest J whose 64-row pass does not fit with a 1024-frame reference motion, derived from pairs_lds_doubles: 58
    (80 * 175 + 353 + 1024 + 4096 = 19473 doubles > 19456; J = 57 needs 19153), and the source's comment says so."""
    J = mc.first_halved_joint_count()
    assert J == 58
    assert mc.pairs_lds_doubles(58, 64, 1024) == 80 * 175 + 353 + 1024 + 4096 == 19473 > mc.PAIRS_LDS_BYTES // 8 == 19456
    assert mc.pairs_lds_doubles(57, 64, 1024) == 19153
    assert all(mc.pass_rows(j, 1024) == 64 for j in range(1, J)) and all(mc.pass_rows(j, 1024) == 32 for j in range(J, mc.DTW_MAX_JOINTS + 1))
    assert "from J = %d on when a reference motion has 1024 frames" % J in _source("mg_dtw_pairs.hip")
    # the GPU case: lengths [1024, 3, 70]; reference motion 1 alone keeps the 64-row pass on both sides, with motion 0 it halves at J
    assert max(mc.PASS_LENGTHS) == mc.PAIRS_MAX_FRAMES and mc.PASS_LENGTHS[1] < mc.PAIRS_SUB and mc.PASS_LENGTHS[2] > mc.PAIRS_PASS_ROWS
    assert [mc.pass_rows(j, mc.PASS_LENGTHS[1]) for j in (J - 1, J)] == [64, 64]
    assert [mc.pass_rows(j, max(mc.PASS_LENGTHS[1], mc.PASS_LENGTHS[0])) for j in (J - 1, J)] == [64, 32]
    assert mc.pairs_lds_doubles(mc.DTW_MAX_JOINTS, 32, 1024) * 8 <= mc.PAIRS_LDS_BYTES       # one halving is enough everywhere


def test_every_case_straddles_its_cut():
    Y, B = mc.GRID_Y, mc.SA_BLOCK
    # launches over the motions: one launch, one launch plus one motion, and a second launch of more than one motion
    for counts in (mc.ALIGN_COUNTS, mc.DTW_COUNTS):
        assert {Y, Y + 1, Y + 4} <= set(counts)
        assert [len(mc.launches(n)) for n in (Y, Y + 1, Y + 4)] == [1, 2, 2] and mc.launches(Y + 4)[1] == (Y, 4)
    assert {B - 1, B, B + 1} <= set(mc.ALIGN_COUNTS)                                   # sa_heading_check_kernel: a lane's second motion
    assert set(mc.DTW_REF_FRAMES) == {1, 2, 3}
    # alignment: blocks_x = 3 from the motion that opens the second launch, 2 below; nearly every workgroup leaves at f0 >= F
    assert mc.ALIGN_LONG == {0: mc.SA_FRAMES + 1, Y: 2 * mc.SA_FRAMES + 1}
    for n, blocks in ((B, 2), (Y, 2), (Y + 1, 3), (Y + 4, 3)):
        lengths, off, table = mc.align_table(n)
        assert (int(lengths.max()) + mc.SA_FRAMES - 1) // mc.SA_FRAMES == blocks and len(table) == off[-1] == lengths.sum()
        assert set(np.unique(np.delete(lengths, [i for i in mc.ALIGN_LONG if i < n]))) == {1, 2, 3}
    motions, host, transforms = mc.align_distinct()
    assert len(motions) == mc.ALIGN_K + 2 and len({m.tobytes() for m in motions.values()}) == len(motions)
    assert len({t.tobytes() for t in transforms.values()}) == len(motions)       # a transform row written for another motion differs
    lengths, off, table = mc.align_table(Y + 4)
    for n in (1, 63, 64, 65, Y - 1, Y, Y + 1, Y + 3):
        assert same_bits(table[off[n]:off[n + 1]], motions[mc.align_key(n)]) and mc.align_key(mc.align_twin(n)) == mc.align_key(n)
        assert mc.align_twin(n) <= n and mc.align_twin(mc.align_twin(n)) == mc.align_twin(n)
    assert mc.align_twin(Y + 1) == 64 and mc.align_twin(Y) == Y and mc.align_twin(Y - 1) == 62 and mc.align_twin(0) == 0
    # refusals: which lane meets which motion on which visit
    visits = [[(n % B, n // B) for n in bad] for _, bad, _, _ in mc.ALIGN_REFUSALS]
    assert visits == [[(5, 1), (188, 2)], [(255, 0), (0, 1)], [(0, 256)]]
    for _, bad, n, named in mc.ALIGN_REFUSALS:
        assert max(bad) < n and named == min(bad) == mc.first_refused(bad, n)
    # preparation: 256 | 257 partials (the final kernel's second visit), 1024 partials with and without a grid stride
    rows = [s[0] * s[1] for s in mc.PREPARE_SHAPES]
    assert rows == [B * B, B * B + 1, mc.SA_MAX_PARTIALS * B, mc.SA_MAX_PARTIALS * B + 1]
    assert [mc.n_partials(r) for r in rows] == [B, B + 1, mc.SA_MAX_PARTIALS, mc.SA_MAX_PARTIALS]
    assert [mc.planted_rows(r) for r in rows] == [(65279, 65279, 65535), (65536, 65280, 65536), (65536, 261887, 262143), (65536, 262144, 262144)]
    assert 65536 // B == B and 65536 % B == 0               # row 65536: partial 256 = lane 0's second partial, that workgroup's lane 0
    assert 262144 == mc.SA_MAX_PARTIALS * B                 # row 262144: workgroup 0, lane 0, second grid stride
    # pair costs: (a) a second n0 chunk whose chunk_r differs, (b) a second r0 chunk, (c) all references in two r0 chunks
    a = mc.pair_launches(mc.PAIRS_A["n"], len(mc.PAIRS_A["refs"]))
    assert a == [(0, Y, 0, 4), (Y, 4, 0, 4)] and (1 << 22) // Y == 64 and min(Y, (1 << 22) // 4) == Y
    assert mc.PAIRS_A["refs"] == [0, Y, Y + 1, Y + 3] and mc.PAIRS_A["n"] == Y + 4
    assert mc.pair_launches(mc.PAIRS_B["n"], mc.PAIRS_B["n_refs"]) == [(0, Y, 0, 64), (0, Y, 64, 2)]
    assert mc.pair_launches(Y, 64) == [(0, Y, 0, 64)]
    refs = mc.pairs_b_refs()
    lengths, _, _ = mc.integer_motions(mc.PAIRS_B["n"])
    assert len(refs) == 66 and Y - 1 in refs and len(set(refs.tolist())) == 65 and np.any(np.diff(refs) < 0) and set(lengths[refs]) == {1, 2, 3}
    assert Y - 1 in refs[:64] and refs[65] != refs[1] and refs[64] != refs[0]      # rows 64, 65 are not rows 0, 1 again
    assert mc.pair_launches(mc.PAIRS_C["n"], mc.PAIRS_C["n"]) == [(0, 2049, 0, 2047), (0, 2049, 2047, 2)] and (1 << 22) // 2049 == 2047


def test_the_integer_reference_is_dtw_paths_host():
    """The vectorised tables against dtw.dtw_paths_host, motion by motion, on the first and the last motions of the largest case
    and every reference length; the integer grids do tie."""
    n = mc.DTW_COUNTS[-1]
    ties = 0
    for fr in mc.DTW_REF_FRAMES:
        c = mc.dtw_case(n, fr)
        off, lengths = c["off"], c["lengths"]
        for m in list(range(150)) + list(range(n - 150, n)):
            f = int(lengths[m])
            S = np.abs(c["ref"][:, None] - c["ys"][off[m]:off[m + 1]][None, :])
            D, path, warp = dtw.dtw_paths_host(S)
            cells = slice(fr * int(off[m]), fr * int(off[m + 1]))
            assert same_bits(c["grids"][cells], S.reshape(-1)) and same_bits(c["acc"][cells], D.reshape(-1)) and c["totals"][m] == D[-1, -1]
            p0 = int(off[m]) + m * (fr - 1)
            assert c["path_len"][m] == len(path) and c["paths"][p0:p0 + len(path)].tolist() == [list(p) for p in path]
            assert np.all(c["paths"][p0 + len(path):p0 + fr + f - 1] == int(mc.SENTINEL)) and c["warp"][m].tolist() == warp
            if fr > 1 and f > 1:
                ties += int(np.any(D[:-1, 1:] == D[1:, :-1]) or np.any(D[:-1, :-1] == D[:-1, 1:]))
        assert c["n_pairs"] == len(c["paths"]) == int(off[-1]) + n * (fr - 1) and not np.any(c["grids"] == mc.SENTINEL)
        assert np.all(c["totals"] == np.floor(c["totals"])) and c["totals"].max() < 2 ** 20
    assert ties >= 20
    # the pair costs: rows of the matrix against the same host function
    lengths, off, ys = mc.integer_motions(300)
    refs = [7, 299, 0, 7, 151]
    want = mc.pair_costs_reference(lengths, off, ys, refs)
    for r, m in enumerate(refs):
        for k in range(300):
            S = np.abs(ys[off[m]:off[m + 1]][:, None] - ys[off[k]:off[k + 1]][None, :])
            assert want[r, k] == dtw.dtw_paths_host(S)[0][-1, -1], (r, k)


def test_a_dropped_cut_changes_what_the_cases_compare():
    """Host models of the four cuts with the cut taken out: each answers something the cases' comparisons reject."""
    Y = mc.GRID_Y
    # n0 dropped from n = n0 + blockIdx.y: the second launch writes motions 0 .. nb - 1 again, motions from 65535 on keep the sentinel
    for n in (Y + 1, Y + 4):
        written = np.zeros(n, dtype=bool)
        for n0, nb in mc.launches(n):
            written[0:nb] = True              # (with n0: written[n0:n0 + nb])
        assert written[:Y].all() and not written[Y:].any()
        c = mc.dtw_case(n, 2)
        assert not np.any(c["totals"] == mc.SENTINEL) and not np.any(c["warp"] == int(mc.SENTINEL)) and not np.any(c["path_len"] == int(mc.SENTINEL))
    # r0 dropped from r = r0 + blockIdx.y: rows 64 and 65 keep the sentinel (and rows 0, 1 are written twice, with the same values)
    launches = mc.pair_launches(mc.PAIRS_B["n"], mc.PAIRS_B["n_refs"])
    rows = np.zeros(mc.PAIRS_B["n_refs"], dtype=bool)
    for _, _, r0, rb in launches:
        rows[0:rb] = True
    assert rows[:64].all() and not rows[64:].any()
    # the b += SA_BLOCK leg of pa_max_final_kernel and the grid-stride leg of pa_max_partial_kernel
    for shape in mc.PREPARE_SHAPES:
        flat = mc.prepare_table(shape).reshape(-1, shape[2])
        n_rows = len(flat)
        whole = mc.final_maxima(mc.partial_maxima(flat))
        assert whole.tolist() == list(mc.PLANTED) == np.abs(flat[:, :3]).max(axis=0).tolist()
        assert np.sort(np.abs(flat[:, :3]), axis=0)[-2].max() < 1.0                 # everything else is strictly smaller
        no_second = mc.final_maxima(mc.partial_maxima(flat), second_leg=False)
        no_stride = mc.final_maxima(mc.partial_maxima(flat, stride_leg=False))
        assert (no_second[0] < mc.PLANTED[0]) == (n_rows > 65536)
        assert (no_stride[1] < mc.PLANTED[1]) == (n_rows > 262144) and (no_stride[2] < mc.PLANTED[2]) == (n_rows > 262144)
    # the n += SA_BLOCK leg of sa_heading_check_kernel: another motion is named, or none
    assert [mc.first_refused(bad, n, second_leg=False) for _, bad, n, _ in mc.ALIGN_REFUSALS] == [701, 255, Y + 4]
    assert mc.first_refused((256,), 257, second_leg=False) == 257
