"""The LDS-staged frames kernels across channel counts and chunk plans, against the oracle.

test_gpu_latent_widths.py sweeps the frames kernels along the latent width.  Two more things select code in them: the channel
count D (the lane-to-channel map of the sweep waves, the store classes, the root columns of the padded rows, the widest chunk
window that fits LDS) and the chunk plan of the time grid (window, samples per chunk, number of chunks, ring depth).  SHAPES
below is one table of small synthetic primitives (F = 20, K = 3) that puts every one of those boundaries in front of the direct,
the tile-major and the chunk-stationary kernel and of the fused step, with the contracts the rest of the suite uses: float32
frames bit for bit the oracle's float32 model, log p bit for bit the stand-alone float32 log-likelihood.

The planner (mg_plan_chunks, csrc/mg_primitive_image.h) and the sweep waves' lane map are restated here in Python; the CPU tests pin the restatements to
the C sources line by line, assert that the table straddles every boundary and that the lane map writes every output float
and none outside its row; the GPU sweep compares the restated plan with what the library reports.  LEDGER records which
(kernel, D class, latent dtype, root mode) ran and matched; test_the_ledger_covers_every_class fails when a shape stops
exercising what it is in the table for.
"""
import numpy as np
import pytest

from morphablegraphs_amd import _capi, synthetic
from oracle import c_oracle
from oracle import mg_oracle as orc
from test_gpu_parity import _bits, _fused_step, pose_tol

MG_ERR_UNSUPPORTED = -4

# ---- the planner and the lane map, restated (kept in step with the C sources by test_restatements_match_the_sources) --------
MG_NCAND = 16                    # mg_hostdefs.h
MG_MAX_WI = 11
MG_MAX_NT = 48
MG_ARG_CHUNKS = 8
MG_RO_PAD = 8
MG_TAP_KS = (MG_MAX_WI + 3) // 4
MG_TAP_FT = MG_MAX_NT // 16
MG_FUSE_MAX_KK = 10              # mg_frames_common.h
LDS_BUDGET = 160 * 1024


def kk_of(L):
    return ((L + 3) // 4 + 1) // 2 * 2 if L <= 64 else 0


def nroot_of(D):
    return min(3, D)


def cshift_of(D):
    return (4 - nroot_of(D)) & 3


def dp_of(D):
    return (D + cshift_of(D) + 3) & ~3


def round_stride(nlocal):
    s = nlocal
    while s % 32 != 4:
        s += 1
    return s


def ro_bytes(nt):
    return MG_NCAND * (nt * 4 + MG_RO_PAD) * 4


def image_bytes(stride):
    return (MG_NCAND * stride * 4 + 255) // 256 * 256


def lds_bytes(D, stride, wi, nbuf=2, max_nt=MG_MAX_NT):
    """mg_lds_bytes."""
    tabs = max_nt * 16 + max_nt * 4
    root = MG_NCAND * (wi * nroot_of(D) + 1) * 8
    return nbuf * (image_bytes(stride) + ro_bytes(max_nt) + tabs) + root + 128


def window_fits(D, wi):
    """mg_plan_chunks: fits(wi, 160 KiB)."""
    nlocal = ((wi * dp_of(D) + 15) // 16 + 1) * 16
    return lds_bytes(D, round_stride(nlocal), wi) <= LDS_BUDGET


def widest_window(D):
    """The widest chunk window whose two-slot ring fits LDS (0: none, the direct kernel only)."""
    if (D - nroot_of(D) + 3) // 4 + 1 > 64:
        return 0
    return max([w for w in range(4, MG_MAX_WI + 1) if window_fits(D, w)], default=0)


def cs_max_tiles(KK):
    """mg_cs_cfg<KK>::MAX_TILES."""
    tpwp = min(120 // KK, 17)
    tpws = min(max(40 // KK, 1), 5)
    return 3 * tpwp + 4 * tpws


def plan_chunks(D, KK, i0, window=0, samples=0, ring=0):
    """mg_plan_chunks for a grid whose samples start at basis functions i0; window / samples / ring: MG_OPT_CHUNK_WINDOW,
    MG_OPT_CHUNK_SAMPLES, MG_OPT_RING_SLOTS."""
    i0 = [int(v) for v in i0]
    T, nroot, Dp = len(i0), nroot_of(D), dp_of(D)
    plan = dict(mfma_ok=False, cs_ok=False, n_chunks=0, chunks=[], lds_bytes=0, cs_lds_bytes=0, max_wi=0, max_nt=16, nbuf=2,
                max_tiles=0, window=0)
    if KK == 0 or T == 0 or (D - nroot + 3) // 4 + 1 > 64:
        return plan
    max_nt = MG_MAX_NT
    if samples:
        max_nt = max(1, min(MG_MAX_NT, samples))

    def count_chunks(w):
        n, a0 = 0, 0
        while a0 < T:
            imin = imax = i0[a0]
            b = a0 + 1
            while b < T and b - a0 < max_nt:
                lo, hi = min(imin, i0[b]), max(imax, i0[b])
                if hi - lo + 4 > w:
                    break
                imin, imax = lo, hi
                b += 1
            a0 = b
            n += 1
        return n

    W, best_n = 0, 0
    for w in range(MG_MAX_WI, 3, -1):
        if not window_fits(D, w):
            continue
        n = count_chunks(w)
        if W == 0 or n <= best_n:
            W, best_n = w, n
    if W == 0:
        return plan
    if window:
        W = max(4, min(W, window))
    n_greedy = count_chunks(W)
    chunks, a = [], 0
    max_stride = max_wi = longest = 0
    while a < T:
        imin = imax = i0[a]
        b = a + 1
        left = max(1, n_greedy - len(chunks))
        target = min(max_nt, (T - a + left - 1) // left)
        while b < T and b - a < target:
            lo, hi = min(imin, i0[b]), max(imax, i0[b])
            if hi - lo + 4 > W:
                break
            imin, imax = lo, hi
            b += 1
        wi = imax - imin + 4
        rt0 = (imin * Dp) // 16
        ntiles = ((imin + wi) * Dp + 15) // 16 - rt0
        chunks.append(dict(t0=a, nT=b - a, imin=imin, wi=wi, rt0=rt0, ntiles=ntiles))
        max_stride = max(max_stride, round_stride(ntiles * 16))
        max_wi = max(max_wi, wi)
        longest = max(longest, b - a)
        a = b
    nt = (longest + 15) // 16 * 16
    nbuf = 3 if lds_bytes(D, max_stride, max_wi, 3, nt) <= LDS_BUDGET else 2
    if ring == 2:
        nbuf = 2
    lds = lds_bytes(D, max_stride, max_wi, nbuf, nt)
    max_tiles = max(c["ntiles"] for c in chunks)
    cs_lds = (2 * (image_bytes(max_stride) + ro_bytes(nt)) + nt * 20 + MG_NCAND * (max_wi * nroot + 1) * 8 + max_tiles * 64 +
              MG_TAP_FT * MG_TAP_KS * 64 * 8 + 512 + 2 * KK * 64 * 4 + 256)
    mfma_ok = lds <= LDS_BUDGET
    cs_ok = mfma_ok and max_tiles <= cs_max_tiles(KK) and cs_lds <= LDS_BUDGET and len(chunks) <= MG_ARG_CHUNKS
    plan.update(mfma_ok=mfma_ok, cs_ok=cs_ok, n_chunks=len(chunks), chunks=chunks, lds_bytes=lds, cs_lds_bytes=cs_lds,
                max_wi=max_wi, max_nt=nt, nbuf=nbuf, max_tiles=max_tiles, window=W)
    return plan


def fused_lds(K):
    """mg_fused_gmm_lds."""
    return 4 * K * 16 * 8


def fused_lds_cs(K, KK, Lg):
    """mg_fused_gmm_lds_cs."""
    JT = (Lg + 15) // 16
    return fused_lds(K) + 2 * KK * 64 * 4 + (K * JT * 16 + (K + 1) // 2 * 2) * 8


def lane_map(D):
    """The sweep waves' lane-to-channel map (mg_frames_ws.hip / mg_frames_cs.hip): per lane that holds a sample
    (fsub, first float of its store inside the row group, floats stored, root lane?), and (rpi, gl, nql, shift3, all4)."""
    nroot = nroot_of(D)
    nql = (D - nroot + 3) >> 2
    gl = nql + 1
    rpi = 64 // gl
    shift3 = gl == 20
    all4 = nql > 0 and nroot == 3 and ((D - nroot) & 3) == 0
    lanes = []
    for lane in range(64):
        lane_s = lane - 4 if (shift3 and lane >= 40) else lane
        fsub = lane_s // gl
        ql = lane_s - fsub * gl
        lane_on = (lane < 40 or lane >= 44) if shift3 else lane < rpi * gl
        root_lane = ql == nql
        d0 = 0 if root_lane else nroot + 4 * ql
        nst = nroot if root_lane else min(D - d0, 4)
        if lane_on:
            lanes.append((fsub, fsub * D + d0, 4 if all4 else nst, root_lane))
    return lanes, dict(rpi=rpi, gl=gl, nql=nql, shift3=shift3, all4=all4, nroot=nroot,
                       nst_last=(D - (nroot + 4 * (nql - 1))) if nql else 0)


def d_classes(D):
    """What a channel count is in the table for."""
    _, m = lane_map(D)
    c = {"nroot%d" % m["nroot"]}
    if m["nql"] and not m["all4"]:
        c.add("nst%d" % m["nst_last"])
    if m["shift3"] and not m["all4"]:
        c.add("shift3_partial")
    if m["gl"] in (16, 21, 32, 33):
        c.add("gl%d" % m["gl"])
    return c


# ---- the table ------------------------------------------------------------------------------------------------------------------
F, K = 20, 3
BATCHES = (7, 8, 15, 16, 17, 33, 130)
LS = (6, 23, 40)                                   # KK 2, 6, 10
WINDOW_STEPS = ((87, 88), (99, 100), (111, 112), (123, 124), (143, 144), (167, 168), (199, 200))


def _row(D, L, NB=8):
    return dict(name="D%d_L%d_NB%d" % (D, L, NB), D=D, L=L, NB=NB)


# NB = 8: the canonical grid is one chunk with a window of 8 basis functions wherever 8 fit (D <= 123), two and more chunks from
# there on; the rows with NB = 11, 10, 9 and 7 need exactly the widest window that fits at their D (the planner takes the
# narrowest window that reaches the smallest chunk count), so windows of 11, 10, 9 and 7 run as well.
SHAPES = [
    _row(1, 6), _row(2, 23), _row(3, 40), _row(4, 6), _row(5, 23), _row(6, 40), _row(7, 6), _row(8, 23), _row(9, 40), _row(10, 6),
    _row(11, 23), _row(15, 40),
    _row(60, 6), _row(63, 23),
    _row(76, 40), _row(77, 6), _row(78, 23), _row(79, 40), _row(80, 6), _row(81, 23), _row(82, 40),
    _row(87, 6, NB=11), _row(88, 23, NB=10), _row(99, 6, NB=10), _row(100, 6, NB=9), _row(111, 23, NB=9), _row(112, 6),
    _row(123, 23), _row(124, 6, NB=7), _row(127, 40), _row(128, 23),
    _row(143, 6, NB=7), _row(144, 23), _row(167, 40), _row(168, 6), _row(199, 23), _row(200, 6),
    _row(251, 6), _row(252, 6), _row(255, 23),
]
SHAPE_IDS = [s["name"] for s in SHAPES]
FORCED_DS = (79, 78)
FORCED_L = 23
FORCED_PLANS = [dict(samples=1), dict(samples=5), dict(samples=16), dict(samples=17), dict(samples=47), dict(window=4), dict(window=7),
                dict(samples=2, window=4), dict(samples=5, ring=2)]

LEDGER = set()       # (kernel, D class, dtype name, root mode) that ran and matched
_DONE = {}


def _note(kernel, classes, dtype, mode):
    for c in classes:
        LEDGER.add((kernel, c, np.dtype(dtype).name, int(mode)))


def _knots(s):
    return orc.cubic_b_spline_knots(s["NB"], F)


def _canonical_times():
    """The reference's canonical time function, np.linspace(0, F, F), as the oracle and the library compute it."""
    t = np.arange(F, dtype=np.float64) * (float(F) / float(F - 1))
    t[F - 1] = float(F)
    return t


def _canonical_plan(s, **opts):
    i0, _ = orc.basis_rows(_knots(s), _canonical_times())
    return plan_chunks(s["D"], kk_of(s["L"]), i0, **opts)


def _eval_times(n_frames):
    """Fractional, repeated, backwards and out-of-range times (test_gpu_latent_widths._eval_times)."""
    return np.array([0.0, 0.25, 0.25, n_frames / 3.0 + 0.5, n_frames - 1.0, n_frames - 1.5, 2.0, 1.0, -3.0, n_frames + 4.0,
                     0.5 * (n_frames - 1), 0.5 * (n_frames - 1)])


def _eval_plan(s, **opts):
    i0, _ = orc.basis_rows(_knots(s), _eval_times(F))
    return plan_chunks(s["D"], kk_of(s["L"]), i0, **opts)


def _shape_classes(s):
    c = d_classes(s["D"])
    plan = _canonical_plan(s)
    if plan["mfma_ok"]:
        c.add("win%d" % plan["max_wi"])
    return c


WANTED_CLASSES = (["nroot1", "nroot2", "nroot3", "nst1", "nst2", "nst3", "shift3_partial", "gl16", "gl21", "gl32", "gl33"] +
                  ["win%d" % w for w in range(4, MG_MAX_WI + 1)])


# ---- CPU checks -----------------------------------------------------------------------------------------------------------------
def _source(name):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "morphablegraphs_amd", "csrc", name)).read()


def test_restatements_match_the_sources():
    """Every formula restated above, pinned to its line in the C sources."""
    host, image, hostdefs, ws, cs, frames = (_source(n) for n in ("mg_host.hip", "mg_primitive_image.h", "mg_hostdefs.h", "mg_frames_ws.hip",
                                                                  "mg_frames_cs.hip", "mg_frames.hip"))
    # (mg_lds_bytes' per-slot and root terms are mg_lds_slot_bytes and mg_lds_root_bytes, which the chunk-stationary kernel's LDS
    # shares; one mg_grow_chunk is the window-growing loop of the greedy count (cap = max_nt) and of the final split (cap = target))
    for line in ("p->nroot = std::min(3, D);", "p->cshift = (4 - p->nroot) & 3;", "p->Dp = (D + p->cshift + 3) & ~3;",
                 "while (s % 32 != 4) s++;", "int buf = (MG_NCAND * stride * 4 + 255) / 256 * 256;",
                 "int rout = MG_RO_BYTES_N(max_nt);", "return buf + rout;", "int tabs = max_nt * 16 + max_nt * 4;",
                 "inline int mg_lds_root_bytes(int nroot, int wi) { return MG_NCAND * (wi * nroot + 1) * 8; }",
                 "return nbuf * (mg_lds_slot_bytes(stride, max_nt) + tabs) + mg_lds_root_bytes(nroot, wi) + 128;",
                 "if (p.KK == 0 || T == 0 || (p.D - p.nroot + 3) / 4 + 1 > 64) return;",
                 "int nlocal = ((wi * Dp + 15) / 16 + 1) * 16;", "return mg_lds_bytes(p.nroot, mg_round_stride(nlocal), wi) <= budget;",
                 "const int budget1 = 160 * 1024;",
                 "if (const int o = opt_samples) max_nt = std::max(1, std::min(MG_MAX_NT, o));",
                 "for (int a0 = 0; a0 < T; n++) a0 = mg_grow_chunk(g.i0, a0, max_nt, w, imin, imax);",
                 "while (b < T && b - a < cap) {", "if (hi - lo + 4 > w) break;",
                 "for (int w = MG_MAX_WI; w >= 4; w--) {", "if (W == 0 || n <= best_n) { W = w; best_n = n; }",
                 "if (const int o = opt_window) W = std::max(4, std::min(W, o));",
                 "const int left = std::max(1, n_greedy - (int)g.chunks.size());",
                 "const int target = std::min(max_nt, (T - a + left - 1) / left);",
                 "const int b = mg_grow_chunk(g.i0, a, target, W, imin, imax);",
                 "c.wi = imax - imin + 4;", "c.rt0 = (imin * Dp) / 16;", "int rt1 = ((imin + c.wi) * Dp + 15) / 16;",
                 "max_stride = std::max(max_stride, mg_round_stride(c.ntiles * 16));", "g.max_nt = (longest + 15) / 16 * 16;",
                 "g.nbuf = mg_lds_bytes(p.nroot, max_stride, max_wi, 3, g.max_nt) <= budget1 ? 3 : 2;",
                 "if (opt_ring == 2) g.nbuf = 2;",
                 "g.lds_bytes = mg_lds_bytes(p.nroot, max_stride, max_wi, g.nbuf, g.max_nt);", "g.mfma_ok = g.lds_bytes <= budget1;",
                 "g.cs_lds_bytes = 2 * mg_lds_slot_bytes(max_stride, g.max_nt) + g.max_nt * 20 + mg_lds_root_bytes(p.nroot, max_wi) + "
                 "g.max_tiles * 64 +",
                 "MG_TAP_FT * MG_TAP_KS * 64 * 8 + 512 + 2 * p.KK * 64 * 4 + 256;",
                 "g.cs_ok = g.mfma_ok && g.max_tiles <= cs_max_tiles && g.cs_lds_bytes <= budget1 && "
                 "(int)g.chunks.size() <= MG_ARG_CHUNKS;"):
        assert line in image, line
    # the options and the chunk-stationary kernel's register bound reach the planner from the context, in this order
    for line in ("mg_grid_image_build(*p, times, T, i0_override, w_override, opt[MG_OPT_CHUNK_SAMPLES], opt[MG_OPT_CHUNK_WINDOW], "
                 "opt[MG_OPT_RING_SLOTS],", "mg_cs_max_tiles(p->KK), im);", "use_mfma = g->mfma_ok && B >= 8;"):
        assert line in host, line
    assert ("inline void mg_plan_chunks(const mg_primitive_model &p, mg_grid_plan &g, int opt_samples, int opt_window, int opt_ring, "
            "int cs_max_tiles) {") in image
    assert "mg_plan_chunks(p, im, opt_samples, opt_window, opt_ring, cs_max_tiles);" in image
    for line in ("#define MG_NCAND %d " % MG_NCAND, "#define MG_MAX_WI %d " % MG_MAX_WI, "#define MG_MAX_NT %d " % MG_MAX_NT,
                 "#define MG_ARG_CHUNKS %d " % MG_ARG_CHUNKS, "#define MG_RO_PAD %d" % MG_RO_PAD,
                 "#define MG_TAP_KS ((MG_MAX_WI + 3) / 4)", "#define MG_TAP_FT (MG_MAX_NT / 16)",
                 "#define MG_RO_CS(nt) ((nt) * 4 + MG_RO_PAD)", "#define MG_RO_BYTES_N(nt) (MG_NCAND * MG_RO_CS(nt) * 4)"):
        assert line in hostdefs, line
    for line in ("static constexpr int TPWP = 120 / KK < 17 ? 120 / KK : 17;", "static constexpr int TPWS_REGS = 160 / MG_CS_NSP;",
                 "static constexpr int TPWS = TPWS_REGS / KK < 5 ? (TPWS_REGS / KK > 0 ? TPWS_REGS / KK : 1) : 5;",
                 "static constexpr int MAX_TILES = (MG_CS_NPW - 1) * TPWP + MG_CS_NSP * TPWS;", "#define MG_CS_NPW 4 ", "#define MG_CS_NSP 4 "):
        assert line in cs, line
    for src in (ws, cs):                              # the sweep waves' lane map: the same statements in both kernels
        for line in ("const int nql = (D - nroot + 3) >> 2;", "const int gl = nql + 1;", "const int rpi = 64 / gl;",
                     "const bool shift3 = gl == 20;", "const int lane_s = (shift3 && lane >= 40) ? lane - 4 : lane;",
                     "const int fsub = lane_s / gl, ql = lane_s - fsub * gl;",
                     "const bool lane_on = shift3 ? (lane < 40 || lane >= 44) : lane < rpi * gl;", "const bool root_lane = ql == nql;",
                     "const int d0 = root_lane ? 0 : nroot + 4 * ql;", "const int nst = root_lane ? nroot : (D - d0 < 4 ? D - d0 : 4);",
                     "const int lane_out = fsub * D + d0;", "const bool all4 = nql > 0 && nroot == 3 && ((D - nroot) & 3) == 0;",
                     "for (int f0 = f_first; f0 < ", "const int fla = f0 + fsub, flb = fla + rpi;",
                     "const bool oa = lane_on && fla < ck.nT, ob = lane_on && flb < ck.nT;", "if (f0 + rpi < ck.nT) {",
                     "if (dp4 == 320 && all4) sweep_rows("):
            assert line in src, line
    for line in ("static int mg_fused_gmm_lds(const mg_primitive *p) { return 4 * p->K * 16 * 8; }",
                 "return mg_fused_gmm_lds(p) + 2 * p->KK * 64 * 4 + (p->K * JT * 16 + (p->K + 1) / 2 * 2) * 8;",
                 "g->lds_bytes + mg_fused_gmm_lds(p) <= 160 * 1024 &&", "if (want == 2 && !cs) return -1;",
                 "bool cs = g->cs_ok && grid_cs >= g->n_chunks && grid_cs <= 4096 &&",
                 "(!fused || (g->cs_lds_bytes + mg_fused_gmm_lds(p) <= 160 * 1024 && (n_tiles + grid_cs - 1) / grid_cs <= 4));"):
        assert line in frames, line
    assert [cs_max_tiles(KK) for KK in (2, 4, 6, 8, 10, 12, 14, 16)] == [71, 71, 71, 65, 52, 42, 32, 29]
    assert [(nroot_of(D), cshift_of(D), dp_of(D)) for D in (1, 2, 3, 4, 5, 78, 79, 80)] == \
        [(1, 3, 4), (2, 2, 4), (3, 1, 4), (3, 1, 8), (3, 1, 8), (3, 1, 80), (3, 1, 80), (3, 1, 84)]
    # the planner's widest window, as computed from mg_lds_bytes: 11 up to D = 87, one less at each listed step, none from 252
    assert [widest_window(D) for D in (1, 79, 87, 88, 99, 100, 111, 112, 123, 124, 143, 144, 167, 168, 199, 200, 251, 252, 255, 256)] == \
        [11, 11, 11, 10, 10, 9, 9, 8, 8, 7, 7, 6, 6, 5, 5, 4, 4, 0, 0, 0]


def test_table_straddles_every_shape_boundary():
    """The table has a shape on both sides of every boundary that selects code in the frames kernels or the planner."""
    ds = [s["D"] for s in SHAPES]
    assert len(set(SHAPE_IDS)) == len(SHAPES)
    assert set(range(1, 11)) | set(range(76, 83)) <= set(ds)
    for lo, hi in WINDOW_STEPS + ((251, 252),):
        assert lo in ds and hi in ds
    maps = {D: lane_map(D)[1] for D in ds}
    assert any(m["all4"] for m in maps.values()) and any(not m["all4"] for m in maps.values())
    assert {m["nroot"] for m in maps.values()} == {1, 2, 3}
    assert {m["nst_last"] for m in maps.values() if m["nql"] and not m["all4"]} == {1, 2, 3}
    assert {1, 2, 16, 20, 21, 32, 33} <= {m["gl"] for m in maps.values()}
    assert any(m["shift3"] and m["all4"] for m in maps.values()) and any(m["shift3"] and not m["all4"] for m in maps.values())
    # every D meets an L; every L meets all4 and not all4
    for L in LS:
        assert {maps[s["D"]]["all4"] for s in SHAPES if s["L"] == L} == {True, False}, L
    assert {kk_of(L) for L in LS} == {2, 6, 10}
    plans = {s["name"]: _canonical_plan(s) for s in SHAPES}
    eplans = {s["name"]: _eval_plan(s) for s in SHAPES}
    # LDS-staged against direct only
    assert plans["D251_L6_NB8"]["mfma_ok"] and not plans["D252_L6_NB8"]["mfma_ok"] and not plans["D255_L23_NB8"]["mfma_ok"]
    assert all(plans[s["name"]]["mfma_ok"] == eplans[s["name"]]["mfma_ok"] == (s["D"] <= 251) for s in SHAPES)
    # every window width runs as the canonical grid's window, in one chunk and in two
    assert {p["max_wi"] for p in plans.values() if p["mfma_ok"]} == set(range(4, MG_MAX_WI + 1))
    assert {p["n_chunks"] for p in plans.values() if p["mfma_ok"]} >= {1, 2}
    # the ring: three slots and two; the chunk-stationary kernel: covered and not (LDS, and the window's tiles against its registers)
    assert {p["nbuf"] for p in plans.values() if p["mfma_ok"]} == {2, 3}
    assert any(p["cs_ok"] for p in plans.values()) and any(p["mfma_ok"] and not p["cs_ok"] for p in plans.values())
    assert any(p["mfma_ok"] and p["cs_lds_bytes"] > LDS_BUDGET for p in plans.values())
    assert any(p["mfma_ok"] and p["cs_lds_bytes"] <= LDS_BUDGET and p["max_tiles"] > cs_max_tiles(kk_of(s["L"]))
               for s, p in ((s, plans[s["name"]]) for s in SHAPES))
    # every class the ledger asks for has a shape that the chunk-stationary kernel covers as well
    have = set().union(*(_shape_classes(s) for s in SHAPES if plans[s["name"]]["cs_ok"]))
    assert set(WANTED_CLASSES) <= have, sorted(set(WANTED_CLASSES) - have)
    # forced plans: T = 1, n_chunks = 8, 9 and above (chunk descriptors from memory; the chunk-stationary kernel declines), max_nt 16 / 32
    for D in FORCED_DS:
        s = _row(D, FORCED_L)
        fp = [_canonical_plan(s, **o) for o in FORCED_PLANS]
        assert all(p["mfma_ok"] for p in fp)
        assert any(p["n_chunks"] == 20 and all(c["nT"] == 1 for c in p["chunks"]) for p in fp)
        ep = [_eval_plan(s, **o) for o in FORCED_PLANS]
        assert any(p["n_chunks"] == MG_ARG_CHUNKS and p["cs_ok"] for p in fp + ep), [p["n_chunks"] for p in fp + ep]
        assert any(p["n_chunks"] > MG_ARG_CHUNKS and not p["cs_ok"] for p in fp)
        assert {p["max_nt"] for p in fp} >= {16, 32} and any(p["max_wi"] == 4 for p in fp)
        assert any(o.get("ring") and p["nbuf"] == 2 and _canonical_plan(s, **dict(o, ring=0))["nbuf"] == 3 for o, p in zip(FORCED_PLANS, fp))
        assert _canonical_plan(s)["cs_ok"]
    assert lane_map(FORCED_DS[0])[1]["all4"] and not lane_map(FORCED_DS[1])[1]["all4"]


def test_the_lane_map_writes_every_float_and_none_outside_its_row():
    """The sweep waves' lane-to-address map over every D the LDS-staged kernels take: a wave instruction's lanes write every
    float of its rpi rows, each lane inside its own row (no float of a neighbouring row, none past the row group: where all
    lanes store four floats the float written twice is the row's channel 3, from the root lane and from its first quad lane),
    and the trip loop hands every sample of a chunk to exactly one (trip, row group, lane group)."""
    for D in range(1, 256):
        lanes, m = lane_map(D)
        rpi, gl = m["rpi"], m["gl"]
        assert 1 <= rpi and rpi * gl <= 64 and len(lanes) == rpi * gl, D
        hits = np.zeros(rpi * D, dtype=int)
        for fsub, off, n, root in lanes:
            assert 0 <= fsub < rpi and n >= 1, (D, fsub)
            assert fsub * D <= off and off + n <= (fsub + 1) * D, "D = %d: a lane of sample %d stores floats %d .. %d" % (D, fsub, off, off + n - 1)
            hits[off:off + n] += 1
        assert hits.min() >= 1, D
        if m["all4"]:
            twice = np.flatnonzero(hits > 1)
            assert hits.max() == 2 and list(twice) == [f * D + 3 for f in range(rpi)], D
        else:
            assert hits.max() == 1, D
        assert m["all4"] == (D >= 7 and D % 4 == 3), D
        for nT in (1, 2, 3, 5, 16, 17, 31, 32, 33, 47, 48):
            seen = np.zeros(nT, dtype=int)
            for f0 in range(0, nT, 2 * rpi):
                both = f0 + rpi < nT
                for fsub in range(rpi):
                    fla, flb = f0 + fsub, f0 + fsub + rpi
                    if fla < nT:
                        seen[fla] += 1
                    if both and flb < nT:
                        seen[flb] += 1
            assert np.all(seen == 1), (D, nT)


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
            c.set_reserved_cus(0)


def _make(s, L=None):
    L = s["L"] if L is None else L
    return synthetic.make_primitive(seed=7000 + 13 * s["D"] + L, name=s["name"], n_components=L, n_frames=F, n_basis=s["NB"],
                                    n_dim=s["D"], n_gmm=K)


def _set_plan_options(ctx, samples=0, window=0, ring=0):
    ctx.set_option(_capi.MG_OPT_CHUNK_SAMPLES, samples)
    ctx.set_option(_capi.MG_OPT_CHUNK_WINDOW, window)
    ctx.set_option(_capi.MG_OPT_RING_SLOTS, ring)


def _check_plan(ctx, prim, s, plan, B, tag):
    """The restated plan against what the library reports: mg_primitive_info slots 6 and 7, step_plan's kernel and LDS."""
    Kk, L = kk_of(s["L"]), s["L"]
    assert prim.mfma_supported == plan["mfma_ok"], (tag, "mfma_ok")
    assert prim.n_chunks == plan["n_chunks"], (tag, "n_chunks", prim.n_chunks, plan["n_chunks"])
    if not plan["mfma_ok"] or B < 8:
        sp = prim.step_plan(B)
        assert sp["kernel"] == "mg_frames_direct_kernel" and not sp["fused"], (tag, sp)
        return
    n_tiles = (B + MG_NCAND - 1) // MG_NCAND
    fused = Kk <= MG_FUSE_MAX_KK and plan["lds_bytes"] + fused_lds(K) <= LDS_BUDGET and n_tiles <= 4 * min(n_tiles * plan["n_chunks"], N_CU[0])
    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 1)
    sp = prim.step_plan(B)
    assert sp["kernel"] == "mg_frames_ws_kernel" and sp["fused"] == fused and sp["lds_bytes"] == plan["lds_bytes"] + (fused_lds(K) if fused else 0), (tag, sp, plan)
    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
    assert prim.step_plan(B) == sp, (tag, "the library's own choice at a batch of under two units per workgroup")
    cs_ok = plan["cs_ok"] and (not fused or plan["cs_lds_bytes"] + fused_lds(K) <= LDS_BUDGET)
    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 2)
    if cs_ok:
        sp = prim.step_plan(B)
        staged = plan["cs_lds_bytes"] + fused_lds_cs(K, Kk, L) <= LDS_BUDGET
        want = plan["cs_lds_bytes"] + ((fused_lds_cs(K, Kk, L) if staged else fused_lds(K)) if fused else 0)
        assert sp["kernel"] == "mg_frames_cs_kernel" and sp["fused"] == fused and sp["lds_bytes"] == want, (tag, sp, plan)
    else:
        with pytest.raises(_capi.MGError):
            prim.step_plan(B)
    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)


N_CU = [256]


def _lds_kernels(ctx, prim, X, want, grid, cs_ok, tag, reps=1):
    """MG_PATH_MFMA with MG_OPT_FRAMES_KERNEL 1, 2 and 0: the oracle's bits; the chunk-stationary kernel may decline only where
    the restated cs_ok is false.  Returns the kernels that ran."""
    ran = []
    for kern in (1, 2, 0):
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, kern)
        for rep in range(reps):
            try:
                out = prim.back_project_frames(X, grid=grid, path=_capi.MG_PATH_MFMA)
            except _capi.MGError as e:
                assert kern == 2 and e.status == MG_ERR_UNSUPPORTED and not cs_ok, (tag, kern, e)
                break
            assert not (kern == 2 and not cs_ok), (tag, "the chunk-stationary kernel ran a plan it does not cover")
            np.testing.assert_array_equal(_bits(out), _bits(want), err_msg="%s kernel %d rep %d" % (tag, kern, rep))
            if rep == 0:
                ran.append(kern)
    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
    return ran


def _step(ctx, prim, cp, X, model, tag, cs_fused_ok, reps=1):
    """mg_step_frames_and_logp under the library's choice and with the chunk-stationary kernel forced: frames the oracle's bits,
    log p the stand-alone float32 log-likelihood's bits and within float32 tolerance of the float64 oracle."""
    lp_sep = prim.gmm_log_prob(X, dtype=np.float32)
    ref = cp.log_prob_f64(X.astype(np.float64))
    ran = []
    for kern in (0, 2):
        ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, kern)
        for rep in range(reps):
            try:
                frames, logp = _fused_step(ctx, prim, X, F, prim.n_dim)
            except _capi.MGError as e:
                assert kern == 2 and e.status == MG_ERR_UNSUPPORTED and not cs_fused_ok, (tag, e)
                break
            np.testing.assert_array_equal(_bits(frames), _bits(model), err_msg="%s step kernel %d" % (tag, kern))
            np.testing.assert_array_equal(_bits(logp), _bits(lp_sep), err_msg="%s step log p kernel %d" % (tag, kern))
            np.testing.assert_allclose(logp, ref, rtol=3e-7, atol=1e-6)
            if rep == 0:
                ran.append(kern)
    ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
    return ran


def _sweep(ctx, s):
    if s["name"] in _DONE:
        return
    N_CU[0] = ctx.device_info()["n_cu"]
    D, L = s["D"], s["L"]
    data = _make(s)
    cp = c_oracle.COraclePrimitive(data)
    rng = np.random.default_rng(100 * D + L)
    S = rng.standard_normal((max(BATCHES), L))
    times = _eval_times(F)
    plan, plan_t = _canonical_plan(s), _eval_plan(s)
    classes = _shape_classes(s)
    _reset(ctx)
    for mode in (1, 2):
        ctx.set_option(_capi.MG_OPT_ROOT_MODE, mode)
        split = mode == 2
        prim = _capi.Primitive(ctx, data)
        grid = prim.time_grid(times)
        try:
            assert prim.root_split == split and prim.kk == kk_of(L)
            for B in (7, 8, max(BATCHES)):
                _check_plan(ctx, prim, s, plan, B, s["name"])
            for dtype in (np.float32, np.float64):
                X = S.astype(dtype)
                X64 = X.astype(np.float64)
                tag = "%s %s mode %d" % (s["name"], np.dtype(dtype).name, mode)
                model, model_t = cp.frames_f32model(X64, root_split=split), cp.frames_f32model(X64, tp=times, root_split=split)
                got = prim.back_project_frames(X, path=_capi.MG_PATH_DIRECT)
                np.testing.assert_array_equal(_bits(got), _bits(model), err_msg=tag + " direct")
                np.testing.assert_array_equal(_bits(prim.back_project_frames(X, grid=grid, path=_capi.MG_PATH_DIRECT)), _bits(model_t))
                if not split:
                    ref = cp.frames_f64(X64)
                    assert np.all(np.abs(got.astype(np.float64) - ref) <= pose_tol(ref)), tag
                # MG_PATH_AUTO: seven candidates go to the direct kernel, eight and more to the LDS-staged ones where they take the shape
                for B in (7, 8, max(BATCHES)):
                    np.testing.assert_array_equal(_bits(prim.back_project_frames(X[:B])), _bits(model[:B]), err_msg=tag + " auto")
                    np.testing.assert_array_equal(_bits(prim.back_project_frames(X[:B], grid=grid)), _bits(model_t[:B]))
                _note("direct", classes, dtype, mode)
                if not plan["mfma_ok"]:
                    for g in (None, grid):
                        with pytest.raises(_capi.MGError) as err:
                            prim.back_project_frames(X, grid=g, path=_capi.MG_PATH_MFMA)
                        assert err.value.status == MG_ERR_UNSUPPORTED
                else:
                    for B in BATCHES:
                        ran = _lds_kernels(ctx, prim, X[:B], model[:B], None, plan["cs_ok"], tag + " B %d" % B)
                        ran_t = _lds_kernels(ctx, prim, X[:B], model_t[:B], grid, plan_t["cs_ok"], tag + " B %d eval grid" % B)
                        assert 1 in ran and 1 in ran_t and 0 in ran and 0 in ran_t
                    _note("ws", classes, dtype, mode)
                    if 2 in ran:
                        _note("cs", classes, dtype, mode)
                # the step: fused where the shape allows it, two launches (direct + log p) at D = 252
                cs_fused_ok = plan["cs_ok"] and plan["cs_lds_bytes"] + fused_lds(K) <= LDS_BUDGET
                for B in BATCHES:
                    _step(ctx, prim, cp, X[:B], model[:B], tag + " B %d" % B, cs_fused_ok)
                _note("step", classes, dtype, mode)
        finally:
            grid.close()
            prim.close()
    _reset(ctx)
    _DONE[s["name"]] = True


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_channel_sweep_against_the_oracle(ctx, shape):
    _sweep(ctx, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("D", sorted({s["D"] for s in SHAPES}))
def test_float64_paths_across_channel_counts(ctx, D):
    """back_project_frames_f64, back_project_coeffs (both output dtypes; float32 from eight candidates on through the LDS-staged
    kernels over the identity grid) and spline_evaluate at every D of the table, L = 6."""
    s = _row(D, LS[0])
    data = _make(s)
    cp = c_oracle.COraclePrimitive(data)
    prim = _capi.Primitive(ctx, data)
    grid = prim.time_grid(_eval_times(F))
    try:
        S = np.random.default_rng(D).standard_normal((33, s["L"]))
        for dtype in (np.float32, np.float64):
            X = S.astype(dtype)
            X64 = X.astype(np.float64)
            ref, ref_t, cref = cp.frames_f64(X64), cp.frames_f64(X64, tp=_eval_times(F)), cp.coeffs_f64(X64)
            scale = max(1.0, np.abs(ref).max())
            np.testing.assert_allclose(prim.back_project_frames_f64(X), ref, rtol=0, atol=4e-12 * scale)
            np.testing.assert_allclose(prim.back_project_frames_f64(X, grid=grid), ref_t, rtol=0, atol=4e-12 * max(1.0, np.abs(ref_t).max()))
            coeffs = prim.back_project_coeffs(X)
            np.testing.assert_allclose(coeffs, cref, rtol=0, atol=4e-12 * max(1.0, np.abs(cref).max()))
            for B in (7, 33):
                c32 = prim.back_project_coeffs(X[:B], dtype=np.float32)
                assert np.all(np.abs(c32 - cref[:B]) <= pose_tol(cref[:B])), (D, B)
            np.testing.assert_allclose(prim.spline_evaluate(cref), ref, rtol=0, atol=4e-12 * scale)
            np.testing.assert_allclose(prim.spline_evaluate(cref, grid), ref_t, rtol=0, atol=4e-12 * max(1.0, np.abs(ref_t).max()))
    finally:
        grid.close()
        prim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D", FORCED_DS)
def test_forced_chunk_plans(ctx, D):
    """MG_OPT_CHUNK_SAMPLES / MG_OPT_CHUNK_WINDOW / MG_OPT_RING_SLOTS set before the primitive and its grids are built: chunks of
    one sample, max_nt 16 and 32, a window of four, eight chunks and more than eight (descriptors from memory in the tile-major
    kernel; the chunk-stationary kernel must decline).  Both kernels and the step, every launch twice."""
    N_CU[0] = ctx.device_info()["n_cu"]
    s = _row(D, FORCED_L)
    data = _make(s)
    cp = c_oracle.COraclePrimitive(data)
    times = _eval_times(F)
    S = np.random.default_rng(D).standard_normal((33, s["L"]))
    models = {}
    for dtype in (np.float32, np.float64):
        X64 = S.astype(dtype).astype(np.float64)
        models[dtype] = (cp.frames_f32model(X64), cp.frames_f32model(X64, tp=times))
    classes = d_classes(D)
    for opts in FORCED_PLANS:
        _reset(ctx)
        _set_plan_options(ctx, **opts)
        plan, plan_t = _canonical_plan(s, **opts), _eval_plan(s, **opts)
        prim = _capi.Primitive(ctx, data)
        grid = prim.time_grid(times)
        try:
            tag = "%s %s" % (s["name"], opts)
            _check_plan(ctx, prim, s, plan, 33, tag)
            cls = classes | ({"chunks>8"} if plan["n_chunks"] > MG_ARG_CHUNKS else set())
            for dtype in (np.float32, np.float64):
                X = S.astype(dtype)
                model, model_t = models[dtype]
                for B in (17, 33):
                    ran = _lds_kernels(ctx, prim, X[:B], model[:B], None, plan["cs_ok"], tag + " B %d" % B, reps=2)
                    _lds_kernels(ctx, prim, X[:B], model_t[:B], grid, plan_t["cs_ok"], tag + " eval grid B %d" % B, reps=2)
                    assert 1 in ran and (2 in ran) == plan["cs_ok"]
                    cs_fused_ok = plan["cs_ok"] and plan["cs_lds_bytes"] + fused_lds(K) <= LDS_BUDGET
                    sran = _step(ctx, prim, cp, X[:B], model[:B], tag + " B %d" % B, cs_fused_ok, reps=2)
                    assert 0 in sran and (2 in sran) == cs_fused_ok
                _note("ws", cls, dtype, 1)
                _note("step", cls, dtype, 1)
                if plan["cs_ok"]:
                    _note("cs", cls, dtype, 1)
        finally:
            grid.close()
            prim.close()
            _reset(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [5, 78, 79])
def test_few_workgroups_walk_every_unit(ctx, D):
    """With all compute units but one, then but three, reserved, one workgroup (three) walks all units of 130 candidates: the bits
    of the unreserved run, from both kernels and the step (two launches where a workgroup would score more than four tiles)."""
    s = _row(D, FORCED_L)
    data = _make(s)
    cp = c_oracle.COraclePrimitive(data)
    n_cu = ctx.device_info()["n_cu"]
    N_CU[0] = n_cu
    plan = _canonical_plan(s)
    prim = _capi.Primitive(ctx, data)
    try:
        S = np.random.default_rng(D).standard_normal((130, s["L"]))
        for dtype in (np.float32, np.float64):
            X = S.astype(dtype)
            model = cp.frames_f32model(X.astype(np.float64))
            free = _lds_kernels(ctx, prim, X, model, None, plan["cs_ok"], "%s unreserved" % s["name"])
            frames0, logp0 = _fused_step(ctx, prim, X, F, D)
            assert 2 in free
            for keep in (1, 3):
                ctx.set_reserved_cus(n_cu - keep)
                N_CU[0] = keep
                assert prim.step_plan(130, dtype=dtype)["workgroups"] == keep
                ran = _lds_kernels(ctx, prim, X, model, None, plan["cs_ok"] and keep >= plan["n_chunks"], "%s %d workgroups" % (s["name"], keep))
                assert ran == free
                frames, logp = _fused_step(ctx, prim, X, F, D)
                np.testing.assert_array_equal(_bits(frames), _bits(frames0))
                np.testing.assert_array_equal(_bits(logp), _bits(logp0))
            ctx.set_reserved_cus(0)
            N_CU[0] = n_cu
    finally:
        ctx.set_reserved_cus(0)
        prim.close()


GUARD = 256                      # sentinel floats on either side of an output
SENTINEL = 0xFFA5C3E1            # a NaN payload no kernel produces


def _guarded(ctx, n):
    buf = ctx.upload(np.full(n + 2 * GUARD, SENTINEL, dtype=np.uint32))
    return buf, buf.address + 4 * GUARD


def _read_guarded(ctx, buf, n, tag):
    raw = ctx.download(buf, (n + 2 * GUARD,), np.uint32)
    assert np.all(raw[:GUARD] == SENTINEL), "%s: wrote in front of the output (float %d)" % (tag, int(np.flatnonzero(raw[:GUARD] != SENTINEL)[-1]) - GUARD)
    assert np.all(raw[GUARD + n:] == SENTINEL), "%s: wrote past the output (float +%d)" % (tag, int(np.flatnonzero(raw[GUARD + n:] != SENTINEL)[0]))
    return raw[GUARD:GUARD + n]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 78, 79, 81])
def test_outputs_stay_inside_their_buffers(ctx, D):
    """Through the device entry points: 256 sentinel floats in front of and behind the frames (and log p) stay untouched after
    every kernel and after the step, and latents with a leading dimension of L + 3 whose extra columns hold NaN give the bits
    of the packed call."""
    N_CU[0] = ctx.device_info()["n_cu"]
    s = _row(D, FORCED_L)
    L = s["L"]
    data = _make(s)
    cp = c_oracle.COraclePrimitive(data)
    plan = _canonical_plan(s)
    for mode in (1, 2):
        ctx.set_option(_capi.MG_OPT_ROOT_MODE, mode)
        prim = _capi.Primitive(ctx, data)
        try:
            for B in (8, 17):
                for dtype in (np.float32, np.float64):
                    X = np.random.default_rng(10 * D + B).standard_normal((B, L)).astype(dtype)
                    model = cp.frames_f32model(X.astype(np.float64), root_split=mode == 2)
                    lp_sep = prim.gmm_log_prob(X, dtype=np.float32)
                    wide = np.full((B, L + 3), np.nan, dtype=dtype)
                    wide[:, :L] = X
                    d_x, d_wide = ctx.upload(X), ctx.upload(wide)
                    n = B * F * D
                    try:
                        for lat, ld in ((d_x, L), (d_wide, L + 3)):
                            for path, kern in ((_capi.MG_PATH_DIRECT, 0), (_capi.MG_PATH_MFMA, 1), (_capi.MG_PATH_MFMA, 2), (_capi.MG_PATH_AUTO, 0)):
                                tag = "D %d B %d %s mode %d ld %d path %d kernel %d" % (D, B, np.dtype(dtype).name, mode, ld, path, kern)
                                ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, kern)
                                buf, out = _guarded(ctx, n)
                                try:
                                    prim.back_project_frames_dev(lat, dtype, B, ld, out, path=path)
                                except _capi.MGError as e:
                                    assert kern == 2 and e.status == MG_ERR_UNSUPPORTED and not plan["cs_ok"], (tag, e)
                                    buf.free()
                                    continue
                                ctx.synchronize()
                                np.testing.assert_array_equal(_read_guarded(ctx, buf, n, tag), _bits(model).ravel(), err_msg=tag)
                                buf.free()
                            for kern in (0, 2):
                                tag = "D %d B %d %s mode %d ld %d step kernel %d" % (D, B, np.dtype(dtype).name, mode, ld, kern)
                                ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, kern)
                                buf, out = _guarded(ctx, n)
                                lbuf, lout = _guarded(ctx, B)
                                try:
                                    prim.step_frames_and_logp_dev(lat, dtype, B, ld, out, lout)
                                except _capi.MGError as e:
                                    cs_fused_ok = plan["cs_ok"] and plan["cs_lds_bytes"] + fused_lds(K) <= LDS_BUDGET
                                    assert kern == 2 and e.status == MG_ERR_UNSUPPORTED and not cs_fused_ok, (tag, e)
                                    buf.free()
                                    lbuf.free()
                                    continue
                                ctx.synchronize()
                                np.testing.assert_array_equal(_read_guarded(ctx, buf, n, tag), _bits(model).ravel(), err_msg=tag)
                                np.testing.assert_array_equal(_read_guarded(ctx, lbuf, B, tag + " log p"), _bits(lp_sep), err_msg=tag)
                                buf.free()
                                lbuf.free()
                            ctx.set_option(_capi.MG_OPT_FRAMES_KERNEL, 0)
                    finally:
                        d_x.free()
                        d_wide.free()
        finally:
            prim.close()
    _reset(ctx)


@pytest.mark.gpu
def test_the_ledger_covers_every_class(ctx):
    """For each of the direct, tile-major and chunk-stationary kernels and the step: every D class of the table ran and matched,
    for both latent dtypes and both root modes (forced plans: the float64 pipeline) -- nroot 1, 2, 3; partial last quads of 1, 2
    and 3 floats; the shifted third sample with partial stores; row groups of 16, 21, 32 and 33 lanes; every window width from 4
    to 11; plans of more than eight chunks (which the chunk-stationary kernel declines).  The chunk-stationary kernel is asked
    for every class in which the restated planner says it covers a shape.  (Shapes the sweep has not run yet are run here.)"""
    for s in SHAPES:
        _sweep(ctx, s)
    if not any(c == "chunks>8" for _, c, _, _ in LEDGER):
        for D in FORCED_DS:
            test_forced_chunk_plans(ctx, D)
    dts, modes = ("float32", "float64"), (1, 2)
    want = {(k, c, dt, m) for k in ("direct", "ws", "step") for c in WANTED_CLASSES for dt in dts for m in modes}
    cs_classes = set()
    for s in SHAPES:
        if _canonical_plan(s)["cs_ok"]:
            cs_classes |= _shape_classes(s)
    want |= {("cs", c, dt, m) for c in cs_classes for dt in dts for m in modes}
    want |= {(k, "chunks>8", dt, 1) for k in ("ws", "step") for dt in dts}
    assert set(WANTED_CLASSES) <= cs_classes
    assert not any(k == "cs" and c == "chunks>8" for k, c, _, _ in LEDGER)
    table = {}
    for k, c, dt, m in sorted(LEDGER):
        table.setdefault(k, set()).add(c)
    print("\nledger (kernel: D classes)")
    for k, cs_ in sorted(table.items()):
        print("  %-7s %s" % (k, sorted(cs_)))
    missing = sorted(want - LEDGER)
    assert not missing, "shapes of the table no longer exercise: %s" % missing
