// Trajectory constraints on the device (gfx950): TrajectoryConstraint.get_residual_vector / evaluate_motion_spline for
// the ROOT joint (reference morphablegraphs/constraints/spatial_constraints/trajectory_constraint.py:79-121):
// per frame of the motion the distance from the root position to the closest point of a Catmull-Rom spline
// (splines/catmull_rom_spline.py:118-168) whose parameter is at or after the previous frame's; the constraint's error is
// the average over the frames.  The reference finds that point with scipy's L-BFGS-B started at the lower bound
// (splines/parameterized_spline.py:303-322).  Round 5: PINNED -- the reference's own function produced
// tests/golden/trajectory_closest_point.npz (with a size-1-array shim for NumPy >= 1.24, oracle/gen_golden.py), and the search here
// IS that algorithm restated for one bounded variable (mg_traj_device.h: mg_traj_closest_lbfgsb; why nothing less reproduces the
// reference is told there).  The deterministic walk of rounds 2-4 -- on the grid u_k = k / granularity forward from the bound while
// the distance falls, parabola, Newton steps: the local minimum of the first basin at or after the bound -- stays as
// MG_OPT_TRAJECTORY_SEARCH = 1: equal to the reference where the distance has one basin ahead of the bound (smooth path following),
// up to 0.9 of the parameter range away from it where it has several.
//
// One thread per candidate (the search is a chain over the frames): the candidate's root coefficient rows
// (n_basis x 3, float64 fma chains over the latents) are staged in LDS, every frame is four taps of them.
// 172 + 8 bytes per candidate: arithmetic / latency bound, a scoring kernel beside mg_score_constraints.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "mg_internal.h"
#include "mg_score_device.h"
#include "mg_spline_device.h"
#include "mg_traj_device.h"
#include "mg_tree_plan.h"

struct mg_traj_args {
    const double *poly, *E, *mean;
    const void *lat;
    const int32_t *i0;
    const double *w;
    double *out, *res;
    int64_t B, ld;
    int32_t T, L, NB, n_seg, G, lat_f64, accumulate, align_mode;   // align_mode 0: none, 1: previous frame (root node), 2: start pose
    double min_u, weight;
    double al[7];   // heading (x, z) or (cos, sin); landing (x, z); ref_dir (3) or height
    const double *al_cand;  // NULL, or (B, 4): the previous unit heading (x, z) and root position (x, z) of EVERY candidate, in place of
                            // al[0..3] (align_mode 1 only; mg_score_trajectory_chained: the layout of mg_score_args::align_cand)
    const double *points;   // NULL, or (B, T, 3): the positions to follow the trajectory with, given instead of derived from the
                            // candidates' root rows (any joint's track from mg_joint_positions; already aligned by the caller)
    double *res_u;          // NULL, or (B, T): the parameter the search settles on in every frame (mg_trajectory_closest_points)
    int32_t *res_n;         // NULL, or (B, T): the (f, g) evaluations every frame's search took (the reference's search only)
    double *paths;          // the reference's search on candidates' root paths: (B, T, 3) scratch the kernel writes the paths to first (a lane
                            // then searches ITS frames at its own pace, mg_traj_chain)
    int32_t search;         // 0: the reference's search (L-BFGS-B restated, mg_traj_closest_lbfgsb), 1: the monotone walk (MG_OPT_TRAJECTORY_SEARCH)
};

#define MG_TRAJ_BLOCK 64

// The candidate's aligning transform (mg_score_device.h: mg_traj_alignment_of, which the one-launch tree search calls as well).
// cand: the candidate's index in the batch, clamped to it by the caller (a lane past the batch reads the last candidate's record and
// writes nothing) -- where every candidate has its own previous heading and position (al_cand) they are read from its row, used as
// they are.
template <typename RootFn>
__device__ __forceinline__ mg_align2d mg_traj_alignment(const mg_traj_args &a, const int64_t cand, RootFn root) {
    return mg_traj_alignment_of(a.align_mode, a.al, a.NB, a.al_cand ? a.al_cand + 4 * cand : nullptr, root);   // (al_cand: uniform, a kernel argument)
}

// POLY_LDS: the target spline's segment polynomials (12 n_seg + 3 doubles) are copied behind the rows and searched from there -- the walk
// is a chain of dependent evaluations (about 17 per frame), each one a look-up of its segment: an LDS read instead of a trip to L2
template <bool POLY_LDS>
__global__ __launch_bounds__(MG_TRAJ_BLOCK) void mg_trajectory_kernel(mg_traj_args a) {
    extern __shared__ double lds[];                 // [L + rows][64]: the latents, then the root coefficient rows; [12 n_seg + 3] the polynomials
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * MG_TRAJ_BLOCK + tid;
    const bool valid = b < a.B;
    const int64_t bb = valid ? b : a.B - 1;
    const int rows = a.NB * 3 + 4;
    double *ls = lds, *lc = lds + (size_t)a.L * MG_TRAJ_BLOCK;
    const double *poly = a.poly;
    if constexpr (POLY_LDS) {
        double *lp = lds + (a.points ? 0 : (size_t)(a.L + rows) * MG_TRAJ_BLOCK);
        for (int e = tid; e < a.n_seg * 12 + 3; e += MG_TRAJ_BLOCK) lp[e] = a.poly[e];
        poly = lp;
        __syncthreads();
    }
    if (!a.points) {
        for (int k = 0; k < a.L; k++)
            ls[k * MG_TRAJ_BLOCK + tid] = mg_load_lat(a.lat, a.lat_f64 != 0, bb * a.ld + k);
        for (int r = 0; r < rows; r++)
            lc[r * MG_TRAJ_BLOCK + tid] = mg_control_point(a.mean[r], a.E + (size_t)r * a.L, 1, a.L, [&](int k) { return ls[k * MG_TRAJ_BLOCK + tid]; });
    }
    const mg_align2d t = mg_traj_alignment(a, bb, [&](int r) { return lc[r * MG_TRAJ_BLOCK + tid]; });
    const int G = a.G;
    const double invG = 1.0 / (double)G;
    double min_u = a.min_u, sum = 0.0;
    auto position = [&](int f, double *q) {        // the candidate's root position in frame f, aligned
        const int i0 = a.i0[f];
        const double *w = a.w + 4 * (size_t)f;
#pragma unroll
        for (int d = 0; d < 3; d++)
            q[d] = mg_taps4(w, lc + (i0 * 3 + d) * MG_TRAJ_BLOCK + tid, 3 * MG_TRAJ_BLOCK);
        if (a.align_mode != 0) mg_align_position(t, q[0], q[1], q[2]);
    };
    if (a.search == 0) {
        // the reference's search: every lane walks ITS frames at its own pace (mg_traj_chain); the positions come from the caller's
        // points or, for the root path, are evaluated per lane from the rows in LDS
        const double *pts = a.points ? a.points + (size_t)bb * a.T * 3 : nullptr;
        mg_traj_chain(poly, a.n_seg, valid ? a.T : 0, a.min_u,
                      [&](int f, double *q) { if (pts) { q[0] = pts[3 * f]; q[1] = pts[3 * f + 1]; q[2] = pts[3 * f + 2]; } else position(f, q); },
                      [&](int f, double dist, double u, int trips) {
                          sum += dist;
                          if (a.res) a.res[b * a.T + f] = a.weight * dist;
                          if (a.res_u) a.res_u[b * a.T + f] = u;
                          if (a.res_n) a.res_n[b * a.T + f] = trips;
                      });
    } else {
        // (given positions: the next frame's point is requested a frame ahead -- its trip to memory would otherwise head every frame's
        // chain of dependent evaluations)
        double qn[3] = {0.0, 0.0, 0.0};
        if (a.points && a.T > 0) { const double *pp = a.points + (size_t)bb * a.T * 3; qn[0] = pp[0]; qn[1] = pp[1]; qn[2] = pp[2]; }
        for (int f = 0; f < a.T; f++) {
            double q[3];
            if (a.points) {
                q[0] = qn[0]; q[1] = qn[1]; q[2] = qn[2];
                if (f + 1 < a.T) { const double *pp = a.points + ((size_t)bb * a.T + f + 1) * 3; qn[0] = pp[0]; qn[1] = pp[1]; qn[2] = pp[2]; }
            } else position(f, q);
            // (mg_traj_device.h; min_u moves to the point's parameter; every lane of the wave is here: the walk's long searches get its help)
            const double dist = mg_traj_closest_dist<true>(poly, a.n_seg, G, invG, &min_u, q);
            sum += dist;
            if (a.res && valid) a.res[b * a.T + f] = a.weight * dist;
            if (a.res_u && valid) a.res_u[b * a.T + f] = min_u;
        }
    }
    if (valid && a.out) {
        const double e = a.weight * (a.T > 0 ? sum / (double)a.T : 0.0);
        a.out[b] = a.accumulate ? a.out[b] + e : e;
    }
}

// The same scorer with MG_TRAJ_W lanes per candidate, for batches that leave most of the chip idle at one lane per candidate (4096
// candidates are 64 waves on 1024 SIMDs, each a chain of ~18 dependent float64 evaluations per frame): the lanes of a candidate split
// its coefficient rows (each row the same fma chain as above), then walk the frames together -- every lane the same q, the grid values
// of the closest-point search side by side (mg_traj_closest_dist_coop).  Same operations on the same values: the same bits.
// (W = 8 or 4: with four lanes a window holds three grid values and a walk of six steps takes three more rounds, but the Newton steps
// are repeated four times, not eight: measured, four lanes win only between ~28 000 and ~40 000 candidates in flight -- 762 us at
// 32 768 against 899 with eight and 888 with one)
#define MG_TRAJ_COOP_BLOCK 64
template <int MG_TRAJ_W>
__device__ __forceinline__ void mg_trajectory_coop_body(const mg_traj_args &a, const int64_t block, double *lds) {
    constexpr int MG_TRAJ_COOP_CANDS = MG_TRAJ_COOP_BLOCK / MG_TRAJ_W;
    // lds: [CANDS][L] latents, [CANDS][rows] root coefficient rows, [12 n_seg + 3] the polynomials
    const int tid = threadIdx.x, grp = tid / MG_TRAJ_W, sub = tid % MG_TRAJ_W;
    const int64_t b = block * MG_TRAJ_COOP_CANDS + grp;
    const bool valid = b < a.B;
    const int64_t bb = valid ? b : a.B - 1;
    const int rows = a.NB * 3 + 4;
    double *ls = lds + (size_t)grp * a.L, *lc = lds + (size_t)MG_TRAJ_COOP_CANDS * a.L + (size_t)grp * rows;
    double *lp = lds + (a.points ? 0 : (size_t)MG_TRAJ_COOP_CANDS * (a.L + rows));
    for (int e = tid; e < a.n_seg * 12 + 3; e += MG_TRAJ_COOP_BLOCK) lp[e] = a.poly[e];
    if (!a.points) {
        for (int k = sub; k < a.L; k += MG_TRAJ_W) ls[k] = mg_load_lat(a.lat, a.lat_f64 != 0, bb * a.ld + k);
        __syncthreads();
        for (int r = sub; r < rows; r += MG_TRAJ_W) lc[r] = mg_control_point(a.mean[r], a.E + (size_t)r * a.L, 1, a.L, [&](int k) { return ls[k]; });
    }
    __syncthreads();
    const mg_align2d t = mg_traj_alignment(a, bb, [&](int r) { return lc[r]; });   // (bb: the group's candidate, the same in its MG_TRAJ_W lanes)
    const int G = a.G;
    const double invG = 1.0 / (double)G;
    double min_u = a.min_u, sum = 0.0;
    // (given positions: the next frame's point is requested a frame ahead -- its trip to memory would otherwise head every frame's
    // chain of dependent evaluations)
    double qn[3] = {0.0, 0.0, 0.0};
    if (a.points && a.T > 0) { const double *pp = a.points + (size_t)bb * a.T * 3; qn[0] = pp[0]; qn[1] = pp[1]; qn[2] = pp[2]; }
    for (int f = 0; f < a.T; f++) {
        double q[3];
        if (a.points) {
            q[0] = qn[0]; q[1] = qn[1]; q[2] = qn[2];
            if (f + 1 < a.T) { const double *pp = a.points + ((size_t)bb * a.T + f + 1) * 3; qn[0] = pp[0]; qn[1] = pp[1]; qn[2] = pp[2]; }
        } else {
            const int i0 = a.i0[f];
            const double *w = a.w + 4 * (size_t)f;
#pragma unroll
            for (int d = 0; d < 3; d++) q[d] = mg_taps4(w, lc + i0 * 3 + d, 3);
        }
        if (a.align_mode != 0) mg_align_position(t, q[0], q[1], q[2]);
        const double dist = mg_traj_closest_dist_coop<MG_TRAJ_W>(lp, a.n_seg, G, invG, &min_u, q);
        sum += dist;
        if (a.res && valid && sub == 0) a.res[b * a.T + f] = a.weight * dist;
        if (a.res_u && valid && sub == 0) a.res_u[b * a.T + f] = min_u;
    }
    if (valid && sub == 0 && a.out) {
        const double e = a.weight * (a.T > 0 ? sum / (double)a.T : 0.0);
        a.out[b] = a.accumulate ? a.out[b] + e : e;
    }
}
template <int W>
__global__ __launch_bounds__(MG_TRAJ_COOP_BLOCK) void mg_trajectory_coop_kernel(mg_traj_args a) {
    extern __shared__ double lds[];
    mg_trajectory_coop_body<W>(a, blockIdx.x, lds);
}

// One lane per candidate for batches that fill the chip that way (from ~32 768 candidates in flight: eight lanes per candidate repeat
// the Newton steps eight times, which is what counts once every SIMD has waves to choose from) -- WITHOUT the candidate's 97
// coefficient rows in LDS: mg_trajectory_kernel keeps them there, 50 KB per wave, three waves per CU.  A frame's position needs the four
// control points of its knot span only, and the span moves one control point at a time: a window of 4 x 3 control points lives in
// registers, the next control point (three fma chains over the latents, the statements of the staged form) is made when the span
// moves (every 5.6 frames for 'walk').  LDS: the latents (20 KB per wave) and the polynomials.  Same operations, same bits.
__device__ __forceinline__ void mg_trajectory_stream_body(const mg_traj_args &a, const int64_t block, double *lds) {
    const int tid = threadIdx.x;
    const int64_t b = block * MG_TRAJ_BLOCK + tid;
    const bool valid = b < a.B;
    const int64_t bb = valid ? b : a.B - 1;
    double *ls = lds, *lp = lds + (size_t)a.L * MG_TRAJ_BLOCK;
    for (int e = tid; e < a.n_seg * 12 + 3; e += MG_TRAJ_BLOCK) lp[e] = a.poly[e];
    for (int k = 0; k < a.L; k++)
        ls[k * MG_TRAJ_BLOCK + tid] = mg_load_lat(a.lat, a.lat_f64 != 0, bb * a.ld + k);
    __syncthreads();
    auto row = [&](int r) { return mg_control_point(a.mean[r], a.E + (size_t)r * a.L, 1, a.L, [&](int k) { return ls[k * MG_TRAJ_BLOCK + tid]; }); };
    const mg_align2d t = mg_traj_alignment(a, bb, row);
    const int G = a.G;
    const double invG = 1.0 / (double)G;
    double min_u = a.min_u, sum = 0.0;
    double cw[4][3];                       // control points cur .. cur + 3 of the three root channels
    int cur = INT_MIN;
    auto position = [&](int f, double *q) {  // frame f's aligned root position (called with f ascending, the same f in every lane)
        const int i0 = a.i0[f];             // (the same for every lane: the branches below are uniform)
        if (i0 != cur) {
            if (cur != INT_MIN && i0 == cur + 1) {
#pragma unroll
                for (int j = 0; j < 3; j++)
#pragma unroll
                    for (int d = 0; d < 3; d++) cw[j][d] = cw[j + 1][d];
#pragma unroll
                for (int d = 0; d < 3; d++) cw[3][d] = row((i0 + 3) * 3 + d);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int d = 0; d < 3; d++) cw[j][d] = row((i0 + j) * 3 + d);
            }
            cur = i0;
        }
        const double *w = a.w + 4 * (size_t)f;
#pragma unroll
        for (int d = 0; d < 3; d++) q[d] = mg_taps4(w, &cw[0][d], 3);
        if (a.align_mode != 0) mg_align_position(t, q[0], q[1], q[2]);
    };
    if (a.search == 0) {
        // the reference's search: first the whole path, frame by frame with the window in registers (the lanes in step), into the
        // caller's scratch; then every lane searches ITS frames at its own pace (a lane reads back what it wrote itself)
        double *mine = a.paths + (size_t)bb * a.T * 3;
        if (valid)
            for (int f = 0; f < a.T; f++) {
                double q[3];
                position(f, q);
                mine[3 * f] = q[0]; mine[3 * f + 1] = q[1]; mine[3 * f + 2] = q[2];
            }
        mg_traj_chain(lp, a.n_seg, valid ? a.T : 0, a.min_u,
                      [&](int f, double *q) { q[0] = mine[3 * f]; q[1] = mine[3 * f + 1]; q[2] = mine[3 * f + 2]; },
                      [&](int f, double dist, double u, int trips) {
                          sum += dist;
                          if (a.res) a.res[b * a.T + f] = a.weight * dist;
                      });
    } else {
        for (int f = 0; f < a.T; f++) {
            double q[3];
            position(f, q);
            const double dist = mg_traj_closest_dist<true>(lp, a.n_seg, G, invG, &min_u, q);   // (every lane of the wave is here: the help is legal)
            sum += dist;
            if (a.res && valid) a.res[b * a.T + f] = a.weight * dist;
        }
    }
    if (valid) {
        const double e = a.weight * (a.T > 0 ? sum / (double)a.T : 0.0);
        a.out[b] = a.accumulate ? a.out[b] + e : e;
    }
}
__global__ __launch_bounds__(MG_TRAJ_BLOCK) void mg_trajectory_stream_kernel(mg_traj_args a) {
    extern __shared__ double lds[];
    mg_trajectory_stream_body(a, blockIdx.x, lds);
}
// Several scorers in ONE launch (mg_score_trajectories): a planner step scores every option's candidates against the option's own
// trajectory -- 4096 candidates at eight lanes each fill a quarter of the chip and take 0.4 ms, sixteen such launches one after the
// other 7 ms; side by side they take what the chip's four quarters take.
#define MG_TRAJ_MULTI_MAX 16
struct mg_traj_multi { int32_t n; int32_t wg0[MG_TRAJ_MULTI_MAX + 1]; mg_traj_args a[MG_TRAJ_MULTI_MAX]; };
template <int W>
__global__ __launch_bounds__(MG_TRAJ_COOP_BLOCK) void mg_trajectory_coop_multi_kernel(const mg_traj_multi m) {
    extern __shared__ double lds[];
    int k = 0;
    while (k + 1 < m.n && (int)blockIdx.x >= m.wg0[k + 1]) k++;
    mg_trajectory_coop_body<W>(m.a[k], (int64_t)blockIdx.x - m.wg0[k], lds);
}
__global__ __launch_bounds__(MG_TRAJ_BLOCK) void mg_trajectory_stream_multi_kernel(const mg_traj_multi m) {
    extern __shared__ double lds[];
    int k = 0;
    while (k + 1 < m.n && (int)blockIdx.x >= m.wg0[k + 1]) k++;
    mg_trajectory_stream_body(m.a[k], (int64_t)blockIdx.x - m.wg0[k], lds);
}
// Lanes per candidate for `total` candidates in flight (measured: tools/probes/trajectory_lanes.py): eight while most SIMDs would idle
// otherwise, four in between, one (the streaming kernel) once one lane per candidate fills the chip.  MG_OPT_TRAJECTORY_LANES forces.
#define MG_TRAJ_COOP_MAX_B 65536       // (no batch above this takes several lanes per candidate, whatever is forced)
#define MG_TRAJ_W8_MAX_TOTAL 28672
#define MG_TRAJ_W4_MAX_TOTAL 40960
static int mg_traj_lanes(const mg_context *ctx, int64_t B, int64_t total) {
    const int opt = ctx->opt[MG_OPT_TRAJECTORY_LANES];
    if (ctx->opt[MG_OPT_TRAJECTORY_SEARCH] != 1) return 1;    // the reference's search is one chain of evaluations: nothing for more lanes to do
    if (opt == 1 || B > MG_TRAJ_COOP_MAX_B) return 1;
    if (opt == 8 || opt == 4) return opt;
    return total <= MG_TRAJ_W8_MAX_TOTAL ? 8 : (total <= MG_TRAJ_W4_MAX_TOTAL ? 4 : 1);
}

// THE DISPATCH, stated once: which kernel scores B candidates per scorer (`total` in flight: n x B for the n scorers of
// mg_score_trajectories, B otherwise) of a primitive with L latents and `rows` root coefficient rows against a spline of n_seg
// segments, on the root rows or on given points -- and with how many lanes per candidate, how much LDS, whether the kernel needs the
// context's path scratch and whether the scorer fits the side-by-side launch.  Pure host arithmetic; every entry point calls it
// and mg_trajectory_plan reports it (tests/test_gpu_trajectory_shapes.py restates it and pins it line by line).
struct mg_traj_plan_t { int kernel, lanes, cands; bool poly_lds, needs_paths, together; size_t lds_bytes; };
static int mg_traj_plan(const mg_context *ctx, int L, int rows, int n_seg, int64_t B, int64_t total, bool points, int search, mg_traj_plan_t *out) {
    mg_traj_plan_t pl = {MG_TRAJ_KERNEL_STAGED_LDS, 1, MG_TRAJ_BLOCK, true, false, false, 0};
    const size_t poly_bytes = ((size_t)n_seg * 12 + 3) * 8;
    if (points) {
        pl.lanes = poly_bytes <= 60 * 1024 ? mg_traj_lanes(ctx, B, B) : 1;
        pl.poly_lds = pl.lanes > 1 || poly_bytes <= 158 * 1024;
        pl.lds_bytes = pl.poly_lds ? poly_bytes : 0;
        pl.kernel = pl.lanes == 8 ? MG_TRAJ_KERNEL_COOP8 : pl.lanes == 4 ? MG_TRAJ_KERNEL_COOP4 : pl.poly_lds ? MG_TRAJ_KERNEL_STAGED_LDS : MG_TRAJ_KERNEL_STAGED_GLOBAL;
        pl.cands = MG_TRAJ_COOP_BLOCK / pl.lanes;
        *out = pl;
        return MG_OK;
    }
    if (total > B) {        // one of several scorers: side by side where its rows and polynomials fit the cooperative or the streaming form
        const int lanes = mg_traj_lanes(ctx, B, total);
        const bool coop = lanes > 1;
        const int coop_cands = MG_TRAJ_COOP_BLOCK / lanes;
        const size_t need = coop ? (size_t)coop_cands * (L + rows) * 8 + poly_bytes
                                 : (size_t)L * MG_TRAJ_BLOCK * 8 + poly_bytes;
        if (need <= 60 * 1024) {
            pl.kernel = lanes == 8 ? MG_TRAJ_KERNEL_COOP8_MULTI : lanes == 4 ? MG_TRAJ_KERNEL_COOP4_MULTI : MG_TRAJ_KERNEL_STREAM_MULTI;
            pl.lanes = lanes; pl.cands = coop ? coop_cands : MG_TRAJ_BLOCK; pl.lds_bytes = need;
            pl.needs_paths = !coop && search == 0; pl.together = true;
            *out = pl;
            return MG_OK;
        }
    }
    size_t lds = (size_t)(L + rows) * MG_TRAJ_BLOCK * 8;
    if (lds > 150 * 1024) { mg_set_error("mg_score_trajectory: %d basis functions x %d components do not fit LDS", (rows - 4) / 3, L); return MG_ERR_UNSUPPORTED; }
    const bool poly_lds = lds + poly_bytes <= 158 * 1024;
    if (poly_lds) lds += poly_bytes;
    int lanes = mg_traj_lanes(ctx, B, B);
    const int coop_cands = MG_TRAJ_COOP_BLOCK / std::max(lanes, 1);
    const size_t coop_lds = (size_t)coop_cands * (L + rows) * 8 + poly_bytes;
    if (coop_lds > 60 * 1024) lanes = 1;
    const size_t stream_lds = (size_t)L * MG_TRAJ_BLOCK * 8 + poly_bytes;
    pl.lanes = lanes; pl.cands = MG_TRAJ_COOP_BLOCK / lanes;
    if (lanes > 1) { pl.kernel = lanes == 8 ? MG_TRAJ_KERNEL_COOP8 : MG_TRAJ_KERNEL_COOP4; pl.lds_bytes = coop_lds; }
    else if (stream_lds <= 60 * 1024) { pl.kernel = MG_TRAJ_KERNEL_STREAM; pl.lds_bytes = stream_lds; pl.needs_paths = search == 0; }
    else { pl.kernel = poly_lds ? MG_TRAJ_KERNEL_STAGED_LDS : MG_TRAJ_KERNEL_STAGED_GLOBAL; pl.poly_lds = poly_lds; pl.lds_bytes = lds; }
    *out = pl;
    return MG_OK;
}
extern "C" int mg_trajectory_plan(const mg_context *ctx, int32_t n_components, int32_t rows, int32_t n_seg, int64_t n_samples, int64_t total, int32_t points,
                                  mg_trajectory_plan_info *out) {
    if (!ctx || !out || n_components < 1 || rows < 4 || n_seg < 1 || n_samples < 1 || total < 1) {
        mg_set_error("mg_trajectory_plan: bad arguments");
        return MG_ERR_INVALID_ARGUMENT;
    }
    mg_traj_plan_t pl;
    const int rc = mg_traj_plan(ctx, n_components, rows, n_seg, n_samples, total, points != 0, ctx->opt[MG_OPT_TRAJECTORY_SEARCH] == 1 ? 1 : 0, &pl);
    if (rc != MG_OK) return rc;
    out->kernel = pl.kernel; out->lanes = pl.lanes; out->poly_lds = pl.poly_lds ? 1 : 0; out->needs_paths = pl.needs_paths ? 1 : 0;
    out->together = pl.together ? 1 : 0; out->candidates_per_workgroup = pl.cands; out->lds_bytes = (int64_t)pl.lds_bytes;
    return MG_OK;
}
// the context's buffer for the candidates' root paths (the reference's search in the streaming kernels): grown on demand, stream ordered
static int mg_traj_paths(mg_context *ctx, size_t bytes, double **out) {
    if (ctx->traj_paths_bytes < bytes) {
        MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));     // a launch may still be reading the old one
        if (ctx->traj_paths) (void)hipFree(ctx->traj_paths);
        ctx->traj_paths = nullptr; ctx->traj_paths_bytes = 0;
        const size_t want = std::max<size_t>(bytes, (size_t)16 << 20);
        MG_HIP_CHECK(hipMalloc(&ctx->traj_paths, want));
        ctx->traj_paths_bytes = want;
    }
    *out = (double *)ctx->traj_paths;
    return MG_OK;
}

template <typename T>
static int mg_traj_upload(const std::vector<T> &h, T **d) {
    *d = nullptr;
    MG_HIP_CHECK(hipMalloc((void **)d, std::max<size_t>(h.size() * sizeof(T), 16)));
    if (!h.empty()) MG_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return MG_OK;
}

extern "C" void mg_trajectory_destroy(mg_trajectory *t) {
    if (!t) return;
    if (t->prim) { (void)hipSetDevice(t->prim->ctx->device); (void)hipStreamSynchronize(t->prim->ctx->stream); }
    (void)hipFree(t->d_poly);
    (void)hipFree(t->d_E);
    (void)hipFree(t->d_mean);
    (void)hipFree(t->d_arc);
    (void)hipFree(t->d_uk);
    delete t;
}

static int mg_traj_finish(mg_primitive *p, const std::vector<double> &poly, int32_t n_seg, int32_t granularity, int32_t spline_type, mg_trajectory **out);

extern "C" int mg_trajectory_create(mg_primitive *p, const double *cp, int32_t n_points, int32_t granularity, mg_trajectory **out) {
    if (!p || !cp || !out || n_points < 2 || granularity < 2 || p->D < 3) {
        mg_set_error("mg_trajectory_create: needs a primitive with root channels, >= 2 control points (x, y, z) and a granularity >= 2");
        return MG_ERR_INVALID_ARGUMENT;
    }
    *out = nullptr;
    for (int i = 0; i < 3 * n_points; i++)
        if (!std::isfinite(cp[i])) { mg_set_error("mg_trajectory_create: control point %d is not finite", i / 3); return MG_ERR_INVALID_ARGUMENT; }
    MG_HIP_CHECK(hipSetDevice(p->ctx->device));
    const int n_seg = n_points - 1;
    // catmull_rom_spline.py:66-71: control points padded to [P0] + P + [Pn, Pn]; segment s (1-based) uses padded[s-1 .. s+2]
    std::vector<double> pad((size_t)(n_points + 3) * 3);
    for (int d = 0; d < 3; d++) {
        pad[d] = cp[d];
        for (int i = 0; i < n_points; i++) pad[(size_t)(i + 1) * 3 + d] = cp[(size_t)i * 3 + d];
        pad[(size_t)(n_points + 1) * 3 + d] = pad[(size_t)(n_points + 2) * 3 + d] = cp[(size_t)(n_points - 1) * 3 + d];
    }
    static const double M[4][4] = {{-1.0, 3.0, -3.0, 1.0}, {2.0, -5.0, 4.0, -1.0}, {-1.0, 0.0, 1.0, 0.0}, {0.0, 2.0, 0.0, 0.0}};
    std::vector<double> poly((size_t)n_seg * 12 + 3);
    for (int s = 0; s < n_seg; s++)           // 0-based segment s = the reference's segment index s + 1
        for (int r = 0; r < 4; r++)
            for (int d = 0; d < 3; d++) {
                double v = 0.0;
                for (int j = 0; j < 4; j++) v += M[r][j] * pad[(size_t)(s + j) * 3 + d];
                poly[(size_t)s * 12 + r * 3 + d] = 0.5 * v;
            }
    for (int d = 0; d < 3; d++) poly[(size_t)n_seg * 12 + d] = cp[(size_t)(n_points - 1) * 3 + d];
    return mg_traj_finish(p, poly, n_seg, granularity, MG_SPLINE_CATMULL_ROM, out);
}

// Everything of a trajectory but its polynomials, the same for every spline type: the primitive's root rows, the arc-length table
// over the curve's points at k / granularity, the uploads.
static int mg_traj_finish(mg_primitive *p, const std::vector<double> &poly, int32_t n_seg, int32_t granularity, int32_t spline_type, mg_trajectory **out) {
    mg_trajectory *t = new (std::nothrow) mg_trajectory();
    if (!t) return MG_ERR_OUT_OF_MEMORY;
    t->prim = p;
    t->n_seg = n_seg;
    t->granularity = granularity;
    t->spline_type = spline_type;
    // root coefficient rows of the primitive (already scaled by translation_maxima), then the root quaternion of the first control point
    const int NB = p->NB, D = p->D, L = p->L;
    t->rows = NB * 3 + 4;
    std::vector<double> E((size_t)t->rows * L, 0.0), mean(t->rows, 0.0);
    for (int i = 0; i < NB; i++)
        for (int d = 0; d < 3; d++) {
            mean[(size_t)i * 3 + d] = p->means_[(size_t)i * D + d];
            for (int k = 0; k < L; k++) E[((size_t)i * 3 + d) * L + k] = p->Es[((size_t)i * D + d) * L + k];
        }
    for (int e = 0; e < 4; e++) {
        const size_t row = (size_t)NB * 3 + e;
        if (D >= 7) {
            mean[row] = p->means_[3 + e];
            for (int k = 0; k < L; k++) E[row * L + k] = p->Es[(size_t)(3 + e) * L + k];
        } else {
            mean[row] = e == 0 ? 1.0 : 0.0;
        }
    }
    // the arc-length parameterisation (splines/arc_length_map.py:45-71): the polyline over granularity + 1 samples, accumulated and
    // normalised -- what the constraints that look targets up BY ARC LENGTH search (mg_frame_constraints.hip)
    std::vector<double> arc((size_t)granularity + 1, 0.0);
    {
        auto point = [&](double u, double *q) {
            const double scaled = t->n_seg * u;
            int index = (int)std::floor(scaled);
            if (index >= t->n_seg) { for (int d = 0; d < 3; d++) q[d] = poly[(size_t)t->n_seg * 12 + d]; return; }
            const double tt = scaled - index;
            const double *A = &poly[(size_t)index * 12];
            for (int d = 0; d < 3; d++) q[d] = ((A[d] * tt + A[3 + d]) * tt + A[6 + d]) * tt + A[9 + d];
        };
        double last[3], cur[3], acc = 0.0;
        point(0.0, last);
        for (int k = 1; k <= granularity; k++) {
            point(k / (double)granularity, cur);
            acc += std::sqrt((cur[0] - last[0]) * (cur[0] - last[0]) + (cur[1] - last[1]) * (cur[1] - last[1]) + (cur[2] - last[2]) * (cur[2] - last[2]));
            arc[(size_t)k] = acc;
            for (int d = 0; d < 3; d++) last[d] = cur[d];
        }
        t->full_arc = acc;
        if (acc > 0.0) for (double &v : arc) v /= acc;
    }
    // the parameters get_absolute_arc_length_of_point scans (parameterized_spline.py:251-268): repeated addition, not k / granularity --
    // the sums drift, so how many there are and every one of them is decided by these roundings (the same in any IEEE double
    // arithmetic, independent of the curve); mg_trajectory_arc.hip reads them, it never forms a parameter itself
    std::vector<double> uk;
    {
        const double step_size = 1.0 / granularity;
        for (double u = 0.0; u <= 1.0 && uk.size() <= (size_t)granularity + 1; u += step_size) uk.push_back(u);
        t->n_uk = (int32_t)uk.size();
    }
    int rc = mg_traj_upload(poly, &t->d_poly);
    if (rc == MG_OK) rc = mg_traj_upload(arc, &t->d_arc);
    if (rc == MG_OK) rc = mg_traj_upload(uk, &t->d_uk);
    if (rc == MG_OK) rc = mg_traj_upload(E, &t->d_E);
    if (rc == MG_OK) rc = mg_traj_upload(mean, &t->d_mean);
    if (rc != MG_OK) { mg_trajectory_destroy(t); return rc; }
    *out = t;
    return MG_OK;
}

// The reference's BSpline (splines/b_spline.py:70-105, 174-188) as cubic pieces: a clamped cubic over n_points - 2 uniform knot values,
// so n_seg = n_points - 3 pieces of equal length.  In units of the knot spacing the knot vector is K_j = clamp(j - 3, 0, n_seg) and on
// piece s the parameter is s + t: de Boor's recurrence d_j <- (1 - alpha) d_(j-1) + alpha d_j with alpha = (s + t - K_j) /
// (K_(j+4-r) - K_j) = a0 + a1 t is carried out on the polynomials' coefficients (ascending powers of t).  The denominators are 1, 2 or
// 3: rounding of a few ulp of the control points.  Statement for statement spline_types.py _b_spline.
static void mg_traj_poly_bspline(const double *cp, int n_seg, std::vector<double> &poly) {
    auto knot = [&](int j) { return (double)std::min(std::max(j - 3, 0), n_seg); };
    for (int s = 0; s < n_seg; s++) {
        const int i = s + 3;                         // the piece's knot span: K_i = s, K_(i+1) = s + 1
        for (int d = 0; d < 3; d++) {
            double c[4][4];
            for (int j = 0; j < 4; j++) { c[j][0] = cp[(size_t)(s + j) * 3 + d]; c[j][1] = c[j][2] = c[j][3] = 0.0; }
            for (int r = 1; r < 4; r++)
                for (int jj = 3; jj >= r; jj--) {    // descending: c[jj - 1] is still the level before
                    const int j = i - 3 + jj;
                    const double den = knot(j + 4 - r) - knot(j);
                    const double a0 = ((double)s - knot(j)) / den, a1 = 1.0 / den;
                    const double *lo = c[jj - 1], *hi = c[jj];
                    double nw[4];
                    nw[0] = (1.0 - a0) * lo[0] + a0 * hi[0];
                    for (int k = 1; k < 4; k++) nw[k] = ((1.0 - a0) * lo[k] + a0 * hi[k]) + a1 * (hi[k - 1] - lo[k - 1]);
                    for (int k = 0; k < 4; k++) c[jj][k] = nw[k];
                }
            for (int r = 0; r < 4; r++) poly[(size_t)s * 12 + r * 3 + d] = c[3][3 - r];
        }
    }
}

// The reference's FittedBSpline (splines/fitted_b_spline.py:44-47): per dimension FITPACK's splrep(linspace(0, 1, n), values, k = 3) with
// s = 0 -- the interpolating cubic spline whose knots are the data sites without the second and the last but one, i.e. whose third
// derivative is continuous there (not-a-knot).  On n - 1 uniform pieces, solved for the second derivatives M_i per unit spacing:
// M_(i-1) + 4 M_i + M_(i+1) = 6 (y_(i-1) - 2 y_i + y_(i+1)); M_0 - 2 M_1 + M_2 = 0 turns the first row into M_1 = y_0 - 2 y_1 + y_2
// (the last likewise), what is left is tridiagonal with 4 on the diagonal: elimination without pivoting is stable.  The first two
// pieces are one cubic re-expanded at the second site, the last two likewise.  Statement for statement spline_types.py _fitted_b_spline.
static void mg_traj_poly_fitted(const double *cp, int m, std::vector<double> &poly) {
    std::vector<double> y(m), D2(m), M(m), cc(m), dd(m);
    for (int d = 0; d < 3; d++) {
        for (int i = 0; i < m; i++) { y[i] = cp[(size_t)i * 3 + d]; D2[i] = M[i] = cc[i] = dd[i] = 0.0; }
        for (int i = 1; i < m - 1; i++) D2[i] = (y[i + 1] - y[i]) - (y[i] - y[i - 1]);
        M[1] = D2[1]; M[m - 2] = D2[m - 2];
        if (m >= 5) {
            const int lo = 2, hi = m - 3;
            for (int i = lo; i <= hi; i++) {
                double rhs = 6.0 * D2[i];
                if (i == lo) rhs -= M[1];
                if (i == hi) rhs -= M[m - 2];
                const double den = i == lo ? 4.0 : 4.0 - cc[i - 1];
                cc[i] = 1.0 / den;
                dd[i] = (i == lo ? rhs : rhs - dd[i - 1]) / den;
            }
            M[hi] = dd[hi];
            for (int i = hi - 1; i >= lo; i--) M[i] = dd[i] - cc[i] * M[i + 1];
        }
        M[0] = 2.0 * M[1] - M[2];
        M[m - 1] = 2.0 * M[m - 2] - M[m - 3];
        for (int s = 0; s < m - 1; s++) {
            poly[(size_t)s * 12 + 0 + d] = (M[s + 1] - M[s]) / 6.0;
            poly[(size_t)s * 12 + 3 + d] = 0.5 * M[s];
            poly[(size_t)s * 12 + 6 + d] = (y[s + 1] - y[s]) - (2.0 * M[s] + M[s + 1]) / 6.0;
            poly[(size_t)s * 12 + 9 + d] = y[s];
        }
    }
}

extern "C" int mg_trajectory_create_typed(mg_primitive *p, const double *cp, int32_t n_points, int32_t granularity, int32_t spline_type, mg_trajectory **out) {
    if (spline_type == MG_SPLINE_CATMULL_ROM) return mg_trajectory_create(p, cp, n_points, granularity, out);
    if (spline_type != MG_SPLINE_BSPLINE && spline_type != MG_SPLINE_FITTED_BSPLINE) {
        mg_set_error("mg_trajectory_create_typed: unknown spline type %d (0 Catmull-Rom, 1 B-spline, 2 fitted B-spline)", spline_type);
        return MG_ERR_INVALID_ARGUMENT;
    }
    if (!p || !cp || !out || n_points < 4 || granularity < 2 || p->D < 3) {
        mg_set_error("mg_trajectory_create_typed: needs a primitive with root channels, >= 4 control points (x, y, z) for a %s and a granularity >= 2",
                     spline_type == MG_SPLINE_BSPLINE ? "B-spline" : "fitted B-spline");
        return MG_ERR_INVALID_ARGUMENT;
    }
    *out = nullptr;
    for (int i = 0; i < 3 * n_points; i++)
        if (!std::isfinite(cp[i])) { mg_set_error("mg_trajectory_create_typed: control point %d is not finite", i / 3); return MG_ERR_INVALID_ARGUMENT; }
    MG_HIP_CHECK(hipSetDevice(p->ctx->device));
    const int n_seg = spline_type == MG_SPLINE_BSPLINE ? n_points - 3 : n_points - 1;
    std::vector<double> poly((size_t)n_seg * 12 + 3);
    if (spline_type == MG_SPLINE_BSPLINE) mg_traj_poly_bspline(cp, n_seg, poly);
    else mg_traj_poly_fitted(cp, n_points, poly);
    // (b_spline.py:134-137: u >= 1 is points[-1]; the fitted spline interpolates its last point)
    for (int d = 0; d < 3; d++) poly[(size_t)n_seg * 12 + d] = cp[(size_t)(n_points - 1) * 3 + d];
    return mg_traj_finish(p, poly, n_seg, granularity, spline_type, out);
}

extern "C" int32_t mg_trajectory_spline_type(const mg_trajectory *t) { return t ? t->spline_type : -1; }

// The two tables as the kernels read them, for tests and tools: poly_host (n_seg * 12 + 3) and arc_host (granularity + 1) are filled
// when not NULL; n_seg, granularity and full_arc_length are reported when not NULL.
extern "C" int mg_trajectory_tables(const mg_trajectory *t, double *poly_host, double *arc_host, int32_t *n_seg, int32_t *granularity, double *full_arc_length) {
    if (!t) { mg_set_error("mg_trajectory_tables: NULL trajectory"); return MG_ERR_INVALID_ARGUMENT; }
    if (n_seg) *n_seg = t->n_seg;
    if (granularity) *granularity = t->granularity;
    if (full_arc_length) *full_arc_length = t->full_arc;
    if (poly_host || arc_host) MG_HIP_CHECK(hipSetDevice(t->prim->ctx->device));
    if (poly_host) MG_HIP_CHECK(hipMemcpy(poly_host, t->d_poly, ((size_t)t->n_seg * 12 + 3) * sizeof(double), hipMemcpyDeviceToHost));
    if (arc_host) MG_HIP_CHECK(hipMemcpy(arc_host, t->d_arc, ((size_t)t->granularity + 1) * sizeof(double), hipMemcpyDeviceToHost));
    return MG_OK;
}

// arguments of one scorer, validated (who: the entry point's name for the message)
static int mg_traj_fill_args(const char *who, mg_primitive *p, const mg_trajectory *t, const mg_time_grid *g, const void *lat, int dt, int64_t B,
                             int64_t ld, double min_u, double weight, const mg_alignment_desc *al, double *errors_dev,
                             int accumulate, double *residuals_dev, mg_traj_args *out) {
    if (!p || !t || t->prim != p || B < 0 || (dt != MG_F32 && dt != MG_F64) || ld < p->L || !(min_u >= 0.0 && min_u <= 1.0) ||
        !std::isfinite(weight)) {
        mg_set_error("%s: bad arguments (trajectory of another primitive, ld < n_components, min_u outside [0, 1] ...)", who);
        return MG_ERR_INVALID_ARGUMENT;
    }
    if (!g) g = p->canonical;
    if (g->prim != p) { mg_set_error("%s: grid belongs to another primitive", who); return MG_ERR_INVALID_ARGUMENT; }
    if (B > 0 && (!lat || !errors_dev)) { mg_set_error("%s: NULL pointer", who); return MG_ERR_INVALID_ARGUMENT; }
    mg_traj_args a;
    a.poly = t->d_poly; a.E = t->d_E; a.mean = t->d_mean; a.lat = lat; a.i0 = g->d_i0; a.w = g->d_w; a.out = errors_dev; a.res = residuals_dev;
    a.B = B; a.ld = ld; a.T = g->T; a.L = p->L; a.NB = p->NB; a.n_seg = t->n_seg; a.G = t->granularity; a.lat_f64 = dt == MG_F64 ? 1 : 0;
    a.accumulate = accumulate ? 1 : 0; a.min_u = min_u; a.weight = weight; a.points = nullptr; a.res_u = nullptr; a.res_n = nullptr; a.paths = nullptr;
    a.search = p->ctx->opt[MG_OPT_TRAJECTORY_SEARCH] == 1 ? 1 : 0;
    a.al_cand = nullptr;
    { const int rc = mg_traj_align_record(who, al, &a.align_mode, a.al); if (rc != MG_OK) return rc; }   // (mg_tree_plan.h)
    *out = a;
    return MG_OK;
}

// (a property of kernel AND device: once per context, not per process -- ADVICE r3)
static hipError_t mg_traj_lds_opt_in(mg_context *ctx) {
    return mg_lds_opt_in_once(ctx, MG_LDS_TRAJECTORY, 160 * 1024, mg_trajectory_kernel<false>, mg_trajectory_kernel<true>);
}

// the launch of one scorer by its plan (the multi kernels are launched by mg_score_trajectories itself)
static void mg_traj_launch(mg_context *ctx, const mg_traj_plan_t &pl, const mg_traj_args &a) {
    const dim3 grid((unsigned)((a.B + pl.cands - 1) / pl.cands)), block(MG_TRAJ_BLOCK);
    switch (pl.kernel) {
    case MG_TRAJ_KERNEL_COOP8: hipLaunchKernelGGL(mg_trajectory_coop_kernel<8>, grid, block, pl.lds_bytes, ctx->stream, a); break;
    case MG_TRAJ_KERNEL_COOP4: hipLaunchKernelGGL(mg_trajectory_coop_kernel<4>, grid, block, pl.lds_bytes, ctx->stream, a); break;
    case MG_TRAJ_KERNEL_STREAM: hipLaunchKernelGGL(mg_trajectory_stream_kernel, grid, block, pl.lds_bytes, ctx->stream, a); break;
    case MG_TRAJ_KERNEL_STAGED_LDS: hipLaunchKernelGGL(mg_trajectory_kernel<true>, grid, block, pl.lds_bytes, ctx->stream, a); break;
    default: hipLaunchKernelGGL(mg_trajectory_kernel<false>, grid, block, pl.lds_bytes, ctx->stream, a); break;
    }
}

// one scorer's launch, for the two entry points below: al_cand NULL (the record's values for every candidate) or (B, 4)
static int mg_traj_score_one(const char *who, mg_primitive *p, const mg_trajectory *t, const mg_time_grid *g, const void *lat, int dt, int64_t B, int64_t ld,
                             double min_u, double weight, const mg_alignment_desc *al, const double *al_cand, double *errors_dev, int accumulate,
                             double *residuals_dev) {
    mg_traj_args a;
    { const int rc = mg_traj_fill_args(who, p, t, g, lat, dt, B, ld, min_u, weight, al, errors_dev, accumulate, residuals_dev, &a); if (rc != MG_OK) return rc; }
    if (B == 0) return MG_OK;
    a.al_cand = al_cand;
    MG_HIP_CHECK(hipSetDevice(p->ctx->device));
    mg_traj_plan_t pl;
    { const int rc = mg_traj_plan(p->ctx, p->L, t->rows, t->n_seg, B, B, false, a.search, &pl); if (rc != MG_OK) return rc; }
    MG_HIP_CHECK(mg_traj_lds_opt_in(p->ctx));
    if (pl.needs_paths) { const int rcp = mg_traj_paths(p->ctx, (size_t)B * a.T * 24, &a.paths); if (rcp != MG_OK) return rcp; }
    mg_prof_begin(p->ctx, MG_PROF_TRAJECTORY);
    mg_traj_launch(p->ctx, pl, a);
    mg_prof_end(p->ctx, MG_PROF_TRAJECTORY);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

extern "C" int mg_score_trajectory(mg_primitive *p, const mg_trajectory *t, const mg_time_grid *g, const void *lat, int dt, int64_t B,
                                   int64_t ld, double min_u, double weight, const mg_alignment_desc *al, double *errors_dev,
                                   int accumulate, double *residuals_dev) {
    return mg_traj_score_one("mg_score_trajectory", p, t, g, lat, dt, B, ld, min_u, weight, al, nullptr, errors_dev, accumulate, residuals_dev);
}

// The same scorer with EVERY candidate aligned to its own previous motion (a step of a graph walk chained on the step before it):
// align_cand_dev (B, 4) = previous unit heading (x, z) and previous root position (x, z) per candidate, used as they are in place of
// the record's; the record states the aligning node (the root) and the reference vector.  The plan, the kernel and the launch are
// mg_score_trajectory's for the same shape.
extern "C" int mg_score_trajectory_chained(mg_primitive *p, const mg_trajectory *t, const mg_time_grid *g, const void *lat, int dt, int64_t B,
                                           int64_t ld, double min_u, double weight, const mg_alignment_desc *al, const double *align_cand_dev,
                                           double *errors_dev, int accumulate, double *residuals_dev) {
    if (!al) { mg_set_error("mg_score_trajectory_chained: NULL alignment record (its node and reference vector; the values are per candidate)"); return MG_ERR_INVALID_ARGUMENT; }
    if (al->joint == MG_ALIGN_START_POSE) {
        mg_set_error("mg_score_trajectory_chained: the record must be a previous-frame alignment, not a start pose");
        return MG_ERR_INVALID_ARGUMENT;
    }
    if (B > 0 && !align_cand_dev) { mg_set_error("mg_score_trajectory_chained: NULL pointer"); return MG_ERR_INVALID_ARGUMENT; }
    return mg_traj_score_one("mg_score_trajectory_chained", p, t, g, lat, dt, B, ld, min_u, weight, al, align_cand_dev, errors_dev, accumulate, residuals_dev);
}

// n scorers of the same batch size side by side in one launch (canonical grids, no residual vectors): option k's candidates
// lat_dev[k] (B, ld[k]) against trajectories[k], errors_dev[k] written or added to.  alignments: NULL, or n records of which any may be
// NULL.  Where the eight-lane walk does not apply (more than 65 536 candidates, MG_OPT_TRAJECTORY_LANES 1, rows that do not fit) the
// scorers are launched one after the other -- the same results either way.
extern "C" int mg_score_trajectories(int32_t n, mg_primitive *const *prims, const mg_trajectory *const *trajectories, const void *const *lat_dev, int dt,
                                     int64_t B, const int64_t *ld, const double *min_u, const double *weight, const mg_alignment_desc *const *alignments,
                                     double *const *errors_dev, int accumulate) {
    if (n < 0 || (n > 0 && (!prims || !trajectories || !lat_dev || !ld || !min_u || !weight || !errors_dev))) {
        mg_set_error("mg_score_trajectories: bad arguments");
        return MG_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return MG_OK;
    for (int k = 0; k < n; k++)
        if (!prims[k] || prims[k]->ctx != prims[0]->ctx) { mg_set_error("mg_score_trajectories: the primitives must share one context"); return MG_ERR_INVALID_ARGUMENT; }
    mg_context *ctx = prims[0]->ctx;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    const int search = ctx->opt[MG_OPT_TRAJECTORY_SEARCH] == 1 ? 1 : 0;
    bool together = B > 0 && n > 1;
    size_t lds = 0;
    mg_traj_plan_t pl = {};
    for (int k = 0; k < n && together; k++) {
        if (!trajectories[k]) { mg_set_error("mg_score_trajectories: trajectory %d is NULL", k); return MG_ERR_INVALID_ARGUMENT; }
        // (a scorer that fits no kernel at all is reported by its own single launch below, after the scorers before it have run)
        if (mg_traj_plan(ctx, prims[k]->L, trajectories[k]->rows, trajectories[k]->n_seg, B, (int64_t)n * B, false, search, &pl) != MG_OK || !pl.together) together = false;
        else lds = std::max(lds, pl.lds_bytes);
    }
    if (!together) {
        for (int k = 0; k < n; k++) {
            const int rc = mg_score_trajectory(prims[k], trajectories[k], nullptr, lat_dev[k], dt, B, ld[k], min_u[k], weight[k], alignments ? alignments[k] : nullptr,
                                               errors_dev[k], accumulate, nullptr);
            if (rc != MG_OK) return rc;
        }
        return MG_OK;
    }
    const int per = (int)((B + pl.cands - 1) / pl.cands);      // (the scorers share B, the options and with them lanes and form)
    for (int k0 = 0; k0 < n; k0 += MG_TRAJ_MULTI_MAX) {
        mg_traj_multi m;
        memset(&m, 0, sizeof(m));
        m.n = std::min(MG_TRAJ_MULTI_MAX, n - k0);
        for (int i = 0; i < m.n; i++) {
            const int k = k0 + i;
            const int rc = mg_traj_fill_args("mg_score_trajectories", prims[k], trajectories[k], nullptr, lat_dev[k], dt, B, ld[k], min_u[k], weight[k],
                                             alignments ? alignments[k] : nullptr, errors_dev[k], accumulate, nullptr, &m.a[i]);
            if (rc != MG_OK) return rc;
            m.wg0[i + 1] = m.wg0[i] + per;
        }
        if (pl.needs_paths) {      // the streaming kernels' root paths: one block of the context's buffer per scorer
            size_t off = 0;
            double *base = nullptr;
            for (int i = 0; i < m.n; i++) off += (size_t)B * m.a[i].T * 3;
            const int rcp = mg_traj_paths(ctx, off * 8, &base);
            if (rcp != MG_OK) return rcp;
            off = 0;
            for (int i = 0; i < m.n; i++) { m.a[i].paths = base + off; off += (size_t)B * m.a[i].T * 3; }
        }
        mg_prof_begin(ctx, MG_PROF_TRAJECTORY);
        if (pl.kernel == MG_TRAJ_KERNEL_COOP8_MULTI) hipLaunchKernelGGL(mg_trajectory_coop_multi_kernel<8>, dim3((unsigned)m.wg0[m.n]), dim3(MG_TRAJ_COOP_BLOCK), lds, ctx->stream, m);
        else if (pl.kernel == MG_TRAJ_KERNEL_COOP4_MULTI) hipLaunchKernelGGL(mg_trajectory_coop_multi_kernel<4>, dim3((unsigned)m.wg0[m.n]), dim3(MG_TRAJ_COOP_BLOCK), lds, ctx->stream, m);
        else hipLaunchKernelGGL(mg_trajectory_stream_multi_kernel, dim3((unsigned)m.wg0[m.n]), dim3(MG_TRAJ_BLOCK), lds, ctx->stream, m);
        mg_prof_end(ctx, MG_PROF_TRAJECTORY);
        MG_HIP_CHECK(hipGetLastError());
    }
    return MG_OK;
}

// The same search for positions the caller supplies: points_dev (B, T, 3) float64 (e.g. one joint's track from mg_joint_positions,
// aligned by the caller) -- TrajectoryConstraint for joints other than the root (trajectory_constraint.py:95-121 with
// skeleton.nodes[joint].get_global_position(frame)).
static int mg_traj_points_launch(const char *who, mg_primitive *p, const mg_trajectory *t, const double *points_dev, int64_t B, int32_t T, double min_u,
                                 double weight, double *errors_dev, int accumulate, double *residuals_dev, double *params_dev, int32_t *evals_dev = nullptr) {
    if (!p || !t || t->prim != p || B < 0 || T < 1 || !(min_u >= 0.0 && min_u <= 1.0) || !std::isfinite(weight)) {
        mg_set_error("%s: bad arguments", who);
        return MG_ERR_INVALID_ARGUMENT;
    }
    if (B == 0) return MG_OK;
    if (!points_dev || (!errors_dev && !params_dev && !residuals_dev && !evals_dev)) { mg_set_error("%s: NULL pointer", who); return MG_ERR_INVALID_ARGUMENT; }
    MG_HIP_CHECK(hipSetDevice(p->ctx->device));
    mg_traj_args a;
    a.poly = t->d_poly; a.E = t->d_E; a.mean = t->d_mean; a.lat = nullptr; a.i0 = nullptr; a.w = nullptr; a.out = errors_dev; a.res = residuals_dev;
    a.B = B; a.ld = 0; a.T = T; a.L = p->L; a.NB = p->NB; a.n_seg = t->n_seg; a.G = t->granularity; a.lat_f64 = 1;
    a.accumulate = accumulate ? 1 : 0; a.min_u = min_u; a.weight = weight; a.points = points_dev; a.res_u = params_dev; a.res_n = evals_dev; a.paths = nullptr;
    a.search = p->ctx->opt[MG_OPT_TRAJECTORY_SEARCH] == 1 ? 1 : 0;
    a.align_mode = 0; a.al_cand = nullptr;
    for (double &v : a.al) v = 0.0;
    mg_traj_plan_t pl;
    { const int rc = mg_traj_plan(p->ctx, p->L, t->rows, t->n_seg, B, B, true, a.search, &pl); if (rc != MG_OK) return rc; }
    MG_HIP_CHECK(mg_traj_lds_opt_in(p->ctx));
    mg_prof_begin(p->ctx, MG_PROF_TRAJECTORY);
    mg_traj_launch(p->ctx, pl, a);
    mg_prof_end(p->ctx, MG_PROF_TRAJECTORY);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}
extern "C" int mg_score_trajectory_points(mg_primitive *p, const mg_trajectory *t, const double *points_dev, int64_t B, int32_t T, double min_u,
                                          double weight, double *errors_dev, int accumulate, double *residuals_dev) {
    if (B > 0 && !errors_dev) { mg_set_error("mg_score_trajectory_points: NULL pointer"); return MG_ERR_INVALID_ARGUMENT; }
    return mg_traj_points_launch("mg_score_trajectory_points", p, t, points_dev, B, T, min_u, weight, errors_dev, accumulate, residuals_dev, nullptr);
}
// ParameterizedSpline.find_closest_point_fast (splines/parameterized_spline.py:303-322) for a batch of point sequences, chained the way
// TrajectoryConstraint.get_residual_vector chains it (trajectory_constraint.py:103-113: every frame's search is bounded below by, and
// started at, the previous frame's parameter): params_dev (B, T) the parameter of every frame's point, distances_dev (B, T) its
// distance, evaluations_dev (B, T) int32 the (f, g) evaluations the frame's search took -- scipy's nfev / 2; the reference's search
// only -- (any may be NULL).
extern "C" int mg_trajectory_closest_points(mg_primitive *p, const mg_trajectory *t, const double *points_dev, int64_t B, int32_t T, double min_u,
                                            double *params_dev, double *distances_dev, int32_t *evaluations_dev) {
    if (B > 0 && !params_dev && !distances_dev && !evaluations_dev) { mg_set_error("mg_trajectory_closest_points: nothing to write"); return MG_ERR_INVALID_ARGUMENT; }
    return mg_traj_points_launch("mg_trajectory_closest_points", p, t, points_dev, B, T, min_u, 1.0, nullptr, 0, distances_dev, params_dev, evaluations_dev);
}
