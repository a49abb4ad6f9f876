// A population of walks in which every walk has its OWN node sequence (gfx950 / MI355X), float64: the shape of random graph walks
// (MotionStateGraph.generate_random_walk, reference motion_model/motion_state_graph.py:52-71, motion_state_group.py:177-214), where
// mg_walk.hip serves the optimiser's batch -- many walks over one sequence.  The nodes that occur travel as a table of per-node
// records (ctx->tab[MG_TABLE_WALKS_MIXED] / [MG_TABLE_WALKS_SAMPLE] / [MG_TABLE_WALKS_WARPED] / [MG_TABLE_WALKS_TIME], one per entry
// point); what mg_walk_step holds per step -- the latent column, the first tile -- is per (walk, step) here.
//
//   mg_walks_sample_kernel   one lane per (walk, step): the mixture component from one Philox word of the row's own stream, then the
//                            lane-per-row sampler's statement (mg_gmm_sample_row, mg_gmm_device.h) for global row w * s_max + i.
//   mg_walks_chain_kernel    one workgroup per walk, its own n_steps[w] steps in order, the node record fetched through node_of.
//   mg_walks_frames_kernel   grid over all tiles of all walks: the walk by bisection in the per-walk tile prefix (mg_item_at's
//                            search), the step by bisection in the walk's per-step tile starts.
//
//   mg_walks_time_kernel     one wave per (walk, step): the step's time row -- mg_timewarp_kernel's statements on the time latents of
//                            the step's own row for a node with a time model, numpy.linspace(0, F, count) for one without.
//
// The chain and frames kernels restate mg_walk_chain_kernel and mg_walk_frames_kernel statement by statement over the same device
// helpers; mg_walk.hip's text is held line by line by tests/test_walk_shapes_host.py and stays where it is.  WARPED = false is the
// canonical grids (mg_walks_frames), WARPED = true every step at its own time row (mg_walks_frames_at): the step's length from the
// lengths table, each frame's basis row by the FITPACK recurrence at its own time, the exit pose at the row's last entry.  The
// contract -- a walk's frames and transforms are the bits of mg_walk_frames for that walk alone -- is tests/test_gpu_random_walks.py's
// and tests/test_gpu_random_walks_warped.py's.
#include <cmath>
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_construct.h"
#include "mg_gmm_device.h"
#include "mg_items_cut.h"
#include "mg_joint_plan.h"
#include "mg_score_device.h"
#include "mg_spline_device.h"
#include "mg_timewarp_device.h"

#define MG_WALKS_TILE 32         // frames per workgroup of the frames kernel: mg_walk.hip's MG_WALK_TILE
#define MG_WALKS_BLOCK 256
#define MG_WALKS_CHAIN_BLOCK 64
#define MG_WALKS_SAMPLE_BLOCK 64
#define MG_WALKS_LDS_MAX (160 * 1024 - 64)
#define MG_WALKS_SAMPLE_LDS_MAX (150 * 1024)

struct mg_walks_node {            // one node's constants on the device (56 bytes): mg_walk_step without lat_off / tile0
    const double *Et64, *mean, *knots;
    const int32_t *i0;            // the canonical grid's tables
    const double *w;
    int32_t L, R, NB, T;          // T: samples of the canonical grid
};

struct mg_walks_time_node {       // what a node's time row is made of (32 bytes)
    const double *tphi, *tmean;   // [F][Lt], [F]; NULL for a node without a time model
    int32_t F, Lt, L;             // canonical frames; time latents, in columns L .. L + Lt of a step's row
    int32_t count;                // Lt == 0: samples of numpy.linspace(0, F, count)
};

struct mg_walks_mixture {         // one node's mixture on the device (32 bytes)
    const double *chol, *mean;    // [K][Lg][Lg] lower, [K][Lg]
    int64_t cum_at;               // bytes from the table's base to cum[K]: the cumulative weights, float64, added in ascending order
    int32_t K, Lg;
};

struct mg_walks_args {
    const mg_walks_node *nodes;
    const int32_t *node_of;       // (n_walks, s_max)
    const int32_t *n_steps;       // (n_walks)
    const int32_t *walk_tile;     // (n_walks + 1): the first tile of every walk
    const int32_t *step_tile;     // (n_walks, s_max): the first tile of a step among its walk's tiles
    const int64_t *frame_offset;  // (n_walks, s_max)
    const int32_t *lengths;       // WARPED: (n_walks, s_max), the samples of every step's time row
    const double *times;          // WARPED: (n_walks, s_max, t_cap)
    const void *lat;              // (n_walks, s_max, ld)
    double *xf;                   // (n_walks, s_max, 8): c, s, tx, tz, ty, cos(phi / 2), sin(phi / 2), 1 if the step is aligned
    double *transforms;           // NULL or (n_walks, s_max, 4)
    double *frames;
    int64_t n_walks, ld, walk_stride;
    int32_t s_max, D, t_cap;
    int32_t lmax, rmax;           // the longest latent row and the most control-point rows of a node: LDS pitches
    int32_t align_mode;           // first step: 0 as it is, 1 previous frame, 2 start pose
    int32_t n_link;               // animated joints along the aligning node's chain
    double h0, h1, px, py, pz, ref[3];
    int32_t link[MG_MAX_CHAIN];   // their quaternion channels, root first
};

struct mg_walks_sample_args {
    const mg_walks_mixture *mix;
    const int32_t *node_of, *n_steps;
    void *x;
    int32_t *comp;
    int64_t rows, ld;             // rows = n_walks * s_max
    uint64_t seed;
    int32_t s_max, lgmax;
};

// The component of row r: one Philox4x32-10 word, key (seed low, seed high), counter (r low, r high, 0, 1) -- the normals of the row
// use counters (r low, r high, column group, 0) -- then u = (word + 0.5) 2^-32 and the first c with u < cum[c]; the last
// component takes what is left.
__device__ __forceinline__ int mg_walks_component(int64_t r, uint64_t seed, const double *cum, int K) {
    uint32_t word[4];
    mg_philox4x32_10((uint32_t)r, (uint32_t)(r >> 32), 0u, 1u, (uint32_t)seed, (uint32_t)(seed >> 32), word);
    const double u = ((double)word[0] + 0.5) * (1.0 / 4294967296.0);
    int c = 0;
    while (c + 1 < K && !(u < cum[c])) c++;
    return c;
}

template <bool X_F64>
__global__ __launch_bounds__(MG_WALKS_SAMPLE_BLOCK) void mg_walks_sample_kernel(const mg_walks_sample_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *z = (double *)smem + (size_t)threadIdx.x * (a.lgmax + 1);   // [MG_WALKS_SAMPLE_BLOCK][lgmax + 1]
    const int64_t r = (int64_t)blockIdx.x * MG_WALKS_SAMPLE_BLOCK + threadIdx.x;
    if (r >= a.rows) return;
    const int64_t wk = r / a.s_max;
    const int i = (int)(r - wk * a.s_max);
    auto store = [&](int64_t col, double v) {
        if (X_F64) ((double *)a.x)[r * a.ld + col] = v;
        else ((float *)a.x)[r * a.ld + col] = (float)v;
    };
    int c = -1, width = 0;
    if (i < a.n_steps[wk]) {
        const mg_walks_mixture m = a.mix[a.node_of[r]];
        c = mg_walks_component(r, a.seed, (const double *)((const char *)a.mix + m.cum_at), m.K);
        width = m.Lg;
        mg_gmm_sample_row(r, a.seed, width, z, m.chol + (size_t)c * width * width, m.mean + (size_t)c * width, store);
    }
    for (int64_t col = width; col < a.ld; col++) store(col, 0.0);
    if (a.comp) a.comp[r] = c;
}

struct mg_walks_time_args {
    const mg_walks_time_node *nodes;
    const int32_t *node_of, *n_steps;
    const void *lat;              // (n_walks, s_max, ld)
    double *times;                // (n_walks, s_max, t_cap)
    int32_t *lens;                // (n_walks, s_max)
    int64_t ld;
    double inv_speed;
    int32_t s_max, t_cap;
    const uint8_t *smooth;        // SMOOTH: one byte per node, other than 0: the node's rows go through the Savitzky-Golay pass
    const double *H;              // SMOOTH: its hat matrix (mg_savgol_table.h)
};

// Row (w, i) of a node with a time model: mg_timewarp_kernel (mg_timewarp.hip) statement by statement, gamma read from the step's own
// latent row.  Of a node without one: numpy.linspace(0, F, count) = arange(count) * (F / (count - 1)), the last one F itself.
// SMOOTH (mg_walks_time_functions_smoothed): as mg_timewarp_kernel<true> for the nodes a.smooth marks, the window behind dp.
template <bool LAT_F64, bool SMOOTH>
__global__ __launch_bounds__(MG_TW_BLOCK) void mg_walks_time_kernel(const mg_walks_time_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t ws = blockIdx.x, wk = ws / a.s_max;
    const int tid = threadIdx.x;
    if ((int)(ws - wk * a.s_max) >= a.n_steps[wk]) {   // a step the walk does not have: length 0, nothing else written
        if (tid == 0) a.lens[ws] = 0;
        return;
    }
    const mg_walks_time_node nd = a.nodes[a.node_of[ws]];
    const int F = nd.F;
    double *tb = a.times + ws * (int64_t)a.t_cap;
    if (nd.Lt == 0) {
        const int T = nd.count;
        if (tid == 0) a.lens[ws] = T <= a.t_cap ? T : -T;
        if (T > a.t_cap) return;
        const double step = T > 1 ? (double)F / (double)(T - 1) : 0.0;
        for (int j = tid; j < T; j += MG_TW_BLOCK) tb[j] = (j == T - 1 && T > 1) ? (double)F : (double)j * step;
        return;
    }
    double *x = (double *)smem;      // [F] the canonical time function t(t'): the spline's abscissae; ordinates are 0 .. F-1
    double *M = x + F;               // [F] second derivatives
    double *cp = M + F;              // [F] Thomas: modified upper diagonal
    double *dp = cp + F;             // [F] Thomas: modified right-hand side
    const int64_t g0 = ws * a.ld + nd.L;
    for (int i = tid; i < F; i += MG_TW_BLOCK)   // the increments (parked in M)
        M[i] = mg_tw_increment(nd.tphi, nd.tmean, i, nd.Lt, [&](int l) { return mg_load_lat<LAT_F64>(a.lat, g0 + l); });
    __syncthreads();
    if (tid == 0) {
        mg_tw_running_sum(M, x, F);
        mg_tw_second_derivatives(x, M, cp, dp, F, 1);
    }
    __syncthreads();
    // the samples: 0, the inverse spline at linspace(1, x[F-2], num), F - 1
    const double stop = x[F - 2];
    int num;
    if (!mg_tw_sample_count(stop, a.inv_speed, num)) {   // no row: length 0, nothing written
        if (tid == 0) a.lens[ws] = 0;
        return;
    }
    const int T = num + 2;
    if (tid == 0) a.lens[ws] = T <= a.t_cap ? T : -T;   // (negative: the caller's rows are too short; nothing else is written)
    if (T > a.t_cap) return;
    const double step = mg_tw_sample_step(stop, num);
    if (SMOOTH && a.smooth[a.node_of[ws]]) {
        if (T >= MG_TW_SMOOTH_W) mg_tw_smoothed_row(x, M, F, T, num, stop, step, a.H, dp + F, tb, tid);
        return;
    }
    for (int j = tid; j < T; j += MG_TW_BLOCK) {
        double v;
        if (j == 0) v = 0.0;
        else if (j == T - 1) v = (double)(F - 1);
        else {
            const double t = mg_tw_sample_point(j - 1, num, stop, step);
            v = mg_tw_inverse_at(x, M, mg_tw_interval(x, F, t), t);
        }
        tb[j] = v;
    }
}

template <bool LAT_F64, bool WARPED>
__global__ __launch_bounds__(MG_WALKS_CHAIN_BLOCK) void mg_walks_chain_kernel(const mg_walks_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nch = 3 + 4 * a.n_link;
    double *s = (double *)smem;            // [lmax]
    double *cpv = s + a.lmax;              // [5][nch]: the first control point, then the last sample's four taps
    double *wl = cpv + 5 * nch;            // [4] the last sample's weights
    int *i0l = (int *)(wl + 4);            // its first tap
    const int64_t wk = blockIdx.x;
    const int tid = threadIdx.x, D = a.D;
    const int ns = a.n_steps[wk];
    double hx = a.h0, hz = a.h1, tpx = a.px, tpz = a.pz;   // what the step is aligned to (lane 0)
    for (int i = 0; i < ns; i++) {
        const int64_t ws = wk * a.s_max + i;
        const mg_walks_node st = a.nodes[a.node_of[ws]];
        for (int k = tid; k < st.L; k += MG_WALKS_CHAIN_BLOCK) s[k] = mg_load_lat<LAT_F64>(a.lat, ws * a.ld + k);
        if (tid == 0) {
            if (WARPED) {              // the exit pose follows the step's time row: its last entry
                mg_basis_row_dev(st.knots, st.NB + 4, a.times[ws * a.t_cap + a.lengths[ws] - 1], i0l, wl);
            } else {
                *i0l = st.i0[st.T - 1];
                for (int j = 0; j < 4; j++) wl[j] = st.w[4 * (size_t)(st.T - 1) + j];
            }
        }
        __syncthreads();
        const int il = *i0l;
        for (int e = tid; e < 5 * nch; e += MG_WALKS_CHAIN_BLOCK) {
            const int j = e / nch, q = e - j * nch;
            const int ch = q < 3 ? q : a.link[(q - 3) >> 2] + ((q - 3) & 3);
            const int r = (j == 0 ? 0 : il + j - 1) * D + ch;
            cpv[e] = mg_control_point(st.mean[r], st.Et64 + r, (size_t)st.R, st.L, [&](int k) { return s[k]; });
        }
        __syncthreads();
        if (tid == 0) {
            auto last = [&](int q) { return mg_taps4(wl, cpv + nch + q, nch); };   // the last sample's channel
            // heading of the aligning node: its global orientation applied to ref_dir, xz, unit.  turn: the root's quaternion
            // carries the step's rotation already (the aligned exit pose)
            auto heading = [&](bool at_last, bool turn, double qaw, double qay, double &ox, double &oz) {
                double q4[4] = {1.0, 0.0, 0.0, 0.0};
                for (int l = 0; l < a.n_link; l++) {
                    const int q = 3 + 4 * l;
                    double qw = at_last ? last(q) : cpv[q], qx = at_last ? last(q + 1) : cpv[q + 1];
                    double qy = at_last ? last(q + 2) : cpv[q + 2], qz = at_last ? last(q + 3) : cpv[q + 3];
                    if (turn && a.link[l] == 3) mg_align_root_quat(qaw, qay, qw, qx, qy, qz);
                    mg_quat_accumulate(q4, qw, qx, qy, qz);
                }
                mg_heading_xz(q4, a.ref[0], a.ref[1], a.ref[2], ox, oz);
            };
            const bool aligned = i > 0 || a.align_mode != 0;
            mg_align2d t = {1.0, 0.0, 0.0, 0.0, 0.0};
            double qaw = 1.0, qay = 0.0;
            if (aligned) {
                const double p0x = cpv[0], p0z = cpv[2];   // the first control point: a clamped spline's value at t = 0
                if (i == 0 && a.align_mode == 2) {
                    t = mg_align2d_onto(a.h0, a.h1, tpx, tpz, p0x, p0z, a.py);
                } else {
                    double bx, bz;
                    heading(false, false, 1.0, 0.0, bx, bz);
                    t = mg_align2d_from(hx, hz, bx, bz, tpx, tpz, p0x, p0z);
                }
                mg_align_half_angle(t.c, t.s, qaw, qay);
            }
            double *xf = a.xf + ws * 8;
            xf[0] = t.c; xf[1] = t.s; xf[2] = t.tx; xf[3] = t.tz; xf[4] = t.ty; xf[5] = qaw; xf[6] = qay; xf[7] = aligned ? 1.0 : 0.0;
            if (a.transforms) { double *tr = a.transforms + ws * 4; tr[0] = t.c; tr[1] = t.s; tr[2] = t.tx; tr[3] = t.tz; }
            if (i + 1 < ns) {              // the aligned last sample: what the next step is aligned to
                double y = 0.0;            // (its height is not needed)
                tpx = last(0); tpz = last(2);
                if (aligned) mg_align_position(t, tpx, y, tpz);
                heading(true, aligned, qaw, qay, hx, hz);
            }
        }
        __syncthreads();
    }
}

// the last entry of starts[0 .. n) that is not past `at` (starts rise; starts[0] <= at)
__device__ __forceinline__ int mg_walks_last_not_past(const int32_t *starts, int n, int at) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= at) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <bool LAT_F64, bool WARPED>
__global__ __launch_bounds__(MG_WALKS_BLOCK) void mg_walks_frames_kernel(const mg_walks_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *cp = (double *)smem;                    // [rows of the tile's window][D], at most rmax doubles
    double *s = cp + a.rmax;                        // [lmax]
    double *wt = s + a.lmax;                        // [MG_WALKS_TILE][4]
    int *i0t = (int *)(wt + MG_WALKS_TILE * 4);     // [MG_WALKS_TILE]
    const int64_t wk = mg_walks_last_not_past(a.walk_tile, (int)a.n_walks, (int)blockIdx.x);
    const int kt = (int)blockIdx.x - a.walk_tile[wk];
    const int i = mg_walks_last_not_past(a.step_tile + wk * a.s_max, a.n_steps[wk], kt);
    const int64_t ws = wk * a.s_max + i;
    const mg_walks_node st = a.nodes[a.node_of[ws]];
    const int len = WARPED ? a.lengths[ws] : st.T;
    const int f0 = (kt - a.step_tile[ws]) * MG_WALKS_TILE;
    if (f0 >= len) return;
    const int nf = len - f0 < MG_WALKS_TILE ? len - f0 : MG_WALKS_TILE;
    const int tid = threadIdx.x, D = a.D;
    if (tid < nf) {
        if (WARPED) {
            mg_basis_row_dev(st.knots, st.NB + 4, a.times[ws * a.t_cap + f0 + tid], &i0t[tid], &wt[4 * tid]);
        } else {
            i0t[tid] = st.i0[f0 + tid];
            for (int j = 0; j < 4; j++) wt[4 * tid + j] = st.w[4 * (size_t)(f0 + tid) + j];
        }
    }
    for (int k = tid; k < st.L; k += MG_WALKS_BLOCK) s[k] = mg_load_lat<LAT_F64>(a.lat, ws * a.ld + k);
    __syncthreads();
    int imin = i0t[0], imax = i0t[0];
    for (int f = 1; f < nf; f++) { const int v = i0t[f]; imin = v < imin ? v : imin; imax = v > imax ? v : imax; }
    const int rows = (imax + 4 - imin) * D, r0 = imin * D;
    for (int e = tid; e < rows; e += MG_WALKS_BLOCK) {   // control points: fma chain over k ascending from the mean
        const int r = r0 + e;
        cp[e] = mg_control_point(st.mean[r], st.Et64 + r, (size_t)st.R, st.L, [&](int k) { return s[k]; });
    }
    __syncthreads();
    const double *xf = a.xf + ws * 8;
    const double c = xf[0], sn = xf[1], tx = xf[2], tz = xf[3], ty = xf[4], qaw = xf[5], qay = xf[6];
    const bool aligned = xf[7] != 0.0;
    auto value = [&](int e) {
        const int f = e / D, d = e - f * D;
        const double *cf = cp + (size_t)(i0t[f] - imin) * D, *wf = wt + 4 * f;
        auto chan = [&](int ch) { return mg_taps4(wf, cf + ch, D); };
        const double v = chan(d);
        if (!aligned || d >= 7) return v;
        // mg_align_position's and mg_align_root_quat's statements, one channel at a time (mg_walk_frames_kernel)
        switch (d) {
        case 0: return c * v + sn * chan(2) + tx;
        case 1: return v + ty;
        case 2: return c * v - sn * chan(0) + tz;
        case 3: return qaw * v - qay * chan(5);
        case 4: return qaw * v + qay * chan(6);
        case 5: return qaw * v + qay * chan(3);
        default: return qaw * v - qay * chan(4);
        }
    };
    // the tile's rows are one run of nf * D doubles; a lane owns a 16-byte aligned pair of them, the run's ends a single one
    double *dst = a.frames + ((wk * a.walk_stride + a.frame_offset[ws] + f0) * (int64_t)D);
    const int n = nf * D, odd = (int)(((uintptr_t)dst >> 3) & 1);
    const int npairs = (n + odd + 1) >> 1;
    for (int p = tid; p < npairs; p += MG_WALKS_BLOCK) {
        const int e0 = 2 * p - odd, e1 = e0 + 1;
        if (e0 >= 0 && e1 < n) {
            double2 v;
            v.x = value(e0);
            v.y = value(e1);
            *(double2 *)(dst + e0) = v;
        } else if (e0 >= 0) {
            dst[e0] = value(e0);
        } else if (e1 < n) {
            dst[e1] = value(e1);
        }
    }
}

#define MG_WALKS_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)

// The tables both entry points share: nodes of one context and one n_dim, node indices inside [0, n_nodes), 1 <= n_steps[w] <= s_max.
// occurs[k]: node k is some walk's step.
static int mg_walks_check_tables(const char *who, int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, int64_t n_walks,
                                 int32_t s_max, std::vector<char> &occurs) {
    MG_WALKS_REQUIRE(n_nodes >= 1 && prims && prims[0], "%s: no nodes", who);
    MG_WALKS_REQUIRE(n_walks >= 0 && s_max >= 1, "%s: %lld walks of up to %d steps", who, (long long)n_walks, s_max);
    MG_WALKS_REQUIRE(n_walks == 0 || (node_of && n_steps), "%s: NULL table", who);
    MG_REQUIRE_AS(n_walks * (int64_t)s_max < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED, "%s: %lld walks x %d steps exceed one call (2^31 - 1 steps)", who,
                  (long long)n_walks, s_max);
    for (int k = 0; k < n_nodes; k++) {
        MG_WALKS_REQUIRE(prims[k] != nullptr, "%s: node %d is NULL", who, k);
        MG_WALKS_REQUIRE(prims[k]->ctx == prims[0]->ctx, "%s: node %d belongs to another context", who, k);
        MG_WALKS_REQUIRE(prims[k]->D == prims[0]->D, "%s: node %d has n_dim %d, the first one %d", who, k, prims[k]->D, prims[0]->D);
    }
    occurs.assign((size_t)n_nodes, 0);
    for (int64_t w = 0; w < n_walks; w++) {
        MG_WALKS_REQUIRE(n_steps[w] >= 1 && n_steps[w] <= s_max, "%s: walk %lld has %d steps (1 .. %d)", who, (long long)w, n_steps[w], s_max);
        for (int i = 0; i < n_steps[w]; i++) {
            const int32_t k = node_of[w * s_max + i];
            MG_WALKS_REQUIRE(k >= 0 && k < n_nodes, "%s: walk %lld, step %d names node %d of %d", who, (long long)w, i, k, n_nodes);
            occurs[(size_t)k] = 1;
        }
    }
    return MG_OK;
}

extern "C" int mg_walks_sample_latents(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, int64_t n_walks,
                                       int32_t s_max, uint64_t seed, void *x_dev, int xdt, int64_t ld, int32_t *comp_dev) {
    const char *who = "mg_walks_sample_latents";
    std::vector<char> occurs;
    int rc = mg_walks_check_tables(who, n_nodes, prims, node_of, n_steps, n_walks, s_max, occurs);
    if (rc != MG_OK) return rc;
    MG_WALKS_REQUIRE((xdt == MG_F32 || xdt == MG_F64) && ld >= 1, "%s: bad arguments", who);
    int lgmax = 0;
    for (int k = 0; k < n_nodes; k++) {
        MG_WALKS_REQUIRE(prims[k]->K > 0, "%s: node %d has no mixture", who, k);
        MG_WALKS_REQUIRE(!occurs[(size_t)k] || prims[k]->Lg <= ld, "%s: node %d draws %d columns, ld is %lld", who, k, prims[k]->Lg, (long long)ld);
        lgmax = std::max(lgmax, (int)prims[k]->Lg);
    }
    if (n_walks == 0) return MG_OK;
    MG_WALKS_REQUIRE(x_dev != nullptr, "%s: NULL pointer", who);
    const size_t lds = (size_t)MG_WALKS_SAMPLE_BLOCK * (lgmax + 1) * 8;
    MG_REQUIRE_AS(lds <= MG_WALKS_SAMPLE_LDS_MAX, MG_ERR_UNSUPPORTED, "%s: a mixture of %d dimensions does not fit LDS", who, lgmax);
    mg_context *ctx = prims[0]->ctx;
    // the table: node records, every node's cumulative weights, node_of, n_steps
    const int64_t rows = n_walks * s_max;
    std::vector<unsigned char> tab((size_t)n_nodes * sizeof(mg_walks_mixture));
    std::vector<size_t> cum_at((size_t)n_nodes);
    for (int k = 0; k < n_nodes; k++) {
        std::vector<double> cum((size_t)prims[k]->K);
        double acc = 0.0;
        for (int c = 0; c < prims[k]->K; c++) cum[(size_t)c] = acc = acc + prims[k]->gw[(size_t)c];
        cum_at[(size_t)k] = mg_table_append(tab, cum.data(), cum.size() * 8);
    }
    const size_t off_node = mg_table_append(tab, node_of, (size_t)rows * 4), off_steps = mg_table_append(tab, n_steps, (size_t)n_walks * 4);
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[MG_TABLE_WALKS_SAMPLE];
    for (int k = 0; k < n_nodes; k++) {
        mg_walks_mixture m;
        m.chol = prims[k]->d_gchol; m.mean = prims[k]->d_gmean; m.cum_at = (int64_t)cum_at[(size_t)k];
        m.K = prims[k]->K; m.Lg = prims[k]->Lg;
        memcpy(tab.data() + (size_t)k * sizeof(m), &m, sizeof(m));
    }
    rc = dt.upload(ctx, who, tab.data(), tab.size());
    if (rc != MG_OK) return rc;
    mg_walks_sample_args a;
    a.mix = (const mg_walks_mixture *)dt.base();
    a.node_of = (const int32_t *)(dt.base() + off_node); a.n_steps = (const int32_t *)(dt.base() + off_steps);
    a.x = x_dev; a.comp = comp_dev; a.rows = rows; a.ld = ld; a.seed = seed; a.s_max = s_max; a.lgmax = lgmax;
    if (lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALKS_SAMPLE, 160 * 1024, mg_walks_sample_kernel<true>, mg_walks_sample_kernel<false>));
    const unsigned grid = (unsigned)((rows + MG_WALKS_SAMPLE_BLOCK - 1) / MG_WALKS_SAMPLE_BLOCK);
    if (xdt == MG_F64) hipLaunchKernelGGL(mg_walks_sample_kernel<true>, dim3(grid), dim3(MG_WALKS_SAMPLE_BLOCK), lds, ctx->stream, a);
    else hipLaunchKernelGGL(mg_walks_sample_kernel<false>, dim3(grid), dim3(MG_WALKS_SAMPLE_BLOCK), lds, ctx->stream, a);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

// mg_walks_frames (WARPED = false: times_dev, lengths NULL) and mg_walks_frames_at (WARPED = true), each with a table of its own
template <bool WARPED>
static int mg_walks_frames_launch(const char *who, int table, unsigned lds_bit, int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of,
                                  const int32_t *n_steps, const void *latents_dev, int dtype, int64_t n_walks, int32_t s_max, int64_t ld, const double *times_dev,
                                  const int32_t *lengths, int32_t t_cap, const int64_t *frame_offset, const mg_alignment_desc *al, const mg_skeleton_desc *sk,
                                  double *frames_dev, int64_t walk_stride, double *transforms_dev) {
    std::vector<char> occurs;
    int rc = mg_walks_check_tables(who, n_nodes, prims, node_of, n_steps, n_walks, s_max, occurs);
    if (rc != MG_OK) return rc;
    MG_WALKS_REQUIRE((dtype == MG_F32 || dtype == MG_F64) && ld >= 1 && walk_stride >= 1, "%s: bad arguments", who);
    if (WARPED) {
        MG_WALKS_REQUIRE(t_cap >= 1, "%s: t_cap %d", who, t_cap);
        MG_WALKS_REQUIRE(n_walks == 0 || (times_dev && lengths && frame_offset), "%s: times, lengths and frame offsets are required", who);
    }
    mg_context *ctx = prims[0]->ctx;
    const int D = prims[0]->D;
    int lmax = 0, rmax = 0;
    for (int k = 0; k < n_nodes; k++) {
        const mg_primitive *p = prims[k];
        MG_WALKS_REQUIRE(!occurs[(size_t)k] || p->L <= ld, "%s: node %d reads %d latent columns, ld is %lld", who, k, p->L, (long long)ld);
        lmax = std::max(lmax, (int)p->L);
        rmax = std::max(rmax, (int)p->R);
    }
    bool aligned_any = al != nullptr;
    for (int64_t w = 0; w < n_walks && !aligned_any; w++) aligned_any = n_steps[w] > 1;
    MG_WALKS_REQUIRE(D >= 3 && (!aligned_any || D >= 7), "%s: n_dim %d has no root channels to align", who, D);
    // the aligning node: the record's, or the root and (0, 0, 1) -- mg_walk_frames' rules
    mg_walks_args a = {};
    int joint = 0;
    a.ref[0] = 0.0; a.ref[1] = 0.0; a.ref[2] = 1.0;
    a.h0 = 1.0;
    if (al) {
        const double hn = std::sqrt(al->heading[0] * al->heading[0] + al->heading[1] * al->heading[1]);
        MG_WALKS_REQUIRE(hn > 0.0 && std::isfinite(hn), "%s: heading is zero or not finite", who);
        a.h0 = al->heading[0] / hn; a.h1 = al->heading[1] / hn;
        a.px = al->position[0]; a.py = al->position[1]; a.pz = al->position[2];
        if (al->joint == MG_ALIGN_START_POSE) {
            a.align_mode = 2;    // (a start pose names no node: later steps go through the root and (0, 0, 1))
        } else {
            a.align_mode = 1;
            joint = al->joint;
            for (int e = 0; e < 3; e++) a.ref[e] = al->ref_dir[e];
            MG_WALKS_REQUIRE(a.ref[0] * a.ref[0] + a.ref[2] * a.ref[2] > 0.0, "%s: ref_dir has no xz part", who);
        }
    }
    if (!aligned_any) {
        a.n_link = 0;            // nothing is aligned: no heading is formed, the chain kernel reads the root translation only
    } else if (joint == 0 && !sk) {
        a.n_link = 1; a.link[0] = 3;
    } else {
        MG_WALKS_REQUIRE(sk != nullptr, "%s: aligning joint %d is not the root: a skeleton is needed", who, joint);
        MG_WALKS_REQUIRE(mg_skeleton_complete(sk, false) && joint >= 0 && joint < sk->n_joints, "%s: incomplete skeleton or aligning joint %d out of range", who,
                         joint);
        std::vector<int32_t> quats;
        const mg_plan_failure f = mg_aligning_quaternions(sk, joint, D, quats);
        MG_WALKS_REQUIRE(!f.of_skeleton(), "%s: joint %d%s", who, f.joint, mg_chain_why(f.kind));
        MG_WALKS_REQUIRE(!f, "%s: the aligning chain does not fit (channel %d, n_dim %d)", who, f.channel, D);
        a.n_link = (int32_t)quats.size();
        std::copy(quats.begin(), quats.end(), a.link);
    }
    // offsets and tiles: every step inside its walk's rows, no two steps on the same row
    const int64_t nws = n_walks * s_max;
    std::vector<int64_t> offs((size_t)nws, 0);
    std::vector<int32_t> step_tile((size_t)nws, 0), walk_tile((size_t)n_walks + 1, 0);
    std::vector<std::pair<int64_t, int64_t>> spans;
    int64_t tiles = 0;
    for (int64_t w = 0; w < n_walks; w++) {
        int64_t next = 0, walk_tiles = 0;
        spans.clear();
        for (int i = 0; i < n_steps[w]; i++) {
            const int64_t ws = w * s_max + i, len = WARPED ? lengths[ws] : prims[node_of[ws]]->canonical->T;
            MG_WALKS_REQUIRE(!WARPED || (len >= 1 && len <= t_cap), "%s: walk %lld, step %d has %lld samples (1 .. t_cap = %d)", who, (long long)w, i, (long long)len,
                             t_cap);
            const int64_t off = frame_offset ? frame_offset[ws] : next;
            MG_WALKS_REQUIRE(off >= 0, "%s: walk %lld, step %d starts at row %lld", who, (long long)w, i, (long long)off);
            offs[(size_t)ws] = off;
            step_tile[(size_t)ws] = (int32_t)walk_tiles;
            spans.push_back({off, len});
            next = off + len;
            walk_tiles += (len + MG_WALKS_TILE - 1) / MG_WALKS_TILE;
        }
        std::sort(spans.begin(), spans.end());
        int64_t end = 0;
        for (const auto &sp : spans) {
            MG_WALKS_REQUIRE(sp.first >= end, "%s: walk %lld: steps overlap at row %lld", who, (long long)w, (long long)sp.first);
            end = sp.first + sp.second;
        }
        MG_WALKS_REQUIRE(end <= walk_stride, "%s: walk %lld ends at row %lld, walk_stride is %lld", who, (long long)w, (long long)end, (long long)walk_stride);
        tiles += walk_tiles;
        MG_REQUIRE_AS(tiles < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED, "%s: the walks' tiles exceed one grid (2^31 - 1 tiles of %d frames)", who, MG_WALKS_TILE);
        walk_tile[(size_t)w + 1] = (int32_t)tiles;
    }
    if (n_walks == 0) return MG_OK;
    MG_WALKS_REQUIRE(latents_dev && frames_dev, "%s: NULL pointer", who);
    const size_t lds_f = ((size_t)rmax + lmax + MG_WALKS_TILE * 4) * 8 + MG_WALKS_TILE * 4;
    const size_t lds_c = ((size_t)lmax + 5 * (3 + 4 * a.n_link) + 4) * 8 + 16;
    MG_REQUIRE_AS(lds_f <= MG_WALKS_LDS_MAX, MG_ERR_UNSUPPORTED, "%s: %d control-point rows per node do not fit LDS", who, rmax);
    // the table: node records, frame offsets, then the int32 tables
    std::vector<unsigned char> tab((size_t)n_nodes * sizeof(mg_walks_node));
    for (int k = 0; k < n_nodes; k++) {
        const mg_primitive *p = prims[k];
        mg_walks_node nd;
        nd.Et64 = p->d_Et64; nd.mean = p->d_mean; nd.knots = p->d_knots; nd.i0 = p->canonical->d_i0; nd.w = p->canonical->d_w;
        nd.L = p->L; nd.R = p->R; nd.NB = p->NB; nd.T = p->canonical->T;
        memcpy(tab.data() + (size_t)k * sizeof(nd), &nd, sizeof(nd));
    }
    const size_t off_offs = mg_table_append(tab, offs.data(), (size_t)nws * 8);
    const size_t off_node = mg_table_append(tab, node_of, (size_t)nws * 4), off_steps = mg_table_append(tab, n_steps, (size_t)n_walks * 4);
    const size_t off_wtile = mg_table_append(tab, walk_tile.data(), walk_tile.size() * 4), off_stile = mg_table_append(tab, step_tile.data(), (size_t)nws * 4);
    const size_t off_lens = WARPED ? mg_table_append(tab, lengths, (size_t)nws * 4) : 0;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[table];
    rc = dt.upload(ctx, who, tab.data(), tab.size(), 0, (size_t)nws * 8 * 8);   // behind the table: the steps' transforms
    if (rc != MG_OK) return rc;
    char *base = dt.base();
    a.nodes = (const mg_walks_node *)base;
    a.frame_offset = (const int64_t *)(base + off_offs);
    a.node_of = (const int32_t *)(base + off_node); a.n_steps = (const int32_t *)(base + off_steps);
    a.walk_tile = (const int32_t *)(base + off_wtile); a.step_tile = (const int32_t *)(base + off_stile);
    a.lengths = WARPED ? (const int32_t *)(base + off_lens) : nullptr;
    a.times = times_dev; a.t_cap = t_cap;
    a.lat = latents_dev;
    a.xf = (double *)dt.scratch();
    a.transforms = transforms_dev; a.frames = frames_dev;
    a.n_walks = n_walks; a.ld = ld; a.walk_stride = walk_stride;
    a.s_max = s_max; a.D = D; a.lmax = lmax; a.rmax = rmax;
    MG_HIP_CHECK(mg_lds_opt_in_once(ctx, lds_bit, 160 * 1024, mg_walks_frames_kernel<true, WARPED>, mg_walks_frames_kernel<false, WARPED>));
    hipStream_t st = ctx->stream;
    const bool lf = dtype == MG_F64;
    if (lf) hipLaunchKernelGGL((mg_walks_chain_kernel<true, WARPED>), dim3((unsigned)n_walks), dim3(MG_WALKS_CHAIN_BLOCK), lds_c, st, a);
    else hipLaunchKernelGGL((mg_walks_chain_kernel<false, WARPED>), dim3((unsigned)n_walks), dim3(MG_WALKS_CHAIN_BLOCK), lds_c, st, a);
    MG_HIP_CHECK(hipGetLastError());
    if (lf) hipLaunchKernelGGL((mg_walks_frames_kernel<true, WARPED>), dim3((unsigned)tiles), dim3(MG_WALKS_BLOCK), lds_f, st, a);
    else hipLaunchKernelGGL((mg_walks_frames_kernel<false, WARPED>), dim3((unsigned)tiles), dim3(MG_WALKS_BLOCK), lds_f, st, a);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

extern "C" int mg_walks_frames(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents_dev, int dtype,
                               int64_t n_walks, int32_t s_max, int64_t ld, const int64_t *frame_offset, const mg_alignment_desc *al,
                               const mg_skeleton_desc *sk, double *frames_dev, int64_t walk_stride, double *transforms_dev) {
    return mg_walks_frames_launch<false>("mg_walks_frames", MG_TABLE_WALKS_MIXED, MG_LDS_WALKS_FRAMES, n_nodes, prims, node_of, n_steps, latents_dev, dtype, n_walks,
                                         s_max, ld, nullptr, nullptr, 0, frame_offset, al, sk, frames_dev, walk_stride, transforms_dev);
}

extern "C" int mg_walks_frames_at(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents_dev, int dtype,
                                  int64_t n_walks, int32_t s_max, int64_t ld, const double *times_dev, const int32_t *lengths, int32_t t_cap,
                                  const int64_t *frame_offset, const mg_alignment_desc *al, const mg_skeleton_desc *sk, double *frames_dev, int64_t walk_stride,
                                  double *transforms_dev) {
    return mg_walks_frames_launch<true>("mg_walks_frames_at", MG_TABLE_WALKS_WARPED, MG_LDS_WALKS_WARPED, n_nodes, prims, node_of, n_steps, latents_dev, dtype,
                                        n_walks, s_max, ld, times_dev, lengths, t_cap, frame_offset, al, sk, frames_dev, walk_stride, transforms_dev);
}

// Every step's time row.  What a row is made of is a node's; which node, and where gamma lies, is the step's.
// SMOOTH: smooth_of_node marks the nodes whose rows go through the Savitzky-Golay pass; a table of the entry point's own
template <bool SMOOTH>
static int mg_walks_time_launch(const char *who, int which_table, unsigned lds_bit, int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of,
                                const int32_t *n_steps, const uint8_t *smooth_of_node, const void *latents_dev, int dtype, int64_t n_walks, int32_t s_max,
                                int64_t ld, double speed, double *times_dev, int32_t *lengths_dev, int32_t t_cap) {
    std::vector<char> occurs;
    int rc = mg_walks_check_tables(who, n_nodes, prims, node_of, n_steps, n_walks, s_max, occurs);
    if (rc != MG_OK) return rc;
    MG_WALKS_REQUIRE((dtype == MG_F32 || dtype == MG_F64) && ld >= 1 && t_cap >= 1, "%s: bad arguments", who);
    MG_WALKS_REQUIRE(speed > 0.0 && std::isfinite(speed), "%s: speed must be positive and finite", who);
    MG_WALKS_REQUIRE(!SMOOTH || smooth_of_node, "%s: smooth_of_node is NULL", who);
    const double inv_speed = 1.0 / speed;
    std::vector<mg_walks_time_node> nodes((size_t)n_nodes);
    int fmax = 0;
    for (int k = 0; k < n_nodes; k++) {
        const mg_primitive *p = prims[k];
        mg_walks_time_node &nd = nodes[(size_t)k];
        nd.tphi = p->Lt > 0 ? p->d_tphi : nullptr; nd.tmean = p->Lt > 0 ? p->d_tmean : nullptr;
        nd.F = p->F; nd.Lt = p->Lt; nd.L = p->L; nd.count = 0;
        if (!occurs[(size_t)k]) continue;
        MG_WALKS_REQUIRE(p->L + p->Lt <= ld, "%s: node %d reads %d latent columns, ld is %lld", who, k, p->L + p->Lt, (long long)ld);
        if (p->Lt > 0) {
            MG_REQUIRE_AS(p->F >= 4 && p->F <= MG_TW_MAX_F, MG_ERR_UNSUPPORTED, "%s: node %d has %d canonical frames (4 .. %d supported)", who, k, p->F, MG_TW_MAX_F);
            fmax = std::max(fmax, (int)p->F);
        } else {
            const double countf = (double)p->F * inv_speed;   // int(F * (1 / speed)), numpy.linspace's num
            MG_WALKS_REQUIRE(countf >= 1.0, "%s: node %d of %d canonical frames has no sample at speed %g", who, k, p->F, speed);
            MG_REQUIRE_AS(countf <= 16777216.0, MG_ERR_UNSUPPORTED, "%s: node %d asks for %g samples at speed %g", who, k, countf, speed);
            nd.count = (int32_t)countf;
        }
    }
    if (n_walks == 0) return MG_OK;
    MG_WALKS_REQUIRE(latents_dev && times_dev && lengths_dev, "%s: NULL pointer", who);
    mg_context *ctx = prims[0]->ctx;
    const int64_t rows = n_walks * s_max;
    std::vector<unsigned char> tab((size_t)n_nodes * sizeof(mg_walks_time_node));
    memcpy(tab.data(), nodes.data(), tab.size());
    const size_t off_node = mg_table_append(tab, node_of, (size_t)rows * 4), off_steps = mg_table_append(tab, n_steps, (size_t)n_walks * 4);
    const size_t off_smooth = SMOOTH ? mg_table_append(tab, smooth_of_node, (size_t)n_nodes) : 0;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[which_table];
    rc = dt.upload(ctx, who, tab.data(), tab.size());
    if (rc != MG_OK) return rc;
    mg_walks_time_args a;
    a.smooth = nullptr; a.H = nullptr;
    if (SMOOTH) {
        a.smooth = (const uint8_t *)(dt.base() + off_smooth);
        if ((rc = mg_savgol_table_dev(ctx, &a.H)) != MG_OK) return rc;
    }
    a.nodes = (const mg_walks_time_node *)dt.base();
    a.node_of = (const int32_t *)(dt.base() + off_node); a.n_steps = (const int32_t *)(dt.base() + off_steps);
    a.lat = latents_dev; a.times = times_dev; a.lens = lengths_dev;
    a.ld = ld; a.inv_speed = inv_speed; a.s_max = s_max; a.t_cap = t_cap;
    const size_t lds = ((size_t)4 * fmax + (SMOOTH ? MG_TW_SMOOTH_LDS : 0)) * 8;   // x, M, cp, dp of the longest timed node that occurs; the smoothed row's window
    MG_HIP_CHECK(mg_lds_opt_in_once(ctx, lds_bit, 160 * 1024, mg_walks_time_kernel<true, SMOOTH>, mg_walks_time_kernel<false, SMOOTH>));
    if (dtype == MG_F64) hipLaunchKernelGGL((mg_walks_time_kernel<true, SMOOTH>), dim3((unsigned)rows), dim3(MG_TW_BLOCK), lds, ctx->stream, a);
    else hipLaunchKernelGGL((mg_walks_time_kernel<false, SMOOTH>), dim3((unsigned)rows), dim3(MG_TW_BLOCK), lds, ctx->stream, a);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

extern "C" int mg_walks_time_functions(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents_dev,
                                       int dtype, int64_t n_walks, int32_t s_max, int64_t ld, double speed, double *times_dev, int32_t *lengths_dev,
                                       int32_t t_cap) {
    return mg_walks_time_launch<false>("mg_walks_time_functions", MG_TABLE_WALKS_TIME, MG_LDS_WALKS_TIME, n_nodes, prims, node_of, n_steps, nullptr, latents_dev, dtype,
                                       n_walks, s_max, ld, speed, times_dev, lengths_dev, t_cap);
}

extern "C" int mg_walks_time_functions_smoothed(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps,
                                                const uint8_t *smooth_of_node, const void *latents_dev, int dtype, int64_t n_walks, int32_t s_max, int64_t ld,
                                                double speed, double *times_dev, int32_t *lengths_dev, int32_t t_cap) {
    return mg_walks_time_launch<true>("mg_walks_time_functions_smoothed", MG_TABLE_WALKS_TIME_SMOOTHED, MG_LDS_WALKS_TIME_SMOOTHED, n_nodes, prims, node_of, n_steps,
                                      smooth_of_node, latents_dev, dtype, n_walks, s_max, ld, speed, times_dev, lengths_dev, t_cap);
}

// host arrays in, host arrays out: one device block for the call, synchronises
extern "C" int mg_walks_sample_latents_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, int64_t n_walks,
                                            int32_t s_max, uint64_t seed, void *x, int xdt, int64_t ld, int32_t *comp) {
    MG_WALKS_REQUIRE(n_nodes >= 1 && prims && prims[0] && n_walks >= 0 && s_max >= 1 && ld >= 1 && (xdt == MG_F32 || xdt == MG_F64),
                     "mg_walks_sample_latents_host: bad arguments");
    MG_WALKS_REQUIRE(n_walks == 0 || x, "mg_walks_sample_latents_host: NULL pointer");
    mg_workspace ws(prims[0]->ctx, "mg_walks_sample_latents_host");
    const mg_staged d_x = ws.out(x, (size_t)(n_walks * s_max * ld) * (xdt == MG_F64 ? 8 : 4));
    const mg_staged d_c = ws.out(comp, (size_t)(n_walks * s_max) * 4);
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    rc = mg_walks_sample_latents(n_nodes, prims, node_of, n_steps, n_walks, s_max, seed, d_x.dev<void>(), xdt, ld, d_c.dev<int32_t>());
    if (rc != MG_OK) return rc;
    return ws.download();
}

extern "C" int mg_walks_frames_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents, int dtype,
                                    int64_t n_walks, int32_t s_max, int64_t ld, const int64_t *frame_offset, const mg_alignment_desc *al,
                                    const mg_skeleton_desc *sk, double *frames, int64_t walk_stride, double *transforms) {
    MG_WALKS_REQUIRE(n_nodes >= 1 && prims && prims[0] && n_walks >= 0 && s_max >= 1 && ld >= 1 && walk_stride >= 1 && (dtype == MG_F32 || dtype == MG_F64),
                     "mg_walks_frames_host: bad arguments");
    MG_WALKS_REQUIRE(n_walks == 0 || (latents && frames), "mg_walks_frames_host: NULL pointer");
    mg_context *ctx = prims[0]->ctx;
    const int64_t D = prims[0]->D;
    mg_workspace ws(ctx, "mg_walks_frames_host");
    const mg_staged d_lat = ws.in(latents, (size_t)(n_walks * s_max * ld) * (dtype == MG_F64 ? 8 : 4));
    const mg_staged d_frames = ws.inout(frames, (size_t)(n_walks * walk_stride * D) * 8);   // rows no step owns stay the caller's
    const mg_staged d_xf = ws.inout(transforms, (size_t)(n_walks * s_max * 4) * 8);          // ... and the entries of steps a walk does not have
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    rc = mg_walks_frames(n_nodes, prims, node_of, n_steps, d_lat.dev<void>(), dtype, n_walks, s_max, ld, frame_offset, al, sk, d_frames.dev<double>(),
                         walk_stride, d_xf.dev<double>());
    if (rc != MG_OK) return rc;
    return ws.download();
}

extern "C" int mg_walks_time_functions_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents,
                                            int dtype, int64_t n_walks, int32_t s_max, int64_t ld, double speed, double *times, int32_t *lengths, int32_t t_cap) {
    MG_WALKS_REQUIRE(n_nodes >= 1 && prims && prims[0] && n_walks >= 0 && s_max >= 1 && ld >= 1 && t_cap >= 1 && (dtype == MG_F32 || dtype == MG_F64),
                     "mg_walks_time_functions_host: bad arguments");
    MG_WALKS_REQUIRE(n_walks == 0 || (latents && times && lengths), "mg_walks_time_functions_host: NULL pointer");
    mg_workspace ws(prims[0]->ctx, "mg_walks_time_functions_host");
    const mg_staged d_lat = ws.in(latents, (size_t)(n_walks * s_max * ld) * (dtype == MG_F64 ? 8 : 4));
    const mg_staged d_times = ws.inout(times, (size_t)(n_walks * s_max * t_cap) * 8);   // rows that are not written stay the caller's
    const mg_staged d_lens = ws.out(lengths, (size_t)(n_walks * s_max) * 4);
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    rc = mg_walks_time_functions(n_nodes, prims, node_of, n_steps, d_lat.dev<void>(), dtype, n_walks, s_max, ld, speed, d_times.dev<double>(),
                                 d_lens.dev<int32_t>(), t_cap);
    if (rc != MG_OK) return rc;
    return ws.download();
}

extern "C" int mg_walks_time_functions_smoothed_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps,
                                                     const uint8_t *smooth_of_node, const void *latents, int dtype, int64_t n_walks, int32_t s_max, int64_t ld,
                                                     double speed, double *times, int32_t *lengths, int32_t t_cap) {
    MG_WALKS_REQUIRE(n_nodes >= 1 && prims && prims[0] && n_walks >= 0 && s_max >= 1 && ld >= 1 && t_cap >= 1 && (dtype == MG_F32 || dtype == MG_F64),
                     "mg_walks_time_functions_smoothed_host: bad arguments");
    MG_WALKS_REQUIRE(n_walks == 0 || (latents && times && lengths), "mg_walks_time_functions_smoothed_host: NULL pointer");
    mg_workspace ws(prims[0]->ctx, "mg_walks_time_functions_smoothed_host");
    const mg_staged d_lat = ws.in(latents, (size_t)(n_walks * s_max * ld) * (dtype == MG_F64 ? 8 : 4));
    const mg_staged d_times = ws.inout(times, (size_t)(n_walks * s_max * t_cap) * 8);   // rows that are not written stay the caller's
    const mg_staged d_lens = ws.out(lengths, (size_t)(n_walks * s_max) * 4);
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    rc = mg_walks_time_functions_smoothed(n_nodes, prims, node_of, n_steps, smooth_of_node, d_lat.dev<void>(), dtype, n_walks, s_max, ld, speed,
                                          d_times.dev<double>(), d_lens.dev<int32_t>(), t_cap);
    if (rc != MG_OK) return rc;
    return ws.download();
}

extern "C" int mg_walks_frames_at_host(int32_t n_nodes, mg_primitive *const *prims, const int32_t *node_of, const int32_t *n_steps, const void *latents, int dtype,
                                       int64_t n_walks, int32_t s_max, int64_t ld, const double *times, const int32_t *lengths, int32_t t_cap,
                                       const int64_t *frame_offset, const mg_alignment_desc *al, const mg_skeleton_desc *sk, double *frames, int64_t walk_stride,
                                       double *transforms) {
    MG_WALKS_REQUIRE(n_nodes >= 1 && prims && prims[0] && n_walks >= 0 && s_max >= 1 && ld >= 1 && walk_stride >= 1 && t_cap >= 1 &&
                         (dtype == MG_F32 || dtype == MG_F64),
                     "mg_walks_frames_at_host: bad arguments");
    MG_WALKS_REQUIRE(n_walks == 0 || (latents && frames && times), "mg_walks_frames_at_host: NULL pointer");
    mg_context *ctx = prims[0]->ctx;
    const int64_t D = prims[0]->D;
    mg_workspace ws(ctx, "mg_walks_frames_at_host");
    const mg_staged d_lat = ws.in(latents, (size_t)(n_walks * s_max * ld) * (dtype == MG_F64 ? 8 : 4));
    const mg_staged d_times = ws.in(times, (size_t)(n_walks * s_max * t_cap) * 8);
    const mg_staged d_frames = ws.inout(frames, (size_t)(n_walks * walk_stride * D) * 8);   // rows no step owns stay the caller's
    const mg_staged d_xf = ws.inout(transforms, (size_t)(n_walks * s_max * 4) * 8);          // ... and the entries of steps a walk does not have
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    rc = mg_walks_frames_at(n_nodes, prims, node_of, n_steps, d_lat.dev<void>(), dtype, n_walks, s_max, ld, d_times.dev<double>(), lengths, t_cap, frame_offset, al,
                            sk, d_frames.dev<double>(), walk_stride, d_xf.dev<double>());
    if (rc != MG_OK) return rc;
    return ws.download();
}
