// A graph walk's motion as one array of frames, for a whole population of walks (gfx950 / MI355X), float64.
//
// The reference turns a finished walk into frames step by step (motion_generator/graph_walk.py:154-176): back_project every
// step's latent vector, MotionVector.append_frames aligns the step to the last frame so far (anim_utils'
// align_quaternion_frames: a rotation about y and a translation in x and z, smoothing off during synthesis, :102) and appends
// it.  Here every walk of a batch shares the node sequence (the shape of the global optimiser's batch) and two launches write all
// frames once, where they end up:
//
//   mg_walk_chain_kernel    one workgroup per walk, the steps in order.  Per step the control points of the channels the
//                           aligning joint's chain reads (root translation + the chain's quaternions) at the FIRST control point
//                           and at the four taps of the LAST sample, lanes over (control point, channel) pairs (fma chains from the
//                           mean: the float64 frames kernels' arithmetic); one lane forms the step's heading, the transform
//                           (mg_align2d_from, mg_align_half_angle) and the aligned exit pose the next step is aligned to.
//   mg_walk_frames_kernel   grid over (walk, step, tile of MG_WALK_TILE frames): the tile's basis rows (the canonical grid's
//                           tables, or the FITPACK recurrence at the walk's own times), the control points of the tile's window,
//                           four taps per channel, the step's transform on the seven root channels, every row stored once at its
//                           final place in 16-byte pieces.
//
// An unaligned step (the first one without an alignment record) goes through no transform at all: its frames are the bits of
// mg_back_project_frames_f64 / mg_back_project_frames_at.  What grows with n_steps travels in a device table (ctx->tab[MG_TABLE_WALK]).
#include <cmath>
#include <cstring>

#include <algorithm>
#include <vector>

#include <hip/hip_ext.h>

#include "mg_construct.h"
#include "mg_joint_plan.h"
#include "mg_score_device.h"
#include "mg_spline_device.h"

#define MG_WALK_TILE 32          // frames per workgroup of the frames kernel
#define MG_WALK_BLOCK 256
#define MG_WALK_CHAIN_BLOCK 64
#define MG_WALK_LDS_MAX (160 * 1024 - 64)

struct mg_walk_step {            // one step's constants on the device (64 bytes)
    const double *Et64, *mean, *knots;
    const int32_t *i0;           // the canonical grid's tables
    const double *w;
    int32_t L, R, NB, T;         // T: samples of the canonical grid
    int32_t lat_off, tile0;      // first column of the step's latents; first tile of the step among a walk's tiles
};

struct mg_walk_args {
    const mg_walk_step *steps;
    const int64_t *frame_offset; // (n_walks, n_steps)
    const int32_t *lengths;      // (n_walks, n_steps) or NULL: the canonical grids
    const double *times;         // (n_walks, n_steps, t_cap) or NULL
    const void *lat;
    double *xf;                  // (n_walks, n_steps, 8): c, s, tx, tz, ty, cos(phi / 2), sin(phi / 2), 1 if the step is aligned
    double *transforms;          // NULL or (n_walks, n_steps, 4)
    double *frames;
    int64_t n_walks, ld, walk_stride;
    int32_t n_steps, D, t_cap, tiles_per_walk;
    int32_t lmax, rmax;          // the longest latent row and the most control-point rows of a step: LDS pitches
    int32_t align_mode;          // first step: 0 as it is, 1 previous frame, 2 start pose
    int32_t n_link;              // animated joints along the aligning node's chain
    double h0, h1, px, py, pz, ref[3];
    int32_t link[MG_MAX_CHAIN];  // their quaternion channels, root first
};

template <bool LAT_F64>
__global__ __launch_bounds__(MG_WALK_CHAIN_BLOCK) void mg_walk_chain_kernel(const mg_walk_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nch = 3 + 4 * a.n_link;
    double *s = (double *)smem;            // [Lmax]
    double *cpv = s + a.lmax;              // [5][nch]: the first control point, then the last sample's four taps
    double *wl = cpv + 5 * nch;            // [4] the last sample's weights
    int *i0l = (int *)(wl + 4);            // its first tap
    const int64_t wk = blockIdx.x;
    const int tid = threadIdx.x, D = a.D;
    double hx = a.h0, hz = a.h1, tpx = a.px, tpz = a.pz;   // what the step is aligned to (lane 0)
    for (int i = 0; i < a.n_steps; i++) {
        const mg_walk_step st = a.steps[i];
        const int64_t ws = wk * a.n_steps + i;
        for (int k = tid; k < st.L; k += MG_WALK_CHAIN_BLOCK) s[k] = mg_load_lat<LAT_F64>(a.lat, wk * a.ld + st.lat_off + k);
        if (tid == 0) {
            if (a.times) {
                const int len = a.lengths[ws];
                mg_basis_row_dev(st.knots, st.NB + 4, a.times[ws * a.t_cap + len - 1], i0l, wl);
            } else {
                *i0l = st.i0[st.T - 1];
                for (int j = 0; j < 4; j++) wl[j] = st.w[4 * (size_t)(st.T - 1) + j];
            }
        }
        __syncthreads();
        const int il = *i0l;
        for (int e = tid; e < 5 * nch; e += MG_WALK_CHAIN_BLOCK) {
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
            if (i + 1 < a.n_steps) {       // the aligned last sample: what the next step is aligned to
                double y = 0.0;            // (its height is not needed)
                tpx = last(0); tpz = last(2);
                if (aligned) mg_align_position(t, tpx, y, tpz);
                heading(true, aligned, qaw, qay, hx, hz);
            }
        }
        __syncthreads();
    }
}

template <bool LAT_F64>
__global__ __launch_bounds__(MG_WALK_BLOCK) void mg_walk_frames_kernel(const mg_walk_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *cp = (double *)smem;                    // [rows of the tile's window][D], at most rmax doubles
    double *s = cp + a.rmax;                        // [lmax]
    double *wt = s + a.lmax;                         // [MG_WALK_TILE][4]
    int *i0t = (int *)(wt + MG_WALK_TILE * 4);      // [MG_WALK_TILE]
    const int64_t wk = blockIdx.x / a.tiles_per_walk;
    const int kt = (int)(blockIdx.x - wk * a.tiles_per_walk);
    int i = 0;
    while (i + 1 < a.n_steps && kt >= a.steps[i + 1].tile0) i++;
    const mg_walk_step st = a.steps[i];
    const int64_t ws = wk * a.n_steps + i;
    const int len = a.lengths ? a.lengths[ws] : st.T;
    const int f0 = (kt - st.tile0) * MG_WALK_TILE;
    if (f0 >= len) return;
    const int nf = len - f0 < MG_WALK_TILE ? len - f0 : MG_WALK_TILE;
    const int tid = threadIdx.x, D = a.D;
    if (tid < nf) {
        if (a.times) {
            mg_basis_row_dev(st.knots, st.NB + 4, a.times[ws * a.t_cap + f0 + tid], &i0t[tid], &wt[4 * tid]);
        } else {
            i0t[tid] = st.i0[f0 + tid];
            for (int j = 0; j < 4; j++) wt[4 * tid + j] = st.w[4 * (size_t)(f0 + tid) + j];
        }
    }
    for (int k = tid; k < st.L; k += MG_WALK_BLOCK) s[k] = mg_load_lat<LAT_F64>(a.lat, wk * a.ld + st.lat_off + k);
    __syncthreads();
    int imin = i0t[0], imax = i0t[0];
    for (int f = 1; f < nf; f++) { const int v = i0t[f]; imin = v < imin ? v : imin; imax = v > imax ? v : imax; }
    const int rows = (imax + 4 - imin) * D, r0 = imin * D;
    for (int e = tid; e < rows; e += MG_WALK_BLOCK) {   // control points: fma chain over k ascending from the mean
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
        // mg_align_position's and mg_align_root_quat's statements, one channel at a time: a lane owns one channel and forms only
        // the partner it needs, which the helpers' whole-pose form cannot express
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
    for (int p = tid; p < npairs; p += MG_WALK_BLOCK) {
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

#define MG_WALK_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)

extern "C" int mg_walk_frames(int32_t n_steps, mg_primitive *const *prims, const int64_t *latent_offset, const void *latents_dev, int dtype,
                              int64_t n_walks, int64_t ld, const double *times_dev, const int32_t *lengths, int32_t t_cap, const int64_t *frame_offset,
                              const mg_alignment_desc *al, const mg_skeleton_desc *sk, double *frames_dev, int64_t walk_stride, double *transforms_dev) {
    MG_WALK_REQUIRE(n_steps >= 1 && n_steps <= MG_WALK_MAX_STEPS, "mg_walk_frames: %d steps (1 .. %d per call)", n_steps, MG_WALK_MAX_STEPS);
    MG_WALK_REQUIRE(prims && latent_offset && prims[0], "mg_walk_frames: NULL pointer");
    MG_WALK_REQUIRE((dtype == MG_F32 || dtype == MG_F64) && n_walks >= 0 && ld >= 1 && walk_stride >= 1, "mg_walk_frames: bad arguments");
    mg_context *ctx = prims[0]->ctx;
    const int D = prims[0]->D;
    int lmax = 0, rmax = 0;
    for (int i = 0; i < n_steps; i++) {
        const mg_primitive *p = prims[i];
        MG_WALK_REQUIRE(p != nullptr, "mg_walk_frames: primitive %d is NULL", i);
        MG_WALK_REQUIRE(p->ctx == ctx, "mg_walk_frames: primitive %d belongs to another context", i);
        MG_WALK_REQUIRE(p->D == D, "mg_walk_frames: primitive %d has n_dim %d, the first one %d", i, p->D, D);
        MG_WALK_REQUIRE(latent_offset[i] >= 0 && latent_offset[i] + p->L <= ld, "mg_walk_frames: step %d reads latent columns %lld .. %lld of %lld", i,
                        (long long)latent_offset[i], (long long)(latent_offset[i] + p->L), (long long)ld);
        lmax = std::max(lmax, (int)p->L);
        rmax = std::max(rmax, (int)p->R);
    }
    const bool aligned_any = n_steps > 1 || al != nullptr;
    MG_WALK_REQUIRE(D >= 3 && (!aligned_any || D >= 7), "mg_walk_frames: n_dim %d has no root channels to align", D);
    MG_WALK_REQUIRE((times_dev == nullptr) == (lengths == nullptr), "mg_walk_frames: times and lengths come together");
    MG_WALK_REQUIRE(!times_dev || (frame_offset && t_cap >= 1), "mg_walk_frames: times need frame offsets and t_cap >= 1");
    // the aligning node: the record's, or the root and (0, 0, 1)
    mg_walk_args a = {};
    int joint = 0;
    a.ref[0] = 0.0; a.ref[1] = 0.0; a.ref[2] = 1.0;
    a.h0 = 1.0;
    if (al) {
        const double hn = std::sqrt(al->heading[0] * al->heading[0] + al->heading[1] * al->heading[1]);
        MG_WALK_REQUIRE(hn > 0.0 && std::isfinite(hn), "mg_walk_frames: heading is zero or not finite");
        a.h0 = al->heading[0] / hn; a.h1 = al->heading[1] / hn;
        a.px = al->position[0]; a.py = al->position[1]; a.pz = al->position[2];
        if (al->joint == MG_ALIGN_START_POSE) {
            a.align_mode = 2;    // (a start pose names no node: later steps go through the root and (0, 0, 1))
        } else {
            a.align_mode = 1;
            joint = al->joint;
            for (int e = 0; e < 3; e++) a.ref[e] = al->ref_dir[e];
            MG_WALK_REQUIRE(a.ref[0] * a.ref[0] + a.ref[2] * a.ref[2] > 0.0, "mg_walk_frames: ref_dir has no xz part");
        }
    }
    if (!aligned_any) {
        a.n_link = 0;            // nothing is aligned: no heading is formed, the chain kernel reads the root translation only (n_dim may be 3)
    } else if (joint == 0 && !sk) {
        a.n_link = 1; a.link[0] = 3;
    } else {
        MG_WALK_REQUIRE(sk != nullptr, "mg_walk_frames: aligning joint %d is not the root: a skeleton is needed", joint);
        MG_WALK_REQUIRE(mg_skeleton_complete(sk, false) && joint >= 0 && joint < sk->n_joints,      // (no position is formed: the offsets are not read)
                        "mg_walk_frames: incomplete skeleton or aligning joint %d out of range", joint);
        std::vector<int32_t> quats;
        const mg_plan_failure f = mg_aligning_quaternions(sk, joint, D, quats);
        MG_WALK_REQUIRE(!f.of_skeleton(), "mg_walk_frames: joint %d%s", f.joint, mg_chain_why(f.kind));
        MG_WALK_REQUIRE(!f, "mg_walk_frames: the aligning chain does not fit (channel %d, n_dim %d)", f.channel, D);
        a.n_link = (int32_t)quats.size();
        std::copy(quats.begin(), quats.end(), a.link);
    }
    // lengths and offsets: every step inside its walk's rows, no two steps on the same row
    const int64_t nws = n_walks * n_steps;
    std::vector<int64_t> offs((size_t)nws);
    std::vector<std::pair<int64_t, int64_t>> spans((size_t)n_steps);
    for (int64_t w = 0; w < n_walks; w++) {
        int64_t next = 0;
        for (int i = 0; i < n_steps; i++) {
            const int64_t len = lengths ? lengths[w * n_steps + i] : prims[i]->canonical->T;
            MG_WALK_REQUIRE(len >= 1, "mg_walk_frames: walk %lld, step %d has length %lld", (long long)w, i, (long long)len);
            MG_WALK_REQUIRE(!lengths || len <= t_cap, "mg_walk_frames: walk %lld, step %d has %lld samples, t_cap is %d", (long long)w, i, (long long)len, t_cap);
            const int64_t off = frame_offset ? frame_offset[w * n_steps + i] : next;
            offs[(size_t)(w * n_steps + i)] = off;
            spans[(size_t)i] = {off, len};
            next = off + len;
        }
        std::sort(spans.begin(), spans.end());
        int64_t end = 0;
        for (int i = 0; i < n_steps; i++) {
            MG_WALK_REQUIRE(spans[(size_t)i].first >= end, "mg_walk_frames: walk %lld: steps overlap at row %lld", (long long)w, (long long)spans[(size_t)i].first);
            end = spans[(size_t)i].first + spans[(size_t)i].second;
        }
        MG_WALK_REQUIRE(end <= walk_stride, "mg_walk_frames: walk %lld ends at row %lld, walk_stride is %lld", (long long)w, (long long)end, (long long)walk_stride);
    }
    if (n_walks == 0) return MG_OK;
    MG_WALK_REQUIRE(latents_dev && frames_dev, "mg_walk_frames: NULL pointer");
    const size_t lds_f = ((size_t)rmax + lmax + MG_WALK_TILE * 4) * 8 + MG_WALK_TILE * 4;
    const size_t lds_c = ((size_t)lmax + 5 * (3 + 4 * a.n_link) + 4) * 8 + 16;
    MG_REQUIRE_AS(lds_f <= MG_WALK_LDS_MAX, MG_ERR_UNSUPPORTED, "mg_walk_frames: %d control-point rows per step do not fit LDS", rmax);
    // the table: steps, offsets, lengths
    const size_t off_steps = 0, off_offs = (size_t)n_steps * sizeof(mg_walk_step), off_lens = off_offs + (size_t)nws * 8;
    std::vector<unsigned char> tab(off_lens + (lengths ? (size_t)nws * 4 : 0));
    int64_t tiles = 0;
    for (int i = 0; i < n_steps; i++) {
        const mg_primitive *p = prims[i];
        mg_walk_step st;
        st.Et64 = p->d_Et64; st.mean = p->d_mean; st.knots = p->d_knots; st.i0 = p->canonical->d_i0; st.w = p->canonical->d_w;
        st.L = p->L; st.R = p->R; st.NB = p->NB; st.T = p->canonical->T;
        st.lat_off = (int32_t)latent_offset[i]; st.tile0 = (int32_t)tiles;
        memcpy(tab.data() + off_steps + (size_t)i * sizeof(mg_walk_step), &st, sizeof(st));
        tiles += ((lengths ? (int64_t)t_cap : (int64_t)st.T) + MG_WALK_TILE - 1) / MG_WALK_TILE;
    }
    MG_REQUIRE_AS(tiles * n_walks < ((int64_t)1 << 31) && n_walks < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED, "mg_walk_frames: %lld walks x %lld tiles exceed one grid",
                  (long long)n_walks, (long long)tiles);
    memcpy(tab.data() + off_offs, offs.data(), (size_t)nws * 8);
    if (lengths) memcpy(tab.data() + off_lens, lengths, (size_t)nws * 4);
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[MG_TABLE_WALK];
    int rc = dt.upload(ctx, "mg_walk_frames", tab.data(), tab.size(), 0, (size_t)nws * 8 * 8);   // behind the table: the steps' transforms
    if (rc != MG_OK) return rc;
    char *base = dt.base();
    a.steps = (const mg_walk_step *)(base + off_steps);
    a.frame_offset = (const int64_t *)(base + off_offs);
    a.lengths = lengths ? (const int32_t *)(base + off_lens) : nullptr;
    a.times = times_dev; a.lat = latents_dev;
    a.xf = (double *)dt.scratch();
    a.transforms = transforms_dev; a.frames = frames_dev;
    a.n_walks = n_walks; a.ld = ld; a.walk_stride = walk_stride;
    a.n_steps = n_steps; a.D = D; a.tiles_per_walk = (int32_t)tiles;
    MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALK_FRAMES, 160 * 1024, mg_walk_frames_kernel<true>, mg_walk_frames_kernel<false>));
    hipStream_t st = ctx->stream;
    const bool lf = dtype == MG_F64;
    a.t_cap = t_cap; a.lmax = lmax; a.rmax = rmax;
    if (lf) hipLaunchKernelGGL(mg_walk_chain_kernel<true>, dim3((unsigned)n_walks), dim3(MG_WALK_CHAIN_BLOCK), lds_c, st, a);
    else hipLaunchKernelGGL(mg_walk_chain_kernel<false>, dim3((unsigned)n_walks), dim3(MG_WALK_CHAIN_BLOCK), lds_c, st, a);
    MG_HIP_CHECK(hipGetLastError());
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const bool timed = mg_prof_kernel(ctx, MG_PROF_WALK_FRAMES, -1, &ev0, &ev1);
    const unsigned grid = (unsigned)(tiles * n_walks);
    if (lf) hipExtLaunchKernelGGL(mg_walk_frames_kernel<true>, dim3(grid), dim3(MG_WALK_BLOCK), lds_f, st, timed ? ev0 : nullptr, timed ? ev1 : nullptr, 0, a);
    else hipExtLaunchKernelGGL(mg_walk_frames_kernel<false>, dim3(grid), dim3(MG_WALK_BLOCK), lds_f, st, timed ? ev0 : nullptr, timed ? ev1 : nullptr, 0, a);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

// host arrays in, host arrays out: one device block for the call, synchronises
extern "C" int mg_walk_frames_host(int32_t n_steps, mg_primitive *const *prims, const int64_t *latent_offset, const void *latents, int dtype, int64_t n_walks,
                                   int64_t ld, const double *times, const int32_t *lengths, int32_t t_cap, const int64_t *frame_offset,
                                   const mg_alignment_desc *al, const mg_skeleton_desc *sk, double *frames, int64_t walk_stride, double *transforms) {
    MG_WALK_REQUIRE(n_steps >= 1 && prims && prims[0] && n_walks >= 0 && ld >= 1 && walk_stride >= 1 && (dtype == MG_F32 || dtype == MG_F64),
                    "mg_walk_frames_host: bad arguments");
    MG_WALK_REQUIRE(n_walks == 0 || (latents && frames), "mg_walk_frames_host: NULL pointer");
    MG_WALK_REQUIRE(!times || t_cap >= 1, "mg_walk_frames_host: times need t_cap >= 1");
    mg_context *ctx = prims[0]->ctx;
    const int64_t D = prims[0]->D;
    mg_workspace ws(ctx, "mg_walk_frames_host");
    const mg_staged d_lat = ws.in(latents, (size_t)(n_walks * ld) * (dtype == MG_F64 ? 8 : 4));
    const mg_staged d_times = ws.in(times, (size_t)(n_walks * n_steps * t_cap) * 8);
    const mg_staged d_frames = ws.inout(frames, (size_t)(n_walks * walk_stride * D) * 8);   // rows no step owns stay the caller's
    const mg_staged d_xf = ws.out(transforms, (size_t)(n_walks * n_steps * 4) * 8);
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    rc = mg_walk_frames(n_steps, prims, latent_offset, d_lat.dev<void>(), dtype, n_walks, ld, d_times.dev<double>(), lengths, t_cap, frame_offset, al, sk,
                        d_frames.dev<double>(), walk_stride, d_xf.dev<double>());
    if (rc != MG_OK) return rc;
    return ws.download();
}
