// Step lengths without frames in memory (gfx950 / MI355X), float64: the ground-plane arc length of the root path over a primitive's
// canonical frames and the distance between its first and last root position, for every candidate of every item, in ONE launch.
//
// What MotionStateGraphNode.get_step_length_for_sample (reference motion_state_graph_node.py:208-230) takes from a whole
// back-projected motion needs the root's three channels alone: 3 x n_basis control points per candidate.  A workgroup owns up to
// MG_SLEN_TILE candidates of ONE item and keeps everything between the latents and the two results in LDS:
//
//   constants   the item's 3 n_basis root rows of E' as [L][3 n_basis], their means, the canonical grid's tap rows: once per workgroup
//   phase 1     control points  c[cand][i * 3 + d] = mean', then fma(E'[k][.], s[k], .) for k ascending (mg_control_point),
//               one (candidate, row) per thread; consecutive lanes read consecutive doubles of E', the latent is a broadcast
//   phase 2     segments        one (candidate, frame) per thread: the positions p[f][d] = w0 c0, then fma(w_j, c_j, .) for j = 1, 2, 3
//               (mg_taps4) of the segment's two ends in registers, d_f = sqrt(dx * dx + dz * dz), every
//               operation rounded on its own
//   phase 3     one lane per candidate adds d_1 .. d_{F-1} in frame order and states the distance; the only stores to global memory
//
// A candidate's values are computed by statements that see nothing but its own row, so they depend on neither the batch nor the other
// items.  Which workgroup serves which item is a prefix table (first workgroup of every item) searched by bisection; the items of a
// call travel in a device table of the context (ctx->tab[MG_TABLE_STEP_LENGTH]), rewritten only when it differs from the last call's, and a launch
// takes MG_STEP_LENGTH_MAX_ITEMS of them: a call with more goes through the table in slices.
#include <cmath>
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_construct.h"
#include "mg_frames_common.h"

#define MG_SLEN_TILE 16                  // candidates per workgroup
#define MG_SLEN_LDS_MAX (150 * 1024)

struct mg_slen_item {                    // one non-empty item as the kernel reads it
    const double *Et, *mean;             // [L][R], (R): E' and mean' (scaled by translation_maxima), row = i * D + d
    const int32_t *i0;                   // [F] first control point of a canonical frame's four taps
    const double *w;                     // [F][4] their weights
    const void *lat;                     // the item's first latent: row b at lat + b * ld
    double *arc, *dist;                  // (n) or NULL
    int64_t n, ld;
    int32_t F, L, NB, D, R;
    int32_t wg0;                         // first workgroup of the item in its launch
};

struct mg_slen_args {
    const mg_slen_item *items;           // the launch's slice of the table
    int32_t n_items;
};

// LDS of a workgroup, in doubles, and where its parts start (host and device agree through this)
struct mg_slen_layout {
    int E, mean, w, lat, cp, seg, ints, total_bytes;
    int NR, FS;
};
__host__ __device__ static inline mg_slen_layout mg_slen_layout_of(int L, int NB, int F) {
    mg_slen_layout y;
    y.NR = 3 * NB;
    y.FS = F | 1;                        // odd: the lanes of phase 3 (one per candidate) read different banks
    y.E = 0;
    y.mean = y.E + L * y.NR;
    y.w = y.mean + y.NR;
    y.lat = y.w + 4 * F;
    y.cp = y.lat + MG_SLEN_TILE * L;
    y.seg = y.cp + MG_SLEN_TILE * y.NR;
    y.ints = y.seg + MG_SLEN_TILE * y.FS;   // then int32: i0[F], bad[MG_SLEN_TILE]
    y.total_bytes = y.ints * 8 + (F + MG_SLEN_TILE) * 4;
    return y;
}

// channel d of the root at canonical frame f from a candidate's control points
__device__ __forceinline__ double mg_slen_position(const double *cp, const double *sw, const int32_t *si0, int f, int d) {
    const double *c = cp + si0[f] * 3 + d;
    return mg_taps4(sw + 4 * f, c, 3);
}

template <bool LAT_F64>
__global__ __launch_bounds__(256) void mg_step_length_kernel(const mg_slen_args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    // the item of this workgroup: the last one whose first workgroup is not past it
    int lo = 0, hi = a.n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.items[mid].wg0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const mg_slen_item it = a.items[lo];
    const int L = it.L, F = it.F, D = it.D;
    const mg_slen_layout y = mg_slen_layout_of(L, it.NB, F);
    const int NR = y.NR, FS = y.FS;
    double *sm = (double *)smem;
    double *sE = sm + y.E, *smean = sm + y.mean, *sw = sm + y.w, *slat = sm + y.lat, *scp = sm + y.cp, *sseg = sm + y.seg;
    int32_t *si0 = (int32_t *)(sm + y.ints), *sbad = si0 + F;
    const int64_t b0 = (int64_t)((int)blockIdx.x - it.wg0) * MG_SLEN_TILE;
    const int ncand = (int)((it.n - b0) < MG_SLEN_TILE ? (it.n - b0) : MG_SLEN_TILE);

    // the item's constants and the tile's latents
    for (int e = tid; e < L * NR; e += 256) {
        const int k = e / NR, j = e - k * NR;
        sE[e] = it.Et[(size_t)k * it.R + (size_t)(j / 3) * D + (j % 3)];
    }
    for (int j = tid; j < NR; j += 256) smean[j] = it.mean[(size_t)(j / 3) * D + (j % 3)];
    for (int e = tid; e < 4 * F; e += 256) sw[e] = it.w[e];
    for (int f = tid; f < F; f += 256) si0[f] = it.i0[f];
    if (tid < MG_SLEN_TILE) sbad[tid] = 0;
    __syncthreads();
    for (int e = tid; e < ncand * L; e += 256) {
        const int c = e / L, k = e - c * L;
        const double s = mg_load_lat<LAT_F64>(it.lat, (b0 + c) * it.ld + k);
        slat[e] = s;
        if (!isfinite(s)) sbad[c] = 1;          // (every writer stores the same value)
    }
    __syncthreads();

    // phase 1: control points of the root rows
    for (int e = tid; e < ncand * NR; e += 256) {
        const int c = e / NR, j = e - c * NR;
        const double *s = slat + c * L;
        scp[e] = mg_control_point(smean[j], sE + j, (size_t)NR, L, [&](int k) { return s[k]; });
    }
    __syncthreads();

    // phase 2: the segments' ground-plane lengths (the positions live in registers; a frame's x and z are formed by both segments it ends)
    for (int e = tid; e < ncand * (F - 1); e += 256) {
        const int c = e / (F - 1), f = e - c * (F - 1) + 1;
        const double *cp = scp + c * NR;
        const double x1 = mg_slen_position(cp, sw, si0, f, 0), z1 = mg_slen_position(cp, sw, si0, f, 2);
        const double x0 = mg_slen_position(cp, sw, si0, f - 1, 0), z0 = mg_slen_position(cp, sw, si0, f - 1, 2);
        const double dx = x1 - x0, dz = z1 - z0;
        const double xx = dx * dx, zz = dz * dz;
        sseg[c * FS + f] = sqrt(xx + zz);
    }
    __syncthreads();

    // phase 3: one lane per candidate
    if (tid < ncand) {
        const double *seg = sseg + tid * FS;
        double arc = 0.0;
        if (F > 1) {
            arc = seg[1];
            for (int f = 2; f < F; f++) arc = arc + seg[f];
        }
        const double *cp = scp + tid * NR;
        const double dx = mg_slen_position(cp, sw, si0, F - 1, 0) - mg_slen_position(cp, sw, si0, 0, 0);
        const double dy = mg_slen_position(cp, sw, si0, F - 1, 1) - mg_slen_position(cp, sw, si0, 0, 1);
        const double dz = mg_slen_position(cp, sw, si0, F - 1, 2) - mg_slen_position(cp, sw, si0, 0, 2);
        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
        double dist = sqrt((xx + yy) + zz);
        if (sbad[tid]) { arc = NAN; dist = NAN; }
        if (it.arc) it.arc[b0 + tid] = arc;
        if (it.dist) it.dist[b0 + tid] = dist;
    }
}

#define MG_SLEN_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)
#define MG_SLEN_REFUSE(cond, ...) MG_REQUIRE_AS(!(cond), MG_ERR_UNSUPPORTED, __VA_ARGS__)

// the checks both entry points make of an item table (nothing is launched or copied before they pass)
static int mg_slen_check(const char *who, int32_t n_items, const mg_step_length_item *items, int latent_dtype) {
    MG_SLEN_REQUIRE(n_items >= 0 && (n_items == 0 || items), "%s: %d items, or NULL item table", who, n_items);
    MG_SLEN_REQUIRE(latent_dtype == MG_F32 || latent_dtype == MG_F64, "%s: bad latent dtype %d", who, latent_dtype);
    const mg_context *ctx = nullptr;
    for (int i = 0; i < n_items; i++) {
        const mg_step_length_item &q = items[i];
        const mg_primitive *p = q.prim;
        MG_SLEN_REQUIRE(p != nullptr, "%s: item %d: the primitive is NULL", who, i);
        if (!ctx) ctx = p->ctx;
        MG_SLEN_REQUIRE(p->ctx == ctx, "%s: item %d: the primitive belongs to another context", who, i);
        MG_SLEN_REQUIRE(q.n_samples >= 0 && q.ld >= 0, "%s: item %d: %lld samples, ld %lld", who, i, (long long)q.n_samples, (long long)q.ld);
        MG_SLEN_REQUIRE(q.latent_offset >= 0 && q.latent_offset + p->L <= q.ld, "%s: item %d reads latent columns %lld .. %lld of %lld", who, i,
                        (long long)q.latent_offset, (long long)(q.latent_offset + p->L), (long long)q.ld);
        MG_SLEN_REQUIRE(q.arc_length_dev || q.distance_dev, "%s: item %d: both outputs are NULL", who, i);
        MG_SLEN_REQUIRE(q.n_samples == 0 || q.latents_dev, "%s: item %d: the latents are NULL", who, i);
    }
    for (int i = 0; i < n_items; i++) {
        const mg_primitive *p = items[i].prim;
        const mg_time_grid *g = p->canonical;
        MG_SLEN_REFUSE(p->D < 3 || !g || g->T < 1 || g->T != p->F || !p->d_Et64 || !p->d_mean || !g->d_i0 || !g->d_w,
                       "%s: item %d: the primitive has no root path (%d channels, %d canonical frames)", who, i, p->D, p->F);
        for (int f = 0; f < g->T; f++)
            MG_SLEN_REFUSE(g->i0[f] < 0 || g->i0[f] + 4 > p->NB, "%s: item %d: frame %d takes control points %d .. %d of %d", who, i, f, g->i0[f],
                           g->i0[f] + 3, p->NB);
        MG_SLEN_REFUSE((int64_t)p->L * 3 * p->NB > (1 << 20) || p->F > (1 << 16) || mg_slen_layout_of(p->L, p->NB, p->F).total_bytes > MG_SLEN_LDS_MAX,
                       "%s: item %d: the root tables (%d x %d control points, %d frames) do not fit LDS", who, i, p->L, 3 * p->NB, p->F);
        MG_SLEN_REFUSE((items[i].n_samples + MG_SLEN_TILE - 1) / MG_SLEN_TILE > 0x7fffffff, "%s: item %d: too many samples", who, i);
    }
    return MG_OK;
}

extern "C" int mg_step_lengths(int32_t n_items, const mg_step_length_item *items, int latent_dtype) {
    int rc = mg_slen_check("mg_step_lengths", n_items, items, latent_dtype);
    if (rc != MG_OK) return rc;
    const size_t elem = latent_dtype == MG_F64 ? 8 : 4;
    // the non-empty items, cut into launches: at most MG_STEP_LENGTH_MAX_ITEMS items and 2^31 - 1 workgroups each
    std::vector<mg_slen_item> ds;
    struct launch { size_t first; int32_t n_items; int64_t grid; int lds; };
    std::vector<launch> launches;
    mg_context *ctx = nullptr;
    for (int i = 0; i < n_items; i++) {
        const mg_step_length_item &q = items[i];
        if (q.n_samples == 0) continue;
        mg_primitive *p = q.prim;
        ctx = p->ctx;
        const int64_t wgs = (q.n_samples + MG_SLEN_TILE - 1) / MG_SLEN_TILE;
        if (launches.empty() || launches.back().n_items == MG_STEP_LENGTH_MAX_ITEMS || launches.back().grid + wgs > 0x7fffffff)
            launches.push_back({ds.size(), 0, 0, 0});
        launch &l = launches.back();
        mg_slen_item d;
        memset(&d, 0, sizeof(d));
        d.Et = p->d_Et64; d.mean = p->d_mean; d.i0 = p->canonical->d_i0; d.w = p->canonical->d_w;
        d.lat = (const char *)q.latents_dev + (size_t)q.latent_offset * elem;
        d.arc = q.arc_length_dev; d.dist = q.distance_dev;
        d.n = q.n_samples; d.ld = q.ld;
        d.F = p->F; d.L = p->L; d.NB = p->NB; d.D = p->D; d.R = p->R;
        d.wg0 = (int32_t)l.grid;
        ds.push_back(d);
        l.n_items++;
        l.grid += wgs;
        l.lds = std::max(l.lds, mg_slen_layout_of(p->L, p->NB, p->F).total_bytes);
    }
    if (ds.empty()) return MG_OK;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[MG_TABLE_STEP_LENGTH];
    const size_t tab_bytes = ds.size() * sizeof(mg_slen_item);
    rc = dt.upload(ctx, "mg_step_lengths", ds.data(), tab_bytes, std::max(tab_bytes * 2, (size_t)32 * 1024));
    if (rc != MG_OK) return rc;
    for (const launch &l : launches) {
        mg_slen_args k;
        k.items = (const mg_slen_item *)dt.base() + l.first;
        k.n_items = l.n_items;
        if (l.lds > 64 * 1024) {
            if (latent_dtype == MG_F64) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_STEP_LENGTH_F64, 160 * 1024, mg_step_length_kernel<true>));
            else MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_STEP_LENGTH_F32, 160 * 1024, mg_step_length_kernel<false>));
        }
        mg_prof_begin(ctx, MG_PROF_STEP_LENGTHS);
        if (latent_dtype == MG_F64) hipLaunchKernelGGL(mg_step_length_kernel<true>, dim3((unsigned)l.grid), dim3(256), l.lds, ctx->stream, k);
        else hipLaunchKernelGGL(mg_step_length_kernel<false>, dim3((unsigned)l.grid), dim3(256), l.lds, ctx->stream, k);
        mg_prof_end(ctx, MG_PROF_STEP_LENGTHS);
        MG_HIP_CHECK(hipGetLastError());
    }
    return MG_OK;
}

// host arrays in, host arrays out: one device block for the call, synchronises.  Items that name the same latent matrix (same
// pointer, rows and ld: the steps of a walk) share one copy of it.
extern "C" int mg_step_lengths_host(int32_t n_items, const mg_step_length_item *items, int latent_dtype) {
    int rc = mg_slen_check("mg_step_lengths_host", n_items, items, latent_dtype);
    if (rc != MG_OK) return rc;
    const size_t elem = latent_dtype == MG_F64 ? 8 : 4;
    mg_context *ctx = nullptr;
    std::vector<mg_step_length_item> dev(items, items + n_items);
    std::vector<size_t> o_lat((size_t)n_items, 0), o_arc((size_t)n_items, 0), o_dist((size_t)n_items, 0);
    std::vector<int> lat_of((size_t)n_items, -1);      // the earlier item whose copy of the latents this one reads
    for (int i = 0; i < n_items; i++) {
        if (items[i].n_samples == 0) continue;
        ctx = items[i].prim->ctx;
    }
    if (!ctx) return MG_OK;
    mg_workspace ws(ctx, "mg_step_lengths_host");
    for (int i = 0; i < n_items; i++) {
        const mg_step_length_item &q = items[i];
        if (q.n_samples == 0) continue;
        for (int j = 0; j < i && lat_of[i] < 0; j++)
            if (items[j].n_samples == q.n_samples && items[j].latents_dev == q.latents_dev && items[j].ld == q.ld) lat_of[i] = lat_of[j] >= 0 ? lat_of[j] : j;
        if (lat_of[i] < 0) o_lat[i] = ws.carve((size_t)(q.n_samples * q.ld) * elem);
        if (q.arc_length_dev) o_arc[i] = ws.carve((size_t)q.n_samples * 8);
        if (q.distance_dev) o_dist[i] = ws.carve((size_t)q.n_samples * 8);
    }
    if ((rc = ws.alloc()) != MG_OK) return rc;
    for (int i = 0; i < n_items; i++) {
        const mg_step_length_item &q = items[i];
        if (q.n_samples == 0) continue;
        if (lat_of[i] < 0)
            MG_HIP_CHECK(hipMemcpyAsync(ws.at<char>(o_lat[i]), q.latents_dev, (size_t)(q.n_samples * q.ld) * elem, hipMemcpyHostToDevice, ctx->stream));
        dev[i].latents_dev = ws.at<void>(o_lat[lat_of[i] < 0 ? i : lat_of[i]]);
        dev[i].arc_length_dev = q.arc_length_dev ? ws.at<double>(o_arc[i]) : nullptr;
        dev[i].distance_dev = q.distance_dev ? ws.at<double>(o_dist[i]) : nullptr;
    }
    if ((rc = mg_step_lengths(n_items, dev.data(), latent_dtype)) != MG_OK) return rc;
    for (int i = 0; i < n_items; i++) {
        const mg_step_length_item &q = items[i];
        if (q.n_samples == 0) continue;
        if (q.arc_length_dev) MG_HIP_CHECK(hipMemcpyAsync(q.arc_length_dev, ws.at<char>(o_arc[i]), (size_t)q.n_samples * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (q.distance_dev) MG_HIP_CHECK(hipMemcpyAsync(q.distance_dev, ws.at<char>(o_dist[i]), (size_t)q.n_samples * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}
