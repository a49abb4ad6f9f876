// Step lengths without frames in memory (gfx950 / MI355X), float64: the ground-plane arc length of the root path over a primitive's
// canonical frames and the distance between its first and last root position, for every candidate of every item, in ONE launch.
//
// What MotionStateGraphNode.get_step_length_for_sample (reference motion_state_graph_node.py:208-230) takes from a whole
// back-projected motion needs the root's three channels alone: 3 x n_basis control points per candidate.  A workgroup owns up to
// MG_SLEN_TILE candidates of ONE item and keeps everything between the latents and the two results in LDS:
//
//   constants   the item's 3 n_basis root rows of E' as [L][3 n_basis], their means, the canonical grid's tap rows: once per workgroup
//   phase 1     control points  c[cand][i * 3 + d] of the root rows (mg_item_control_points)
//   phase 2     segments        one (candidate, frame) per thread: the positions p[f][d] = w0 c0, then fma(w_j, c_j, .) for j = 1, 2, 3
//               (mg_taps4) of the segment's two ends in registers, d_f = sqrt(dx * dx + dz * dz), every
//               operation rounded on its own
//   phase 3     one lane per candidate adds d_1 .. d_{F-1} in frame order and states the distance; the only stores to global memory
//
// The launch shape -- which workgroup serves which item, the items' device table (ctx->tab[MG_TABLE_STEP_LENGTH]), the slices of
// MG_STEP_LENGTH_MAX_ITEMS items, the _host twin -- is mg_items.h's.
#include <cmath>
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_frames_common.h"
#include "mg_items.h"
#include "mg_step_length_layout.h"   // MG_SLEN_TILE, MG_SLEN_LDS_MAX, mg_slen_layout_of: the workgroup's LDS, host-only

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
    const mg_slen_item it = a.items[mg_item_of_workgroup(a.items, a.n_items)];
    const int L = it.L, F = it.F, D = it.D;
    const mg_slen_layout y = mg_slen_layout_of(L, it.NB, F);
    const int NR = y.NR, FS = y.FS;
    double *sm = (double *)smem;
    double *sE = sm + y.E, *smean = sm + y.mean, *sw = sm + y.w, *slat = sm + y.lat, *scp = sm + y.cp, *sseg = sm + y.seg;
    int32_t *si0 = (int32_t *)(sm + y.ints), *sbad = si0 + F;
    int ncand;
    const int64_t b0 = mg_item_tile_of<MG_SLEN_TILE>(it.wg0, it.n, ncand);

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
    mg_item_stage_latents<LAT_F64>(it.lat, it.ld, b0, ncand, L, slat, sbad);
    __syncthreads();

    // phase 1: control points of the root rows
    mg_item_control_points(smean, sE, slat, ncand, NR, L, scp, NR);
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

// the checks both entry points make of an item table (nothing is launched or copied before they pass)
static int mg_slen_check(const char *who, int32_t n_items, const mg_step_length_item *items, int latent_dtype) {
    const int rc = mg_items_check(
        who, n_items, items, latent_dtype,
        [&](int i, const mg_step_length_item &q) -> int {
            MG_ITEM_REQUIRE(q.arc_length_dev || q.distance_dev, "%s: item %d: both outputs are NULL", who, i);
            return MG_OK;
        },
        [](int, const mg_step_length_item &) { return (int)MG_OK; });
    if (rc != MG_OK) return rc;
    for (int i = 0; i < n_items; i++) {
        const mg_primitive *p = items[i].prim;
        const mg_time_grid *g = p->canonical;
        MG_ITEM_REFUSE(p->D < 3 || !g || g->T < 1 || g->T != p->F || !p->d_Et64 || !p->d_mean || !g->d_i0 || !g->d_w,
                       "%s: item %d: the primitive has no root path (%d channels, %d canonical frames)", who, i, p->D, p->F);
        for (int f = 0; f < g->T; f++)
            MG_ITEM_REFUSE(g->i0[f] < 0 || g->i0[f] + 4 > p->NB, "%s: item %d: frame %d takes control points %d .. %d of %d", who, i, f, g->i0[f],
                           g->i0[f] + 3, p->NB);
        // (the first two never refuse on their own: 8 L 3 NB bytes past 2^20 entries, or 160 F bytes past 2^16 frames, are megabytes
        // beyond MG_SLEN_LDS_MAX, and tests/step_length_cases.py's sweep is refused by the LDS limit at L 56, NB 64, F 209.  They stand in
        // front of mg_slen_layout_of so that its int arithmetic cannot overflow into a size that passes)
        MG_ITEM_REFUSE((int64_t)p->L * 3 * p->NB > (1 << 20) || p->F > (1 << 16) || mg_slen_layout_of(p->L, p->NB, p->F).total_bytes > MG_SLEN_LDS_MAX,
                       "%s: item %d: the root tables (%d x %d control points, %d frames) do not fit LDS", who, i, p->L, 3 * p->NB, p->F);
        MG_ITEM_REFUSE_GRID(who, i, items[i].n_samples, MG_SLEN_TILE);
    }
    return MG_OK;
}

extern "C" int mg_step_lengths(int32_t n_items, const mg_step_length_item *items, int latent_dtype) {
    const int rc = mg_slen_check("mg_step_lengths", n_items, items, latent_dtype);
    if (rc != MG_OK) return rc;
    const size_t elem = latent_dtype == MG_F64 ? 8 : 4;
    std::vector<int32_t> wg0;
    const std::vector<mg_item_launch> launches = mg_cut_items(
        n_items, [&](int i) { return items[i].n_samples; },
        [&](int i) { return mg_slen_layout_of(items[i].prim->L, items[i].prim->NB, items[i].prim->F).total_bytes; }, MG_SLEN_TILE, MG_STEP_LENGTH_MAX_ITEMS, wg0);
    if (launches.empty()) return MG_OK;
    std::vector<mg_slen_item> ds;        // the non-empty items
    mg_context *ctx = nullptr;
    for (int i = 0; i < n_items; i++) {
        const mg_step_length_item &q = items[i];
        if (q.n_samples == 0) continue;
        mg_primitive *p = q.prim;
        ctx = p->ctx;
        mg_slen_item d;
        memset(&d, 0, sizeof(d));
        d.Et = p->d_Et64; d.mean = p->d_mean; d.i0 = p->canonical->d_i0; d.w = p->canonical->d_w;
        d.lat = (const char *)q.latents_dev + (size_t)q.latent_offset * elem;
        d.arc = q.arc_length_dev; d.dist = q.distance_dev;
        d.n = q.n_samples; d.ld = q.ld;
        d.F = p->F; d.L = p->L; d.NB = p->NB; d.D = p->D; d.R = p->R;
        d.wg0 = wg0[i];
        ds.push_back(d);
    }
    const size_t tab_bytes = ds.size() * sizeof(mg_slen_item);
    return mg_items_launch(
        ctx, "mg_step_lengths", ctx->tab[MG_TABLE_STEP_LENGTH], ds.data(), tab_bytes, std::max(tab_bytes * 2, (size_t)32 * 1024), launches, latent_dtype,
        MG_LDS_STEP_LENGTH_F32, MG_LDS_STEP_LENGTH_F64, MG_PROF_STEP_LENGTHS, [](auto LAT_F64) { return mg_step_length_kernel<decltype(LAT_F64)::value>; },
        [](const char *base, const mg_item_launch &l) { return mg_slen_args{(const mg_slen_item *)base + l.first, l.n_items}; });
}

extern "C" int mg_step_lengths_host(int32_t n_items, const mg_step_length_item *items, int latent_dtype) {
    const int rc = mg_slen_check("mg_step_lengths_host", n_items, items, latent_dtype);
    if (rc != MG_OK) return rc;
    const mg_item_output<mg_step_length_item> outs[2] = {{&mg_step_length_item::arc_length_dev, 1, nullptr}, {&mg_step_length_item::distance_dev, 1, nullptr}};
    return mg_items_host("mg_step_lengths_host", n_items, items, latent_dtype, outs,
                         [&](const mg_step_length_item *dev) { return mg_step_lengths(n_items, dev, latent_dtype); });
}
