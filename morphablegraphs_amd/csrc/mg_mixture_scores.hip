// Targets against the reachability mixtures of many nodes (gfx950 / MI355X), float64: the weighted log-probabilities, log p and the
// reachable flag of every target of every item, in ONE launch.  The statements are mg_mixture_image.h's; the launch shape -- which
// workgroup serves which item, the slices of MG_MIXTURE_SCORES_MAX_ITEMS items, the device table -- is mg_items_cut.h's.
//
// A workgroup is ONE wave and owns up to MG_MIX_TILE = 64 targets of one item, a target per lane.  Everything a lane needs of the
// mixture is wave-uniform, so a factor's entry is read once per wave, and plain float64 FMAs do the work: the statement fixes each
// y_j as one fma chain in ascending i, which a 16x16x4 MFMA tile neither keeps (its k-steps accumulate inside the instruction) nor
// fills (the factor is a triangle, and at 3 or 4 dimensions 13 of a tile's 16 columns would be padding).  By dimension:
//
//   dim <= 4, dim <= 8   the target's coordinates in registers (the loops unrolled to 4 or 8), the whole mixture -- at most 64 blocks of
//                        45 doubles, 23 KB -- staged into LDS once per workgroup and read as broadcasts.  Pass 1 finds the largest
//                        wlp_k (and stores the row where asked), pass 2 forms every wlp_k again for the sum of exp: a dozen FMAs
//                        against an exp, and no per-target storage at all.
//   dim >= 9             the tile's targets in LDS, coordinate-major ([dim][65]: a lane reads its own column without a bank
//                        conflict), the factors streamed from global memory through L2 with wave-uniform addresses.  Four components
//                        advance together, so one LDS read of x_i feeds four independent fma chains; wlp_k waits in LDS ([K][64])
//                        for the sum.  At 96 dimensions and 64 components that is 81 KB: above 64 KB the kernel takes the
//                        large-LDS opt-in, and nothing within the caps is refused.
//
// Every result leaves through vector stores, one lane per target.
#include <cmath>
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_items.h"
#include "mg_mixture_image.h"

struct mg_feature_mixture : mg_mixture_image {
    mg_context *ctx = nullptr;           // NULL: no device copy (mg_mixture_scores_host only)
    double *d_blocks = nullptr;
};

struct mg_mix_item {                     // one non-empty item as the kernel reads it
    const double *blocks;                // the mixture's image on the device
    const double *x;                     // the item's first coordinate: target t at x + t * ld
    double *logp, *wlp;                  // (n), (n, K) or NULL
    int32_t *reach;                      // (n) or NULL
    double threshold;
    int64_t n, ld;
    int32_t K, dim, route;
    int32_t wg0;                         // first workgroup of the item in its launch
};

struct mg_mix_args {
    const mg_mix_item *items;            // the launch's slice of the table
    int32_t n_items;
};

// what a lane leaves of its target
__device__ __forceinline__ void mg_mix_store(const mg_mix_item &it, int64_t t, double logp) {
    if (it.logp) it.logp[t] = logp;
    if (it.reach) it.reach[t] = mg_mix_reachable(logp, it.threshold);
}

template <int DMAX>
__device__ __forceinline__ void mg_mix_registers(const mg_mix_item &it, double *sblk, int64_t b0, int ncand) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, K = it.K, dim = it.dim, stride = mg_mix_stride(dim);
    for (int e = lane; e < K * stride; e += MG_MIX_TILE) sblk[e] = it.blocks[e];
    __syncthreads();
    if (lane >= ncand) return;
    const int64_t t = b0 + lane;
    double x[DMAX];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < DMAX; i++) {
        x[i] = i < dim ? it.x[t * it.ld + i] : 0.0;
        bad = bad || !isfinite(x[i]);
    }
    auto wlp = [&](int k) { return mg_mix_wlp_unrolled<DMAX>(sblk + k * stride, dim, [&](int i) { return x[i]; }); };
    if (it.wlp)
        for (int k = 0; k < K; k++) it.wlp[t * K + k] = bad ? NAN : wlp(k);
    if (it.logp || it.reach) mg_mix_store(it, t, bad ? NAN : mg_mix_logp(K, wlp));
}

__device__ __forceinline__ void mg_mix_stream(const mg_mix_item &it, double *sm, int64_t b0, int ncand) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, K = it.K, dim = it.dim, tri = mg_mix_tri(dim), stride = mg_mix_stride(dim);
    double *sx = sm, *swlp = sm + dim * MG_MIX_XS;
    for (int e = lane; e < MG_MIX_TILE * dim; e += MG_MIX_TILE) {           // consecutive lanes read consecutive doubles where ld == dim
        const int c = e / dim, i = e - c * dim;
        sx[i * MG_MIX_XS + c] = c < ncand ? it.x[(b0 + c) * it.ld + i] : 0.0;
    }
    __syncthreads();
    const double *xl = sx + lane;
    bool bad = false;
    for (int i = 0; i < dim; i++) bad = bad || !isfinite(xl[i * MG_MIX_XS]);
    const int64_t t = b0 + lane;
    for (int k0 = 0; k0 < K; k0 += 4) {
        // four components side by side (past the last one: the last one again, not kept); each chain is mg_mix_wlp's
        const double *blk[4];
        double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 4; b++) blk[b] = it.blocks + (size_t)(k0 + b < K ? k0 + b : K - 1) * stride;
        for (int j = 0; j < dim; j++) {
            const int at = j * (j + 1) / 2;
            double acc[4];
            const double x0 = xl[0];
#pragma unroll
            for (int b = 0; b < 4; b++) acc[b] = x0 * blk[b][at];
            for (int i = 1; i <= j; i++) {
                const double xi = xl[i * MG_MIX_XS];
#pragma unroll
                for (int b = 0; b < 4; b++) acc[b] = fma(xi, blk[b][at + i], acc[b]);
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const double y = acc[b] - blk[b][tri + j];
                q[b] = j == 0 ? y * y : fma(y, y, q[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (k0 + b < K) {
                const double w = bad ? NAN : fma(-0.5, q[b], blk[b][tri + dim]);
                swlp[(k0 + b) * MG_MIX_TILE + lane] = w;
                if (it.wlp && lane < ncand) it.wlp[t * K + k0 + b] = w;
            }
    }
    if (lane >= ncand || !(it.logp || it.reach)) return;
    mg_mix_store(it, t, bad ? NAN : mg_mix_logp(K, [&](int k) { return swlp[k * MG_MIX_TILE + lane]; }));
}

__global__ __launch_bounds__(MG_MIX_TILE) void mg_mixture_scores_kernel(const mg_mix_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const mg_mix_item it = a.items[mg_item_of_workgroup(a.items, a.n_items)];
    int ncand;
    const int64_t b0 = mg_item_tile_of<MG_MIX_TILE>(it.wg0, it.n, ncand);
    if (it.route == MG_MIX_ROUTE_REG4) mg_mix_registers<4>(it, (double *)smem, b0, ncand);
    else if (it.route == MG_MIX_ROUTE_REG8) mg_mix_registers<8>(it, (double *)smem, b0, ncand);
    else mg_mix_stream(it, (double *)smem, b0, ncand);
}

// ---- the mixture ------------------------------------------------------------------------------------------------------------------
extern "C" int mg_feature_mixture_create(mg_context *ctx, int32_t n_components, int32_t dim, const double *weights, const double *means,
                                         const double *covars, double threshold, mg_feature_mixture **out) {
    MG_REQUIRE(out != nullptr, "mg_feature_mixture_create: out is NULL");
    *out = nullptr;
    mg_mixture_image img;
    const int rc = mg_mixture_image_build("mg_feature_mixture_create", n_components, dim, weights, means, covars, threshold, img);
    if (rc != MG_OK) return rc;
    mg_feature_mixture *m = new mg_feature_mixture();
    static_cast<mg_mixture_image &>(*m) = std::move(img);
    m->ctx = ctx;
    if (ctx) {
        const size_t bytes = m->blocks.size() * sizeof(double);
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipMalloc((void **)&m->d_blocks, bytes);
        if (e == hipSuccess) e = hipMemcpy(m->d_blocks, m->blocks.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (m->d_blocks) (void)hipFree(m->d_blocks);
            delete m;
            return mg_hip_fail(e, "mg_feature_mixture_create: the image's device copy");
        }
    }
    *out = m;
    return MG_OK;
}

extern "C" void mg_feature_mixture_destroy(mg_feature_mixture *m) {
    if (!m) return;
    if (m->d_blocks) {
        (void)hipStreamSynchronize(m->ctx->stream);      // a launch that reads the image may still be in flight
        (void)hipFree(m->d_blocks);
    }
    delete m;
}

extern "C" int mg_feature_mixture_info(const mg_feature_mixture *m, int32_t *n_components, int32_t *dim, double *threshold) {
    MG_REQUIRE(m != nullptr, "mg_feature_mixture_info: the mixture is NULL");
    if (n_components) *n_components = m->K;
    if (dim) *dim = m->dim;
    if (threshold) *threshold = m->threshold;
    return MG_OK;
}

extern "C" int mg_feature_mixture_get_image(const mg_feature_mixture *m, double *prec_chol, double *mean_prec, double *log_const) {
    MG_REQUIRE(m != nullptr, "mg_feature_mixture_get_image: the mixture is NULL");
    const int dim = m->dim, tri = mg_mix_tri(dim), stride = mg_mix_stride(dim);
    for (int k = 0; k < m->K; k++) {
        const double *blk = m->blocks.data() + (size_t)k * stride;
        if (prec_chol)
            for (int i = 0; i < dim; i++)
                for (int j = 0; j < dim; j++) prec_chol[((size_t)k * dim + i) * dim + j] = i <= j ? blk[j * (j + 1) / 2 + i] : 0.0;
        if (mean_prec) memcpy(mean_prec + (size_t)k * dim, blk + tri, (size_t)dim * sizeof(double));
        if (log_const) log_const[k] = blk[tri + dim];
    }
    return MG_OK;
}

// ---- the scores -------------------------------------------------------------------------------------------------------------------
// the checks both entry points make of an item table (nothing is launched, copied or written before they pass); ctx: the context every
// mixture must have a device copy on, or NULL for the host twin, which asks for none
static int mg_mix_check(const char *who, const mg_context *ctx, bool device, int32_t n_items, const mg_mixture_score_item *items) {
    MG_ITEM_REQUIRE(!device || ctx, "%s: the context is NULL", who);
    MG_ITEM_REQUIRE(n_items >= 0 && (n_items == 0 || items), "%s: %d items, or NULL item table", who, n_items);
    for (int i = 0; i < n_items; i++) {
        const mg_mixture_score_item &q = items[i];
        const mg_feature_mixture *m = q.mixture;
        MG_ITEM_REQUIRE(m != nullptr, "%s: item %d: the mixture is NULL", who, i);
        if (device) {
            MG_ITEM_REQUIRE(m->d_blocks != nullptr, "%s: item %d: the mixture has no device copy", who, i);
            MG_ITEM_REQUIRE(m->ctx == ctx, "%s: item %d: the mixture belongs to another context", who, i);
        }
        MG_ITEM_REQUIRE(q.n_targets >= 0 && q.ld >= 0, "%s: item %d: %lld targets, ld %lld", who, i, (long long)q.n_targets, (long long)q.ld);
        MG_ITEM_REQUIRE(q.target_offset >= 0 && q.target_offset + m->dim <= q.ld, "%s: item %d reads target columns %lld .. %lld of %lld", who, i,
                        (long long)q.target_offset, (long long)(q.target_offset + m->dim), (long long)q.ld);
        MG_ITEM_REQUIRE(q.logp_dev || q.wlp_dev || q.reachable_dev, "%s: item %d: all outputs are NULL", who, i);
        MG_ITEM_REQUIRE(q.n_targets == 0 || q.targets_dev, "%s: item %d: the targets are NULL", who, i);
        MG_ITEM_REFUSE_GRID(who, i, q.n_targets, MG_MIX_TILE);
    }
    return MG_OK;
}

extern "C" int mg_mixture_scores(mg_context *ctx, int32_t n_items, const mg_mixture_score_item *items) {
    const char *who = "mg_mixture_scores";
    const int rc = mg_mix_check(who, ctx, true, n_items, items);
    if (rc != MG_OK) return rc;
    std::vector<int32_t> wg0;
    const std::vector<mg_item_launch> launches = mg_cut_items(
        n_items, [&](int i) { return items[i].n_targets; }, [&](int i) { return mg_mix_lds_of(items[i].mixture->K, items[i].mixture->dim); }, MG_MIX_TILE,
        MG_MIXTURE_SCORES_MAX_ITEMS, wg0);
    if (launches.empty()) return MG_OK;
    std::vector<mg_mix_item> ds;         // the non-empty items
    for (int i = 0; i < n_items; i++) {
        const mg_mixture_score_item &q = items[i];
        if (q.n_targets == 0) continue;
        mg_mix_item d;
        memset((void *)&d, 0, sizeof(d));
        d.blocks = q.mixture->d_blocks;
        d.x = q.targets_dev + q.target_offset;
        d.logp = q.logp_dev; d.wlp = q.wlp_dev; d.reach = q.reachable_dev;
        d.threshold = q.mixture->threshold;
        d.n = q.n_targets; d.ld = q.ld;
        d.K = q.mixture->K; d.dim = q.mixture->dim; d.route = mg_mix_route_of(d.dim);
        d.wg0 = wg0[(size_t)i];
        ds.push_back(d);
    }
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[MG_TABLE_MIXTURE_SCORES];
    const size_t tab_bytes = ds.size() * sizeof(mg_mix_item);
    const int urc = dt.upload(ctx, who, ds.data(), tab_bytes, std::max(tab_bytes * 2, (size_t)32 * 1024));
    if (urc != MG_OK) return urc;
    for (const mg_item_launch &l : launches) {
        if (l.lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_MIXTURE_SCORES, 160 * 1024, mg_mixture_scores_kernel));
        mg_prof_begin(ctx, MG_PROF_MIXTURE_SCORES);
        hipLaunchKernelGGL(mg_mixture_scores_kernel, dim3((unsigned)l.grid), dim3(MG_MIX_TILE), l.lds, ctx->stream,
                           mg_mix_args{(const mg_mix_item *)dt.base() + l.first, l.n_items});
        mg_prof_end(ctx, MG_PROF_MIXTURE_SCORES);
        MG_HIP_CHECK(hipGetLastError());
    }
    return MG_OK;
}

extern "C" int mg_mixture_scores_host(mg_context *ctx, int32_t n_items, const mg_mixture_score_item *items) {
    const int rc = mg_mix_check("mg_mixture_scores_host", ctx, false, n_items, items);
    if (rc != MG_OK) return rc;
    std::vector<double> w;
    for (int i = 0; i < n_items; i++) {
        const mg_mixture_score_item &q = items[i];
        const mg_feature_mixture *m = q.mixture;
        const int K = m->K, dim = m->dim, stride = mg_mix_stride(dim);
        w.resize((size_t)K);
        for (int64_t t = 0; t < q.n_targets; t++) {
            const double *x = q.targets_dev + t * q.ld + q.target_offset;
            bool bad = false;
            for (int c = 0; c < dim; c++) bad = bad || !std::isfinite(x[c]);
            for (int k = 0; k < K; k++) w[(size_t)k] = bad ? NAN : mg_mix_wlp(m->blocks.data() + (size_t)k * stride, dim, [&](int c) { return x[c]; });
            const double logp = bad ? NAN : mg_mix_logp(K, [&](int k) { return w[(size_t)k]; });
            if (q.wlp_dev) memcpy(q.wlp_dev + t * K, w.data(), (size_t)K * sizeof(double));
            if (q.logp_dev) q.logp_dev[t] = logp;
            if (q.reachable_dev) q.reachable_dev[t] = mg_mix_reachable(logp, m->threshold);
        }
    }
    return MG_OK;
}
