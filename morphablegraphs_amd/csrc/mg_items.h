// What the item-table entry points share (mg_step_length.hip, mg_feature_points.hip): a call brings a table of items -- one
// primitive, one latent matrix, its outputs each -- and every candidate of every item is served by ONE launch.
//
// The launch shape.  A workgroup of 256 threads owns up to TILE candidates of ONE item and keeps everything between the latents and
// the outputs in LDS.  Which workgroup serves which item is a prefix table (wg0, the first workgroup of every item) searched by
// bisection.  A candidate's values are computed by statements that see nothing but its own row, so they depend on neither the batch
// nor the other items.  The non-empty items of a call travel in a device table of the context (ctx->tab[]), rewritten only when it
// differs from the last call's; a launch takes a slice of it, a call with more items than a launch holds goes through the table in
// slices (mg_items_cut.h: the cut, the bisection, the table's layout and the shared-latents search as host-only code).  An entry point
// fills its own kernel-side item and names the arrays that travel behind the items (mg_items_table); the rest is here.
#pragma once
#include "mg_construct.h"
#include "mg_items_cut.h"
#include "mg_spline_device.h"

#define MG_ITEM_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)
#define MG_ITEM_REFUSE(cond, ...) MG_REQUIRE_AS(!(cond), MG_ERR_UNSUPPORTED, __VA_ARGS__)
#define MG_ITEM_REFUSE_GRID(who, i, n, tile) MG_ITEM_REFUSE(((n) + (tile) - 1) / (tile) > 0x7fffffff, "%s: item %d: too many samples", who, i)

// the item of this workgroup: the last one whose first workgroup is not past it
template <class Item>
__device__ __forceinline__ int mg_item_of_workgroup(const Item *items, int n_items) {
    return mg_item_at(items, n_items, (int)blockIdx.x);
}

// the workgroup's candidates: b0 (returned) .. b0 + ncand of the item's n
template <int TILE>
__device__ __forceinline__ int64_t mg_item_tile_of(int32_t wg0, int64_t n, int &ncand) {
    const int64_t b0 = (int64_t)((int)blockIdx.x - wg0) * TILE;
    ncand = (int)((n - b0) < TILE ? (n - b0) : TILE);
    return b0;
}

// the tile's latents into slat[ncand][L]; sbad[c] (zeroed before the barrier in front of this) marks a candidate with a non-finite one
template <bool LAT_F64>
__device__ __forceinline__ void mg_item_stage_latents(const void *lat, int64_t ld, int64_t b0, int ncand, int L, double *slat, int32_t *sbad) {
    for (int e = threadIdx.x; e < ncand * L; e += 256) {
        const int c = e / L, k = e - c * L;
        const double s = mg_load_lat<LAT_F64>(lat, (b0 + c) * ld + k);
        slat[e] = s;
        if (!isfinite(s)) sbad[c] = 1;          // (every writer stores the same value)
    }
}

// phase 1: control points c[cand * CS + row] = mean', then fma(E'[k][.], s[k], .) for k ascending (mg_control_point) over the item's
// NR staged rows (sE[L][NR], smean[NR]); one (candidate, row) per thread: consecutive lanes read consecutive doubles of E', the latent
// is a broadcast.  A kernel that keeps some waves for other work names the first of the `stride` threads that take part
__device__ __forceinline__ void mg_item_control_points(const double *smean, const double *sE, const double *slat, int ncand, int NR, int L, double *scp, int CS,
                                                       int first = threadIdx.x, int stride = 256) {
    for (int e = first; e < ncand * NR; e += stride) {
        const int c = e / NR, j = e - c * NR;
        const double *s = slat + c * L;
        scp[c * CS + j] = mg_control_point(smean[j], sE + j, (size_t)NR, L, [&](int k) { return s[k]; });
    }
}

// The argument checks every item table gets, on the members all public item structs share (prim, n_samples, ld, latent_offset,
// latents_dev); the entry point's own checks of an item run in its place among them: before_latents(i, q), after_latents(i, q).
template <class Item, class Before, class After>
static int mg_items_check(const char *who, int32_t n_items, const Item *items, int latent_dtype, Before before_latents, After after_latents) {
    MG_ITEM_REQUIRE(n_items >= 0 && (n_items == 0 || items), "%s: %d items, or NULL item table", who, n_items);
    MG_ITEM_REQUIRE(latent_dtype == MG_F32 || latent_dtype == MG_F64, "%s: bad latent dtype %d", who, latent_dtype);
    const mg_context *ctx = nullptr;
    for (int i = 0; i < n_items; i++) {
        const Item &q = items[i];
        const mg_primitive *p = q.prim;
        MG_ITEM_REQUIRE(p != nullptr, "%s: item %d: the primitive is NULL", who, i);
        if (!ctx) ctx = p->ctx;
        MG_ITEM_REQUIRE(p->ctx == ctx, "%s: item %d: the primitive belongs to another context", who, i);
        MG_ITEM_REQUIRE(q.n_samples >= 0 && q.ld >= 0, "%s: item %d: %lld samples, ld %lld", who, i, (long long)q.n_samples, (long long)q.ld);
        MG_ITEM_REQUIRE(q.latent_offset >= 0 && q.latent_offset + p->L <= q.ld, "%s: item %d reads latent columns %lld .. %lld of %lld", who, i,
                        (long long)q.latent_offset, (long long)(q.latent_offset + p->L), (long long)q.ld);
        int rc = before_latents(i, q);
        if (rc != MG_OK) return rc;
        MG_ITEM_REQUIRE(q.n_samples == 0 || q.latents_dev, "%s: item %d: the latents are NULL", who, i);
        if ((rc = after_latents(i, q)) != MG_OK) return rc;
    }
    return MG_OK;
}

// The table of a call: its non-empty items as the kernel reads them (DItem, zeroed, then item_of(i, d, append): the caller's item i
// into d), then the arrays item_of names: append(vector) puts one behind the table, 8-byte aligned, and returns its offset from the
// table's base for d to keep.  A table of 2 GiB or more is MG_ERR_UNSUPPORTED.
template <class DItem, class SamplesOf, class ItemOf>
static int mg_items_table(const char *who, int n_items, SamplesOf samples_of, std::vector<unsigned char> &table, ItemOf item_of) {
    const std::vector<int> of = mg_nonempty_items(n_items, samples_of);
    std::vector<DItem> ds(of.size());
    table.assign(ds.size() * sizeof(DItem), 0);
    if (!ds.empty()) memset((void *)ds.data(), 0, table.size());
    for (size_t e = 0; e < ds.size(); e++) {
        item_of(of[e], ds[e], [&](const auto &v) { return (uint32_t)mg_table_append(table, v.data(), v.size() * sizeof(*v.data())); });
        MG_REQUIRE_AS(table.size() < ((size_t)1 << 31), MG_ERR_UNSUPPORTED, "%s: the item table exceeds 2 GiB", who);
    }
    if (!ds.empty()) memcpy(table.data(), ds.data(), ds.size() * sizeof(DItem));
    return MG_OK;
}

// The table (the items first) into dt, then every launch on the context's stream.  kernel_of(tag): the kernel for float64
// (std::true_type) or float32 latents, lds_bit_f64 / _f32 their MG_LDS_* bits; args_of(base, launch): the kernel's argument for one
// launch, base: the table on the device.
template <class KernelOf, class ArgsOf>
static int mg_items_launch(mg_context *ctx, const char *who, mg_device_table &dt, const void *table, size_t bytes, size_t reserve,
                           const std::vector<mg_item_launch> &launches, int latent_dtype, unsigned lds_bit_f32, unsigned lds_bit_f64, int prof_slot,
                           KernelOf kernel_of, ArgsOf args_of) {
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    const int rc = dt.upload(ctx, who, table, bytes, reserve);
    if (rc != MG_OK) return rc;
    return mg_dispatch_flags(latent_dtype == MG_F64, [&](auto LAT_F64) {
        const auto kernel = kernel_of(LAT_F64);
        for (const mg_item_launch &l : launches) {
            if (l.lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, decltype(LAT_F64)::value ? lds_bit_f64 : lds_bit_f32, 160 * 1024, kernel));
            mg_prof_begin(ctx, prof_slot);
            hipLaunchKernelGGL(kernel, dim3((unsigned)l.grid), dim3(256), l.lds, ctx->stream, args_of(dt.base(), l));
            mg_prof_end(ctx, prof_slot);
            MG_HIP_CHECK(hipGetLastError());
        }
        return (int)MG_OK;
    });
}

// one output array of an item: `width` doubles per candidate, times the item's `times` member where one is named
template <class Item>
struct mg_item_output {
    double *Item::*member;
    int width;
    int32_t Item::*times;
};

// The _host twin: host arrays in, host arrays out, one device block for the call, synchronises.  run(items): the checked table with
// device arrays in place of the caller's; items that name the same latent matrix share one copy of it (mg_shared_latents).  A table
// without samples allocates nothing; a refused call copies nothing back.
template <class Item, size_t N, class Run>
static int mg_items_host(const char *who, int32_t n_items, const Item *items, int latent_dtype, const mg_item_output<Item> (&outs)[N], Run run) {
    const size_t elem = latent_dtype == MG_F64 ? 8 : 4;
    mg_context *ctx = nullptr;
    for (int i = 0; i < n_items; i++)
        if (items[i].n_samples > 0) ctx = items[i].prim->ctx;
    if (!ctx) return MG_OK;
    std::vector<Item> dev(items, items + n_items);
    const std::vector<int> lat_of = mg_shared_latents(items, n_items);
    std::vector<mg_staged> lat((size_t)n_items), out((size_t)n_items * N);
    mg_workspace ws(ctx, who);
    for (int i = 0; i < n_items; i++) {
        const Item &q = items[i];
        if (q.n_samples == 0) continue;
        lat[i] = lat_of[i] < 0 ? ws.in(q.latents_dev, (size_t)(q.n_samples * q.ld) * elem) : lat[lat_of[i]];
        for (size_t o = 0; o < N; o++)
            out[i * N + o] = ws.out(q.*(outs[o].member), (size_t)q.n_samples * outs[o].width * (outs[o].times ? (size_t)(q.*(outs[o].times)) : 1) * 8);
    }
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    for (int i = 0; i < n_items; i++) {
        if (items[i].n_samples == 0) continue;
        dev[i].latents_dev = lat[i].dev<void>();
        for (size_t o = 0; o < N; o++) dev[i].*(outs[o].member) = out[i * N + o].dev<double>();
    }
    if ((rc = run(dev.data())) != MG_OK) return rc;
    return ws.download();
}
