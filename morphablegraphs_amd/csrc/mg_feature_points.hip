// Feature points without frames in memory (gfx950 / MI355X), float64: what the reference's FeaturePointModel (construction/
// feature_point_model.py: create_feature_points, create_root_pos_ori) takes from a whole back-projected motion -- the root position of
// frame 0, the position of a few joints at one frame relative to it, the root's ground position and heading at the last frame -- for
// every candidate of every item, in ONE launch.
//
// Of a candidate's n_basis x D control points the three frames 0, frame_idx and F - 1 touch at most twelve, and of their channels only
// the root's three (frame 0), the root's seven (frame F - 1) and the root position plus the quaternions along the listed joints' chains
// (frame_idx).  The host lists those rows of E' once per item (mg_fp_plan); a workgroup owns up to MG_FP_TILE candidates of ONE item and
// keeps everything between the latents and the outputs in LDS:
//
//   constants   the listed rows of E' as [L][rows], their means, the three tap rows, where (control point, channel) sits among the
//               rows, the chain records of the listed joints (mg_fk_position_table's layout): once per workgroup.  A row two frames
//               share (frame_idx 0 or F - 1, overlapping tap windows) is listed once
//   phase 1     control points  c[cand][row] of the listed rows (mg_item_control_points)
//   phase 2     one (candidate, joint) per thread walks its chain (mg_fk_position_table) on channels evaluated from LDS (mg_taps4) and
//               subtracts the root position of frame 0; one more thread per candidate states start_root, root_end and the heading
//               (mg_chain_orientation, mg_rotate, mg_heading_xz).  The only stores to global memory
//
// The launch shape -- which workgroup serves which item, the slices of MG_FEATURE_POINTS_MAX_ITEMS items, the _host twin -- is
// mg_items.h's; behind the items their row lists and chain records travel in the same device table (ctx->tab[MG_TABLE_FEATURE_POINTS]).
#include <cmath>
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_items.h"
#include "mg_pack.h"
#include "mg_score_device.h"

#define MG_FP_TILE 16                    // candidates per workgroup
#define MG_FP_LDS_MAX (150 * 1024)
#define MG_FP_SLOTS 3                    // the frames 0, frame_idx, F - 1
#define MG_FP_REC_HDR 5                  // mg_fk_position_table's record: [4] = chain length m, then m x (quaternion channel or -1, offset xyz)

struct mg_fp_item {                      // one non-empty item as the kernel reads it
    const double *Et, *mean;             // [L][R], (R): E' and mean' (scaled by translation_maxima), row = i * D + d
    const void *lat;                     // the item's first latent: row b at lat + b * ld
    double *start_root, *points, *root_end, *heading_end, *heading_len;   // outputs or NULL
    int64_t n, ld;
    double w[MG_FP_SLOTS * 4];           // the three frames' tap rows
    int32_t tap[MG_FP_SLOTS];            // where each frame's first tap sits in the item's list of control points
    int32_t L, D, R, J;
    int32_t NRS, NCP;                    // listed rows; listed control points (<= 12)
    int32_t rec_stride;                  // doubles per chain record
    int32_t wg0;                         // first workgroup of the item in its launch
    uint32_t off_src, off_map, off_rec;  // bytes from the table's base: int32 src[NRS] (row of E'), int32 map[NCP * D] (listed row of
    uint32_t reserved;                   // (control point, channel) or -1), double rec[J][rec_stride]
};

struct mg_fp_args {
    const char *base;                    // the table
    const mg_fp_item *items;             // the launch's slice of it
    int32_t n_items;
};

// LDS of a workgroup, in doubles, and where its parts start (host and device agree through this)
struct mg_fp_layout {
    int E, mean, w, lat, cp, rec, ints, total_bytes;
    int CS;
};
__host__ __device__ static inline mg_fp_layout mg_fp_layout_of(int L, int NRS, int NCP, int D, int J, int rec_stride) {
    mg_fp_layout y;
    y.CS = NRS | 1;                      // odd: the lanes of phase 2 (candidates at the same row) read different banks
    y.E = 0;
    y.mean = y.E + L * NRS;
    y.w = y.mean + NRS;
    y.lat = y.w + MG_FP_SLOTS * 4;
    y.cp = y.lat + MG_FP_TILE * L;
    y.rec = y.cp + MG_FP_TILE * y.CS;
    y.ints = y.rec + J * rec_stride;     // then int32: map[NCP * D], tap[MG_FP_SLOTS], bad[MG_FP_TILE]
    y.total_bytes = y.ints * 8 + (NCP * D + MG_FP_SLOTS + MG_FP_TILE) * 4;
    return y;
}

template <bool LAT_F64>
__global__ __launch_bounds__(256) void mg_feature_points_kernel(const mg_fp_args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const mg_fp_item *ip = a.items + mg_item_of_workgroup(a.items, a.n_items);
    const int L = ip->L, D = ip->D, J = ip->J, NRS = ip->NRS, NCP = ip->NCP, RS = ip->rec_stride;
    const int64_t n = ip->n, ld = ip->ld;
    const size_t R = (size_t)ip->R;
    const mg_fp_layout y = mg_fp_layout_of(L, NRS, NCP, D, J, RS);
    const int CS = y.CS;
    double *sm = (double *)smem;
    double *sE = sm + y.E, *smean = sm + y.mean, *sw = sm + y.w, *slat = sm + y.lat, *scp = sm + y.cp, *srec = sm + y.rec;
    int32_t *smap = (int32_t *)(sm + y.ints), *stap = smap + NCP * D, *sbad = stap + MG_FP_SLOTS;
    int ncand;
    const int64_t b0 = mg_item_tile_of<MG_FP_TILE>(ip->wg0, n, ncand);

    // the item's constants and the tile's latents
    {
        const double *Et = ip->Et, *mean = ip->mean;
        const int32_t *src = (const int32_t *)(a.base + ip->off_src), *map = (const int32_t *)(a.base + ip->off_map);
        const double *rec = (const double *)(a.base + ip->off_rec);
        for (int e = tid; e < L * NRS; e += 256) {
            const int k = e / NRS, j = e - k * NRS;
            sE[e] = Et[(size_t)k * R + (size_t)src[j]];
        }
        for (int j = tid; j < NRS; j += 256) smean[j] = mean[src[j]];
        for (int e = tid; e < NCP * D; e += 256) smap[e] = map[e];
        for (int e = tid; e < J * RS; e += 256) srec[e] = rec[e];
        if (tid < MG_FP_SLOTS * 4) sw[tid] = ip->w[tid];
        if (tid < MG_FP_SLOTS) stap[tid] = ip->tap[tid];
        if (tid < MG_FP_TILE) sbad[tid] = 0;
    }
    __syncthreads();
    mg_item_stage_latents<LAT_F64>(ip->lat, ld, b0, ncand, L, slat, sbad);
    __syncthreads();

    // phase 1: control points of the listed rows
    mg_item_control_points(smean, sE, slat, ncand, NRS, L, scp, CS);
    __syncthreads();

    // phase 2: one (candidate, joint) per thread, and one thread per candidate for the root's outputs
    for (int e = tid; e < ncand * (J + 1); e += 256) {
        const int c = e / (J + 1), u = e - c * (J + 1);
        const double *cp = scp + c * CS;
        // channel d of frame slot s: the four taps of its knot span
        auto channel = [&](int s, int d) {
            const int32_t *m = smap + stap[s] * D + d;
            const double c4[4] = {cp[m[0]], cp[m[D]], cp[m[2 * D]], cp[m[3 * D]]};
            return mg_taps4(sw + 4 * s, c4, 1);
        };
        const bool bad = sbad[c] != 0;
        const int64_t b = b0 + c;
        const double s0[3] = {channel(0, 0), channel(0, 1), channel(0, 2)};
        if (u < J) {
            double p[3];
            mg_fk_position_table([&](int r) { return channel(1, r); }, 0, srec + u * RS, p);
            double *o = ip->points + (b * J + u) * 3;
#pragma unroll
            for (int i = 0; i < 3; i++) o[i] = bad ? NAN : p[i] - s0[i];
        } else {
            auto last = [&](int r) { return channel(2, r); };
            const double ex = last(0), ez = last(2);
            double q[4], v[3], hx, hz;
            mg_chain_orientation(last, 3, 1, q);
            mg_rotate(q, 0.0, 0.0, 1.0, v);
            const double len = sqrt(v[0] * v[0] + v[2] * v[2]);
            mg_heading_xz(q, 0.0, 0.0, 1.0, hx, hz);
            if (ip->start_root) {
                double *o = ip->start_root + b * 3;
#pragma unroll
                for (int i = 0; i < 3; i++) o[i] = bad ? NAN : s0[i];
            }
            if (ip->root_end) { ip->root_end[b * 2] = bad ? NAN : ex; ip->root_end[b * 2 + 1] = bad ? NAN : ez; }
            if (ip->heading_end) { ip->heading_end[b * 2] = bad ? NAN : hx; ip->heading_end[b * 2 + 1] = bad ? NAN : hz; }
            if (ip->heading_len) ip->heading_len[b] = bad ? NAN : len;
        }
    }
}

// What the host prepares of one item: the listed rows, where a (control point, channel) sits among them, the chain records
struct mg_fp_plan {
    std::vector<int32_t> src, map;
    std::vector<double> rec;
    int32_t NCP = 0, NRS = 0, rec_stride = MG_FP_REC_HDR;
    int32_t tap[MG_FP_SLOTS] = {0, 0, 0};
    double w[MG_FP_SLOTS * 4] = {0};
};

// the argument errors of one item's joint list (MG_ERR_INVALID_ARGUMENT)
static int mg_fp_check_joints(const char *who, int i, const mg_feature_point_item &q) {
    MG_ITEM_REQUIRE(q.n_joints >= 0 && q.n_joints <= MG_FEATURE_POINTS_MAX_JOINTS, "%s: item %d: %d joints (0 .. %d)", who, i, q.n_joints,
                    MG_FEATURE_POINTS_MAX_JOINTS);
    MG_ITEM_REQUIRE((q.n_joints > 0) == (q.points_dev != nullptr), "%s: item %d: %d joints and %s points output", who, i, q.n_joints,
                    q.points_dev ? "a" : "no");
    if (q.n_joints == 0) return MG_OK;
    const mg_skeleton_desc *sk = q.skeleton;
    MG_ITEM_REQUIRE(sk && q.joints, "%s: item %d: joints without a skeleton or a joint list", who, i);
    MG_ITEM_REQUIRE(sk->n_joints > 0 && sk->parents && sk->offsets && sk->quat_channel && sk->parents[0] < 0, "%s: item %d: incomplete skeleton", who, i);
    for (int j = 0; j < q.n_joints; j++) {
        std::vector<int> ch;
        int bad;
        const int st = mg_joint_chain(sk->parents, sk->n_joints, q.joints[j], ch, &bad);
        MG_ITEM_REQUIRE(st == MG_CHAIN_OK, "%s: item %d: joint %d%s", who, i, bad, mg_chain_why(st));
    }
    return MG_OK;
}

// the plan of one item whose arguments passed; what the kernels do not take is MG_ERR_UNSUPPORTED
static int mg_fp_plan_of(const char *who, int i, const mg_feature_point_item &q, mg_fp_plan &pl) {
    const mg_primitive *p = q.prim;
    const mg_time_grid *g = p->canonical;
    const int D = p->D, F = p->F;
    MG_ITEM_REFUSE(D < 7, "%s: item %d: the primitive has %d channels, a root pose needs 7", who, i, D);
    MG_ITEM_REFUSE(!g || g->T < 1 || g->T != F || !p->d_Et64 || !p->d_mean || (int)g->i0.size() != F || (int)g->w.size() != 4 * F,
                   "%s: item %d: the primitive has no canonical grid (%d canonical frames)", who, i, F);
    const mg_skeleton_desc *sk = q.skeleton;
    if (sk && sk->quat_channel)
        for (int j = 0; j < sk->n_joints; j++)
            MG_ITEM_REFUSE(sk->quat_channel[j] >= 0 && sk->quat_channel[j] + 4 > D, "%s: item %d: the skeleton's joint %d has channels %d .. %d, the primitive %d",
                           who, i, j, sk->quat_channel[j], sk->quat_channel[j] + 3, D);
    const int frames[MG_FP_SLOTS] = {0, q.frame_idx, F - 1};
    std::vector<int32_t> cps;
    for (int s = 0; s < MG_FP_SLOTS; s++) {
        const int i0 = g->i0[(size_t)frames[s]];
        MG_ITEM_REFUSE(i0 < 0 || i0 + 4 > p->NB, "%s: item %d: frame %d takes control points %d .. %d of %d", who, i, frames[s], i0, i0 + 3, p->NB);
        for (int j = 0; j < 4; j++) {
            cps.push_back(i0 + j);
            pl.w[4 * s + j] = g->w[4 * (size_t)frames[s] + j];
        }
    }
    std::sort(cps.begin(), cps.end());
    cps.erase(std::unique(cps.begin(), cps.end()), cps.end());
    pl.NCP = (int32_t)cps.size();
    // the channels every listed control point is wanted for
    std::vector<char> need((size_t)pl.NCP * D, 0);
    auto want = [&](int s, int d0, int count) {
        pl.tap[s] = (int32_t)(std::lower_bound(cps.begin(), cps.end(), g->i0[(size_t)frames[s]]) - cps.begin());
        for (int j = 0; j < 4; j++)
            for (int d = d0; d < d0 + count; d++) need[(size_t)(pl.tap[s] + j) * D + d] = 1;
    };
    want(0, 0, 3);
    want(1, 0, 3);
    want(2, 0, 7);
    std::vector<std::vector<int>> chains((size_t)q.n_joints);
    int longest = 0;
    for (int j = 0; j < q.n_joints; j++) {
        mg_joint_chain(sk->parents, sk->n_joints, q.joints[j], chains[(size_t)j]);
        const int m = (int)chains[(size_t)j].size() - 1;
        MG_ITEM_REFUSE(m > MG_MAX_CHAIN, "%s: item %d: chain of %d joints exceeds %d", who, i, m, MG_MAX_CHAIN);
        longest = std::max(longest, m);
        for (int k = 0; k < m; k++) {
            const int qc = sk->quat_channel[chains[(size_t)j][(size_t)k]];
            if (qc >= 0) want(1, qc, 4);
        }
    }
    pl.map.assign((size_t)pl.NCP * D, -1);
    for (int c = 0; c < pl.NCP; c++)
        for (int d = 0; d < D; d++)
            if (need[(size_t)c * D + d]) {
                pl.map[(size_t)c * D + d] = (int32_t)pl.src.size();
                pl.src.push_back(cps[(size_t)c] * D + d);
            }
    pl.NRS = (int32_t)pl.src.size();
    pl.rec_stride = MG_FP_REC_HDR + 4 * longest;
    pl.rec.assign((size_t)q.n_joints * pl.rec_stride, 0.0);
    for (int j = 0; j < q.n_joints; j++) {
        double *rec = &pl.rec[(size_t)j * pl.rec_stride];
        rec[4] = (double)(chains[(size_t)j].size() - 1);
        mg_chain_links(chains[(size_t)j], sk->offsets, [&](int joint) { return sk->quat_channel[joint]; }, rec + MG_FP_REC_HDR);
    }
    MG_ITEM_REFUSE((int64_t)p->L * pl.NRS > (1 << 20) || mg_fp_layout_of(p->L, pl.NRS, pl.NCP, D, q.n_joints, pl.rec_stride).total_bytes > MG_FP_LDS_MAX,
                   "%s: item %d: the tables (%d x %d control-point values, %d joints) do not fit LDS", who, i, p->L, pl.NRS, q.n_joints);
    MG_ITEM_REFUSE_GRID(who, i, q.n_samples, MG_FP_TILE);
    return MG_OK;
}

// the checks both entry points make of an item table (nothing is launched or copied before they pass); plans: one per item
static int mg_fp_check(const char *who, int32_t n_items, const mg_feature_point_item *items, int latent_dtype, std::vector<mg_fp_plan> &plans) {
    int rc = mg_items_check(
        who, n_items, items, latent_dtype, [](int, const mg_feature_point_item &) { return (int)MG_OK; },
        [&](int i, const mg_feature_point_item &q) -> int {
            MG_ITEM_REQUIRE(q.frame_idx >= 0 && q.frame_idx < q.prim->F, "%s: item %d: frame %d of %d", who, i, q.frame_idx, q.prim->F);
            MG_ITEM_REQUIRE(q.start_root_dev || q.points_dev || q.root_end_dev || q.heading_end_dev || q.heading_len_dev, "%s: item %d: all outputs are NULL", who, i);
            return mg_fp_check_joints(who, i, q);
        });
    if (rc != MG_OK) return rc;
    plans.resize((size_t)n_items);
    for (int i = 0; i < n_items; i++)
        if ((rc = mg_fp_plan_of(who, i, items[i], plans[(size_t)i])) != MG_OK) return rc;
    return MG_OK;
}

static int mg_fp_run(const char *who, int32_t n_items, const mg_feature_point_item *items, int latent_dtype, const std::vector<mg_fp_plan> &plans) {
    const size_t elem = latent_dtype == MG_F64 ? 8 : 4;
    auto lds_of = [&](int i) {
        const mg_fp_plan &pl = plans[(size_t)i];
        return mg_fp_layout_of(items[i].prim->L, pl.NRS, pl.NCP, items[i].prim->D, items[i].n_joints, pl.rec_stride).total_bytes;
    };
    std::vector<int32_t> wg0;
    const std::vector<mg_item_launch> launches =
        mg_cut_items(n_items, [&](int i) { return items[i].n_samples; }, lds_of, MG_FP_TILE, MG_FEATURE_POINTS_MAX_ITEMS, wg0);
    if (launches.empty()) return MG_OK;
    std::vector<mg_fp_item> ds;          // the non-empty items
    std::vector<int> of;                 // the caller's item behind every entry of ds
    mg_context *ctx = nullptr;
    for (int i = 0; i < n_items; i++) {
        const mg_feature_point_item &q = items[i];
        if (q.n_samples == 0) continue;
        mg_primitive *p = q.prim;
        const mg_fp_plan &pl = plans[(size_t)i];
        ctx = p->ctx;
        mg_fp_item d;
        memset(&d, 0, sizeof(d));
        d.Et = p->d_Et64; d.mean = p->d_mean;
        d.lat = (const char *)q.latents_dev + (size_t)q.latent_offset * elem;
        d.start_root = q.start_root_dev; d.points = q.points_dev; d.root_end = q.root_end_dev; d.heading_end = q.heading_end_dev;
        d.heading_len = q.heading_len_dev;
        d.n = q.n_samples; d.ld = q.ld;
        memcpy(d.w, pl.w, sizeof(d.w));
        memcpy(d.tap, pl.tap, sizeof(d.tap));
        d.L = p->L; d.D = p->D; d.R = p->R; d.J = q.n_joints; d.NRS = pl.NRS; d.NCP = pl.NCP; d.rec_stride = pl.rec_stride;
        d.wg0 = wg0[i];
        ds.push_back(d);
        of.push_back(i);
    }
    // the table: the items, then every item's row list, map and chain records
    std::vector<unsigned char> blob(ds.size() * sizeof(mg_fp_item));
    auto append = [&](const void *data, size_t bytes) {
        const size_t at = (blob.size() + 7) & ~(size_t)7;
        blob.resize(at + bytes, 0);
        if (bytes) memcpy(blob.data() + at, data, bytes);
        return at;
    };
    for (size_t e = 0; e < ds.size(); e++) {
        const mg_fp_plan &pl = plans[(size_t)of[e]];
        const size_t o_src = append(pl.src.data(), pl.src.size() * 4), o_map = append(pl.map.data(), pl.map.size() * 4);
        const size_t o_rec = append(pl.rec.data(), pl.rec.size() * 8);
        MG_REQUIRE_AS(blob.size() < ((size_t)1 << 31), MG_ERR_UNSUPPORTED, "%s: the item table exceeds 2 GiB", who);
        ds[e].off_src = (uint32_t)o_src; ds[e].off_map = (uint32_t)o_map; ds[e].off_rec = (uint32_t)o_rec;
    }
    memcpy(blob.data(), ds.data(), ds.size() * sizeof(mg_fp_item));
    return mg_items_launch(
        ctx, who, ctx->tab[MG_TABLE_FEATURE_POINTS], blob.data(), blob.size(), std::max(blob.size() * 2, (size_t)64 * 1024), launches, latent_dtype,
        MG_LDS_FEATURE_POINTS_F32, MG_LDS_FEATURE_POINTS_F64, MG_PROF_FEATURE_POINTS, [](auto LAT_F64) { return mg_feature_points_kernel<decltype(LAT_F64)::value>; },
        [](const char *base, const mg_item_launch &l) { return mg_fp_args{base, (const mg_fp_item *)base + l.first, l.n_items}; });
}

extern "C" int mg_feature_points(int32_t n_items, const mg_feature_point_item *items, int latent_dtype) {
    std::vector<mg_fp_plan> plans;
    const int rc = mg_fp_check("mg_feature_points", n_items, items, latent_dtype, plans);
    if (rc != MG_OK) return rc;
    return mg_fp_run("mg_feature_points", n_items, items, latent_dtype, plans);
}

extern "C" int mg_feature_points_host(int32_t n_items, const mg_feature_point_item *items, int latent_dtype) {
    typedef mg_feature_point_item item;
    std::vector<mg_fp_plan> plans;
    const int rc = mg_fp_check("mg_feature_points_host", n_items, items, latent_dtype, plans);
    if (rc != MG_OK) return rc;
    const mg_item_output<item> outs[5] = {{&item::start_root_dev, 3, nullptr}, {&item::points_dev, 3, &item::n_joints}, {&item::root_end_dev, 2, nullptr},
                                          {&item::heading_end_dev, 2, nullptr}, {&item::heading_len_dev, 1, nullptr}};
    return mg_items_host("mg_feature_points_host", n_items, items, latent_dtype, outs,
                         [&](const item *dev) { return mg_fp_run("mg_feature_points_host", n_items, dev, latent_dtype, plans); });
}
