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
// mg_items.h's, the table's layout included; behind the items their row lists and chain records travel in the same device table
// (ctx->tab[MG_TABLE_FEATURE_POINTS]).  The row list is mg_feature_rows.h's (host-only).  What the time-warped kernel further down
// shares with this one is stated once, between the layouts and the kernels: the item's leading members (mg_fp_item), the staging of
// its constants (mg_fp_stage_constants), the four-tap read (mg_fp_channel), the root thread (mg_fp_root_outputs); on the host the
// shared refusals (mg_fp_refuse), the chains and their records, the members of the device item (mg_fp_fill).
#include <climits>
#include <cmath>
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_feature_rows.h"
#include "mg_items.h"
#include "mg_joint_plan.h"
#include "mg_score_device.h"
#include "mg_timewarp_device.h"

#define MG_FP_TILE 16                    // candidates per workgroup
#define MG_FP_LDS_MAX (150 * 1024)
#define MG_FP_SLOTS 3                    // the frames 0, frame_idx, F - 1
#define MG_FP_REC_HDR 5                  // mg_fk_position_table's record: [4] = chain length m, then m x (quaternion channel or -1, offset xyz)

struct mg_fp_item {                      // one non-empty item as the kernel reads it; the time-warped kernel's item starts with it
    const double *Et, *mean;             // [L][R], (R): E' and mean' (scaled by translation_maxima), row = i * D + d
    const void *lat;                     // the item's first latent: row b at lat + b * ld
    double *start_root, *points, *root_end, *heading_end, *heading_len;   // outputs or NULL
    int64_t n, ld;
    double w[MG_FP_SLOTS * 4];           // the host-planned frames' tap rows (three; two of the time-warped motion)
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

// ---- the statements both kernels make (inlined into them, under their fp contract(off)) ---------------------------------------------
// the item's constants into LDS: the listed rows of E' as sE[L][NRS], their means, where (control point, channel) sits among the rows,
// the chain records, the tap rows and tap positions of the `slots` host-planned frames; the tile's not-finite flags zeroed
__device__ __forceinline__ void mg_fp_stage_constants(const char *base, const mg_fp_item *ip, int slots, double *sE, double *smean, double *sw, double *srec,
                                                      int32_t *smap, int32_t *stap, int32_t *sbad) {
    const int tid = threadIdx.x, L = ip->L, NRS = ip->NRS, n_map = ip->NCP * ip->D, n_rec = ip->J * ip->rec_stride;
    const size_t R = (size_t)ip->R;
    const double *Et = ip->Et, *mean = ip->mean;
    const int32_t *src = (const int32_t *)(base + ip->off_src), *map = (const int32_t *)(base + ip->off_map);
    const double *rec = (const double *)(base + ip->off_rec);
    for (int e = tid; e < L * NRS; e += 256) {
        const int k = e / NRS, j = e - k * NRS;
        sE[e] = Et[(size_t)k * R + (size_t)src[j]];
    }
    for (int j = tid; j < NRS; j += 256) smean[j] = mean[src[j]];
    for (int e = tid; e < n_map; e += 256) smap[e] = map[e];
    for (int e = tid; e < n_rec; e += 256) srec[e] = rec[e];
    if (tid < slots * 4) sw[tid] = ip->w[tid];
    if (tid < slots) stap[tid] = ip->tap[tid];
    if (tid < MG_FP_TILE) sbad[tid] = 0;
}

// channel d of host-planned frame slot s from a candidate's control points cp: the four taps of its knot span
__device__ __forceinline__ double mg_fp_channel(const double *cp, const double *sw, const int32_t *smap, const int32_t *stap, int D, int s, int d) {
#pragma clang fp contract(off)
    const int32_t *m = smap + stap[s] * D + d;
    const double c4[4] = {cp[m[0]], cp[m[D]], cp[m[2 * D]], cp[m[3 * D]]};
    return mg_taps4(sw + 4 * s, c4, 1);
}

// the root thread of phase 2: start_root (s0), root_end and the heading of frame slot `slot` (the last frame) for candidate b of the
// item; NaN throughout for a bad one.  channel(s, d): mg_fp_channel on the candidate's control points
template <class Channel>
__device__ __forceinline__ void mg_fp_root_outputs(const mg_fp_item *ip, int64_t b, bool bad, const double *s0, Channel channel, int slot) {
#pragma clang fp contract(off)
    auto last = [&](int r) { return channel(slot, r); };
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

template <bool LAT_F64>
__global__ __launch_bounds__(256) void mg_feature_points_kernel(const mg_fp_args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const mg_fp_item *ip = a.items + mg_item_of_workgroup(a.items, a.n_items);
    const int L = ip->L, D = ip->D, J = ip->J, NRS = ip->NRS, NCP = ip->NCP, RS = ip->rec_stride;
    const int64_t n = ip->n, ld = ip->ld;
    const mg_fp_layout y = mg_fp_layout_of(L, NRS, NCP, D, J, RS);
    const int CS = y.CS;
    double *sm = (double *)smem;
    double *sE = sm + y.E, *smean = sm + y.mean, *sw = sm + y.w, *slat = sm + y.lat, *scp = sm + y.cp, *srec = sm + y.rec;
    int32_t *smap = (int32_t *)(sm + y.ints), *stap = smap + NCP * D, *sbad = stap + MG_FP_SLOTS;
    int ncand;
    const int64_t b0 = mg_item_tile_of<MG_FP_TILE>(ip->wg0, n, ncand);

    // the item's constants and the tile's latents
    mg_fp_stage_constants(a.base, ip, MG_FP_SLOTS, sE, smean, sw, srec, smap, stap, sbad);
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
        auto channel = [&](int s, int d) { return mg_fp_channel(cp, sw, smap, stap, D, s, d); };
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
            mg_fp_root_outputs(ip, b, bad, s0, channel, 2);
        }
    }
}

// What the host prepares of one item: the listed rows and where a (control point, channel) sits among them (mg_feature_rows.h), the
// chain records, the host-planned frames' tap rows, the LDS bytes of a workgroup; the time-warped item's plan starts with it
struct mg_fp_plan {
    mg_feature_rows rows;
    mg_joint_plan joints;                // the listed joints' chains, formed while the arguments are checked
    std::vector<double> rec;
    int32_t rec_stride = MG_FP_REC_HDR;
    double w[MG_FP_SLOTS * 4] = {0};
    int lds = 0;
};

// What both plans refuse of the channels (MG_ERR_UNSUPPORTED), in the order they always had: a primitive without a root pose, then the
// plan's own refusals of the primitive (own()), then a skeleton channel beyond the primitive's
template <class Own>
static int mg_fp_refuse(const char *who, int i, int D, const mg_skeleton_desc *sk, Own own) {
    MG_ITEM_REFUSE(D < 7, "%s: item %d: the primitive has %d channels, a root pose needs 7", who, i, D);
    const int rc = own();
    if (rc != MG_OK) return rc;
    if (sk && sk->quat_channel)
        for (int j = 0; j < sk->n_joints; j++)
            MG_ITEM_REFUSE(sk->quat_channel[j] >= 0 && sk->quat_channel[j] + 4 > D, "%s: item %d: the skeleton's joint %d has channels %d .. %d, the primitive %d",
                           who, i, j, sk->quat_channel[j], sk->quat_channel[j] + 3, D);
    return MG_OK;
}

// the argument errors of one item's joint list (MG_ERR_INVALID_ARGUMENT); jp: the chains of its joints (mg_joint_plan.h)
template <class Item>
static int mg_fp_joint_list(const char *who, int i, const Item &q, mg_joint_plan &jp) {
    MG_ITEM_REQUIRE(q.n_joints >= 0 && q.n_joints <= MG_FEATURE_POINTS_MAX_JOINTS, "%s: item %d: %d joints (0 .. %d)", who, i, q.n_joints,
                    MG_FEATURE_POINTS_MAX_JOINTS);
    MG_ITEM_REQUIRE((q.n_joints > 0) == (q.points_dev != nullptr), "%s: item %d: %d joints and %s points output", who, i, q.n_joints,
                    q.points_dev ? "a" : "no");
    if (q.n_joints == 0) return MG_OK;
    const mg_skeleton_desc *sk = q.skeleton;
    MG_ITEM_REQUIRE(sk && q.joints, "%s: item %d: joints without a skeleton or a joint list", who, i);
    MG_ITEM_REQUIRE(mg_skeleton_complete(sk), "%s: item %d: incomplete skeleton", who, i);
    const mg_plan_failure f = jp.check(sk, q.joints, q.n_joints);
    MG_ITEM_REQUIRE(!f, "%s: item %d: joint %d%s", who, i, f.joint, mg_chain_why(f.kind));
    return MG_OK;
}

// what the kernels do not take of those chains (MG_ERR_UNSUPPORTED), then the channels they read (pl.joints.need; root_xyz: the root
// position among them) and their records (mg_fk_position_table's layout), all as long as the longest chain's
static int mg_fp_measure(const char *who, int i, int D, bool root_xyz, mg_fp_plan &pl) {
    const mg_plan_failure f = pl.joints.measure(D, root_xyz);
    MG_ITEM_REFUSE(f.kind == MG_PLAN_TOO_LONG, "%s: item %d: chain of %d joints exceeds %d", who, i, f.length, MG_MAX_CHAIN);
    MG_ITEM_REFUSE(f.kind == MG_PLAN_CHANNEL_OUTSIDE, "%s: item %d: the skeleton's joint %d has channels %d .. %d, the primitive %d", who, i, f.joint, f.channel,
                   f.channel + 3, D);      // (mg_fp_refuse has said so of any joint already)
    pl.rec_stride = pl.joints.records(MG_FP_REC_HDR, 0, pl.rec);
    return MG_OK;
}

// the plan of one item whose arguments passed; what the kernels do not take is MG_ERR_UNSUPPORTED
static int mg_fp_plan_of(const char *who, int i, const mg_feature_point_item &q, mg_fp_plan &pl) {
    const mg_primitive *p = q.prim;
    const mg_time_grid *g = p->canonical;
    const int D = p->D, F = p->F;
    int rc = mg_fp_refuse(who, i, D, q.skeleton, [&]() -> int {
        MG_ITEM_REFUSE(!g || g->T < 1 || g->T != F || !p->d_Et64 || !p->d_mean || (int)g->i0.size() != F || (int)g->w.size() != 4 * F,
                       "%s: item %d: the primitive has no canonical grid (%d canonical frames)", who, i, F);
        return MG_OK;
    });
    if (rc != MG_OK) return rc;
    // the three frames' taps, from the canonical grid
    const int frames[MG_FP_SLOTS] = {0, q.frame_idx, F - 1};
    std::vector<int32_t> first;
    for (int s = 0; s < MG_FP_SLOTS; s++) {
        const int i0 = g->i0[(size_t)frames[s]];
        MG_ITEM_REFUSE(i0 < 0 || i0 + 4 > p->NB, "%s: item %d: frame %d takes control points %d .. %d of %d", who, i, frames[s], i0, i0 + 3, p->NB);
        first.push_back(i0);
        for (int j = 0; j < 4; j++) pl.w[4 * s + j] = g->w[4 * (size_t)frames[s] + j];
    }
    // the root position of frame 0; the root position and the quaternions along the listed joints' chains of frame_idx; the root pose of F - 1
    std::vector<mg_feature_range> wanted = {{0, 0, 3}, {1, 0, 3}, {2, 0, 7}};
    if ((rc = mg_fp_measure(who, i, D, false, pl)) != MG_OK) return rc;
    for (int d = 0; d < D; d++)
        if (pl.joints.need[(size_t)d]) wanted.push_back({1, d, 1});
    pl.rows = mg_feature_rows_of(D, first, wanted);
    pl.lds = (int64_t)p->L * pl.rows.NRS > (1 << 20) ? INT_MAX : mg_fp_layout_of(p->L, pl.rows.NRS, pl.rows.NCP, D, q.n_joints, pl.rec_stride).total_bytes;
    MG_ITEM_REFUSE(pl.lds > MG_FP_LDS_MAX, "%s: item %d: the tables (%d x %d control-point values, %d joints) do not fit LDS", who, i, p->L, pl.rows.NRS, q.n_joints);
    MG_ITEM_REFUSE_GRID(who, i, q.n_samples, MG_FP_TILE);
    return MG_OK;
}

// the checks both entry points make of an item table (nothing is launched or copied before they pass); plans: one per item
static int mg_fp_check(const char *who, int32_t n_items, const mg_feature_point_item *items, int latent_dtype, std::vector<mg_fp_plan> &plans) {
    plans.resize((size_t)std::max(n_items, 0));
    int rc = mg_items_check(
        who, n_items, items, latent_dtype, [](int, const mg_feature_point_item &) { return (int)MG_OK; },
        [&](int i, const mg_feature_point_item &q) -> int {
            MG_ITEM_REQUIRE(q.frame_idx >= 0 && q.frame_idx < q.prim->F, "%s: item %d: frame %d of %d", who, i, q.frame_idx, q.prim->F);
            MG_ITEM_REQUIRE(q.start_root_dev || q.points_dev || q.root_end_dev || q.heading_end_dev || q.heading_len_dev, "%s: item %d: all outputs are NULL", who, i);
            return mg_fp_joint_list(who, i, q, plans[(size_t)i].joints);
        });
    if (rc != MG_OK) return rc;
    for (int i = 0; i < n_items; i++)
        if ((rc = mg_fp_plan_of(who, i, items[i], plans[(size_t)i])) != MG_OK) return rc;
    return MG_OK;
}

// the members both kernels read of the caller's item q, from it and its plan; append: mg_items_table's
template <class Item, class Append>
static void mg_fp_fill(mg_fp_item &d, const Item &q, const mg_fp_plan &pl, size_t elem, int32_t wg0, Append append) {
    const mg_primitive *p = q.prim;
    d.Et = p->d_Et64; d.mean = p->d_mean;
    d.lat = (const char *)q.latents_dev + (size_t)q.latent_offset * elem;
    d.start_root = q.start_root_dev; d.points = q.points_dev; d.root_end = q.root_end_dev; d.heading_end = q.heading_end_dev;
    d.heading_len = q.heading_len_dev;
    d.n = q.n_samples; d.ld = q.ld;
    memcpy(d.w, pl.w, sizeof(d.w));
    std::copy(pl.rows.tap.begin(), pl.rows.tap.end(), d.tap);
    d.L = p->L; d.D = p->D; d.R = p->R; d.J = q.n_joints; d.NRS = pl.rows.NRS; d.NCP = pl.rows.NCP; d.rec_stride = pl.rec_stride;
    d.wg0 = wg0;
    d.off_src = append(pl.rows.src); d.off_map = append(pl.rows.map);
}

static int mg_fp_run(const char *who, int32_t n_items, const mg_feature_point_item *items, int latent_dtype, const std::vector<mg_fp_plan> &plans) {
    const size_t elem = latent_dtype == MG_F64 ? 8 : 4;
    auto samples_of = [&](int i) { return items[i].n_samples; };
    std::vector<int32_t> wg0;
    const std::vector<mg_item_launch> launches =
        mg_cut_items(n_items, samples_of, [&](int i) { return plans[(size_t)i].lds; }, MG_FP_TILE, MG_FEATURE_POINTS_MAX_ITEMS, wg0);
    if (launches.empty()) return MG_OK;
    mg_context *ctx = nullptr;
    std::vector<unsigned char> table;    // the items, then every item's row list, map and chain records
    const int rc = mg_items_table<mg_fp_item>(who, n_items, samples_of, table, [&](int i, mg_fp_item &d, auto append) {
        ctx = items[i].prim->ctx;
        mg_fp_fill(d, items[i], plans[(size_t)i], elem, wg0[(size_t)i], append);
        d.off_rec = append(plans[(size_t)i].rec);
    });
    if (rc != MG_OK) return rc;
    return mg_items_launch(
        ctx, who, ctx->tab[MG_TABLE_FEATURE_POINTS], table.data(), table.size(), std::max(table.size() * 2, (size_t)64 * 1024), launches, latent_dtype,
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

// ---- the time-warped motion ---------------------------------------------------------------------------------------------------------
// mg_feature_points_warped: the same features of back_project(s, use_time_parameters=True) -- frame 0 at time 0, frame -1 at time
// F - 1, frame frame_idx at a time of the candidate's own: the frame_idx-th sample of the inverse of its canonical time function
// (mg_timewarp_device.h).  A workgroup owns MG_FP_TILE candidates of one item, as above:
//
//   constants   the rows of E' the two END frames touch (host-planned: their times do not depend on the candidate), their means and
//               tap rows, the chain records, the channels the mid frame is wanted for
//   warp 1      increments exp(mean_t(i) + phi(i) . gamma), one (canonical frame, candidate) per thread, into x[i][cand]
//   warp 2      ONE LANE PER CANDIDATE (the tile's 16 lanes of wave 0): running sum, sample count, the sample point of frame_idx and
//               its interval, the tridiagonal sweep (x, cp, dp: 3 F doubles per candidate, [i][cand] so the 16 lanes read
//               consecutive doubles), the back-substitution down to that interval only, the sample -> time_mid, n_frames; the basis
//               row of time_mid.  Meanwhile waves 1 .. 3 form the end frames' control points (phase 1 above)
//   mid         the tap window differs per candidate, so no row list: one (candidate, channel) per thread forms its four control
//               points straight from E' in global memory (L2: consecutive threads read consecutive channels of one row of E') and
//               takes the four taps -> mid[cand][channel]
//   phase 2     as above, the mid frame's channels from mid[][]
// An item without joints and without the time_mid output needs no sample: its lanes stop after the count, and x alone is kept.
#define MG_FPW_SLOTS 2                   // the host-planned frames: time 0, time F - 1

struct mg_fpw_item : mg_fp_item {       // (w, tap: the two end frames'; the rows: theirs)
    const double *knots, *tphi, *tmean;
    const void *gam;                     // the item's first time latent: row b at gam + b * ld
    double *time_mid;
    int32_t *n_frames;
    int32_t Lt, F, NB, NC;               // NC: channels of the mid frame
    int32_t frame_idx, need_mid;
    uint32_t off_chan;                   // int32 chan[NC] (the mid frame's channels, ascending), pos[D] (where a channel sits among them)
};

struct mg_fpw_args {
    const char *base;
    const mg_fpw_item *items;
    int32_t n_items;
};

// mg_feature_points_warped_smoothed: an item whose `smooth` is not 0 takes its three times from the SMOOTHED time function
// (mg_timewarp_device.h: mg_tw_smooth_window, mg_tw_smoothed over H, the hat matrix of mg_savgol_table.h) -- the first one row 0 of H
// on the first 15 samples, the last one row 14 on the last 15, time_mid the case split at frame_idx -- so all three frames have tap
// windows of the candidate's own: the end frames go the mid frame's way (control points straight from E', four taps) into
// ends[cand][3 + 7], and the host-planned rows are not read.  The lane evaluates the <= 45 unsmoothed samples itself from the whole
// set of second derivatives; a candidate of fewer than 15 frames is NaN in every output but n_frames.  smooth = 0: the statements above.
struct mg_fpws_item : mg_fpw_item {
    const double *H;
    int32_t smooth, pad;
};

struct mg_fpws_args {
    const char *base;
    const mg_fpws_item *items;
    int32_t n_items;
};
#define MG_FPW_ENDS 10                  // doubles per candidate: the root position at the first time, the root pose at the last one

struct mg_fpw_layout {
    int x, cpt, dpt, gam, tmid, wm, E, mean, w, lat, cp, mid, ends, rec, ints, total_bytes;
    int CS, MS;
};
// smooth: three basis rows and three first taps per candidate (first, mid, last) instead of the mid frame's one, and ends[cand][10]
__host__ __device__ static inline mg_fpw_layout mg_fpw_layout_of(int F, int Lt, int need_mid, int L, int NRS, int NCP, int NC, int D, int J, int rec_stride,
                                                                 int smooth = 0) {
    mg_fpw_layout y;
    const int slots = smooth ? 3 : 1;
    y.CS = NRS | 1;
    y.MS = NC | 1;
    y.x = 0;
    y.cpt = y.x + F * MG_FP_TILE;
    y.dpt = y.cpt + (need_mid ? F * MG_FP_TILE : 0);
    y.gam = y.dpt + (need_mid ? F * MG_FP_TILE : 0);
    y.tmid = y.gam + MG_FP_TILE * Lt;
    y.wm = y.tmid + MG_FP_TILE;
    y.E = y.wm + MG_FP_TILE * 4 * slots;
    y.mean = y.E + L * NRS;
    y.w = y.mean + NRS;
    y.lat = y.w + MG_FPW_SLOTS * 4;
    y.cp = y.lat + MG_FP_TILE * L;
    y.mid = y.cp + MG_FP_TILE * y.CS;
    y.ends = y.mid + MG_FP_TILE * y.MS;
    y.rec = y.ends + (smooth ? MG_FP_TILE * MG_FPW_ENDS : 0);
    y.ints = y.rec + J * rec_stride;     // then int32: map[NCP * D], chan[NC], pos[D], tap[MG_FPW_SLOTS], bad[TILE], nf[TILE], i0[TILE][slots]
    y.total_bytes = y.ints * 8 + (NCP * D + NC + D + MG_FPW_SLOTS + (2 + slots) * MG_FP_TILE) * 4;
    return y;
}

template <bool SMOOTH> struct mg_fpw_types { typedef mg_fpw_item item; typedef mg_fpw_args args; };
template <> struct mg_fpw_types<true> { typedef mg_fpws_item item; typedef mg_fpws_args args; };
__device__ __forceinline__ int mg_fpw_smooth_of(const mg_fpw_item *) { return 0; }
__device__ __forceinline__ int mg_fpw_smooth_of(const mg_fpws_item *ip) { return ip->smooth; }
__device__ __forceinline__ const double *mg_fpw_table_of(const mg_fpw_item *) { return nullptr; }
__device__ __forceinline__ const double *mg_fpw_table_of(const mg_fpws_item *ip) { return ip->H; }

template <bool LAT_F64, bool SMOOTH>
__global__ __launch_bounds__(256) void mg_feature_points_warped_kernel(const typename mg_fpw_types<SMOOTH>::args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const typename mg_fpw_types<SMOOTH>::item *ip = a.items + mg_item_of_workgroup(a.items, a.n_items);
    const bool smooth = SMOOTH && mg_fpw_smooth_of(ip) != 0;
    const double *H = mg_fpw_table_of(ip);
    const int L = ip->L, Lt = ip->Lt, D = ip->D, F = ip->F, J = ip->J, NRS = ip->NRS, NCP = ip->NCP, NC = ip->NC, RS = ip->rec_stride;
    const int frame_idx = ip->frame_idx, need_mid = ip->need_mid;
    const int64_t n = ip->n, ld = ip->ld;
    const size_t R = (size_t)ip->R;
    const mg_fpw_layout y = mg_fpw_layout_of(F, Lt, need_mid, L, NRS, NCP, NC, D, J, RS, smooth ? 1 : 0);
    const int CS = y.CS, MS = y.MS;
    double *sends = (double *)smem + y.ends;
    double *sm = (double *)smem;
    double *sx = sm + y.x, *scpt = sm + y.cpt, *sdpt = sm + y.dpt, *sgam = sm + y.gam, *stmid = sm + y.tmid, *swm = sm + y.wm;
    double *sE = sm + y.E, *smean = sm + y.mean, *sw = sm + y.w, *slat = sm + y.lat, *scp = sm + y.cp, *smid = sm + y.mid, *srec = sm + y.rec;
    int32_t *smap = (int32_t *)(sm + y.ints), *schan = smap + NCP * D, *spos = schan + NC, *stap = spos + D, *sbad = stap + MG_FPW_SLOTS;
    int32_t *snf = sbad + MG_FP_TILE, *si0 = snf + MG_FP_TILE;
    int ncand;
    const int64_t b0 = mg_item_tile_of<MG_FP_TILE>(ip->wg0, n, ncand);
    const double *Et = ip->Et, *mean = ip->mean;

    // the item's constants and the tile's latents
    mg_fp_stage_constants(a.base, ip, MG_FPW_SLOTS, sE, smean, sw, srec, smap, stap, sbad);
    {
        const int32_t *chan = (const int32_t *)(a.base + ip->off_chan);
        for (int e = tid; e < NC + D; e += 256) schan[e] = chan[e];      // (chan, then pos)
    }
    __syncthreads();
    mg_item_stage_latents<LAT_F64>(ip->lat, ld, b0, ncand, L, slat, sbad);
    for (int e = tid; e < ncand * Lt; e += 256) {                        // the time latents carry no flag: one that is not finite shows in the count
        const int c = e / Lt, k = e - c * Lt;
        sgam[e] = mg_load_lat<LAT_F64>(ip->gam, (b0 + c) * ld + k);
    }
    __syncthreads();

    // warp 1: the increments, x[i][cand]
    for (int e = tid; e < F * MG_FP_TILE; e += 256) {
        const int i = e / MG_FP_TILE, c = e - i * MG_FP_TILE;
        if (c < ncand) {
            const double *g = sgam + c * Lt;
            sx[e] = mg_tw_increment(ip->tphi, ip->tmean, i, Lt, [&](int l) { return g[l]; });
        }
    }
    __syncthreads();

    if (tid < 64) {
        // warp 2: one lane per candidate
        if (tid < ncand) {
            const int c = tid;
            const mg_tw_strided x = {sx + c, MG_FP_TILE};
            mg_tw_running_sum(x, x, F);
            const double stop = x[F - 2];
            int num = 0, T = 0, i0 = 0;
            double tmid = NAN;
            if (smooth) {
                // all three times from the smoothed row: the whole set of second derivatives, then 15 unsmoothed samples per time
                if (mg_tw_sample_count(stop, 1.0, num)) {
                    T = num + 2;
                    if (T >= MG_TW_SMOOTH_W) {
                        const double step = mg_tw_sample_step(stop, num);
                        const mg_tw_strided cpt = {scpt + c, MG_FP_TILE}, dpt = {sdpt + c, MG_FP_TILE};
                        mg_tw_second_derivatives(x, dpt, cpt, dpt, F, 1);   // (M takes dp's place)
                        auto smoothed_at = [&](int q) {
                            int row, base;
                            double u[MG_TW_SMOOTH_W];
                            mg_tw_smooth_window(q, T, &row, &base);
                            for (int k = 0; k < MG_TW_SMOOTH_W; k++) u[k] = mg_tw_row_sample(x, dpt, F, base + k, T, num, stop, step);
                            return mg_tw_smoothed(H + MG_TW_SMOOTH_W * row, u);
                        };
                        const double tfirst = smoothed_at(0), tlast = smoothed_at(T - 1);
                        mg_basis_row_dev(ip->knots, ip->NB + 4, tfirst, &si0[3 * c], swm + 12 * c);
                        mg_basis_row_dev(ip->knots, ip->NB + 4, tlast, &si0[3 * c + 2], swm + 12 * c + 8);
                        si0[3 * c + 1] = 0;
                        if (frame_idx < T) {
                            tmid = smoothed_at(frame_idx);
                            if (NC > 0) mg_basis_row_dev(ip->knots, ip->NB + 4, tmid, &si0[3 * c + 1], swm + 12 * c + 4);
                        }
                    } else {
                        sbad[c] = 1;                                        // no smoothed form: NaN in every output but n_frames
                    }
                }
                snf[c] = T;
                stmid[c] = tmid;
                if (ip->n_frames) ip->n_frames[b0 + c] = T;
                if (ip->time_mid) ip->time_mid[b0 + c] = tmid;
            } else {
                if (mg_tw_sample_count(stop, 1.0, num)) {
                    T = num + 2;
                    if (frame_idx == 0) tmid = 0.0;
                    else if (frame_idx == T - 1) tmid = (double)(F - 1);
                    else if (frame_idx < T && need_mid) {
                        const double t = mg_tw_sample_point(frame_idx - 1, num, stop, mg_tw_sample_step(stop, num));
                        const int i = mg_tw_interval(x, F, t);
                        const mg_tw_strided cpt = {scpt + c, MG_FP_TILE}, dpt = {sdpt + c, MG_FP_TILE};
                        const int top = F - 3 > 1 ? F - 3 : 1;
                        mg_tw_second_derivatives(x, dpt, cpt, dpt, F, i < 1 ? 1 : (i > top ? top : i));   // (M takes dp's place)
                        tmid = mg_tw_inverse_at(x, dpt, i, t);
                    }
                }
                const bool mid_ok = T > 0 && frame_idx < T;
                if (mid_ok && NC > 0) mg_basis_row_dev(ip->knots, ip->NB + 4, tmid, &i0, swm + 4 * c);
                snf[c] = T;
                si0[c] = i0;
                stmid[c] = tmid;
                if (ip->n_frames) ip->n_frames[b0 + c] = T;
                if (ip->time_mid) ip->time_mid[b0 + c] = mid_ok ? tmid : NAN;
            }
        }
    } else {
        // phase 1 on the other three waves: the end frames' control points
        mg_item_control_points(smean, sE, slat, ncand, NRS, L, scp, CS, tid - 64, 192);
    }
    __syncthreads();

    // smoothed: the root position at the candidate's first time, the root pose at its last one, the mid frame's channels at time_mid
    if (smooth) {
        const int NE = NC + MG_FPW_ENDS;
        for (int e = tid; e < ncand * NE; e += 256) {
            const int c = e / NE, ch = e - c * NE;
            if (sbad[c] || snf[c] <= 0) continue;
            if (ch < NC && frame_idx >= snf[c]) continue;
            const int slot = ch < NC ? 1 : (ch < NC + 3 ? 0 : 2);
            const int chan = ch < NC ? schan[ch] : (ch < NC + 3 ? ch - NC : ch - NC - 3);
            const double *s = slat + c * L;
            const size_t r0 = (size_t)si0[3 * c + slot] * D + (size_t)chan;
            double c4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const size_t r = r0 + (size_t)j * D;
                c4[j] = mg_control_point(mean[r], Et + r, R, L, [&](int k) { return s[k]; });
            }
            const double v = mg_taps4(swm + 12 * c + 4 * slot, c4, 1);
            if (ch < NC) smid[c * MS + ch] = v;
            else sends[c * MG_FPW_ENDS + (ch - NC)] = v;
        }
    }
    // mid: channel schan[ch] of every candidate's frame at ITS time_mid
    for (int e = tid; e < (smooth ? 0 : ncand * NC); e += 256) {
        const int c = e / NC, ch = e - c * NC;
        if (sbad[c] || snf[c] <= 0 || frame_idx >= snf[c]) continue;
        const double *s = slat + c * L;
        const size_t r0 = (size_t)si0[c] * D + (size_t)schan[ch];
        double c4[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const size_t r = r0 + (size_t)j * D;
            c4[j] = mg_control_point(mean[r], Et + r, R, L, [&](int k) { return s[k]; });
        }
        smid[c * MS + ch] = mg_taps4(swm + 4 * c, c4, 1);
    }
    __syncthreads();

    // phase 2: one (candidate, joint) per thread, and one thread per candidate for the root's outputs
    for (int e = tid; e < ncand * (J + 1); e += 256) {
        const int c = e / (J + 1), u = e - c * (J + 1);
        const double *cp = scp + c * CS;
        const int T = snf[c];
        const bool bad = sbad[c] != 0 || T <= 0;
        const double *ends = sends + c * MG_FPW_ENDS;
        auto channel = [&](int s, int d) {
            if (smooth) return bad ? 0.0 : ends[3 * s + d];                 // (slot 0: the first time's, slot 1: the last time's)
            return mg_fp_channel(cp, sw, smap, stap, D, s, d);
        };
        const int64_t b = b0 + c;
        const double s0[3] = {channel(0, 0), channel(0, 1), channel(0, 2)};
        if (u < J) {
            double *o = ip->points + (b * J + u) * 3;
            if (bad || frame_idx >= T) { o[0] = NAN; o[1] = NAN; o[2] = NAN; continue; }
            const double *mid = smid + c * MS;
            double p[3];
            mg_fk_position_table([&](int r) { return mid[spos[r]]; }, 0, srec + u * RS, p);
#pragma unroll
            for (int i = 0; i < 3; i++) o[i] = p[i] - s0[i];
        } else {
            mg_fp_root_outputs(ip, b, bad, s0, channel, 1);
        }
    }
}

struct mg_fpw_plan : mg_fp_plan {       // (w: the two end frames')
    std::vector<int32_t> chan;           // the mid frame's channels, then pos[D]
    int32_t NC = 0, need_mid = 0;
};

static int mg_fpw_plan_of(const char *who, int i, const mg_warped_feature_point_item &q, mg_fpw_plan &pl, bool smooth) {
    const mg_primitive *p = q.prim;
    const int D = p->D, F = p->F, NB = p->NB;
    int rc = mg_fp_refuse(who, i, D, q.skeleton, [&]() -> int {
        MG_ITEM_REFUSE(F < 4 || F > MG_FEATURE_POINTS_WARPED_MAX_F, "%s: item %d: %d canonical frames (4 .. %d supported)", who, i, F, MG_FEATURE_POINTS_WARPED_MAX_F);
        MG_ITEM_REFUSE(!p->d_Et64 || !p->d_mean || !p->d_knots || !p->d_tphi || !p->d_tmean || NB < 4 || (int)p->knots.size() != NB + 4,
                       "%s: item %d: the primitive has no float64 tables (%d basis functions)", who, i, NB);
        return MG_OK;
    });
    if (rc != MG_OK) return rc;
    // the two end frames: their basis rows (the host's mg_basis_row is mg_basis_row_dev statement for statement); of the rows of E' they
    // touch, the root position at time 0 and the root pose at time F - 1
    const double times[MG_FPW_SLOTS] = {0.0, (double)(F - 1)};
    std::vector<int32_t> first(MG_FPW_SLOTS);
    for (int s = 0; s < MG_FPW_SLOTS; s++) {
        mg_basis_row(p->knots.data(), NB + 4, times[s], &first[(size_t)s], &pl.w[4 * s]);
        MG_ITEM_REFUSE(first[(size_t)s] < 0 || first[(size_t)s] + 4 > NB, "%s: item %d: time %g takes control points %d .. %d of %d", who, i, times[s], first[(size_t)s],
                       first[(size_t)s] + 3, NB);
    }
    pl.rows = mg_feature_rows_of(D, first, {{0, 0, 3}, {1, 0, 7}});
    // the mid frame's channels: the root position and the quaternions along the listed joints' chains
    if ((rc = mg_fp_measure(who, i, D, q.n_joints > 0, pl)) != MG_OK) return rc;
    std::vector<int32_t> pos;
    pl.joints.compact(pl.chan, pos);
    pl.NC = (int32_t)pl.chan.size();
    pl.chan.insert(pl.chan.end(), pos.begin(), pos.end());
    pl.need_mid = smooth || q.n_joints > 0 || q.time_mid_dev != nullptr;   // (a smoothed item always inverts: its end times are the candidate's own)
    pl.lds = mg_fpw_layout_of(F, p->Lt, pl.need_mid, p->L, pl.rows.NRS, pl.rows.NCP, pl.NC, D, q.n_joints, pl.rec_stride, smooth ? 1 : 0).total_bytes;
    MG_ITEM_REFUSE(pl.lds > MG_FP_LDS_MAX, "%s: item %d: the tables (%d canonical frames x %d candidates, %d x %d control-point values, %d joints) do not fit LDS", who,
                   i, F, MG_FP_TILE, p->L, pl.rows.NRS, q.n_joints);
    MG_ITEM_REFUSE_GRID(who, i, q.n_samples, MG_FP_TILE);
    return MG_OK;
}

static int mg_fpw_check(const char *who, int32_t n_items, const mg_warped_feature_point_item *items, int latent_dtype, std::vector<mg_fpw_plan> &plans,
                        const uint8_t *smooth = nullptr) {
    typedef mg_warped_feature_point_item item;
    plans.resize((size_t)std::max(n_items, 0));
    int rc = mg_items_check(
        who, n_items, items, latent_dtype,
        [&](int i, const item &q) -> int {
            const mg_primitive *p = q.prim;
            MG_ITEM_REQUIRE(p->Lt > 0, "%s: item %d: the primitive has no time model", who, i);
            MG_ITEM_REQUIRE(q.time_offset >= 0 && q.time_offset + p->Lt <= q.ld, "%s: item %d reads time latent columns %lld .. %lld of %lld", who, i,
                            (long long)q.time_offset, (long long)(q.time_offset + p->Lt), (long long)q.ld);
            MG_ITEM_REQUIRE(q.time_offset >= q.latent_offset + p->L || q.latent_offset >= q.time_offset + p->Lt,
                            "%s: item %d: the spatial columns %lld .. %lld and the time columns %lld .. %lld overlap", who, i, (long long)q.latent_offset,
                            (long long)(q.latent_offset + p->L), (long long)q.time_offset, (long long)(q.time_offset + p->Lt));
            return MG_OK;
        },
        [&](int i, const item &q) -> int {
            MG_ITEM_REQUIRE(q.frame_idx >= 0, "%s: item %d: frame %d", who, i, q.frame_idx);
            MG_ITEM_REQUIRE(q.start_root_dev || q.points_dev || q.root_end_dev || q.heading_end_dev || q.heading_len_dev || q.time_mid_dev || q.n_frames_dev,
                            "%s: item %d: all outputs are NULL", who, i);
            return mg_fp_joint_list(who, i, q, plans[(size_t)i].joints);
        });
    if (rc != MG_OK) return rc;
    for (int i = 0; i < n_items; i++)
        if ((rc = mg_fpw_plan_of(who, i, items[i], plans[(size_t)i], smooth && smooth[i])) != MG_OK) return rc;
    return MG_OK;
}

// the members of the smoothed item beyond mg_fpw_item's (nothing for the plain one)
static void mg_fpw_fill_smooth(mg_fpw_item &, int, const uint8_t *, const double *) {}
static void mg_fpw_fill_smooth(mg_fpws_item &d, int i, const uint8_t *smooth, const double *H) { d.H = H; d.smooth = smooth[i] ? 1 : 0; }

// SMOOTH: mg_feature_points_warped_smoothed -- `smooth` one byte per item, a device table, LDS bits and a profile slot of its own
template <bool SMOOTH>
static int mg_fpw_run(const char *who, int32_t n_items, const mg_warped_feature_point_item *items, int latent_dtype, const std::vector<mg_fpw_plan> &plans,
                      const uint8_t *smooth = nullptr) {
    typedef typename mg_fpw_types<SMOOTH>::item ditem;
    typedef typename mg_fpw_types<SMOOTH>::args dargs;
    const size_t elem = latent_dtype == MG_F64 ? 8 : 4;
    auto samples_of = [&](int i) { return items[i].n_samples; };
    std::vector<int32_t> wg0;
    const std::vector<mg_item_launch> launches =
        mg_cut_items(n_items, samples_of, [&](int i) { return plans[(size_t)i].lds; }, MG_FP_TILE, MG_FEATURE_POINTS_MAX_ITEMS, wg0);
    if (launches.empty()) return MG_OK;
    mg_context *ctx = nullptr;
    for (int i = 0; i < n_items; i++)
        if (items[i].n_samples > 0) ctx = items[i].prim->ctx;
    const double *H = nullptr;
    if (SMOOTH) {
        const int rc0 = mg_savgol_table_dev(ctx, &H);
        if (rc0 != MG_OK) return rc0;
    }
    std::vector<unsigned char> table;    // the items, then every item's row list, map, channel list and chain records
    const int rc = mg_items_table<ditem>(who, n_items, samples_of, table, [&](int i, ditem &d, auto append) {
        const mg_warped_feature_point_item &q = items[i];
        const mg_primitive *p = q.prim;
        const mg_fpw_plan &pl = plans[(size_t)i];
        ctx = p->ctx;
        mg_fp_fill(d, q, pl, elem, wg0[(size_t)i], append);
        d.knots = p->d_knots; d.tphi = p->d_tphi; d.tmean = p->d_tmean;
        d.gam = (const char *)q.latents_dev + (size_t)q.time_offset * elem;
        d.time_mid = q.time_mid_dev; d.n_frames = q.n_frames_dev;
        d.Lt = p->Lt; d.F = p->F; d.NB = p->NB; d.NC = pl.NC;
        d.frame_idx = q.frame_idx; d.need_mid = pl.need_mid;
        d.off_chan = append(pl.chan); d.off_rec = append(pl.rec);
        mg_fpw_fill_smooth(d, i, smooth, H);
    });
    if (rc != MG_OK) return rc;
    return mg_items_launch(
        ctx, who, ctx->tab[SMOOTH ? MG_TABLE_FEATURE_POINTS_SMOOTHED : MG_TABLE_FEATURE_POINTS_WARPED], table.data(), table.size(),
        std::max(table.size() * 2, (size_t)64 * 1024), launches, latent_dtype, SMOOTH ? MG_LDS_FEATURE_POINTS_SMOOTHED_F32 : MG_LDS_FEATURE_POINTS_WARPED_F32,
        SMOOTH ? MG_LDS_FEATURE_POINTS_SMOOTHED_F64 : MG_LDS_FEATURE_POINTS_WARPED_F64, SMOOTH ? MG_PROF_FEATURE_POINTS_SMOOTHED : MG_PROF_FEATURE_POINTS_WARPED,
        [](auto LAT_F64) { return mg_feature_points_warped_kernel<decltype(LAT_F64)::value, SMOOTH>; },
        [](const char *base, const mg_item_launch &l) { return dargs{base, (const ditem *)base + l.first, l.n_items}; });
}

extern "C" int mg_feature_points_warped(int32_t n_items, const mg_warped_feature_point_item *items, int latent_dtype) {
    std::vector<mg_fpw_plan> plans;
    const int rc = mg_fpw_check("mg_feature_points_warped", n_items, items, latent_dtype, plans);
    if (rc != MG_OK) return rc;
    return mg_fpw_run<false>("mg_feature_points_warped", n_items, items, latent_dtype, plans);
}

// the _host twin of either form: host arrays in, host arrays out
template <bool SMOOTH>
static int mg_fpw_host(const char *who, int32_t n_items, const mg_warped_feature_point_item *items, const uint8_t *smooth, int latent_dtype) {
    typedef mg_warped_feature_point_item item;
    std::vector<mg_fpw_plan> plans;
    const int rc = mg_fpw_check(who, n_items, items, latent_dtype, plans, smooth);
    if (rc != MG_OK) return rc;
    const mg_item_output<item> outs[6] = {{&item::start_root_dev, 3, nullptr}, {&item::points_dev, 3, &item::n_joints}, {&item::root_end_dev, 2, nullptr},
                                          {&item::heading_end_dev, 2, nullptr}, {&item::heading_len_dev, 1, nullptr}, {&item::time_mid_dev, 1, nullptr}};
    return mg_items_host(who, n_items, items, latent_dtype, outs, [&](item *dev) {
        // the lengths are int32: a block of their own beside the float64 outputs'
        mg_workspace lens(dev[0].prim->ctx, who);
        std::vector<mg_staged> at((size_t)n_items);
        for (int i = 0; i < n_items; i++)
            if (items[i].n_samples > 0 && items[i].n_frames_dev) at[(size_t)i] = lens.out(items[i].n_frames_dev, (size_t)items[i].n_samples * 4);
        int rc2 = lens.upload();
        if (rc2 != MG_OK) return rc2;
        for (int i = 0; i < n_items; i++)
            if (items[i].n_samples > 0 && items[i].n_frames_dev) dev[i].n_frames_dev = at[(size_t)i].dev<int32_t>();
        if ((rc2 = mg_fpw_run<SMOOTH>(who, n_items, dev, latent_dtype, plans, smooth)) != MG_OK) return rc2;
        return lens.download();
    });
}

extern "C" int mg_feature_points_warped_host(int32_t n_items, const mg_warped_feature_point_item *items, int latent_dtype) {
    return mg_fpw_host<false>("mg_feature_points_warped_host", n_items, items, nullptr, latent_dtype);
}

extern "C" int mg_feature_points_warped_smoothed(int32_t n_items, const mg_warped_feature_point_item *items, const uint8_t *smooth, int latent_dtype) {
    const char *who = "mg_feature_points_warped_smoothed";
    MG_ITEM_REQUIRE(n_items <= 0 || smooth, "%s: smooth is NULL", who);
    std::vector<mg_fpw_plan> plans;
    const int rc = mg_fpw_check(who, n_items, items, latent_dtype, plans, smooth);
    if (rc != MG_OK) return rc;
    return mg_fpw_run<true>(who, n_items, items, latent_dtype, plans, smooth);
}

extern "C" int mg_feature_points_warped_smoothed_host(int32_t n_items, const mg_warped_feature_point_item *items, const uint8_t *smooth, int latent_dtype) {
    MG_ITEM_REQUIRE(n_items <= 0 || smooth, "mg_feature_points_warped_smoothed_host: smooth is NULL");
    return mg_fpw_host<true>("mg_feature_points_warped_smoothed_host", n_items, items, smooth, latent_dtype);
}
