// Point clouds without frames in memory (gfx950 / MI355X), float64: what the reference's map_motions_to_euclidean_space
// (space_partitioning/features.py:133-153) takes from every back-projected sample of a feature cluster tree's training set -- the global
// positions of a list of joints in every frame of a time grid (the builder's: the integer canonical frames 0 .. F - 1), a frame whose index
// is not a multiple of `step` repeating the cloud of the last one that is -- for n latent rows of one primitive in ONE launch: out (n, F, J, 3).
//
// A workgroup owns MG_PC_CANDS candidates, as mg_joint_tracks_kernel does, and keeps everything between the latents and the positions in
// LDS:
//
//   constants   the chain records of the J joints (mg_track_point's layout: chain length m, then m x (quaternion channel or -1, offset
//               xyz)) and the channel -> slot map, from the context's cached table (ctx->tab[MG_TABLE_POINT_CLOUDS])
//   staging     the candidates' latents and their control points of the channels the chains read (mg_track_control_points,
//               mg_frame_device.h: the float64 frames kernel's fma chains, E' from L2 once for all MG_PC_CANDS candidates)
//   clouds      one (candidate, kept frame, joint) per thread: the frame's channels by four taps, the chain walked (mg_track_point,
//               unaligned), then the position stored for the kept frame step * k and, from the same registers, for each of the up to
//               step - 1 frames that repeat it.  Nothing is evaluated twice
//
// The same operations on the same values as mg_back_project_frames_f64 -> mg_joint_positions -> the host's repeat rule: the clouds are
// that route's, bit for bit (tests/test_gpu_point_cloud_features.py), and 24 bytes per (candidate, frame, joint) leave the chip.
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_frame_device.h"
#include "mg_joint_plan.h"

#define MG_PC_BLOCK 256
#define MG_PC_CANDS 4
#define MG_PC_LDS_MAX (160 * 1024 - 64)

struct mg_pc_args {
    const double *Et64, *mean;
    const void *lat;
    int64_t B, ld;
    int32_t L, R, D, NB, lat_f64, n_chan, J, F, step, NK, rec_stride, reserved;   // NK: kept frames, ceil(F / step)
    const double *records;           // [J][rec_stride]
    const int32_t *chan, *slot;      // [n_chan] kept channels; [D] channel -> slot or -1
    const int32_t *i0;               // the grid's first taps [F] and basis rows [F][4]
    const double *w;
    double *out;                     // (B, F, J, 3)
};

// LDS of a workgroup in bytes: cp [CANDS][NB][n_chan], latents [CANDS][L], records [J][rec_stride], then int32 slot[D]
static inline size_t mg_pc_lds_bytes(int NB, int n_chan, int L, int J, int rec_stride, int D) {
    return ((size_t)MG_PC_CANDS * ((size_t)NB * n_chan + L) + (size_t)J * rec_stride) * 8 + (size_t)D * 4 + 16;
}

__global__ __launch_bounds__(MG_PC_BLOCK) void mg_point_clouds_kernel(const mg_pc_args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, nc = a.n_chan, D = a.D, L = a.L, J = a.J, F = a.F, step = a.step, NK = a.NK, RS = a.rec_stride;
    const int ncp = a.NB * nc;
    double *cp_all = (double *)smem;
    double *s_all = cp_all + (size_t)MG_PC_CANDS * ncp;
    double *srec = s_all + (size_t)MG_PC_CANDS * L;
    int *slot = (int *)(srec + (size_t)J * RS);
    const int64_t b0 = (int64_t)blockIdx.x * MG_PC_CANDS;
    for (int e = tid; e < J * RS; e += MG_PC_BLOCK) srec[e] = a.records[e];
    for (int d = tid; d < D; d += MG_PC_BLOCK) slot[d] = a.slot[d];
    for (int e = tid; e < MG_PC_CANDS * L; e += MG_PC_BLOCK) {
        const int c = e / L, k = e - c * L;
        const int64_t bb = b0 + c < a.B ? b0 + c : a.B - 1;        // (unconditional loads on a clamped row: a short last group repeats the last candidate)
        s_all[e] = mg_load_lat(a.lat, a.lat_f64 != 0, bb * a.ld + k);
    }
    __syncthreads();
    mg_track_control_points<MG_PC_CANDS, MG_PC_BLOCK>(a.Et64, a.mean, L, a.R, D, a.NB, nc, a.chan, s_all, cp_all);
    __syncthreads();
    const int n_here = a.B - b0 < MG_PC_CANDS ? (int)(a.B - b0) : MG_PC_CANDS;
    const int per = NK * J;
    for (int ce = tid; ce < n_here * per; ce += MG_PC_BLOCK) {
        const int c = ce / per, e = ce - c * per;
        const int kf = e / J, j = e - kf * J;
        const int f0 = kf * step;                                  // (NK = ceil(F / step): f0 < F)
        const int f1 = F - f0 < step ? F : f0 + step;              // its repeats end here
        double p[3];
        mg_track_point(cp_all + (size_t)c * ncp, nc, [&](int ch) { return slot[ch]; }, a.i0[f0], a.w + 4 * (size_t)f0, srec + (size_t)j * RS, false, nullptr, D, p);
        double *o = a.out + (((b0 + c) * (int64_t)F + f0) * J + j) * 3;
        for (int f = f0; f < f1; f++, o += (size_t)J * 3) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
    }
}

extern "C" int mg_point_cloud_features(mg_primitive *p, const mg_time_grid *grid, const mg_skeleton_desc *sk, const int32_t *joints, int32_t n_joints, int32_t step, const void *latents_dev,
                                       int latent_dtype, int64_t n, int64_t ld, double *out_dev) {
    const char *who = "mg_point_cloud_features";
    MG_REQUIRE(p && p->ctx, "%s: the primitive is NULL", who);
    MG_REQUIRE(latent_dtype == MG_F32 || latent_dtype == MG_F64, "%s: bad latent dtype %d", who, latent_dtype);
    MG_REQUIRE(n >= 0 && ld >= p->L, "%s: %lld samples, ld %lld for %d components", who, (long long)n, (long long)ld, p->L);
    MG_REQUIRE(step >= 1, "%s: step %d", who, step);
    MG_REQUIRE(n_joints >= 1 && n_joints <= MG_FEATURE_POINTS_MAX_JOINTS, "%s: %d joints (1 .. %d)", who, n_joints, MG_FEATURE_POINTS_MAX_JOINTS);
    MG_REQUIRE(sk && joints, "%s: no skeleton or no joint list", who);
    MG_REQUIRE(mg_skeleton_complete(sk), "%s: incomplete skeleton", who);
    MG_REQUIRE(out_dev && (n == 0 || latents_dev), "%s: NULL buffer", who);
    mg_joint_plan plan;
    mg_plan_failure f = plan.check(sk, joints, n_joints);
    MG_REQUIRE(!f, "%s: joint %d%s", who, f.joint, mg_chain_why(f.kind));
    // what the kernel does not take
    const mg_time_grid *g = grid ? grid : p->canonical;
    MG_REQUIRE(!grid || grid->prim == p, "%s: the grid belongs to another primitive", who);
    const int D = p->D, F = g ? g->T : 0, NB = p->NB;
    MG_REQUIRE_AS(D >= 7, MG_ERR_UNSUPPORTED, "%s: the primitive has %d channels, a root pose needs 7", who, D);
    MG_REQUIRE_AS(g && F >= 1 && p->d_Et64 && p->d_mean && g->d_i0 && g->d_w && (int)g->i0.size() == F, MG_ERR_UNSUPPORTED,
                  "%s: the primitive has no float64 tables or the grid no basis rows (%d frames)", who, F);
    for (int f = 0; f < F; f++)
        MG_REQUIRE_AS(g->i0[(size_t)f] >= 0 && g->i0[(size_t)f] + 4 <= NB, MG_ERR_UNSUPPORTED, "%s: frame %d takes control points %d .. %d of %d", who, f,
                      g->i0[(size_t)f], g->i0[(size_t)f] + 3, NB);
    f = plan.measure(D, true);
    MG_REQUIRE_AS(f.kind != MG_PLAN_TOO_LONG, MG_ERR_UNSUPPORTED, "%s: chain of %d joints exceeds %d", who, f.length, MG_MAX_CHAIN);
    MG_REQUIRE_AS(f.kind != MG_PLAN_CHANNEL_OUTSIDE, MG_ERR_UNSUPPORTED, "%s: the skeleton's joint %d has channels %d .. %d, the primitive %d", who, f.joint, f.channel,
                  f.channel + 3, D);
    // the cached table: the records, then the kept channels and the channel -> slot map
    std::vector<double> rec;
    const int32_t RS = plan.records(1, 0, rec);
    std::vector<int32_t> chan, slot;
    plan.compact(chan, slot);
    const int n_chan = (int)chan.size();
    const size_t lds = (int64_t)NB * n_chan > (1 << 20) ? (size_t)MG_PC_LDS_MAX + 1 : mg_pc_lds_bytes(NB, n_chan, p->L, n_joints, RS, D);
    MG_REQUIRE_AS(lds <= MG_PC_LDS_MAX, MG_ERR_UNSUPPORTED, "%s: %d basis functions x %d channels for %d candidates and %d joints' chains do not fit LDS", who, NB,
                  n_chan, MG_PC_CANDS, n_joints);
    MG_REQUIRE_AS((n + MG_PC_CANDS - 1) / MG_PC_CANDS <= 0x7fffffff, MG_ERR_UNSUPPORTED, "%s: too many samples", who);
    if (n == 0) return MG_OK;
    mg_context *ctx = p->ctx;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<unsigned char> table(rec.size() * 8 + (chan.size() + slot.size()) * 4);
    memcpy(table.data(), rec.data(), rec.size() * 8);
    memcpy(table.data() + rec.size() * 8, chan.data(), chan.size() * 4);
    memcpy(table.data() + rec.size() * 8 + chan.size() * 4, slot.data(), slot.size() * 4);
    mg_device_table &dt = ctx->tab[MG_TABLE_POINT_CLOUDS];
    const int rc = dt.upload(ctx, who, table.data(), table.size(), 64 * 1024);
    if (rc != MG_OK) return rc;
    mg_pc_args a = {};
    a.Et64 = p->d_Et64; a.mean = p->d_mean; a.lat = latents_dev; a.B = n; a.ld = ld;
    a.L = p->L; a.R = p->R; a.D = D; a.NB = NB; a.lat_f64 = latent_dtype == MG_F64 ? 1 : 0; a.n_chan = n_chan; a.J = n_joints; a.F = F; a.step = step;
    a.NK = (int32_t)(((int64_t)F + step - 1) / step); a.rec_stride = RS;
    a.records = (const double *)dt.base();
    a.chan = (const int32_t *)(dt.base() + rec.size() * 8);
    a.slot = a.chan + chan.size();
    a.i0 = g->d_i0; a.w = g->d_w; a.out = out_dev;
    if (lds > 48 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_POINT_CLOUDS, 160 * 1024, mg_point_clouds_kernel));
    mg_prof_begin(ctx, MG_PROF_POINT_CLOUDS);
    hipLaunchKernelGGL(mg_point_clouds_kernel, dim3((unsigned)((n + MG_PC_CANDS - 1) / MG_PC_CANDS)), dim3(MG_PC_BLOCK), lds, ctx->stream, a);
    mg_prof_end(ctx, MG_PROF_POINT_CLOUDS);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}
