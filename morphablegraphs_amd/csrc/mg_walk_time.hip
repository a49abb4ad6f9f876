// The TIME objective of a graph walk in ONE launch (gfx950 / MI355X), float64.
//
// The time optimisation of a walk (reference motion_generator/graph_walk_optimizer.py:107-123 over
// optimization/objective_functions.py:270-287 and constraints/time_constraints.py:40-102) scores the concatenated time latents of
// the steps of a window: the canonical time function of every step, the squared distance of the constrained keyframes from their
// desired times, and the average log-likelihood of the steps' mixtures on [spatial latents of the step | time latents of the
// candidate].  Step by step that is mg_time_function_canonical and mg_gmm_log_prob per step with a table of (n, F) numbers read
// back for the two or three of a row the error needs; here a workgroup owns 16 candidates for the WHOLE window:
//
//   units      2 per step, dealt round-robin to the workgroup's four waves:
//     time function   increments exp(tmean[i] + sum_l tphi[i][l] gamma[l]) (ascending fma chain from tmean[i]) by all lanes, 64
//                     canonical frames at a time into the wave's LDS; lanes < 16 add them in frame order, one chain per
//                     candidate carried across the chunks, t(i) = sum - 1: the bits of mg_time_function_kernel.  Of t only
//                     t(F - 1) and t at the step's constrained keyframes are kept (LDS); no (n, F) table exists.
//     mixture         the 16 x Lg tile [spatial | time] through mg_gmm_load_component / mg_gmm_apply_component / mg_gmm_exp_entry /
//                     mg_gmm_logsumexp with KK = the mixture's: the bits of mg_gmm_log_prob (float64 output) on those rows.
//   one workgroup barrier, then lanes < 16 of the workgroup state time_constraints.py:68-87 per candidate: every product and sum
//   rounded on its own (no contraction), constraints in list order, steps in step order.
//
// No grid barrier, no fences, nothing between the steps goes through global memory.  What grows with n_steps or n_constraints
// travels in a device table of the context (ctx->tab[MG_TABLE_WALK_TIME]), rewritten only when it differs from the last call's.
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_construct.h"
#include "mg_gmm_device.h"

#define MG_WTIME_LDS_MAX (150 * 1024)
#define MG_WTIME_CHUNK 64                     // canonical frames of a time function in LDS at a time
#define MG_WTIME_BS (MG_WTIME_CHUNK + 1)      // doubles per candidate in the chunk buffer (odd: lane-per-candidate reads hit 16 banks)

struct mg_wtime_step {              // one step as the kernel reads it
    const double *tphi, *tmean;     // [F][Lt], [F]; unused when Lt == 0 (t(i) = i)
    const double *spatial;          // [L] the step's fixed spatial latents
    const double *Ppack, *mPpad, *cst;
    int64_t lat_off;                // first column of the step's time latents in a row
    int32_t F, Lt, L, Lg, K, KKg, JT;
    int32_t con_first, con_count;   // the step's constraints: order[con_first .. con_first + con_count)
    int32_t pad;
};
struct mg_wtime_con {
    int32_t step;                   // -1: beyond the window (contributes 10000)
    int32_t kf;                     // the keyframe, from the start; -1: at or past F (contributes 0)
    double desired;
};

struct mg_wtime_args {
    const mg_wtime_step *steps;
    const mg_wtime_con *cons;       // list order
    const int32_t *order;           // constraint indices grouped by step
    const double *lat;
    double *obj, *err, *ll;
    int64_t B, ld;
    double start_keyframe, frame_time, error_scale, quality_scale;
    int32_t n_steps, n_cons, wave_doubles;
};

#define MG_WTIME_LDS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")   // one wave: its own LDS writes are visible to its reads in order

// the canonical time function of step s for the tile's candidates: t(F - 1) -> tend[s][16], t(keyframe) -> tkey[constraint][16]
__device__ __forceinline__ void mg_wtime_function(const mg_wtime_args &a, const mg_wtime_step &st, int s, int64_t b0, int ncand, double *buf, double *tend,
                                                  double *tkey, int lane) {
    const int cl = lane & 15, jj = lane >> 4;
    const int F = st.F, Lt = st.Lt;
    if (Lt == 0) {   // no time model: the identity
        if (lane < 16) tend[s * 16 + lane] = (double)(F - 1);
        for (int e = lane; e < 16 * st.con_count; e += 64) {
            const int ci = a.order[st.con_first + (e >> 4)];
            const int kf = a.cons[ci].kf;
            if (kf >= 0) tkey[ci * 16 + (e & 15)] = (double)kf;
        }
        MG_WTIME_LDS_SYNC();
        return;
    }
    const int c = cl < ncand ? cl : ncand - 1;                 // rows past the batch repeat the last one: finite work, never stored
    const double *gam = a.lat + (b0 + c) * a.ld + st.lat_off;
    double gl[16];
#pragma unroll
    for (int l = 0; l < 16; l++) gl[l] = gam[l < Lt ? l : Lt - 1];
    double acc = 0.0;                                          // lanes < 16: the candidate's running sum, one chain over all chunks
    for (int i0 = 0; i0 < F; i0 += MG_WTIME_CHUNK) {
        const int nfr = (F - i0) < MG_WTIME_CHUNK ? (F - i0) : MG_WTIME_CHUNK;
        for (int it = 0; it < MG_WTIME_CHUNK / 4; it++) {      // lane: candidate cl, frames jj, jj + 4, ...
            const int j = 4 * it + jj;
            if (j < nfr) {
                const int i = i0 + j;
                const double *ph = st.tphi + (size_t)i * Lt;
                double e = st.tmean[i];
#pragma unroll
                for (int l = 0; l < 16; l++)
                    if (l < Lt) e = fma(ph[l], gl[l], e);
                for (int l = 16; l < Lt; l++) e = fma(ph[l], gam[l], e);
                buf[cl * MG_WTIME_BS + j] = exp(e);
            }
        }
        MG_WTIME_LDS_SYNC();
        if (lane < 16) {
            double *r = buf + lane * MG_WTIME_BS;
            for (int j = 0; j < nfr; j++) {
                acc += r[j];
                r[j] = acc - 1.0;
            }
            if (i0 + nfr == F) tend[s * 16 + lane] = acc - 1.0;
        }
        MG_WTIME_LDS_SYNC();
        for (int e = lane; e < 16 * st.con_count; e += 64) {
            const int cand = e & 15, ci = a.order[st.con_first + (e >> 4)];
            const int kf = a.cons[ci].kf;
            if (kf >= i0 && kf < i0 + nfr) tkey[ci * 16 + cand] = buf[cand * MG_WTIME_BS + (kf - i0)];
        }
        MG_WTIME_LDS_SYNC();
    }
}

// log p of step s on the tile's rows [spatial | time latents]: mg_gmm_logp_mfma_kernel's statements by one wave -> out16[16]
template <int KK>
__device__ __forceinline__ void mg_wtime_logp(const mg_wtime_args &a, const mg_wtime_step &st, int64_t b0, int ncand, mg_lds_f64 *terms, mg_lds_f64 *out16,
                                              int lane) {
    const int cl = lane & 15, g = lane >> 4;
    const int L = st.L, Lg = st.Lg, K = st.K;
    const int c = cl < ncand ? cl : ncand - 1;
    const bool rok = cl < ncand;
    const double *row = a.lat + (b0 + c) * a.ld + st.lat_off;
    // A fragments: lane l holds [candidate l & 15][k = 4 kk + (l >> 4)], zero outside the tile / the mixture's width (mg_gmm_load_x)
    double xf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
        const int kq = 4 * kk + g;
        double v = 0.0;
        if (kq < L) v = st.spatial[kq];
        else if (kq < Lg) v = row[kq - L];
        xf[kk] = rok ? v : 0.0;
    }
    mg_lds_f64 *exps = terms + K * 16;
    for (int k = 0; k < K; k++) {
        mg_gmm_frag<KK> f;
        mg_gmm_load_component<KK>(f, st.Ppack, st.mPpad, st.cst, k, st.JT, lane, cl, K);
        mg_gmm_apply_component(f, k, st.JT, xf, terms, cl, g);
    }
    MG_WTIME_LDS_SYNC();
    for (int e = lane; e < K * 16; e += 64) exps[e] = mg_gmm_exp_entry(terms, K, e);
    MG_WTIME_LDS_SYNC();
    if (lane < 16) out16[lane] = mg_gmm_logsumexp(terms, exps, K, lane);
    MG_WTIME_LDS_SYNC();
}

// time_constraints.py:68-87 and objective_functions.py:270-287 for candidate `cand` of the tile; every operation rounded on its own
__device__ __forceinline__ void mg_wtime_finish(const mg_wtime_args &a, const double *tend, const double *logp, double *pref, const double *tkey, int cand,
                                                int64_t b) {
#pragma clang fp contract(off)
    bool finite = true;
    double n_before = a.start_keyframe;                         // frames before step k: start_keyframe + t_0(F - 1) + ... in step order
    double lp = 0.0;
    for (int k = 0; k < a.n_steps; k++) {
        pref[k * 16 + cand] = n_before;
        const double te = tend[k * 16 + cand];
        finite = finite && isfinite(te);
        n_before = n_before + te;
        lp = lp + logp[k * 16 + cand];
    }
    double err = 0.0;
    for (int ci = 0; ci < a.n_cons; ci++) {
        const mg_wtime_con con = a.cons[ci];
        double e;
        if (con.step < 0) e = 10000.0;
        else if (con.kf < 0) e = 0.0;
        else {
            const double t = tkey[ci * 16 + cand];
            finite = finite && isfinite(t);
            const double whole = isfinite(t) ? (double)(long long)t : 0.0;     // int(): towards zero
            const double n_frames = pref[con.step * 16 + cand] + (whole + 1.0);
            const double d = con.desired - n_frames * a.frame_time;
            e = d * d;
        }
        err = err + e;
    }
    const double avg = lp / (double)a.n_steps;
    const double nll = -avg;
    const double e_part = a.error_scale * err, q_part = nll * a.quality_scale;
    double obj = e_part + q_part;
    if (!finite) { err = NAN; obj = NAN; }
    a.obj[b] = obj;
    if (a.err) a.err[b] = err;
    if (a.ll) a.ll[b] = avg;
}

__global__ __launch_bounds__(256) void mg_walk_time_kernel(const mg_wtime_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ns = a.n_steps;
    double *tend = (double *)smem;                 // [n_steps][16] t_k(F_k - 1)
    double *logp = tend + 16 * ns;                 // [n_steps][16]
    double *pref = logp + 16 * ns;                 // [n_steps][16] frames before step k
    double *tkey = pref + 16 * ns;                 // [n_cons][16]  t at the constraint's keyframe
    const size_t shared = (size_t)48 * ns + (size_t)16 * a.n_cons;
    double *wbuf = (double *)smem + shared + (size_t)wave * a.wave_doubles;   // the wave's: a chunk of increments, or terms + exponentials
    mg_lds_f64 *wterms = (mg_lds_f64 *)smem + shared + (size_t)wave * a.wave_doubles;
    mg_lds_f64 *logp3 = (mg_lds_f64 *)smem + 16 * ns;
    const int64_t b0 = (int64_t)blockIdx.x * 16;
    const int ncand = (int)((a.B - b0) < 16 ? (a.B - b0) : 16);
    for (int u = wave; u < 2 * ns; u += 4) {
        const int s = u >> 1;
        const mg_wtime_step st = a.steps[s];
        if (u & 1) {
            mg_lds_f64 *o = logp3 + s * 16;
            switch (st.KKg) {
                case 2: mg_wtime_logp<2>(a, st, b0, ncand, wterms, o, lane); break;
                case 4: mg_wtime_logp<4>(a, st, b0, ncand, wterms, o, lane); break;
                case 6: mg_wtime_logp<6>(a, st, b0, ncand, wterms, o, lane); break;
                case 8: mg_wtime_logp<8>(a, st, b0, ncand, wterms, o, lane); break;
                case 10: mg_wtime_logp<10>(a, st, b0, ncand, wterms, o, lane); break;
                case 12: mg_wtime_logp<12>(a, st, b0, ncand, wterms, o, lane); break;
                case 14: mg_wtime_logp<14>(a, st, b0, ncand, wterms, o, lane); break;
                default: mg_wtime_logp<16>(a, st, b0, ncand, wterms, o, lane); break;
            }
        } else {
            mg_wtime_function(a, st, s, b0, ncand, wbuf, tend, tkey, lane);
        }
    }
    __syncthreads();
    if (tid < ncand) mg_wtime_finish(a, tend, logp, pref, tkey, tid, b0 + tid);
}

#define MG_WTIME_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)
#define MG_WTIME_REFUSE(cond, ...) MG_REQUIRE_AS(!(cond), MG_ERR_UNSUPPORTED, __VA_ARGS__)

extern "C" int mg_score_walk_time(int32_t n_steps, const mg_walk_time_step *steps, const void *latents_dev, int latent_dtype, int64_t n_samples, int64_t ld,
                                  int32_t n_constraints, const mg_walk_time_constraint *constraints, double start_keyframe, double frame_time, double error_scale,
                                  double quality_scale, double *objective_dev, double *error_dev, double *loglik_dev) {
    MG_WTIME_REQUIRE(n_steps >= 1 && steps && steps[0].prim, "mg_score_walk_time: no steps, or NULL pointer");
    MG_WTIME_REQUIRE(n_constraints >= 0 && (n_constraints == 0 || constraints), "mg_score_walk_time: %d constraints, or NULL pointer", n_constraints);
    MG_WTIME_REQUIRE((latent_dtype == MG_F32 || latent_dtype == MG_F64) && n_samples >= 0 && ld >= 0, "mg_score_walk_time: bad arguments");
    MG_WTIME_REFUSE(latent_dtype != MG_F64, "mg_score_walk_time: float64 latents only (the time optimisation's)");
    MG_WTIME_REFUSE(n_steps > MG_WALK_MAX_STEPS, "mg_score_walk_time: %d steps (1 .. %d per call)", n_steps, MG_WALK_MAX_STEPS);
    mg_context *ctx = steps[0].prim->ctx;
    const size_t o_cons = (size_t)n_steps * sizeof(mg_wtime_step), o_order = o_cons + (size_t)n_constraints * sizeof(mg_wtime_con);
    std::vector<unsigned char> tab(o_order + (size_t)n_constraints * sizeof(int32_t), 0);
    std::vector<mg_wtime_step> ds((size_t)n_steps);
    int kmax = 1;
    for (int i = 0; i < n_steps; i++) {
        const mg_walk_time_step &s = steps[i];
        const mg_primitive *p = s.prim;
        MG_WTIME_REQUIRE(p != nullptr, "mg_score_walk_time: primitive %d is NULL", i);
        MG_WTIME_REFUSE(p->ctx != ctx, "mg_score_walk_time: primitive %d belongs to another context", i);
        MG_WTIME_REQUIRE(s.spatial_dev != nullptr, "mg_score_walk_time: step %d: the spatial latents are NULL", i);
        MG_WTIME_REQUIRE(s.latent_offset >= 0 && s.latent_offset + p->Lt <= ld, "mg_score_walk_time: step %d reads latent columns %lld .. %lld of %lld", i,
                         (long long)s.latent_offset, (long long)(s.latent_offset + p->Lt), (long long)ld);
        MG_WTIME_REFUSE(p->K <= 0 || !p->d_gPpack || p->KKg < 2 || p->KKg > MG_MAX_KK || (p->KKg & 1) || (size_t)p->K * 16 * 16 > 60 * 1024,
                        "mg_score_walk_time: step %d: no in-kernel form of this mixture (%d components over %d dimensions)", i, p->K, p->Lg);
        MG_WTIME_REFUSE(p->Lg != p->L + p->Lt, "mg_score_walk_time: step %d: the mixture spans %d dimensions, the step's row %d + %d", i, p->Lg, p->L, p->Lt);
        MG_WTIME_REFUSE(p->Lt > 0 && (!p->d_tphi || !p->d_tmean), "mg_score_walk_time: step %d: the time model is not on the device", i);
        mg_wtime_step &d = ds[i];
        memset(&d, 0, sizeof(d));
        d.tphi = p->d_tphi; d.tmean = p->d_tmean; d.spatial = s.spatial_dev;
        d.Ppack = p->d_gPpack; d.mPpad = p->d_gmPpad; d.cst = p->d_gconst;
        d.lat_off = s.latent_offset;
        d.F = p->F; d.Lt = p->Lt; d.L = p->L; d.Lg = p->Lg; d.K = p->K; d.KKg = p->KKg; d.JT = (p->Lg + 15) / 16;
        kmax = std::max(kmax, (int)p->K);
    }
    std::vector<mg_wtime_con> dc((size_t)n_constraints);
    for (int c = 0; c < n_constraints; c++) {
        const mg_walk_time_constraint &q = constraints[c];
        const int si = q.step_index < 0 ? 0 : q.step_index;    // (the reference's loop takes the first step it meets: `k < step_index` never holds)
        mg_wtime_con &d = dc[c];
        d.desired = q.desired_time;
        if (si >= n_steps) { d.step = -1; d.kf = -1; continue; }
        const int F = ds[si].F;
        int64_t kf = q.keyframe_index;
        if (kf >= F) kf = -1;                                   // `keyframe_index >= len(time_function)`: no error
        else if (kf < 0) {
            kf += F;                                            // Python's indexing from the end
            MG_WTIME_REQUIRE(kf >= 0, "mg_score_walk_time: constraint %d: keyframe %d of a step with %d canonical frames", c, q.keyframe_index, F);
        }
        d.step = si; d.kf = (int32_t)kf;
        if (kf >= 0) ds[si].con_count++;
    }
    // the constraints whose keyframe value a step's time-function unit keeps, grouped by step
    std::vector<int32_t> order((size_t)n_constraints, 0), fill((size_t)n_steps, 0);
    for (int i = 0, first = 0; i < n_steps; i++) { ds[i].con_first = first; first += ds[i].con_count; }
    for (int c = 0; c < n_constraints; c++)
        if (dc[c].step >= 0 && dc[c].kf >= 0) order[(size_t)ds[dc[c].step].con_first + fill[dc[c].step]++] = c;
    if (n_steps) memcpy(tab.data(), ds.data(), o_cons);
    if (n_constraints) {
        memcpy(tab.data() + o_cons, dc.data(), (size_t)n_constraints * sizeof(mg_wtime_con));
        memcpy(tab.data() + o_order, order.data(), (size_t)n_constraints * sizeof(int32_t));
    }
    const int wave_doubles = std::max(16 * MG_WTIME_BS, 2 * kmax * 16);
    const size_t lds = ((size_t)48 * n_steps + (size_t)16 * n_constraints + (size_t)4 * wave_doubles) * 8;
    MG_WTIME_REFUSE(lds > MG_WTIME_LDS_MAX, "mg_score_walk_time: %d steps, %d constraints and mixtures of up to %d components do not fit LDS", n_steps, n_constraints, kmax);
    const int64_t grid = (n_samples + 15) / 16;
    MG_WTIME_REFUSE(grid > 0x7fffffff, "mg_score_walk_time: too many samples");
    if (n_samples == 0) return MG_OK;
    MG_WTIME_REQUIRE(latents_dev && objective_dev, "mg_score_walk_time: NULL pointer");
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[MG_TABLE_WALK_TIME];
    int rc = dt.upload(ctx, "mg_score_walk_time", tab.data(), tab.size(), (size_t)16 * 1024);
    if (rc != MG_OK) return rc;
    mg_wtime_args k = {};
    k.steps = (const mg_wtime_step *)dt.base();
    k.cons = (const mg_wtime_con *)(dt.base() + o_cons);
    k.order = (const int32_t *)(dt.base() + o_order);
    k.lat = (const double *)latents_dev; k.obj = objective_dev; k.err = error_dev; k.ll = loglik_dev;
    k.B = n_samples; k.ld = ld;
    k.start_keyframe = start_keyframe; k.frame_time = frame_time; k.error_scale = error_scale; k.quality_scale = quality_scale;
    k.n_steps = n_steps; k.n_cons = n_constraints; k.wave_doubles = wave_doubles;
    if (lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALK_TIME, 160 * 1024, mg_walk_time_kernel));
    mg_prof_begin(ctx, MG_PROF_WALK_TIME);
    hipLaunchKernelGGL(mg_walk_time_kernel, dim3((unsigned)grid), dim3(256), lds, ctx->stream, k);
    mg_prof_end(ctx, MG_PROF_WALK_TIME);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

// host arrays in (the steps' spatial latents too), host arrays out: one device block for the call, synchronises
extern "C" int mg_score_walk_time_host(int32_t n_steps, const mg_walk_time_step *steps, const void *latents, int latent_dtype, int64_t n_samples, int64_t ld,
                                       int32_t n_constraints, const mg_walk_time_constraint *constraints, double start_keyframe, double frame_time,
                                       double error_scale, double quality_scale, double *objective, double *error, double *loglik) {
    MG_WTIME_REQUIRE(n_steps >= 1 && steps && steps[0].prim && n_samples >= 0 && ld >= 0 && (latent_dtype == MG_F32 || latent_dtype == MG_F64),
                     "mg_score_walk_time_host: bad arguments");
    MG_WTIME_REFUSE(latent_dtype != MG_F64, "mg_score_walk_time_host: float64 latents only (the time optimisation's)");
    MG_WTIME_REFUSE(n_steps > MG_WALK_MAX_STEPS, "mg_score_walk_time_host: %d steps (1 .. %d per call)", n_steps, MG_WALK_MAX_STEPS);
    MG_WTIME_REQUIRE(n_samples == 0 || (latents && objective), "mg_score_walk_time_host: NULL pointer");
    for (int i = 0; i < n_steps; i++) MG_WTIME_REQUIRE(steps[i].prim && steps[i].spatial_dev, "mg_score_walk_time_host: step %d: NULL pointer", i);
    mg_context *ctx = steps[0].prim->ctx;
    const size_t lat_b = (size_t)(n_samples * ld) * 8, out_b = (size_t)n_samples * 8;
    mg_workspace ws(ctx, "mg_score_walk_time_host");
    const mg_staged d_lat = lat_b ? ws.in(latents, lat_b) : ws.room(8);    // (rows without columns still want a pointer)
    const mg_staged d_obj = ws.out(objective, out_b), d_err = ws.out(error, out_b), d_ll = ws.out(loglik, out_b);
    std::vector<mg_walk_time_step> dsteps(steps, steps + n_steps);
    std::vector<mg_staged> d_sp((size_t)n_steps);
    for (int i = 0; i < n_steps; i++) d_sp[i] = ws.in(steps[i].spatial_dev, (size_t)steps[i].prim->L * 8);
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    for (int i = 0; i < n_steps; i++) dsteps[i].spatial_dev = d_sp[i].dev<double>();
    rc = mg_score_walk_time(n_steps, dsteps.data(), d_lat.dev<void>(), latent_dtype, n_samples, ld, n_constraints, constraints, start_keyframe, frame_time,
                            error_scale, quality_scale, d_obj.dev<double>(), d_err.dev<double>(), d_ll.dev<double>());
    if (rc != MG_OK) return rc;
    return ws.download();
}
