// The objective of a whole graph walk in ONE launch (gfx950 / MI355X), float64.
//
// The global spatial optimisation of a walk (reference motion_generator/graph_walk_optimizer.py:78-105 over
// optimization/objective_functions.py:290-380) scores the concatenated latents of all steps: every step's constraints are
// evaluated against the step before it, and the four numbers of the aligned motion's exit pose (heading x, z; root x, z) are what
// the next step is aligned to.  mg_score_constraint_residuals[_chained] does one step per launch and hands the four numbers
// through the host; here a wave owns 16 candidates for the WHOLE walk and keeps them in its LDS:
//
//   per step, per constraint set of the step (the scored one, then -- a local step -- the set of the four exit values):
//     channels   X (16 x L) . W^T + bias on the float64 matrix pipe, chained v_mfma_f64_16x16x4_f64 from the set's Wpack / bpad, k
//                ascending from the bias: the chains of mg_score_mfma_kernel<KK> with KK read from the step's record.  A set
//                without packed matrix (n_components > 64) stages the latent tile in LDS and forms a channel where the residual
//                reads it, an fma chain over W / bias: mg_score_kernel's statement;
//     residuals  mg_constraint_residual on the wave's slab, lanes over (candidate, constraint) pairs; a chained set reads its
//                candidate's alignment values from the wave's state instead of the set's record;
//     own part   the step's own columns go to their place in the residual row, lanes < 16 add them in constraint order;
//     state      the set's last four residuals become the wave's state ([16][4]).
//
// No workgroup-wide barrier, no grid barrier, nothing between the steps goes through global memory.  What grows with n_steps
// travels in a device table of the context (ctx->tab[MG_TABLE_WALK_SCORE]), rewritten only when it differs from the last call's.
#include <cstring>

#include <algorithm>
#include <vector>

#include "mg_construct.h"
#include "mg_gmm_device.h"
#include "mg_score_device.h"

#define MG_WSCORE_LDS_MAX (150 * 1024)

struct mg_wscore_set {           // one constraint set of a step as the kernel reads it
    mg_score_args a;             // the set's tables, n, nch, L (lat, out, res, B, ld unused; align_cand set by the kernel)
    const double *Wpack, *bpad;  // NULL: the fma chains over a.W / a.bias
    int32_t RT;
    int32_t chained;             // the alignment values are the wave's state
    int32_t carries_exit;        // its last four residuals are the next state
    int32_t n_own;               // its first n_own residuals are columns of the residual row ...
    int64_t col_off;             // ... from this column on
};
struct mg_wscore_step {
    mg_wscore_set set[2];
    int64_t lat_off;
    int32_t n_sets, KK, L, pad;
};

struct mg_wscore_args {
    const mg_wscore_step *steps;
    const void *lat;
    double *res, *err, *exit_state;
    double *step_exits;          // NULL, or (B, n_steps, 4): the state every step hands on (mg_score_walk_residuals_steps)
    int64_t B, ld, ld_res;
    int32_t n_steps;
    int32_t vs;                  // doubles per candidate in the channel slab (16 x the most row tiles of a set, + 1)
    int32_t nmax;                // the most constraints of a set
    int32_t xs;                  // doubles per candidate in the staged latent tile (0: every set has a packed matrix)
};

template <bool LAT_F64>
__global__ __launch_bounds__(256) void mg_walk_score_kernel(const mg_wscore_args k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef typename mg_gmm_xt<LAT_F64>::type T;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 15, g = lane >> 4;
    const int vs = k.vs;
    const size_t per_wave = (size_t)16 * vs + (size_t)k.nmax * 16 + 64 + (size_t)16 * k.xs;
    double *vals = (double *)smem + (size_t)wave * per_wave;   // [16][vs]
    double *resid = vals + 16 * vs;                             // [nmax][16]
    double *state = resid + (size_t)k.nmax * 16;                // [16][4]: previous heading (x, z), previous root (x, z)
    double *xt = state + 64;                                    // [16][xs]
    const int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (b0 >= k.B) return;                                      // no workgroup-wide barrier below
    const int ncand = (int)((k.B - b0) < 16 ? (k.B - b0) : 16);
    const int crow = cl < ncand ? cl : ncand - 1;
    const bool rok = cl < ncand;
    double err = 0.0;                                           // lanes < ncand: the candidate's sum so far
    for (int i = 0; i < k.n_steps; i++) {
        const mg_wscore_step *st = k.steps + i;
        const int L = st->L, KK = st->KK;
        const T *row = (const T *)k.lat + (b0 + crow) * k.ld + st->lat_off;
        // A fragments of the step's latent tile: lane l holds [candidate l & 15][k = 4 kk + (l >> 4)], zero outside (what
        // mg_gmm_load_x returns); KK is the step's, so the registers are those of the widest and the loads stop at KK
        T xf[MG_MAX_KK];
#pragma unroll
        for (int kk = 0; kk < MG_MAX_KK; kk++) {
            xf[kk] = (T)0;
            if (kk < KK) {
                const int kq = 4 * kk + g;
                const T v = row[kq < L ? kq : L - 1];
                xf[kk] = (rok && kq < L) ? v : (T)0;
            }
        }
        for (int s = 0; s < st->n_sets; s++) {
            const mg_wscore_set *ws = &st->set[s];
            mg_score_args a = ws->a;
            a.align_cand = ws->chained ? state : nullptr;       // mg_candidate_alignment reads align_cand + cand * 4: cand is the tile's
            const double *Wpack = ws->Wpack, *bpad = ws->bpad;
            const bool packed = Wpack != nullptr;
            if (packed) {
                const int RT = ws->RT;
                for (int rt = 0; rt < RT; rt++) {
                    const double *wp = Wpack + ((size_t)rt * KK) * 64 + lane;
                    const double c0 = bpad[rt * 16 + cl];
                    mg_f64x4 acc = {c0, c0, c0, c0};
#pragma unroll
                    for (int kk = 0; kk < MG_MAX_KK; kk++)
                        if (kk < KK) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xf[kk], wp[kk * 64], acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; r++) vals[(g + 4 * r) * vs + rt * 16 + cl] = acc[r];   // C layout: col = row index, row = candidate
                }
            } else {
                for (int e = lane; e < 16 * L; e += 64) {       // the latent tile, rows past the batch zero
                    const int c = e / L, j = e - c * L;
                    double v = 0.0;
                    if (c < ncand) v = (double)((const T *)k.lat)[(b0 + c) * k.ld + st->lat_off + j];
                    xt[c * k.xs + j] = v;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // one wave: its own LDS writes are visible to its reads in order
            for (int e = lane; e < 16 * a.n; e += 64) {
                const int cand = e & 15, c = e >> 4;
                const double *v = vals + cand * vs;
                const double *x = xt + cand * k.xs;
                auto channel = [&](int r) {
                    if (packed) return v[r];
                    const double *wr = a.W + (size_t)r * L;     // mg_score_kernel's dot product: fma chain over k from the bias
                    double acc = a.bias[r];
                    for (int q = 0; q < L; q++) acc = fma(wr[q], x[q], acc);
                    return acc;
                };
                resid[c * 16 + cand] = mg_constraint_residual(a, c, channel, cand);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int n_own = ws->n_own;
            if (k.res)
                for (int e = lane; e < ncand * n_own; e += 64) {
                    const int cand = e / n_own, c = e - cand * n_own;
                    k.res[(b0 + cand) * k.ld_res + ws->col_off + c] = resid[c * 16 + cand];
                }
            if (lane < ncand && n_own > 0) {
                double sum = 0.0;
                for (int c = 0; c < n_own; c++) sum += resid[c * 16 + lane];
                err += sum;
            }
            if (ws->carries_exit) state[cl * 4 + g] = resid[(a.n - 4 + g) * 16 + cl];   // every residual that read the old state is in `resid`
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        // the state the wave is about to hand on (a lane reads back the value it wrote itself)
        if (k.step_exits && cl < ncand) k.step_exits[((b0 + cl) * k.n_steps + i) * 4 + g] = state[cl * 4 + g];
    }
    if (k.err && lane < ncand) k.err[b0 + lane] = err;
    if (k.exit_state && cl < ncand) k.exit_state[(b0 + cl) * 4 + g] = state[cl * 4 + g];
}

#define MG_WSCORE_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)

// the four exit values a set may end with: heading x, z, then position x, z (par rows: type, weight, component)
static bool mg_wscore_ends_with_exits(const mg_constraint_set *cs) {
    if (cs->n < 4 || (int)cs->structure.size() != cs->n) return false;
    const mg_keyframe_constraint *c = cs->structure.data() + (cs->n - 4);
    return c[0].type == MG_CONSTRAINT_VALUE_HEADING && c[1].type == MG_CONSTRAINT_VALUE_HEADING && c[2].type == MG_CONSTRAINT_VALUE_POSITION &&
           c[3].type == MG_CONSTRAINT_VALUE_POSITION;
}

extern "C" int mg_score_walk_residuals_steps(int32_t n_steps, const mg_walk_score_step *steps, const void *latents_dev, int latent_dtype, int64_t n_samples,
                                             int64_t ld, double *residuals_dev, int64_t ld_res, double *errors_dev, double *exit_state_dev,
                                             double *step_exits_dev) {
    MG_WSCORE_REQUIRE(n_steps >= 1 && n_steps <= MG_WALK_MAX_STEPS, "mg_score_walk_residuals: %d steps (1 .. %d per call)", n_steps, MG_WALK_MAX_STEPS);
    MG_WSCORE_REQUIRE(steps && steps[0].prim, "mg_score_walk_residuals: NULL pointer");
    MG_WSCORE_REQUIRE((latent_dtype == MG_F32 || latent_dtype == MG_F64) && n_samples >= 0 && ld >= 1 && ld_res >= 0, "mg_score_walk_residuals: bad arguments");
    mg_context *ctx = steps[0].prim->ctx;
    const bool force_valu = ctx->opt[MG_OPT_FORCE_VALU_SCORE] != 0;
    std::vector<unsigned char> tab((size_t)n_steps * sizeof(mg_wscore_step), 0);
    std::vector<std::pair<int64_t, int64_t>> spans;
    int rtmax = 0, nmax = 1, xs = 0;
    for (int i = 0; i < n_steps; i++) {
        const mg_walk_score_step &s = steps[i];
        const mg_primitive *p = s.prim;
        MG_WSCORE_REQUIRE(p != nullptr, "mg_score_walk_residuals: primitive %d is NULL", i);
        MG_WSCORE_REQUIRE(p->ctx == ctx, "mg_score_walk_residuals: primitive %d belongs to another context", i);
        MG_WSCORE_REQUIRE(s.latent_offset >= 0 && s.latent_offset + p->L <= ld, "mg_score_walk_residuals: step %d reads latent columns %lld .. %lld of %lld", i,
                          (long long)s.latent_offset, (long long)(s.latent_offset + p->L), (long long)ld);
        MG_WSCORE_REQUIRE(!s.scored || s.scored->prim == p, "mg_score_walk_residuals: step %d: the scored set belongs to another primitive", i);
        MG_WSCORE_REQUIRE(!s.exit || s.exit->prim == p, "mg_score_walk_residuals: step %d: the exit set belongs to another primitive", i);
        const bool scored_exits = s.scored && mg_wscore_ends_with_exits(s.scored);
        if (s.exit) {
            MG_WSCORE_REQUIRE(s.exit->n == 4 && mg_wscore_ends_with_exits(s.exit), "mg_score_walk_residuals: step %d: the exit set must hold exactly the four exit values", i);
            MG_WSCORE_REQUIRE(!s.scored || s.n_own == s.scored->n, "mg_score_walk_residuals: step %d: n_own %d, the scored set has %d constraints beside an exit set", i,
                              s.n_own, s.scored->n);
            MG_WSCORE_REQUIRE(s.scored || s.n_own == 0, "mg_score_walk_residuals: step %d: n_own %d without a scored set", i, s.n_own);
        } else {
            MG_WSCORE_REQUIRE(scored_exits, "mg_score_walk_residuals: step %d: no exit set, and the scored set does not end with the four exit values", i);
            MG_WSCORE_REQUIRE(s.n_own == s.scored->n - 4, "mg_score_walk_residuals: step %d: n_own %d, the scored set has %d constraints and the four exit values", i,
                              s.n_own, s.scored->n - 4);
        }
        const mg_constraint_set *carrier = s.exit ? s.exit : s.scored;
        if (i > 0) {
            MG_WSCORE_REQUIRE(carrier->d_align != nullptr && carrier->align_joint >= 0,
                              "mg_score_walk_residuals: step %d: the set with the exit values needs a previous-frame alignment (its node and reference vector; the values are per candidate)", i);
            MG_WSCORE_REQUIRE(!s.exit || !s.scored || !s.scored->d_align || s.scored->align_joint >= 0,
                              "mg_score_walk_residuals: step %d: the scored set's alignment is not a previous-frame record", i);
        }
        if (s.n_own > 0) {
            MG_WSCORE_REQUIRE(s.column_offset >= 0 && s.column_offset + s.n_own <= ld_res, "mg_score_walk_residuals: step %d writes residual columns %lld .. %lld of %lld", i,
                              (long long)s.column_offset, (long long)(s.column_offset + s.n_own), (long long)ld_res);
            spans.push_back({s.column_offset, (int64_t)s.n_own});
        }
        mg_wscore_step d;
        memset(&d, 0, sizeof(d));
        d.lat_off = s.latent_offset; d.KK = p->KK; d.L = p->L;
        const mg_constraint_set *sets[2] = {s.scored, s.exit};
        for (int e = 0; e < 2; e++) {
            const mg_constraint_set *cs = sets[e];
            if (!cs || cs->n == 0) continue;
            mg_wscore_set &w = d.set[d.n_sets++];
            w.a = mg_score_args_of(cs, p->L);
            const bool packed = cs->d_Wpack && !force_valu;
            w.Wpack = packed ? cs->d_Wpack : nullptr; w.bpad = packed ? cs->d_bpad : nullptr; w.RT = packed ? cs->RT : 0;
            w.chained = (i > 0 && cs->d_align) ? 1 : 0;
            w.carries_exit = cs == carrier ? 1 : 0;
            w.n_own = cs == s.scored ? s.n_own : 0;
            w.col_off = s.column_offset;
            if (packed) rtmax = std::max(rtmax, (int)cs->RT);
            else xs = std::max(xs, (int)p->L + 1);
            nmax = std::max(nmax, (int)cs->n);
        }
        memcpy(tab.data() + (size_t)i * sizeof(mg_wscore_step), &d, sizeof(d));
    }
    std::sort(spans.begin(), spans.end());
    int64_t end = 0;
    for (const auto &sp : spans) {
        MG_WSCORE_REQUIRE(sp.first >= end, "mg_score_walk_residuals: steps' residual columns overlap at column %lld", (long long)sp.first);
        end = sp.first + sp.second;
    }
    const int vs = rtmax * 16 + 1;
    const size_t lds = (size_t)4 * ((size_t)16 * vs + (size_t)nmax * 16 + 64 + (size_t)16 * xs) * 8;
    MG_REQUIRE_AS(lds <= MG_WSCORE_LDS_MAX, MG_ERR_UNSUPPORTED, "mg_score_walk_residuals: %d row tiles, %d constraints and %d staged latents per step do not fit LDS", rtmax,
                  nmax, xs);
    const int64_t grid = (n_samples + 63) / 64;
    MG_REQUIRE_AS(grid <= 0x7fffffff, MG_ERR_UNSUPPORTED, "mg_score_walk_residuals: too many samples");
    if (n_samples == 0) return MG_OK;
    MG_WSCORE_REQUIRE(latents_dev && (residuals_dev || errors_dev || exit_state_dev || step_exits_dev), "mg_score_walk_residuals: NULL pointer");
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[MG_TABLE_WALK_SCORE];
    int rc = dt.upload(ctx, "mg_score_walk_residuals", tab.data(), tab.size(), (size_t)MG_WALK_MAX_STEPS * sizeof(mg_wscore_step));   // one allocation per context
    if (rc != MG_OK) return rc;
    mg_wscore_args k = {};
    k.steps = (const mg_wscore_step *)dt.base();
    k.lat = latents_dev; k.res = residuals_dev; k.err = errors_dev; k.exit_state = exit_state_dev; k.step_exits = step_exits_dev;
    k.B = n_samples; k.ld = ld; k.ld_res = ld_res;
    k.n_steps = n_steps; k.vs = vs; k.nmax = nmax; k.xs = xs;
    if (lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALK_SCORE, 160 * 1024, mg_walk_score_kernel<true>, mg_walk_score_kernel<false>));
    mg_prof_begin(ctx, MG_PROF_SCORE_CONSTRAINTS);
    if (latent_dtype == MG_F64) hipLaunchKernelGGL(mg_walk_score_kernel<true>, dim3((unsigned)grid), dim3(256), lds, ctx->stream, k);
    else hipLaunchKernelGGL(mg_walk_score_kernel<false>, dim3((unsigned)grid), dim3(256), lds, ctx->stream, k);
    mg_prof_end(ctx, MG_PROF_SCORE_CONSTRAINTS);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

extern "C" int mg_score_walk_residuals(int32_t n_steps, const mg_walk_score_step *steps, const void *latents_dev, int latent_dtype, int64_t n_samples,
                                       int64_t ld, double *residuals_dev, int64_t ld_res, double *errors_dev, double *exit_state_dev) {
    return mg_score_walk_residuals_steps(n_steps, steps, latents_dev, latent_dtype, n_samples, ld, residuals_dev, ld_res, errors_dev, exit_state_dev, nullptr);
}

// host arrays in, host arrays out: one device block for the call, synchronises.  `residuals` is read first, so columns no step
// owns keep their values.
extern "C" int mg_score_walk_residuals_steps_host(int32_t n_steps, const mg_walk_score_step *steps, const void *latents, int latent_dtype, int64_t n_samples,
                                                  int64_t ld, double *residuals, int64_t ld_res, double *errors, double *exit_state, double *step_exits) {
    MG_WSCORE_REQUIRE(n_steps >= 1 && steps && steps[0].prim && n_samples >= 0 && ld >= 1 && ld_res >= 0 && (latent_dtype == MG_F32 || latent_dtype == MG_F64),
                      "mg_score_walk_residuals_host: bad arguments");
    MG_WSCORE_REQUIRE(n_samples == 0 || (latents && (residuals || errors || exit_state || step_exits)), "mg_score_walk_residuals_host: NULL pointer");
    mg_context *ctx = steps[0].prim->ctx;
    mg_workspace ws(ctx, "mg_score_walk_residuals_host");
    const mg_staged d_lat = ws.in(latents, (size_t)(n_samples * ld) * (latent_dtype == MG_F64 ? 8 : 4));
    const mg_staged d_res = ws.inout(residuals, (size_t)(n_samples * ld_res) * 8);
    const mg_staged d_err = ws.out(errors, (size_t)n_samples * 8), d_ex = ws.out(exit_state, (size_t)n_samples * 32);
    const mg_staged d_st = ws.out(step_exits, (size_t)n_samples * n_steps * 32);
    int rc = ws.upload();
    if (rc != MG_OK) return rc;
    rc = mg_score_walk_residuals_steps(n_steps, steps, d_lat.dev<void>(), latent_dtype, n_samples, ld, d_res.dev<double>(), ld_res, d_err.dev<double>(),
                                       d_ex.dev<double>(), d_st.dev<double>());
    if (rc != MG_OK) return rc;
    return ws.download();
}

extern "C" int mg_score_walk_residuals_host(int32_t n_steps, const mg_walk_score_step *steps, const void *latents, int latent_dtype, int64_t n_samples, int64_t ld,
                                            double *residuals, int64_t ld_res, double *errors, double *exit_state) {
    return mg_score_walk_residuals_steps_host(n_steps, steps, latents, latent_dtype, n_samples, ld, residuals, ld_res, errors, exit_state, nullptr);
}
