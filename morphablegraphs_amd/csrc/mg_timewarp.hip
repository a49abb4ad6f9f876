// Time-warped synthesis for a batch (gfx950 / MI355X), float64.
//
// The reference turns a finished graph walk into the motion it returns with back_project(s, use_time_parameters=True)
// (motion_generator/graph_walk.py:154-176): the latent vector's time part gamma gives the canonical time function t(t')
// (motion_model/motion_primitive.py:289-302, on the device since round 2: mg_time_function_kernel), its INVERSE t'(t) sampled at the
// integer sample times is the spline's time function (motion_primitive.py:304-319: scipy.interpolate.splrep through the points
// (t(t'), t'), i.e. FITPACK's interpolating cubic with knots at the data points but the second and the second-to-last one -- the
// not-a-knot cubic -- evaluated by splev at linspace(1, t(F - 2), num), num = round(t(F - 2)) / speed, with 0 put in front and
// F - 1 behind), and the frames are the spline evaluated at those times (motion_spline.py:71-86).
//
//   mg_timewarp_kernel        one wave per candidate: increments exp(mean_t + phi . gamma) in parallel, their running sum by one lane
//                             in canonical-frame order (np's cumulative order: the same bits as mg_time_function_kernel), the
//                             not-a-knot cubic through (t(t'), t') by its second derivatives (a tridiagonal solve, one lane),
//                             the samples in parallel (the statements: mg_timewarp_device.h).  The not-a-knot cubic is unique, so this is FITPACK's spline up to rounding
//                             (1e-12 of F on the fixtures); the sample count is int(round(t(F-2)) * (1 / speed)), the value NumPy
//                             before 1.18 made of the float the reference passes (newer NumPy raises TypeError there: SURVEY 8c).
//   mg_frames_at_kernel       one workgroup per candidate: its control points (mean' + E' . s, fma chain over k ascending from the
//                             mean: the arithmetic of mg_back_project_frames_f64) in LDS, the basis row of each of ITS time samples
//                             by the FITPACK recurrence, the 4 taps -- the frames of a candidate at its own times, what
//                             mg_back_project_frames_f64 gives with a time grid per candidate, without a grid per candidate.
#include "mg_internal.h"
#include "mg_spline_device.h"
#include "mg_timewarp_device.h"

// SMOOTH: the row goes through the Savitzky-Golay pass (H: the hat matrix, mg_savgol_table.h) on its way out -- mg_tw_smoothed_row, whose
// window lies behind dp; a row of fewer than 15 samples reports its length and is not written.  false: H is not read.
template <bool SMOOTH>
__global__ __launch_bounds__(MG_TW_BLOCK) void mg_timewarp_kernel(const double *__restrict__ tphi, const double *__restrict__ tmean,
                                                                  const void *__restrict__ gamma, int gamma_f64, int64_t ld, int F, int Lt,
                                                                  double inv_speed, double *__restrict__ times, int32_t *__restrict__ lens,
                                                                  int32_t t_cap, int64_t row_pitch, double *__restrict__ canonical_out,
                                                                  const double *__restrict__ H) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *x = (double *)smem;      // [F] the canonical time function t(t'): the spline's abscissae; ordinates are 0 .. F-1
    double *M = x + F;               // [F] second derivatives
    double *cp = M + F;              // [F] Thomas: modified upper diagonal
    double *dp = cp + F;             // [F] Thomas: modified right-hand side
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const void *gb = gamma_f64 ? (const void *)((const double *)gamma + b * ld) : (const void *)((const float *)gamma + b * ld);
    for (int i = tid; i < F; i += MG_TW_BLOCK)   // the increments (parked in M)
        M[i] = mg_tw_increment(tphi, tmean, i, Lt, [&](int l) { return gamma_f64 ? ((const double *)gb)[l] : (double)((const float *)gb)[l]; });
    __syncthreads();
    if (tid == 0) {
        mg_tw_running_sum(M, x, F);
        mg_tw_second_derivatives(x, M, cp, dp, F, 1);
    }
    __syncthreads();
    if (canonical_out)
        for (int i = tid; i < F; i += MG_TW_BLOCK) canonical_out[b * F + i] = x[i];
    // the samples: 0, the inverse spline at linspace(1, x[F-2], num), F - 1
    const double stop = x[F - 2];
    int num;
    if (!mg_tw_sample_count(stop, inv_speed, num)) {   // no row: length 0, nothing written
        if (tid == 0) lens[b] = 0;
        return;
    }
    const int T = num + 2;
    if (tid == 0) lens[b] = T <= t_cap ? T : -T;   // (negative: the caller's rows are too short; nothing else is written)
    if (T > t_cap) return;
    double *tb = times + b * row_pitch;   // (a row holds t_cap samples; row_pitch >= t_cap doubles lie between two rows' starts)
    const double step = mg_tw_sample_step(stop, num);
    if (SMOOTH) {
        if (T >= MG_TW_SMOOTH_W) mg_tw_smoothed_row(x, M, F, T, num, stop, step, H, dp + F, tb, tid);
        return;
    }
    for (int j = tid; j < T; j += MG_TW_BLOCK) {
        double v;
        if (j == 0) v = 0.0;
        else if (j == T - 1) v = (double)(F - 1);
        else {
            const double t = mg_tw_sample_point(j - 1, num, stop, step);
            v = mg_tw_inverse_at(x, M, mg_tw_interval(x, F, t), t);
        }
        tb[j] = v;
    }
}

#define MG_FA_BLOCK 256
template <bool LAT_F64, bool OUT_F64>
__global__ __launch_bounds__(MG_FA_BLOCK) void mg_frames_at_kernel(const double *__restrict__ Et64,   // [L][R]
                                                                   const double *__restrict__ mean,   // [R]
                                                                   const double *__restrict__ knots,  // [NB + 4]
                                                                   const void *__restrict__ lat, int64_t ld, int L, int R, int D, int NB,
                                                                   const double *__restrict__ times, const int32_t *__restrict__ lens, int32_t t_cap,
                                                                   void *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *c = (double *)smem;                 // [R] the candidate's control points
    double *s = c + R;                          // [L]
    double *w = s + L;                          // [t_cap][4]
    int *i0 = (int *)(w + (size_t)t_cap * 4);   // [t_cap]
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int T = lens ? lens[b] : t_cap;
    if (T <= 0 || T > t_cap) return;     // (a length beyond the rows' capacity would overrun w / i0 and the row in `out`: the row is skipped)
    for (int k = tid; k < L; k += MG_FA_BLOCK) s[k] = mg_load_lat<LAT_F64>(lat, b * ld + k);
    __syncthreads();
    for (int r = tid; r < R; r += MG_FA_BLOCK) c[r] = mg_control_point(mean[r], Et64 + r, (size_t)R, L, [&](int k) { return s[k]; });
    const double *tb = times + b * (int64_t)t_cap;
    for (int f = tid; f < T; f += MG_FA_BLOCK) mg_basis_row_dev(knots, NB + 4, tb[f], &i0[f], &w[4 * f]);
    __syncthreads();
    const int64_t TD = (int64_t)T * D;
    for (int64_t e = tid; e < TD; e += MG_FA_BLOCK) {
        const int f = (int)(e / D), d = (int)(e - (int64_t)f * D);
        const double *cf = c + (size_t)i0[f] * D + d;
        const double *wf = w + 4 * f;
        const double v = mg_taps4(wf, cf, D);
        if (OUT_F64) ((double *)out)[(b * t_cap + f) * D + d] = v;
        else ((float *)out)[(b * t_cap + f) * D + d] = (float)v;
    }
}

// (a property of kernel AND device: once per context)
static hipError_t mg_tw_lds_opt_in(mg_context *ctx) {
    return mg_lds_opt_in_once(ctx, MG_LDS_TIMEWARP, 160 * 1024, mg_timewarp_kernel<false>, mg_timewarp_kernel<true>, mg_frames_at_kernel<true, true>, mg_frames_at_kernel<true, false>,
                              mg_frames_at_kernel<false, true>, mg_frames_at_kernel<false, false>);
}

int mg_launch_timewarp(mg_primitive *p, const void *gamma, int gdt, int64_t B, int64_t ld, double speed, double *times, int32_t *lens, int32_t t_cap,
                       int64_t row_pitch, double *canonical_out, bool smooth) {
    const size_t lds = ((size_t)4 * p->F + (smooth ? MG_TW_SMOOTH_LDS : 0)) * 8;   // x, M, cp, dp; the smoothed row's window behind them
    const double *H = nullptr;
    if (smooth) {
        const int rc = mg_savgol_table_dev(p->ctx, &H);
        if (rc != MG_OK) return rc;
    }
    if (p->F < 4 || p->F > MG_TW_MAX_F) { mg_set_error("mg_time_function_sample: %d canonical frames (4 .. %d supported)", p->F, MG_TW_MAX_F); return MG_ERR_UNSUPPORTED; }
    MG_HIP_CHECK(mg_tw_lds_opt_in(p->ctx));
    mg_dispatch_flags(smooth, [&](auto SMOOTH) {
        hipLaunchKernelGGL(mg_timewarp_kernel<SMOOTH>, dim3((unsigned)B), dim3(MG_TW_BLOCK), lds, p->ctx->stream, (const double *)p->d_tphi, (const double *)p->d_tmean,
                           gamma, gdt == MG_F64 ? 1 : 0, ld, (int)p->F, (int)p->Lt, 1.0 / speed, times, lens, t_cap, row_pitch, canonical_out, H);
    });
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

int mg_launch_frames_at(mg_primitive *p, const void *lat, int ldt, int64_t B, int64_t ld, const double *times, const int32_t *lens, int32_t t_cap,
                        void *out, int odt) {
    const size_t lds = ((size_t)p->R + p->L + (size_t)t_cap * 4) * 8 + (size_t)t_cap * 4 + 16;
    if (lds > 160 * 1024 - 64) {
        mg_set_error("mg_back_project_frames_at: %d control-point rows + %d time samples per candidate do not fit LDS", p->R, t_cap);
        return MG_ERR_UNSUPPORTED;
    }
    MG_HIP_CHECK(mg_tw_lds_opt_in(p->ctx));
    mg_dispatch_flags(ldt == MG_F64, odt == MG_F64, [&](auto LAT_F64, auto OUT_F64) {
        hipLaunchKernelGGL((mg_frames_at_kernel<LAT_F64, OUT_F64>), dim3((unsigned)B), dim3(MG_FA_BLOCK), lds, p->ctx->stream, (const double *)p->d_Et64, (const double *)p->d_mean,
                           (const double *)p->d_knots, lat, ld, (int)p->L, (int)p->R, (int)p->D, (int)p->NB, times, lens, t_cap, out);
    });
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}
