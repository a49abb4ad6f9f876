// The time warp of one candidate on the device (gfx950), float64, stated once: mg_timewarp_kernel (mg_timewarp.hip: a whole row of
// samples, one wave per candidate) and mg_feature_points_warped_kernel (mg_feature_points.hip: the one sample of frame_idx, one lane
// per candidate) compile these very statements, so a sample has the same bits whichever kernel evaluates it.  The contract is the
// header comment of mg_timewarp.hip.  The arrays are anything with operator[] -- a pointer, or mg_tw_strided for a candidate whose
// elements lie a tile apart:
//   mg_tw_increment            exp(mean_t(i) + phi(i) . gamma), the harmonics taken in by fma for l ascending
//   mg_tw_running_sum          t(i) = (inc_0 + .. + inc_i) - 1 in canonical-frame order (in place if inc and x are one array)
//   mg_tw_second_derivatives   the not-a-knot cubic through (t(i), i) by its second derivatives: a tridiagonal sweep by one lane (the
//                              2 x 2 system for F = 4), back-substituted down to `lowest` only
//   mg_tw_sample_count         int(round(t(F - 2)) * (1 / speed)), or "no row" for a time function that is not finite or absurd
//   mg_tw_sample_point         numpy.linspace(1, t(F - 2), num)[q]
//   mg_tw_interval, mg_tw_inverse_at   the piece that holds a sample point, and the cubic on it
//   mg_tw_row_sample           sample j of the row: 0, the inverse at sample point j - 1, F - 1
// The smoothed row (smooth_time_parameters: scipy.signal.savgol_filter(row, 15, 3), stated as the table of mg_savgol_table.h):
//   mg_tw_smooth_window        which row of the hat matrix H and which 15 unsmoothed samples make smoothed sample q
//   mg_tw_smoothed             H's row times those samples, every product and sum rounded on its own, k ascending
//   mg_tw_smoothed_row         a wave's whole row, 64 samples at a time through an LDS window of MG_TW_SMOOTH_LDS doubles
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#define MG_TW_BLOCK 64      // one wave per row of samples (mg_timewarp_kernel, mg_walks_time_kernel)
#define MG_TW_MAX_F 2048   // canonical frames the inversion holds in LDS (4 arrays of doubles)

struct mg_tw_strided {
    double *p;
    int stride;
    __device__ __forceinline__ double &operator[](int i) const { return p[(size_t)i * stride]; }
};

template <class GammaFn>
__device__ __forceinline__ double mg_tw_increment(const double *tphi, const double *tmean, int i, int Lt, GammaFn gamma) {
    double e = tmean[i];
    for (int l = 0; l < Lt; l++) e = fma(tphi[(size_t)i * Lt + l], gamma(l), e);
    return exp(e);
}

template <class Inc, class X>
__device__ __forceinline__ void mg_tw_running_sum(const Inc &inc, const X &x, int F) {
    double acc = 0.0;
    for (int i = 0; i < F; i++) { acc += inc[i]; x[i] = acc - 1.0; }
}

// not-a-knot cubic through (x_i, i): h_{i-1} M_{i-1} + 2 (h_{i-1} + h_i) M_i + h_i M_{i+1} = 6 ((y_{i+1} - y_i) / h_i - (y_i - y_{i-1}) / h_{i-1}),
// i = 1 .. m-2, with M_0 and M_{m-1} eliminated by the continuity of the third derivative at x_1 and x_{m-2}.  cp, dp: the sweep's
// modified upper diagonal and right-hand side; M may be dp itself (M_i takes dp_i's place).  Only M[lowest .. m-1] are formed, and M[0]
// with lowest <= 1 (1 <= lowest <= max(1, m - 3): the last one needs M[m-3]); lowest = 1: all of them.
template <class X, class MA, class CA, class DA>
__device__ __forceinline__ void mg_tw_second_derivatives(const X &x, const MA &M, const CA &cp, const DA &dp, int m, int lowest) {
    auto h = [&](int i) { return x[i + 1] - x[i]; };
    auto rhs = [&](int i) { return 6.0 * (1.0 / h(i) - 1.0 / h(i - 1)); };   // y_{i+1} - y_i = 1
    // rows 1 .. m-2: (lo, di, up); the first and the last one carry the end conditions
    auto row = [&](int i, double &lo, double &di, double &up) {
        const double h0 = h(i - 1), h1 = h(i);
        if (i == 1) { lo = 0.0; di = 2.0 * (h0 + h1) + h0 * (1.0 + h0 / h1); up = h1 - h0 * h0 / h1; }
        else if (i == m - 2) { lo = h0 - h1 * h1 / h0; di = 2.0 * (h0 + h1) + h1 * (1.0 + h1 / h0); up = 0.0; }
        else { lo = h0; di = 2.0 * (h0 + h1); up = h1; }
    };
    if (m == 4) {   // rows 1 and 2, both with an end condition: row 1 keeps its `up`, row 2 its `lo`
        const double h0 = h(0), h1 = h(1), h2 = h(2);
        const double d1 = 2.0 * (h0 + h1) + h0 * (1.0 + h0 / h1), u1 = h1 - h0 * h0 / h1;
        const double l2 = h1 - h2 * h2 / h1, d2 = 2.0 * (h1 + h2) + h2 * (1.0 + h2 / h1);
        const double r1 = rhs(1), r2 = rhs(2);
        const double det = d1 * d2 - u1 * l2;
        M[1] = (r1 * d2 - u1 * r2) / det;
        M[2] = (d1 * r2 - l2 * r1) / det;
        lowest = 1;
    } else {
        double lo, di, up;
        row(1, lo, di, up);
        cp[1] = up / di;
        dp[1] = rhs(1) / di;
        for (int i = 2; i <= m - 2; i++) {
            row(i, lo, di, up);
            const double den = di - lo * cp[i - 1];
            cp[i] = up / den;
            dp[i] = (rhs(i) - lo * dp[i - 1]) / den;
        }
        M[m - 2] = dp[m - 2];
        for (int i = m - 3; i >= lowest; i--) M[i] = dp[i] - cp[i] * M[i + 1];
    }
    {
        const double h0 = h(0), h1 = h(1), a = h(m - 2) / h(m - 3);
        if (lowest <= 1) M[0] = (1.0 + h0 / h1) * M[1] - (h0 / h1) * M[2];
        M[m - 1] = (1.0 + a) * M[m - 2] - a * M[m - 3];
    }
}

// The inner samples' count.  false: a time function that is not finite (exp() overflowed on a wild gamma) or asks for more than 2^24
// samples has no row (the conversion of such a float to int is undefined, and T = num + 2 could wrap -- ADVICE r4)
__device__ __forceinline__ bool mg_tw_sample_count(double stop, double inv_speed, int &num) {
    const double numf = rint(stop) * inv_speed;
    if (!(numf == numf) || !(fabs(stop) <= 1.0e300) || numf > 16777216.0) return false;
    num = numf > 0.0 ? (int)numf : 0;
    return true;
}

__device__ __forceinline__ double mg_tw_sample_step(double stop, int num) { return num > 1 ? (stop - 1.0) / (double)(num - 1) : 0.0; }

// numpy.linspace: arange * step + start, the last one = stop
__device__ __forceinline__ double mg_tw_sample_point(int q, int num, double stop, double step) {
    return (q == num - 1 && num > 1) ? stop : (double)q * step + 1.0;
}

// the interval [x_i, x_{i+1}) that holds t, the end intervals for anything outside
template <class X>
__device__ __forceinline__ int mg_tw_interval(const X &x, int F, double t) {
    int lo = 0, hi = F - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (x[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the cubic with second derivatives M through (x_i, i) and (x_{i+1}, i + 1), at t
template <class X, class MA>
__device__ __forceinline__ double mg_tw_inverse_at(const X &x, const MA &M, int i, double t) {
    const double hi_ = x[i + 1] - x[i], A = x[i + 1] - t, Bq = t - x[i];
    return M[i] * A * A * A / (6.0 * hi_) + M[i + 1] * Bq * Bq * Bq / (6.0 * hi_) + ((double)i / hi_ - M[i] * hi_ / 6.0) * A +
           ((double)(i + 1) / hi_ - M[i + 1] * hi_ / 6.0) * Bq;
}

// sample j of a row of T = num + 2 samples: 0 in front, F - 1 behind, between them the inverse at numpy.linspace(1, stop, num)[j - 1]
template <class X, class MA>
__device__ __forceinline__ double mg_tw_row_sample(const X &x, const MA &M, int F, int j, int T, int num, double stop, double step) {
    if (j == 0) return 0.0;
    if (j == T - 1) return (double)(F - 1);
    const double t = mg_tw_sample_point(j - 1, num, stop, step);
    return mg_tw_inverse_at(x, M, mg_tw_interval(x, F, t), t);
}

// ---- the smoothed row: savgol_filter(row, 15, 3), mode "interp" (mg_savgol_table.h) --------------------------------------------------
#define MG_TW_SMOOTH_W 15                                            // the window; a row shorter than this has no smoothed form
#define MG_TW_SMOOTH_HALF 7
#define MG_TW_SMOOTH_MID (MG_TW_BLOCK + 2 * MG_TW_SMOOTH_HALF)       // unsmoothed samples the inner windows of 64 outputs span (78)
#define MG_TW_SMOOTH_LDS (MG_TW_SMOOTH_MID + 2 * MG_TW_SMOOTH_W)     // ... then the row's first 15 and its last 15

// smoothed sample q of a row of T >= 15: row `row` of H times unsmoothed samples base .. base + 14 (head and tail cannot overlap)
__device__ __forceinline__ void mg_tw_smooth_window(int q, int T, int *row, int *base) {
    if (q < MG_TW_SMOOTH_HALF) { *row = q; *base = 0; }
    else if (q >= T - MG_TW_SMOOTH_HALF) { *row = MG_TW_SMOOTH_W - (T - q); *base = T - MG_TW_SMOOTH_W; }
    else { *row = MG_TW_SMOOTH_HALF; *base = q - MG_TW_SMOOTH_HALF; }
}

// Hrow . u over the window, k ascending: every product and every sum rounded on its own (time_smoothing.smooth_time_row_host's bits)
template <class U>
__device__ __forceinline__ double mg_tw_smoothed(const double *Hrow, const U &u) {
#pragma clang fp contract(off)
    double acc = Hrow[0] * u[0];
    for (int k = 1; k < MG_TW_SMOOTH_W; k++) {
        const double prod = Hrow[k] * u[k];
        acc = acc + prod;
    }
    return acc;
}

// The whole smoothed row of one wave (MG_TW_BLOCK lanes), T >= 15, into tb[0 .. T): per chunk of 64 outputs the unsmoothed samples the
// chunk needs go to win[MG_TW_SMOOTH_LDS] -- win[e] = sample c0 - 7 + e for e < 78, where the row has one; the row's first 15 behind
// them where the chunk holds an output below 7, its last 15 where it holds one from T - 7 on -- then every lane forms its output.
// The row is never smoothed in place: nothing is read back from tb.
template <class X, class MA>
__device__ __forceinline__ void mg_tw_smoothed_row(const X &x, const MA &M, int F, int T, int num, double stop, double step, const double *H,
                                                   double *win, double *tb, int tid) {
    double *head = win + MG_TW_SMOOTH_MID, *tail = head + MG_TW_SMOOTH_W;
    for (int c0 = 0; c0 < T; c0 += MG_TW_BLOCK) {
        const int lo = c0 - MG_TW_SMOOTH_HALF;
        const bool want_head = c0 < MG_TW_SMOOTH_HALF, want_tail = c0 + MG_TW_BLOCK > T - MG_TW_SMOOTH_HALF;
        for (int e = tid; e < MG_TW_SMOOTH_LDS; e += MG_TW_BLOCK) {
            int j = -1;
            if (e < MG_TW_SMOOTH_MID) j = lo + e;
            else if (e < MG_TW_SMOOTH_MID + MG_TW_SMOOTH_W) { if (want_head) j = e - MG_TW_SMOOTH_MID; }
            else if (want_tail) j = T - MG_TW_SMOOTH_W + (e - MG_TW_SMOOTH_MID - MG_TW_SMOOTH_W);
            if (j >= 0 && j < T) win[e] = mg_tw_row_sample(x, M, F, j, T, num, stop, step);
        }
        __syncthreads();
        const int q = c0 + tid;
        if (q < T) {
            int row, base;
            mg_tw_smooth_window(q, T, &row, &base);
            const double *u = q < MG_TW_SMOOTH_HALF ? head : (q >= T - MG_TW_SMOOTH_HALF ? tail : win + (base - lo));
            tb[q] = mg_tw_smoothed(H + MG_TW_SMOOTH_W * row, u);
        }
        __syncthreads();   // (the next chunk overwrites the window)
    }
}
