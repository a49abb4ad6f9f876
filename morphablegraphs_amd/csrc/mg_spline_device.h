// The float64 spline arithmetic on the device (gfx950), stated once: every kernel that forms a candidate's control points or
// evaluates its spline calls these, so that they produce the same bits.  What this header guarantees:
//   mg_load_lat        a latent component "as double" (float32 latents are widened, never rounded)
//   mg_control_point   acc = mean'; acc = fma(E'[k], s[k], acc) for k ascending (float: fmaf)
//   mg_taps4           v = w0 c0; v = fma(w_j, c_j, v) for j = 1, 2, 3 (splev.f sums j ascending; float: fmaf)
//   mg_basis_row_dev   FITPACK's basis row at a time of the caller's own
// (The MFMA frames kernels state the float32 taps for their own LDS layout: mg_frames_common.h.  mg_joint_tracks' control-point
// phase runs four candidates' chains side by side from one load of E' and is not a caller of mg_control_point.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

template <bool F64>
__device__ __forceinline__ double mg_load_lat(const void *lat, int64_t idx) {
    if (F64) return ((const double *)lat)[idx];
    return (double)((const float *)lat)[idx];
}

__device__ __forceinline__ double mg_load_lat(const void *lat, bool f64, int64_t idx) {   // the dtype known at run time only
    return f64 ? mg_load_lat<true>(lat, idx) : mg_load_lat<false>(lat, idx);
}

// One control point (or any row of mean' + E' s): the accumulator starts at the mean and takes the eigenvector elements
// e[0], e[stride], e[2 stride], ... for k ascending; latent(k) is the candidate's k-th latent component.
template <typename T, typename LatFn>
__device__ __forceinline__ T mg_control_point(T acc, const T *e, size_t stride, int L, LatFn latent) {
    for (int k = 0; k < L; k++) {
        if constexpr (std::is_same<T, float>::value) acc = fmaf(e[(size_t)k * stride], latent(k), acc);
        else acc = fma(e[(size_t)k * stride], latent(k), acc);
    }
    return acc;
}

// One channel of one sample: the four taps c[0], c[stride], c[2 stride], c[3 stride] of its knot span under the basis row w[0 .. 3]
// (rounded to T first).
template <typename T>
__device__ __forceinline__ T mg_taps4(const double *w, const T *c, int stride) {
    T v = (T)w[0] * c[0];
    if constexpr (std::is_same<T, float>::value) {
        v = fmaf((T)w[1], c[stride], v);
        v = fmaf((T)w[2], c[2 * stride], v);
        v = fmaf((T)w[3], c[3 * stride], v);
    } else {
        v = fma(w[1], c[stride], v);
        v = fma(w[2], c[2 * stride], v);
        v = fma(w[3], c[3 * stride], v);
    }
    return v;
}

// FITPACK fpbspl at x on the span l found like splev does (ext = 0): the host's mg_basis_row, statement for statement
__device__ __forceinline__ void mg_basis_row_dev(const double *t, int n, double x, int *i0, double *h) {
    const int k = 3;
    int l = k;
    while (!(x < t[l + 1] || l == n - k - 2)) l++;
    double hh[4];
    h[0] = 1.0; h[1] = h[2] = h[3] = 0.0;
    for (int j = 1; j <= k; j++) {
        for (int i = 0; i < j; i++) hh[i] = h[i];
        h[0] = 0.0;
        for (int i = 1; i <= j; i++) {
            const int li = l + i, lj = li - j;
            if (t[li] == t[lj]) { h[i] = 0.0; continue; }
            const double f = hh[i - 1] / (t[li] - t[lj]);
            h[i - 1] = h[i - 1] + f * (t[li] - x);
            h[i] = f * (x - t[lj]);
        }
    }
    *i0 = l - k;
}
