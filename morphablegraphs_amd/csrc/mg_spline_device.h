// The spline's basis row on the device (gfx950), shared by the kernels that evaluate a candidate at times of its own
// (mg_timewarp.hip: mg_frames_at_kernel; mg_walk.hip: the graph-walk kernels) so that they produce the same bits.
#pragma once
#include <hip/hip_runtime.h>

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
