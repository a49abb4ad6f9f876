// What the host-only headers (mg_constraint_image.h) and the translation units share, as plain host code: the entry points' argument
// checks, the pose tables' sizes and the float64 spline basis row.  Standard headers and the C ABI only, no HIP call; a stand-alone
// check program under tests/native supplies its own mg_set_error.
#pragma once
#include <cstdint>

#include "../../include/mg_hip.h"

void mg_set_error(const char *fmt, ...);

// argument checks of the entry points: set the error text and return `code`
#define MG_REQUIRE_AS(cond, code, ...) \
    do {                               \
        if (!(cond)) {                 \
            mg_set_error(__VA_ARGS__); \
            return (code);             \
        }                              \
    } while (0)
#define MG_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)

// Device table of one pose constraint inside d_pose (doubles): header, then one record per point
#define MG_POSE_HDR 8                            // [0] n_points, [1] has_velocity, [2..4] velocity, [5] rows of one pose block
#define MG_POSE_REC (5 + 4 * MG_MAX_CHAIN)       // target xyz, weight, chain length m, then m x (quaternion row or -1, offset xyz)

// host-side float64 spline basis (FITPACK splev/fpbspl semantics): splev.f interval search + fpbspl.f recurrence
// (scipy.interpolate.splev, ext=0), the arithmetic behind reference motion_spline.py:86,92.
inline void mg_basis_row(const double *t, int n, double x, int32_t *i0, double *h) {
    const int k = 3;
    int l = k;
    while (!(x < t[l + 1] || l == n - k - 2)) l++;
    double hh[4];
    h[0] = 1.0; h[1] = h[2] = h[3] = 0.0;
    for (int j = 1; j <= k; j++) {
        for (int i = 0; i < j; i++) hh[i] = h[i];
        h[0] = 0.0;
        for (int i = 1; i <= j; i++) {
            int li = l + i, lj = li - j;
            if (t[li] == t[lj]) { h[i] = 0.0; continue; }
            double f = hh[i - 1] / (t[li] - t[lj]);
            h[i - 1] = h[i - 1] + f * (t[li] - x);
            h[i] = f * (x - t[lj]);
        }
    }
    *i0 = l - k;
}
