// What the host-only headers (mg_constraint_image.h, mg_primitive_image.h) and the translation units share, as plain host code: the
// entry points' argument checks, the pose tables' sizes, the chunk planner's constants and the float64 spline basis row.
// Standard headers and the C ABI only, no HIP call; a stand-alone check program under tests/native supplies its own mg_set_error.
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

// What the chunk planner (mg_primitive_image.h) and the frames kernels agree on
#define MG_NCAND 16         // candidates per MFMA tile (N of v_mfma_f32_16x16x4_f32)
#define MG_MAX_KK 16        // k-steps of 4 -> n_components <= 64 on the MFMA path
// One chunk of a time grid handled by one workgroup of the MFMA kernel.
#define MG_MAX_WI 11         // basis functions per chunk window (11 x 3 root rows still span <= 3 row tiles of 16)
#define MG_MAX_NT 48         // time samples per chunk
#define MG_TAP_KS ((MG_MAX_WI + 3) / 4)   // k-steps of the banded root-tap MFMA (4 basis functions each)
#define MG_TAP_FT (MG_MAX_NT / 16)       // sample tiles of 16 of the root-tap MFMA
#define MG_ARG_CHUNKS 8   // chunk descriptors that travel in the frames kernels' arguments
// LDS of the frames kernels per ring slot: per-sample tables (tap weights + tap row offsets) and the root outputs
// [candidate][sample][4] float32.  nt = the grid's longest chunk, rounded up to 16 samples.  A candidate's root outputs are
// MG_RO_PAD floats apart from a multiple of 32: wave 0 writes them one float per lane, (candidate, channel) x sample, and with a
// stride of 4 nt floats (0 mod 32 banks for nt = 16, 32, 48) the six candidates of a column tile meet in the same banks.
#define MG_RO_PAD 8
#define MG_RO_CS(nt) ((nt) * 4 + MG_RO_PAD)              // floats per candidate
#define MG_TB_BYTES_N(nt) ((nt) * 16 + (nt) * 4)
#define MG_RO_BYTES_N(nt) (MG_NCAND * MG_RO_CS(nt) * 4)
#define MG_ROOT_SPLIT_MAX_EST 5e-6   // the mean/delta split's accuracy gate (mg_primitive_root_mode)
struct mg_chunk {
    int32_t t0;        // first time index (chunks are runs of consecutive time indices)
    int32_t nT;        // number of time samples in the chunk, <= MG_MAX_NT
    int32_t rt0;       // first global 16-row tile of the (padded-row) coefficient window
    int32_t ntiles;    // number of 16-row tiles
    int32_t imin;      // first coefficient index of the window
    int32_t wi;        // coefficient rows (basis functions) in the window, <= MG_MAX_WI
    int32_t rrt0;      // first 16-row tile of the root-row window (rows = i*nroot + d)
    int32_t nrt;       // number of root tiles
};

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
