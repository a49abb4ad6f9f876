// THE ROUTE of the keyframe scorers (mg_score_constraints, mg_score_constraint_residuals[_chained], mg_best_candidate), stated once as
// plain host code: standard headers, the C ABI and mg_dispatch.h only, no HIP call, so that tests/native/score_route_check.cpp compiles
// this file alone.  mg_launch_score (mg_score.hip) launches what it says and mg_score_plan reports it; tests/score_shape_cases.py
// restates it and tests/test_score_shapes_host.py pins the restatement to these lines.
#pragma once
#include <cstddef>
#include <cstdint>

#include <algorithm>

#include "../../include/mg_hip.h"
#include "mg_dispatch.h"

#define MG_SCORE_WIDE_MIN_B 49152   // measured crossover (tools/probes/score_kernel_ab.py): below, the tile kernel's eight waves per SIMD hide more latency than its idle lanes cost

// why a call is refused (both MG_ERR_UNSUPPORTED; the launch code owns the texts)
enum { MG_SCORE_ROUTE_OK = 0, MG_SCORE_REFUSED_LDS, MG_SCORE_REFUSED_SAMPLES };

struct mg_score_route {
    int kernel;      // MG_SCORE_KERNEL_VALU / _TILE / _WIDE
    size_t lds;      // dynamic LDS bytes of a workgroup
    bool opt_in;     // the kernel is opted in to more than 64 KiB of LDS before the launch
    int64_t grid;    // workgroups
};

// For a primitive of L components (KK k-steps; 0: no matrix-pipe form) and a set of n constraints whose rows fill RT 16-row tiles
// (has_wpack: the set has the packed operand image at all), B >= 1 candidates, under MG_OPT_SCORE_KERNEL = kernel_opt and
// MG_OPT_FORCE_VALU_SCORE = force_valu.  The wide kernel keeps 64 candidates' channels per wave in LDS without the opt-in, which
// holds ONE row tile: a set of more than 16 rows takes the tile kernel whatever the option or the batch.  A matrix-pipe kernel that
// does not fit (LDS, workgroup count) is no refusal: the VALU kernel takes the call, and only what it cannot take is refused.
inline int mg_score_route_of(int KK, int L, int RT, int n, int64_t B, int kernel_opt, int force_valu, bool has_wpack, mg_score_route *out) {
    const bool packed = has_wpack && !force_valu && mg_dispatch_kk(KK, false, [](auto) { return true; });
    if (packed) {
        const bool wide = kernel_opt == 2 || (kernel_opt == 0 && B >= MG_SCORE_WIDE_MIN_B);
        const size_t wide_lds = (size_t)4 * 64 * ((size_t)RT * 16 + 1) * 8;
        bool fits = true;
        if (wide && wide_lds <= 64 * 1024) {
            const int64_t grid = (B + 255) / 256;
            if (grid <= 0x7fffffff) { *out = {MG_SCORE_KERNEL_WIDE, wide_lds, false, grid}; return MG_SCORE_ROUTE_OK; }
            fits = false;
        }
        const size_t lds = (size_t)4 * (16 * ((size_t)RT * 16 + 1) + (size_t)std::max(n, 1) * 16) * 8;
        const int64_t grid = (B + 63) / 64;
        if (fits && lds <= 150 * 1024 && grid <= 0x7fffffff) { *out = {MG_SCORE_KERNEL_TILE, lds, lds > 64 * 1024, grid}; return MG_SCORE_ROUTE_OK; }
    }
    const size_t lds = ((size_t)64 * ((size_t)L + 1) + (size_t)std::max(n, 1) * 64) * 8;
    const int64_t grid = (B + 63) / 64;
    *out = {MG_SCORE_KERNEL_VALU, lds, lds > 64 * 1024, grid};
    if (lds > 150 * 1024) return MG_SCORE_REFUSED_LDS;
    if (grid > 0x7fffffff) return MG_SCORE_REFUSED_SAMPLES;
    return MG_SCORE_ROUTE_OK;
}
