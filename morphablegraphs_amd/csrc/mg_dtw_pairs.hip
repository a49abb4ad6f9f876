// All-pairs DTW costs: the total cost of the optimal warping path of every motion against every reference motion of a set, with no
// grid, no accumulated cost and no path in device memory (what the reference's find_optimal_dtw averages per candidate reference
// motion, construction/dtw.py:125-146), float64.
//
//   mg_dtw_pair_costs   costs[r][n] = D[Fr - 1][F - 1] of mg_dtw.hip's header comment for reference motion ref_indices[r] (Fr frames)
//                       and motion n (F frames) of one ragged cloud table: bit for bit the `totals` value mg_dtw_paths returns for
//                       the grid mg_dtw_distance_grids computes for that pair.  The cells are the statements of mg_dtw_device.h (the
//                       ones dtw_distance_grids_kernel and keyframe_distances_kernel compile), the recurrence makes one addition per
//                       cell and takes the minimum as Python's min does (diagonal, (i-1, j), (i, j-1); the first of equals stays).
//                       A workgroup of 512 lanes per (reference motion, motion) pair walks the grid in strips of 64 columns and, inside
//                       a strip, in passes of R rows (64; 32 at the largest J, so that everything fits the CU's LDS):
//                         * the strip's 64 rows of B and their one-cloud sums are staged once per strip, the rows of A 16 at a time;
//                           a wave takes one row of A (a broadcast) and its lanes the 64 columns (LDS rows an odd number of doubles
//                           apart: 32 lanes read 32 different bank pairs), a cell per lane, two rows per wave and 16-row step, and
//                           writes S into an (R, 64) LDS image;
//                         * wave 0 then runs the recurrence over the pass: lane c owns column c and handles row t - c at step t
//                           (R + 63 steps at most); D[i-1][j] is the lane's own last value, D[i][j-1] the left neighbour's last value
//                           (one cross-lane move per step), D[i-1][j-1] the value that move delivered the step before.  The state
//                           simply carries over from pass to pass (in LDS while the cells are computed).  Lane 0's left neighbour is the strip
//                           before: a boundary column of Fr doubles in LDS, read by lane 0 at row i and overwritten with this
//                           strip's last column 63 steps later.  No workgroup barrier inside the recurrence.
//                       While a workgroup's wave 0 runs its (latency-bound) recurrence, the CU's other workgroup computes cells.
//                       LDS: (80 (3J | 1) + 64 R + 353 + the longest reference motion) doubles: 73.3 KB at J = 19, Fr = 156; 150.9 KB
//                       at J = 64, Fr = 1024.
//
// Nothing depends on the schedule: no float atomics, no grid barriers, every sum in an order the shapes fix, so a pair gives the
// same bits alone or in any batch.  The matrix is not symmetric (the fit of B onto A is not bitwise the fit of A onto B).  Limits
// are answered before any launch; a non-finite cloud is found by the check kernel, which runs in front of the pairs on the same
// stream, and is answered when the call's one synchronisation returns (the costs are then without meaning).
#include "mg_dtw_device.h"

#include <algorithm>

#define PAIRS_MAX_FRAMES 1024
#define PAIRS_BLOCK 512
#define PAIRS_WAVES (PAIRS_BLOCK / 64)
#define PAIRS_STRIP 64         // columns of a strip = lanes of the recurrence's wave
#define PAIRS_SUB 16           // rows of A staged at a time
#define PAIRS_PASS_ROWS 64     // rows of a pass, halved while the workgroup's LDS would exceed PAIRS_LDS_BYTES
#define PAIRS_LDS_BYTES (152 * 1024)

// doubles of LDS for J joints, passes of `rows` rows and reference motions of at most `bnd` frames (the kernel carves in this order)
static inline size_t pairs_lds_doubles(int32_t J, int32_t rows, int32_t bnd) {
    const size_t stride = (size_t)(3 * J) | 1;
    return (PAIRS_STRIP + PAIRS_SUB) * stride + DTW_MAX_JOINTS + 2 * PAIRS_STRIP + 2 * PAIRS_SUB + 1 + 2 * PAIRS_STRIP + (size_t)bnd + (size_t)rows * PAIRS_STRIP;
}

__global__ __launch_bounds__(PAIRS_BLOCK, 4) void dtw_pair_costs_kernel(const double *__restrict__ clouds, const int64_t *__restrict__ off, int32_t J,
                                                                     const double *__restrict__ w, const int64_t *__restrict__ refs, int64_t n_motions,
                                                                     int32_t pass_rows, int32_t bnd_len, double *__restrict__ costs, int64_t n0,
                                                                     int64_t r0) {
    extern __shared__ double pairs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // the wave's index in scalar registers
    const int64_t n = n0 + blockIdx.x, r = r0 + blockIdx.y, m = refs ? refs[r] : r;
    const int64_t a0 = off[m], b0 = off[n];
    const int32_t Fr = (int32_t)(off[m + 1] - a0), F = (int32_t)(off[n + 1] - b0);
    const int row_len = 3 * J, stride = row_len | 1;
    double *sB = pairs_lds, *sA = sB + PAIRS_STRIP * stride, *sW = sA + PAIRS_SUB * stride, *sumB = sW + DTW_MAX_JOINTS, *sumA = sumB + 2 * PAIRS_STRIP,
           *sSw = sumA + 2 * PAIRS_SUB, *carry = sSw + 1, *bnd = carry + 2 * PAIRS_STRIP, *sS = bnd + bnd_len;
    if (tid < J) sW[tid] = w[tid];
    if (tid < 2 * PAIRS_STRIP) carry[tid] = 0.0;   // read before it means anything: row 0 of a strip uses neither value
    for (int j0 = 0; j0 < F; j0 += PAIRS_STRIP) {
        const int ncols = F - j0 < PAIRS_STRIP ? F - j0 : PAIRS_STRIP;
        __syncthreads();   // the strip before is finished with sB
        for (int rr = wave; rr < PAIRS_STRIP; rr += PAIRS_WAVES)   // a wave per row; the columns past the motion's end are zeros
            for (int c = lane; c < row_len; c += 64) sB[rr * stride + c] = rr < ncols ? clouds[(b0 + j0 + rr) * row_len + c] : 0.0;
        __syncthreads();
        if (tid < PAIRS_STRIP) {
            dtw_cloud_sums(sB + tid * stride, sW, J, &sumB[2 * tid], &sumB[2 * tid + 1]);
        } else if (tid == PAIRS_STRIP && j0 == 0) {
            *sSw = dtw_weight_sum(sW, J);
        }
        for (int i0 = 0; i0 < Fr; i0 += pass_rows) {
            const int rows = Fr - i0 < pass_rows ? Fr - i0 : pass_rows;
            for (int s0 = 0; s0 < rows; s0 += PAIRS_SUB) {
                const int nsub = rows - s0 < PAIRS_SUB ? rows - s0 : PAIRS_SUB;
                __syncthreads();   // the cells before are finished with sA and sumA, the recurrence before with sS
                for (int rr = wave; rr < nsub; rr += PAIRS_WAVES)
                    for (int c = lane; c < row_len; c += 64) sA[rr * stride + c] = clouds[(a0 + i0 + s0 + rr) * row_len + c];
                __syncthreads();
                if (tid < nsub) dtw_cloud_sums(sA + tid * stride, sW, J, &sumA[2 * tid], &sumA[2 * tid + 1]);
                __syncthreads();   // and the strip's sumB, sSw
#pragma unroll 1
                for (int rr = wave; rr < nsub; rr += PAIRS_WAVES)
                    sS[(s0 + rr) * PAIRS_STRIP + lane] =
                        dtw_cell(sA + rr * stride, sB + lane * stride, sW, J, sumA[2 * rr], sumA[2 * rr + 1], sumB[2 * lane], sumB[2 * lane + 1], *sSw);
            }
            __syncthreads();
            if (wave != 0) continue;   // they wait at the next barrier
            const int j = j0 + lane, steps = rows + ncols - 1;
            const bool col = lane < ncols;
            double sv = lane == 0 ? sS[0] : 0.0;
            double up = carry[lane], diag = carry[PAIRS_STRIP + lane];   // D[i-1][j] and D[i-1][j-1] of the lane's column j, from the pass before
            for (int t = 0; t < steps; t++) {
                const int k = t - lane, i = i0 + k;   // the lane's row, in the pass and in the grid
                double left = __shfl_up(up, 1);       // D[i][j-1]: what the left neighbour made the step before
                if (col && k >= 0 && k < rows) {
                    if (lane == 0 && j0 > 0) left = bnd[i];
                    double val;
                    if (i == 0) {
                        val = j == 0 ? sv : left + sv;
                    } else if (j == 0) {
                        val = up + sv;
                    } else {
                        double mn = diag;
                        if (up < mn) mn = up;
                        if (left < mn) mn = left;
                        val = mn + sv;
                    }
                    diag = left;
                    up = val;
                    if (lane == ncols - 1) bnd[i] = val;   // lane 0 has read bnd[i] by now (this very step when the strip has one column)
                    if (i == Fr - 1 && j == F - 1) costs[r * n_motions + n] = val;
                }
                if (col && k + 1 >= 0 && k + 1 < rows) sv = sS[(k + 1) * PAIRS_STRIP + lane];   // one step ahead
            }
            carry[lane] = up, carry[PAIRS_STRIP + lane] = diag;   // in LDS, not in registers, while the cells are computed
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
#define PAIRS_STR2(x) #x
#define PAIRS_STR(x) PAIRS_STR2(x)

extern "C" int mg_dtw_pair_costs(mg_context *ctx, const double *clouds_dev, const int64_t *offsets, int64_t n_motions, int32_t n_joints,
                                 const double *weights, const int64_t *ref_indices, int64_t n_refs, double *costs_dev) {
    const char *who = "mg_dtw_pair_costs";
    MG_REQUIRE_AS(ctx && offsets, MG_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    MG_REQUIRE_AS(n_motions >= 0 && n_refs >= 0 && n_joints >= 1, MG_ERR_INVALID_ARGUMENT, "%s: n_motions = %lld, n_refs = %lld, n_joints = %d", who,
                  (long long)n_motions, (long long)n_refs, n_joints);
    MG_REQUIRE_AS(n_joints <= DTW_MAX_JOINTS, MG_ERR_UNSUPPORTED, "%s: %d joints (at most %d)", who, n_joints, DTW_MAX_JOINTS);
    MG_REQUIRE_AS(n_motions < ((int64_t)1 << 24) && n_refs < ((int64_t)1 << 24), MG_ERR_UNSUPPORTED, "%s: %lld motions, %lld reference motions (fewer than 2^24)",
                  who, (long long)n_motions, (long long)n_refs);
    int64_t longest = 0;
    const int rc = mg_check_offsets(who, offsets, n_motions, PAIRS_MAX_FRAMES, "at most " PAIRS_STR(PAIRS_MAX_FRAMES), MG_ERR_UNSUPPORTED, &longest);
    if (rc != MG_OK) return rc;
    MG_REQUIRE_AS(ref_indices || n_refs == n_motions, MG_ERR_INVALID_ARGUMENT, "%s: no reference indices means all %lld motions, not %lld", who,
                  (long long)n_motions, (long long)n_refs);
    if (n_motions == 0 || n_refs == 0) return MG_OK;
    int64_t longest_ref = ref_indices ? 0 : longest;
    for (int64_t r = 0; ref_indices && r < n_refs; r++) {
        const int64_t m = ref_indices[r];
        MG_REQUIRE_AS(m >= 0 && m < n_motions, MG_ERR_INVALID_ARGUMENT, "%s: reference index %lld is %lld (%lld motions)", who, (long long)r, (long long)m,
                      (long long)n_motions);
        longest_ref = std::max(longest_ref, offsets[m + 1] - offsets[m]);
    }
    MG_REQUIRE_AS(clouds_dev && costs_dev, MG_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    double ones[DTW_MAX_JOINTS];
    const int rw = dtw_weights(who, weights, n_joints, ones);
    if (rw != MG_OK) return rw;
    dtw_block blk(ctx, who);
    const int rb = dtw_block_create(&blk, offsets, n_motions, ones, n_joints, ref_indices ? (size_t)n_refs * 8 : 0);
    if (rb != MG_OK) return rb;
    if (ref_indices) MG_HIP_CHECK(hipMemcpyAsync(blk.extra, ref_indices, (size_t)n_refs * 8, hipMemcpyHostToDevice, ctx->stream));
    dtw_launch_nonfinite(ctx, clouds_dev, offsets[n_motions] * 3 * (int64_t)n_joints, blk.flag);
    int32_t pass_rows = PAIRS_PASS_ROWS;
    while (pairs_lds_doubles(n_joints, pass_rows, (int32_t)longest_ref) * 8 > PAIRS_LDS_BYTES) pass_rows /= 2;   // 32 at J = 64, and from J = 58 on when a reference motion has 1024 frames
    const size_t lds = pairs_lds_doubles(n_joints, pass_rows, (int32_t)longest_ref) * 8;
    if (lds > 64 * 1024)
        MG_HIP_CHECK(mg_lds_opt_in(PAIRS_LDS_BYTES, dtw_pair_costs_kernel));
    const int64_t chunk_n = 65535;                                        // workgroups of a launch: at most 2^22, of 2^9 lanes
    for (int64_t n0 = 0; n0 < n_motions; n0 += chunk_n) {
        const int64_t nb = std::min(chunk_n, n_motions - n0), chunk_r = std::min<int64_t>(65535, ((int64_t)1 << 22) / nb);
        for (int64_t r0 = 0; r0 < n_refs; r0 += chunk_r) {
            const int64_t rb_ = std::min(chunk_r, n_refs - r0);
            hipLaunchKernelGGL(dtw_pair_costs_kernel, dim3((unsigned)nb, (unsigned)rb_), dim3(PAIRS_BLOCK), lds, ctx->stream, clouds_dev,
                               (const int64_t *)blk.off, n_joints, (const double *)blk.w, ref_indices ? (const int64_t *)blk.extra : (const int64_t *)nullptr,
                               n_motions, pass_rows, (int32_t)longest_ref, costs_dev, n0, r0);
        }
    }
    int32_t flag = 0;
    const int rf = dtw_flag_after(ctx, blk, &flag);   // the call's one synchronisation
    if (rf != MG_OK) return rf;
    MG_REQUIRE_AS(!flag, MG_ERR_INVALID_ARGUMENT, "%s: the point clouds hold non-finite values", who);
    return MG_OK;
}
