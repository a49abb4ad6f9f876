// Temporal alignment of motions: exact dynamic time warping of N motions against one reference motion (reference
// construction/dtw.py: get_distgrid, find_path, get_warping_function, warp_motion), float64.
//
//   mg_dtw_distance_grids   S[n] (Fr, F_n): cell (i, j) = the distance of the reference motion's cloud A[i] and motion n's cloud
//                           B[j] after the best rigid fit about the y axis.  With joint weights w (ones when NULL), every sum over
//                           the joints k = 0 .. J - 1 in index order, one product and one addition at a time (no fma):
//                             sw = sum w_k, sax = sum w_k ax_k, saz = sum w_k az_k, sbx = sum w_k bx_k, sbz = sum w_k bz_k,
//                             num = sum w_k (ax_k bz_k - bx_k az_k) - (sax sbz - sbx saz) / sw,
//                             den = sum w_k (ax_k bx_k + az_k bz_k) - (sax sbx + saz sbz) / sw,
//                             theta = atan2(num, den), c = cos theta, s = sin theta,
//                             ox = ((sax - sbx c) - sbz s) / sw, oz = ((saz + sbx s) - sbz c) / sw,
//                             x'_k = (bx_k c + bz_k s) + ox, z'_k = ((-bx_k) s + bz_k c) + oz,
//                             S = (sum sqrt(((ax_k - x'_k)^2 + (ay_k - by_k)^2) + (az_k - z'_k)^2)) / J
//                           (oracle/mg_oracle.py align_point_clouds_2d / transform_point_cloud and the mean point distance of
//                           pose_constraint_error; PARITY UNPINNED: the reference's own distance lives in anim_utils).
//                           A workgroup of 256 lanes per (motion, 16 x 16 tile of the grid), a cell per lane; the tile's 16 rows of
//                           A and 16 rows of B are staged in LDS (rows an odd number of doubles apart), the five one-cloud sums are
//                           formed once per row by 32 lanes, then each lane runs the two cross sums, the fit and the J square
//                           roots.  Plain VALU: the cross sums carry the weights inside the sum and are added in joint order, which
//                           an MFMA's four-deep inner sum does not promise, and they are a tenth of a cell's work.
//   mg_dtw_paths            per motion one workgroup, a lane per row of the grid, walks the anti-diagonals: D[0,0] = S[0,0], first
//                           column and row the running sums, D[i,j] = min(D[i-1,j-1], D[i-1,j], D[i,j-1]) + S[i,j], the minimum
//                           taken as Python's min takes it (the first of equals stays), one addition per cell: D is the
//                           reference's bit for bit.  Three diagonals live in LDS; each cell's back-step (0 diagonal, 1 (i-1, j),
//                           2 (i, j-1): the first minimum in that order, numpy.argmin's) is kept in two bits, 16 to a word that only
//                           the row's lane writes, in LDS while the grid's codes fit 96 KiB and in device memory beyond.  Lane 0
//                           then walks back from the last cell (at most Fr + F - 1 steps), writes the path and, per row, the last
//                           column the path has in it (get_warping_function); the workgroup turns the path front to back.
//   mg_warp_motions         warped[n][i][:] = frames_n[w_n[i]][:], a gather.
//
// Nothing depends on the schedule: no float atomics, no grid barriers, every sum in an order the shapes fix, so a motion gives
// the same bits alone or in any batch.  Limits are answered before any of these kernels is launched.
#include "mg_dtw_device.h"

#include <algorithm>

#define DTW_MAX_FRAMES 1024
#define DTW_TILE 16
#define DTW_CODE_LDS_BYTES (96 * 1024)

__global__ __launch_bounds__(DTW_BLOCK) void dtw_distance_grids_kernel(const double *__restrict__ A, int32_t Fr, const double *__restrict__ B,
                                                                       const int64_t *__restrict__ off, int32_t J, const double *__restrict__ w,
                                                                       double *__restrict__ S, int32_t tiles_j, int64_t n0) {
    extern __shared__ double dtw_lds[];
    const int tid = threadIdx.x;
    const int64_t n = n0 + blockIdx.y, b0 = off[n];
    const int32_t F = (int32_t)(off[n + 1] - b0);
    const int ti = blockIdx.x / tiles_j, tj = blockIdx.x % tiles_j;
    if (tj * DTW_TILE >= F) return;   // whole workgroup: this motion is shorter than the longest
    const int row_len = 3 * J, stride = row_len | 1;
    double *sA = dtw_lds, *sB = sA + DTW_TILE * stride, *sW = sB + DTW_TILE * stride, *sums = sW + DTW_MAX_JOINTS;   // sums: [32][2], then sw
    for (int e = tid; e < DTW_TILE * row_len; e += DTW_BLOCK) {
        const int r = e / row_len, c = e % row_len;
        const int i = ti * DTW_TILE + r, j = tj * DTW_TILE + r;
        sA[r * stride + c] = i < Fr ? A[(int64_t)i * row_len + c] : 0.0;
        sB[r * stride + c] = j < F ? B[(b0 + j) * row_len + c] : 0.0;
    }
    if (tid < J) sW[tid] = w[tid];
    __syncthreads();
    if (tid < 2 * DTW_TILE) {
        dtw_cloud_sums((tid < DTW_TILE ? sA : sB) + (tid & (DTW_TILE - 1)) * stride, sW, J, &sums[2 * tid], &sums[2 * tid + 1]);
    } else if (tid == 2 * DTW_TILE) {
        sums[4 * DTW_TILE] = dtw_weight_sum(sW, J);
    }
    __syncthreads();
    const int r = tid >> 4, c = tid & 15;
    const int i = ti * DTW_TILE + r, j = tj * DTW_TILE + c;
    const double *a = sA + r * stride, *b = sB + c * stride;
    const double sax = sums[2 * r], saz = sums[2 * r + 1], sbx = sums[2 * (DTW_TILE + c)], sbz = sums[2 * (DTW_TILE + c) + 1], sw = sums[4 * DTW_TILE];
    const double cell = dtw_cell(a, b, sW, J, sax, saz, sbx, sbz, sw);
    if (i < Fr && j < F) S[(int64_t)Fr * b0 + (int64_t)i * F + j] = cell;
}

__global__ __launch_bounds__(DTW_MAX_FRAMES) void dtw_paths_kernel(const double *__restrict__ S, int32_t Fr, const int64_t *__restrict__ off,
                                                                    double *__restrict__ Dout, double *__restrict__ totals, int32_t *__restrict__ paths,
                                                                    int32_t *__restrict__ path_len, int32_t *__restrict__ warp, uint32_t *codes_dev,
                                                                    int32_t words_per_row_max, int32_t codes_in_lds, int64_t n0) {
    __shared__ double diag[3][DTW_MAX_FRAMES];
    __shared__ int32_t s_len;
    extern __shared__ uint32_t dtw_codes[];
    const int i = threadIdx.x;
    const int64_t n = n0 + blockIdx.x, b0 = off[n];
    const int32_t F = (int32_t)(off[n + 1] - b0);
    const double *s = S + (int64_t)Fr * b0 + (int64_t)i * F;
    double *dd = Dout ? Dout + (int64_t)Fr * b0 + (int64_t)i * F : nullptr;
    const int wpr = (F + 15) >> 4;
    uint32_t *codes = codes_in_lds ? (uint32_t *)dtw_codes : codes_dev + (int64_t)blockIdx.x * Fr * words_per_row_max;
    const bool row = i < Fr;
    double left = 0.0, sv = row ? s[0] : 0.0;
    uint32_t word = 0;
    const int n_diag = Fr + F - 1;
    for (int d = 0; d < n_diag; d++) {
        const int j = d - i;
        if (row && j >= 0 && j < F) {
            double val;
            uint32_t code;
            if (i == 0) {
                val = j == 0 ? sv : left + sv;
                code = 2;
            } else if (j == 0) {
                val = diag[(d + 2) % 3][i - 1] + sv;
                code = 1;
            } else {
                double m = diag[(d + 1) % 3][i - 1];   // (i-1, j-1) lies on diagonal d - 2
                const double up = diag[(d + 2) % 3][i - 1];
                code = 0;
                if (up < m) m = up, code = 1;
                if (left < m) m = left, code = 2;
                val = m + sv;
            }
            diag[d % 3][i] = val;
            left = val;
            if (dd) dd[j] = val;
            word |= code << (2 * (j & 15));
            if ((j & 15) == 15 || j == F - 1) {
                codes[i * wpr + (j >> 4)] = word;
                word = 0;
            }
            if (j + 1 < F) sv = s[j + 1];
            if (i == Fr - 1 && j == F - 1) totals[n] = val;
        }
        __syncthreads();   // diagonal d is complete before d + 1 reads it, and d - 2 is read before d + 1 overwrites it
    }
    __threadfence_block();
    __syncthreads();
    int32_t *p = paths + 2 * (b0 + n * (int64_t)(Fr - 1));
    if (i == 0) {
        int xi = Fr - 1, yi = F - 1, k = 0, last_row = -1;
        while (k < n_diag) {
            p[2 * k] = xi, p[2 * k + 1] = yi;
            k++;
            if (xi != last_row) warp[n * Fr + xi] = yi, last_row = xi;
            if (xi == 0 && yi == 0) break;
            const uint32_t code = xi == 0 ? 2u : yi == 0 ? 1u : (codes[xi * wpr + (yi >> 4)] >> (2 * (yi & 15))) & 3u;
            if (code != 2) xi--;
            if (code != 1) yi--;
        }
        path_len[n] = k;
        s_len = k;
    }
    __threadfence_block();
    __syncthreads();
    const int len = s_len;
    for (int k = i; k < len / 2; k += blockDim.x) {   // front to back, as find_path returns it
        const int o = len - 1 - k;
        const int32_t x0 = p[2 * k], y0 = p[2 * k + 1], x1 = p[2 * o], y1 = p[2 * o + 1];
        p[2 * k] = x1, p[2 * k + 1] = y1, p[2 * o] = x0, p[2 * o + 1] = y0;
    }
}

// flag[0] = 1 for a warping index outside its motion (nothing is read for it)
__global__ __launch_bounds__(DTW_BLOCK) void dtw_warp_kernel(const double *__restrict__ frames, const int64_t *__restrict__ off, int32_t n_dim,
                                                             const int32_t *__restrict__ warp, int32_t Fr, double *__restrict__ out, int64_t n_rows,
                                                             int32_t *__restrict__ flag) {
    const int64_t rowi = (int64_t)blockIdx.x * (DTW_BLOCK / 64) + (threadIdx.x >> 6);   // a wave per output frame
    if (rowi >= n_rows) return;
    const int64_t n = rowi / Fr, b0 = off[n];
    const int32_t F = (int32_t)(off[n + 1] - b0), src = warp[rowi];
    if (src < 0 || src >= F) {
        if ((threadIdx.x & 63) == 0) flag[0] = 1;
        return;
    }
    const double *f = frames + (b0 + src) * n_dim;
    double *o = out + rowi * n_dim;
    for (int e = threadIdx.x & 63; e < n_dim; e += 64) o[e] = f[e];
}

// ---- host --------------------------------------------------------------------------------------------------------------------
#define DTW_STR2(x) #x
#define DTW_STR(x) DTW_STR2(x)

static int dtw_check_offsets(const char *who, const int64_t *offsets, int64_t n_motions, int32_t n_ref_frames, int32_t *f_max) {
    MG_REQUIRE_AS(n_ref_frames >= 1, MG_ERR_INVALID_ARGUMENT, "%s: %d reference frames", who, n_ref_frames);
    MG_REQUIRE_AS(n_ref_frames <= DTW_MAX_FRAMES, MG_ERR_UNSUPPORTED, "%s: %d reference frames (at most %d)", who, n_ref_frames, DTW_MAX_FRAMES);
    MG_REQUIRE_AS(n_motions < ((int64_t)1 << 24), MG_ERR_UNSUPPORTED, "%s: %lld motions (fewer than 2^24)", who, (long long)n_motions);
    int64_t longest = 0;
    const int rc = mg_check_offsets(who, offsets, n_motions, DTW_MAX_FRAMES, "at most " DTW_STR(DTW_MAX_FRAMES), MG_ERR_UNSUPPORTED, &longest);
    *f_max = (int32_t)longest;
    return rc;
}

extern "C" int mg_dtw_distance_grids(mg_context *ctx, const double *ref_cloud_dev, int32_t n_ref_frames, const double *clouds_dev, const int64_t *offsets,
                                     int64_t n_motions, int32_t n_joints, const double *weights, double *grids_dev) {
    MG_REQUIRE_AS(ctx && ref_cloud_dev && offsets, MG_ERR_INVALID_ARGUMENT, "mg_dtw_distance_grids: NULL argument");
    MG_REQUIRE_AS(n_motions >= 0 && n_joints >= 1, MG_ERR_INVALID_ARGUMENT, "mg_dtw_distance_grids: n_motions = %lld, n_joints = %d", (long long)n_motions,
                  n_joints);
    MG_REQUIRE_AS(n_joints <= DTW_MAX_JOINTS, MG_ERR_UNSUPPORTED, "mg_dtw_distance_grids: %d joints (at most %d)", n_joints, DTW_MAX_JOINTS);
    int32_t f_max = 0;
    const int rc = dtw_check_offsets("mg_dtw_distance_grids", offsets, n_motions, n_ref_frames, &f_max);
    if (rc != MG_OK || n_motions == 0) return rc;
    MG_REQUIRE_AS(clouds_dev && grids_dev, MG_ERR_INVALID_ARGUMENT, "mg_dtw_distance_grids: NULL argument");
    double ones[DTW_MAX_JOINTS];
    const int rw = dtw_weights("mg_dtw_distance_grids", weights, n_joints, ones);
    if (rw != MG_OK) return rw;
    dtw_block blk(ctx, "mg_dtw_distance_grids");
    const int rb = dtw_block_create(&blk, offsets, n_motions, ones, n_joints, 0);
    if (rb != MG_OK) return rb;
    const int64_t row_len = 3 * (int64_t)n_joints;
    dtw_launch_nonfinite(ctx, ref_cloud_dev, n_ref_frames * row_len, blk.flag);
    dtw_launch_nonfinite(ctx, clouds_dev, offsets[n_motions] * row_len, blk.flag);
    int32_t flag = 0;
    const int rf = dtw_flag_after(ctx, blk, &flag);
    if (rf != MG_OK) return rf;
    MG_REQUIRE_AS(!flag, MG_ERR_INVALID_ARGUMENT, "mg_dtw_distance_grids: the point clouds hold non-finite values");
    const int tiles_i = (n_ref_frames + DTW_TILE - 1) / DTW_TILE, tiles_j = (f_max + DTW_TILE - 1) / DTW_TILE;
    const size_t lds = ((size_t)2 * DTW_TILE * ((3 * n_joints) | 1) + DTW_MAX_JOINTS + 4 * DTW_TILE + 1) * 8;   // at most 50 440 bytes
    for (int64_t n0 = 0; n0 < n_motions; n0 += 65535) {     // grid.y limit
        const int64_t nb = std::min<int64_t>(65535, n_motions - n0);
        hipLaunchKernelGGL(dtw_distance_grids_kernel, dim3((unsigned)(tiles_i * tiles_j), (unsigned)nb), dim3(DTW_BLOCK), lds, ctx->stream, ref_cloud_dev,
                           n_ref_frames, clouds_dev, (const int64_t *)blk.off, n_joints, (const double *)blk.w, grids_dev, tiles_j, n0);
    }
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

extern "C" int mg_dtw_paths(mg_context *ctx, const double *grids_dev, int32_t n_ref_frames, const int64_t *offsets, int64_t n_motions,
                            double *accumulated_dev, double *totals_dev, int32_t *paths_dev, int32_t *path_lengths_dev, int32_t *warping_dev) {
    MG_REQUIRE_AS(ctx && offsets, MG_ERR_INVALID_ARGUMENT, "mg_dtw_paths: NULL argument");
    MG_REQUIRE_AS(n_motions >= 0, MG_ERR_INVALID_ARGUMENT, "mg_dtw_paths: n_motions = %lld", (long long)n_motions);
    int32_t f_max = 0;
    const int rc = dtw_check_offsets("mg_dtw_paths", offsets, n_motions, n_ref_frames, &f_max);
    if (rc != MG_OK || n_motions == 0) return rc;
    MG_REQUIRE_AS(grids_dev && totals_dev && paths_dev && path_lengths_dev && warping_dev, MG_ERR_INVALID_ARGUMENT, "mg_dtw_paths: NULL argument");
    const int32_t wpr_max = (f_max + 15) / 16;
    const size_t code_bytes = (size_t)n_ref_frames * wpr_max * 4;
    const bool in_lds = code_bytes <= DTW_CODE_LDS_BYTES;
    const int64_t chunk = 65535;
    dtw_block blk(ctx, "mg_dtw_paths");
    const int rb = dtw_block_create(&blk, offsets, n_motions, nullptr, 0, in_lds ? 0 : code_bytes * (size_t)std::min(chunk, n_motions));
    if (rb != MG_OK) return rb;
    dtw_launch_nonfinite(ctx, grids_dev, (int64_t)n_ref_frames * offsets[n_motions], blk.flag);
    int32_t flag = 0;
    const int rf = dtw_flag_after(ctx, blk, &flag);
    if (rf != MG_OK) return rf;
    MG_REQUIRE_AS(!flag, MG_ERR_INVALID_ARGUMENT, "mg_dtw_paths: the grids hold non-finite values");
    if (in_lds && code_bytes + sizeof(double) * 3 * DTW_MAX_FRAMES + 64 > 64 * 1024)
        MG_HIP_CHECK(mg_lds_opt_in(DTW_CODE_LDS_BYTES, dtw_paths_kernel));
    const unsigned block = (unsigned)((n_ref_frames + 63) / 64 * 64);
    for (int64_t n0 = 0; n0 < n_motions; n0 += chunk) {
        const int64_t nb = std::min(chunk, n_motions - n0);
        hipLaunchKernelGGL(dtw_paths_kernel, dim3((unsigned)nb), dim3(block), in_lds ? code_bytes : 0, ctx->stream, grids_dev, n_ref_frames,
                           (const int64_t *)blk.off, accumulated_dev, totals_dev, paths_dev, path_lengths_dev, warping_dev, (uint32_t *)blk.extra, wpr_max,
                           in_lds ? 1 : 0, n0);
    }
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

extern "C" int mg_warp_motions(mg_context *ctx, const double *frames_dev, const int64_t *offsets, int64_t n_motions, int32_t n_dim,
                               const int32_t *warping_dev, int32_t n_ref_frames, double *warped_dev) {
    MG_REQUIRE_AS(ctx && offsets, MG_ERR_INVALID_ARGUMENT, "mg_warp_motions: NULL argument");
    MG_REQUIRE_AS(n_motions >= 0 && n_dim >= 1, MG_ERR_INVALID_ARGUMENT, "mg_warp_motions: n_motions = %lld, n_dim = %d", (long long)n_motions, n_dim);
    MG_REQUIRE_AS(n_dim <= (1 << 20), MG_ERR_UNSUPPORTED, "mg_warp_motions: %d channels (at most 2^20)", n_dim);
    int32_t f_max = 0;
    const int rc = dtw_check_offsets("mg_warp_motions", offsets, n_motions, n_ref_frames, &f_max);
    if (rc != MG_OK || n_motions == 0) return rc;
    MG_REQUIRE_AS(frames_dev && warping_dev && warped_dev, MG_ERR_INVALID_ARGUMENT, "mg_warp_motions: NULL argument");
    dtw_block blk(ctx, "mg_warp_motions");
    const int rb = dtw_block_create(&blk, offsets, n_motions, nullptr, 0, 0);
    if (rb != MG_OK) return rb;
    const int64_t n_rows = n_motions * n_ref_frames, per_wg = DTW_BLOCK / 64;
    MG_REQUIRE_AS(n_rows / per_wg < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED, "mg_warp_motions: %lld output frames", (long long)n_rows);
    hipLaunchKernelGGL(dtw_warp_kernel, dim3((unsigned)((n_rows + per_wg - 1) / per_wg)), dim3(DTW_BLOCK), 0, ctx->stream, frames_dev,
                       (const int64_t *)blk.off, n_dim, warping_dev, n_ref_frames, warped_dev, n_rows, blk.flag);
    int32_t flag = 0;
    const int rf = dtw_flag_after(ctx, blk, &flag);
    if (rf != MG_OK) return rf;
    MG_REQUIRE_AS(!flag, MG_ERR_INVALID_ARGUMENT, "mg_warp_motions: a warping function points outside its motion");
    return MG_OK;
}
