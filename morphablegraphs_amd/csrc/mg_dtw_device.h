// What mg_dtw.hip and mg_segment.hip share: the arithmetic of one cell of a distance grid (the contract is the header comment
// of mg_dtw.hip; both files compile these very statements, so a cell has the same bits whichever kernel evaluates it), the
// non-finite check kernel, the per-call device block with its flag and the check of the joint weights.
#pragma once
#include "mg_construct.h"

#include <cmath>

#define DTW_MAX_JOINTS 64
#define DTW_BLOCK 256

// ---- one cell ------------------------------------------------------------------------------------------------------------------
// sx = sum w_k x_k, sz = sum w_k z_k of the cloud p (J rows of x, y, z), in joint order
__device__ __forceinline__ void dtw_cloud_sums(const double *p, const double *w, int J, double *sx_out, double *sz_out) {
    double sx = 0.0, sz = 0.0;
    for (int k = 0; k < J; k++) {
        sx = sx + w[k] * p[3 * k];
        sz = sz + w[k] * p[3 * k + 2];
    }
    *sx_out = sx, *sz_out = sz;
}

__device__ __forceinline__ double dtw_weight_sum(const double *w, int J) {
    double s = 0.0;
    for (int k = 0; k < J; k++) s = s + w[k];
    return s;
}

// the mean point distance of the clouds a and b after the weighted 2-D rigid fit of b onto a; (sax, saz), (sbx, sbz): their
// dtw_cloud_sums, sw: dtw_weight_sum
__device__ __forceinline__ double dtw_cell(const double *a, const double *b, const double *w, int J, double sax, double saz, double sbx, double sbz,
                                           double sw) {
    double num = 0.0, den = 0.0;
    for (int k = 0; k < J; k++) {
        const double ax = a[3 * k], az = a[3 * k + 2], bx = b[3 * k], bz = b[3 * k + 2], wk = w[k];
        num = num + wk * (ax * bz - bx * az);
        den = den + wk * (ax * bx + az * bz);
    }
    num = num - (sax * sbz - sbx * saz) / sw;
    den = den - (sax * sbx + saz * sbz) / sw;
    const double theta = atan2(num, den);
    double sn, cs;
    sincos(theta, &sn, &cs);
    const double ox = ((sax - sbx * cs) - sbz * sn) / sw;
    const double oz = ((saz + sbx * sn) - sbz * cs) / sw;
    double total = 0.0;
    for (int k = 0; k < J; k++) {
        const double bx = b[3 * k], bz = b[3 * k + 2];
        const double dx = a[3 * k] - ((bx * cs + bz * sn) + ox);
        const double dy = a[3 * k + 1] - b[3 * k + 1];
        const double dz = a[3 * k + 2] - (((-bx) * sn + bz * cs) + oz);
        total = total + sqrt((dx * dx + dy * dy) + dz * dz);
    }
    return total / (double)J;
}

// ---- flag[0] = 1 if any of x[0 .. n) is not finite (every writer stores the same value) ------------------------------------
static __global__ __launch_bounds__(DTW_BLOCK) void dtw_nonfinite_kernel(const double *__restrict__ x, int64_t n, int32_t *__restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * DTW_BLOCK + threadIdx.x;
    if (e < n && !isfinite(x[e])) flag[0] = 1;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// the device block of one call: the offsets, 64 doubles, a 256-byte flag area, then `extra` bytes
struct dtw_block : mg_workspace {
    using mg_workspace::mg_workspace;
    int64_t *off = nullptr;
    double *w = nullptr;
    int32_t *flag = nullptr;
    char *extra = nullptr;
};

static inline int dtw_block_create(dtw_block *b, const int64_t *offsets, int64_t n_motions, const double *weights, int32_t n_w, size_t extra) {
    const size_t o_off = b->carve(((size_t)n_motions + 1) * 8), o_w = b->carve(512), o_flag = b->carve(256), o_extra = b->carve(extra);
    const int rc = b->alloc();
    if (rc != MG_OK) return rc;
    mg_context *ctx = b->ctx;
    b->off = b->at<int64_t>(o_off), b->w = b->at<double>(o_w), b->flag = b->at<int32_t>(o_flag), b->extra = b->at<char>(o_extra);
    MG_HIP_CHECK(hipMemcpyAsync(b->off, offsets, ((size_t)n_motions + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_w > 0) MG_HIP_CHECK(hipMemcpyAsync(b->w, weights, (size_t)n_w * 8, hipMemcpyHostToDevice, ctx->stream));
    MG_HIP_CHECK(hipMemsetAsync(b->flag, 0, 256, ctx->stream));
    return MG_OK;
}

static inline int dtw_flag_after(mg_context *ctx, const dtw_block &b, int32_t *flag) {
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipMemcpyAsync(flag, b.flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

// w[0 .. n_joints) = the caller's weights, or ones: finite, none negative, not all zero
static inline int dtw_weights(const char *who, const double *weights, int32_t n_joints, double *w) {
    double wsum = 0.0;
    for (int k = 0; k < n_joints; k++) {
        w[k] = weights ? weights[k] : 1.0;
        MG_REQUIRE_AS(std::isfinite(w[k]) && w[k] >= 0.0, MG_ERR_INVALID_ARGUMENT, "%s: weight %d is %g", who, k, w[k]);
        wsum += w[k];
    }
    MG_REQUIRE_AS(wsum > 0.0, MG_ERR_INVALID_ARGUMENT, "%s: the weights add up to 0", who);
    return MG_OK;
}

static inline void dtw_launch_nonfinite(mg_context *ctx, const double *x, int64_t n, int32_t *flag) {
    if (n > 0) hipLaunchKernelGGL(dtw_nonfinite_kernel, dim3((unsigned)((n + DTW_BLOCK - 1) / DTW_BLOCK)), dim3(DTW_BLOCK), 0, ctx->stream, x, n, flag);
}
