// What mg_dtw.hip and mg_segment.hip share: the arithmetic of one cell of a distance grid (the contract is the header comment
// of mg_dtw.hip; both files compile these very statements, so a cell has the same bits whichever kernel evaluates it), the
// non-finite check kernel and the per-call device block with its flag.
#pragma once
#include "mg_internal.h"

#include <cmath>

#define DTW_MAX_JOINTS 64
#define DTW_BLOCK 256

#define DTW_REQUIRE(cond, code, ...)   \
    do {                               \
        if (!(cond)) {                 \
            mg_set_error(__VA_ARGS__); \
            return (code);             \
        }                              \
    } while (0)

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
// a device block for one call: the offsets, 64 doubles, a 256-byte flag area, then `extra` bytes
struct dtw_block {
    char *base = nullptr;
    int64_t *off = nullptr;
    double *w = nullptr;
    int32_t *flag = nullptr;
    char *extra = nullptr;
    ~dtw_block() { if (base) (void)hipFree(base); }
};

static inline int dtw_block_create(const char *who, mg_context *ctx, dtw_block *b, const int64_t *offsets, int64_t n_motions, const double *weights,
                                   int32_t n_w, size_t extra) {
    const size_t o_w = (((size_t)n_motions + 1) * 8 + 255) & ~(size_t)255, o_flag = o_w + 512, o_extra = o_flag + 256, total = o_extra + extra;
    if (hipMalloc(&b->base, total) != hipSuccess) {
        (void)hipGetLastError();
        b->base = nullptr;
        mg_set_error("%s: cannot allocate %zu bytes of device memory", who, total);
        return MG_ERR_OUT_OF_MEMORY;
    }
    b->off = (int64_t *)b->base, b->w = (double *)(b->base + o_w), b->flag = (int32_t *)(b->base + o_flag), b->extra = b->base + o_extra;
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

static inline void dtw_launch_nonfinite(mg_context *ctx, const double *x, int64_t n, int32_t *flag) {
    if (n > 0) hipLaunchKernelGGL(dtw_nonfinite_kernel, dim3((unsigned)((n + DTW_BLOCK - 1) / DTW_BLOCK)), dim3(DTW_BLOCK), 0, ctx->stream, x, n, flag);
}
