// What the model-construction entry points share (mg_kmeans.hip, mg_gmm_em.hip, mg_fpca.hip, mg_dtw.hip, mg_segment.hip): the
// workgroup sum of the kernels, the per-call device block and the check of an offsets table.  The rules of a call live here:
//   * one hipMalloc per call, carved at 256-byte boundaries; one that fails is MG_ERR_OUT_OF_MEMORY with the size in the text;
//   * the block is freed when the call returns, after the stream has drained: a copy into the caller's (or the call's own)
//     host memory may still be in flight when an error cuts the call short;
//   * a call that fails leaves no HIP error behind for the next one's hipGetLastError.
#pragma once
#include "mg_internal.h"

// sum over the workgroup (BLOCK threads, red[BLOCK] in LDS) of one value per thread, in a fixed tree order
template <int BLOCK>
__device__ __forceinline__ double mg_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One host array's region of a call's block (mg_workspace).  Made from a NULL pointer or zero bytes it is absent: dev() is NULL and
// nothing is copied.
struct mg_staged {
    char *const *base = nullptr;
    size_t offset = 0;
    template <class T>
    T *dev() const { return base ? (T *)(*base + offset) : nullptr; }   // after upload()
};

// The device block of one call: carve() every region, alloc(), at<T>(offset); the destructor does the rest.  A call whose regions
// mirror host arrays states each once -- in(), out(), inout() -- then upload(), its kernels on h.dev<T>(), download().
struct mg_workspace {
    mg_context *ctx;
    const char *who;     // the entry point, for the error text
    char *base = nullptr;
    size_t bytes = 0;
    struct copy { size_t offset; void *host; size_t bytes; bool in, out; };
    std::vector<copy> copies;

    mg_workspace(mg_context *c, const char *w) : ctx(c), who(w) {}
    mg_workspace(const mg_workspace &) = delete;
    mg_workspace &operator=(const mg_workspace &) = delete;
    ~mg_workspace() {
        if (!base) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(base);
        (void)hipGetLastError();
    }
    static size_t align(size_t b) { return (b + 255) & ~(size_t)255; }
    size_t carve(size_t b) {
        const size_t o = bytes;
        bytes += align(b);
        return o;
    }
    int alloc() {
        MG_HIP_CHECK(hipSetDevice(ctx->device));
        if (hipMalloc(&base, bytes) != hipSuccess) {
            (void)hipGetLastError();
            base = nullptr;
            mg_set_error("%s: cannot allocate %zu bytes of device memory", who, bytes);
            return MG_ERR_OUT_OF_MEMORY;
        }
        return MG_OK;
    }
    template <class T>
    T *at(size_t offset) const { return (T *)(base + offset); }

    mg_staged stage(const void *host, size_t b, bool in, bool out) {
        if (!host || !b) return {};
        copies.push_back({carve(b), (void *)host, b, in, out});
        return {&base, copies.back().offset};
    }
    mg_staged room(size_t b) { return {&base, carve(b)}; }                             // the kernels' own: no host array, always present
    mg_staged in(const void *host, size_t b) { return stage(host, b, true, false); }    // copied to the device by upload()
    mg_staged out(void *host, size_t b) { return stage(host, b, false, true); }         // copied back by download()
    mg_staged inout(void *host, size_t b) { return stage(host, b, true, true); }        // both: what the kernels leave alone stays the caller's
    // alloc() and the copies in, on the context's stream (a call without regions allocates nothing)
    int upload() {
        if (!bytes) return MG_OK;
        const int rc = alloc();
        if (rc != MG_OK) return rc;
        for (const copy &c : copies)
            if (c.in) MG_HIP_CHECK(hipMemcpyAsync(base + c.offset, c.host, c.bytes, hipMemcpyHostToDevice, ctx->stream));
        return MG_OK;
    }
    // the copies out, then the stream drains: the host arrays are the caller's to read when it returns
    int download() {
        if (!base) return MG_OK;
        for (const copy &c : copies)
            if (c.out) MG_HIP_CHECK(hipMemcpyAsync(c.host, base + c.offset, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
        MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MG_OK;
    }
};

// mg_fpca.hip's batched float64 MFMA product on the context's stream, no synchronise: C[b] (M, Nc; rows ldc apart) = A[b] (M, K; rows lda
// apart) . B[b] (+ bias[col]), B's element (k, j) at k * sbk + j * sbj; batch b's matrices sAb, sBb, sCb doubles on
int mg_fpca_gemm(mg_context *ctx, const double *A, const double *B, const double *bias, double *C, int64_t batch, int64_t sAb, int64_t sBb, int64_t sCb,
                 int64_t M, int64_t Nc, int64_t K, int64_t lda, int64_t sbk, int64_t sbj, int64_t ldc);

// An offsets table of n_motions + 1 entries starts at 0 and rises, no motion longer than max_frames (`limit`: that bound in the
// caller's words, code_too_long: its status); *longest: the longest motion.
static inline int mg_check_offsets(const char *who, const int64_t *offsets, int64_t n_motions, int64_t max_frames, const char *limit, int code_too_long,
                                   int64_t *longest) {
    MG_REQUIRE_AS(offsets[0] == 0, MG_ERR_INVALID_ARGUMENT, "%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    *longest = 0;
    for (int64_t n = 0; n < n_motions; n++) {
        const int64_t f = offsets[n + 1] - offsets[n];
        MG_REQUIRE_AS(f >= 1, MG_ERR_INVALID_ARGUMENT, "%s: motion %lld has %lld frames (offsets must rise)", who, (long long)n, (long long)f);
        MG_REQUIRE_AS(f <= max_frames, code_too_long, "%s: motion %lld has %lld frames (%s)", who, (long long)n, (long long)f, limit);
        if (f > *longest) *longest = f;
    }
    return MG_OK;
}
