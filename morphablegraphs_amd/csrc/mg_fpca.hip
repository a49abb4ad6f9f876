// Functional PCA of aligned motions (reference construction/fpca: FunctionalData, PCAFunctionalData, run_pca), float64.
//
//   mg_spline_fit_batch   C[n] = P . Y[n]: the (n_basis, F) least-squares operator of the cubic B-spline design matrix (the
//                         host factors it once, the same for every motion) applied to each motion's (F, D) frames.
//   mg_pca_fit            column mean, centred matrix, and the singular values / right singular vectors of the centred
//                         matrix by one-sided (Hestenes) Jacobi on the short side: no Gram matrix is formed.
//   mg_pca_project / mg_pca_backproject     low = X . Vt^T and high = low . Vt + mean.
//
// The three products run on one kernel, fpca_gemm_kernel: one wave per 16 x 16 output tile, v_mfma_f64_16x16x4_f64 over K
// in steps of 4 (A: lane l supplies A[row l & 15][k l >> 4], B: B[k l >> 4][col l & 15], D: col l & 15, row (l >> 4) + 4 reg).
// Tiles are padded with zeros by a select on a clamped in-bounds address; nothing is read past a row.
//
// Jacobi: the work matrix W holds the short side in its m rows of length L (N <= P: the centred rows, L = P; N > P: the
// centred columns, L = N, with the companion G = I (m, m) rotated alongside, so that G ends as Vt).  A sweep is m' - 1
// rounds (m' = m rounded up to even) of the round-robin schedule, one launch per round, one workgroup per disjoint pair:
// a = |w_i|^2, b = |w_j|^2, c = w_i . w_j by a strided partial sum per thread and a tree over the workgroup, then the
// rotation that makes the pair orthogonal if |c| > tol sqrt(a b), tol = eps sqrt(L).  The host reads the sweep's rotation
// count (an integer counter) once per sweep and stops at zero.  Every sum runs in an order fixed by the shapes alone, the
// schedule does not depend on the device: the same input gives the same bits.  No float atomics, no grid barriers.
// G takes every rotation of every sweep, so its orthonormality drifts with their number (7e-14 at m = 255 after 13 sweeps);
// after the last sweep one Newton-Schulz step G <- G - (G G^T G - G) / 2 on the GEMM kernel brings it back to rounding level.
// The step costs two m x m x m products and two more m x m buffers next to G for the length of the call (3 x 128 MiB at m = 4096).
#include "mg_construct.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#define FP_BLOCK 256
#define FP_MAX_BASIS 64
#define FP_MAX_FRAMES 1024
#define FP_MAX_SHORT 4096
#define FP_MAX_LONG ((int64_t)1 << 20)
#define FP_MAX_SWEEPS 30

typedef double fp_f64x4 __attribute__((ext_vector_type(4)));

// ---- C[b] = A[b] . B[b] (+ bias): A (M, K) rows lda apart; B element (k, j) at k * sbk + j * sbj; C (M, Nc) rows ldc apart ----
struct fp_gemm_args {
    const double *A, *B, *bias;
    double *C;
    int64_t sAb, sBb, sCb, lda, sbk, sbj, ldc;
    int32_t M, Nc, K, tiles_n, n_tiles;
};

__global__ __launch_bounds__(FP_BLOCK) void fpca_gemm_kernel(fp_gemm_args g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * (FP_BLOCK / 64) + wave;
    if (tile >= g.n_tiles) return;   // whole wave
    const int ti = tile / g.tiles_n, tj = tile % g.tiles_n;
    const int cl = lane & 15, q = lane >> 4;
    const int row = ti * 16 + cl, col = tj * 16 + cl;
    const bool rok = row < g.M, cok = col < g.Nc;
    const double *a = g.A + (int64_t)blockIdx.y * g.sAb + (int64_t)(rok ? row : g.M - 1) * g.lda;
    const double *b = g.B + (int64_t)blockIdx.y * g.sBb + (int64_t)(cok ? col : g.Nc - 1) * g.sbj;
    fp_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < g.K; k0 += 4) {
        const int k = k0 + q;
        const bool kok = k < g.K;
        const int kc = kok ? k : g.K - 1;
        const double av = a[kc], bv = b[(int64_t)kc * g.sbk];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((rok && kok) ? av : 0.0, (cok && kok) ? bv : 0.0, acc, 0, 0, 0);
    }
    if (!cok) return;
    const double bias = g.bias ? g.bias[col] : 0.0;
    double *c = g.C + (int64_t)blockIdx.y * g.sCb;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int orow = ti * 16 + q + 4 * r;
        if (orow < g.M) c[(int64_t)orow * g.ldc + col] = acc[r] + bias;
    }
}

static int fp_gemm(mg_context *ctx, const double *A, const double *B, const double *bias, double *C, int64_t batch, int64_t sAb,
                   int64_t sBb, int64_t sCb, int64_t M, int64_t Nc, int64_t K, int64_t lda, int64_t sbk, int64_t sbj, int64_t ldc) {
    fp_gemm_args g;
    g.A = A, g.B = B, g.bias = bias, g.C = C;
    g.sAb = sAb, g.sBb = sBb, g.sCb = sCb, g.lda = lda, g.sbk = sbk, g.sbj = sbj, g.ldc = ldc;
    g.M = (int32_t)M, g.Nc = (int32_t)Nc, g.K = (int32_t)K;
    const int64_t tm = (M + 15) / 16, tn = (Nc + 15) / 16, tiles = tm * tn;
    g.tiles_n = (int32_t)tn, g.n_tiles = (int32_t)tiles;
    const int64_t wg = (tiles + FP_BLOCK / 64 - 1) / (FP_BLOCK / 64);
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {     // grid.y limit
        const int64_t nb = std::min<int64_t>(65535, batch - b0);
        fp_gemm_args h = g;
        h.A += b0 * sAb, h.B += b0 * sBb, h.C += b0 * sCb;
        hipLaunchKernelGGL(fpca_gemm_kernel, dim3((unsigned)wg, (unsigned)nb), dim3(FP_BLOCK), 0, ctx->stream, h);
        MG_HIP_CHECK(hipGetLastError());
    }
    return MG_OK;
}

// the same launches for the other construction files (mg_construct.h)
int mg_fpca_gemm(mg_context *ctx, const double *A, const double *B, const double *bias, double *C, int64_t batch, int64_t sAb, int64_t sBb, int64_t sCb,
                 int64_t M, int64_t Nc, int64_t K, int64_t lda, int64_t sbk, int64_t sbj, int64_t ldc) {
    return fp_gemm(ctx, A, B, bias, C, batch, sAb, sBb, sCb, M, Nc, K, lda, sbk, sbj, ldc);
}

extern "C" int mg_spline_fit_batch(mg_context *ctx, const double *motions_dev, int64_t n_motions, int32_t n_frames, int32_t n_dims,
                                   const double *operator_dev, int32_t n_basis, double *coeffs_dev) {
    MG_REQUIRE_AS(ctx && motions_dev && operator_dev && coeffs_dev, MG_ERR_INVALID_ARGUMENT, "mg_spline_fit_batch: NULL argument");
    MG_REQUIRE_AS(n_motions >= 0 && n_dims >= 1 && n_frames >= 1 && n_basis >= 1, MG_ERR_INVALID_ARGUMENT,
                  "mg_spline_fit_batch: n_motions = %lld, n_frames = %d, n_dims = %d, n_basis = %d", (long long)n_motions, n_frames, n_dims, n_basis);
    MG_REQUIRE_AS(n_basis <= FP_MAX_BASIS && n_frames <= FP_MAX_FRAMES, MG_ERR_UNSUPPORTED,
                  "mg_spline_fit_batch: n_basis = %d (at most %d), n_frames = %d (at most %d)", n_basis, FP_MAX_BASIS, n_frames, FP_MAX_FRAMES);
    MG_REQUIRE_AS(n_basis <= n_frames, MG_ERR_INVALID_ARGUMENT, "mg_spline_fit_batch: %d basis functions for %d frames", n_basis, n_frames);
    MG_REQUIRE_AS(n_dims <= (1 << 20) && n_motions < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED, "mg_spline_fit_batch: table too large");
    if (n_motions == 0) return MG_OK;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    const int rc = fp_gemm(ctx, operator_dev, motions_dev, nullptr, coeffs_dev, n_motions, 0, (int64_t)n_frames * n_dims, (int64_t)n_basis * n_dims,
                           n_basis, n_dims, n_frames, n_frames, n_dims, 1, n_dims);
    if (rc != MG_OK) return rc;
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

static int fp_check_project(const char *who, mg_context *ctx, const void *a, const void *b, const void *c, int64_t n, int64_t p, int64_t l) {
    MG_REQUIRE_AS(ctx && a && b && c, MG_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    MG_REQUIRE_AS(n >= 0 && p >= 1 && l >= 1, MG_ERR_INVALID_ARGUMENT, "%s: n = %lld, p = %lld, l = %lld", who, (long long)n, (long long)p, (long long)l);
    MG_REQUIRE_AS(l <= p, MG_ERR_INVALID_ARGUMENT, "%s: %lld components of a %lld-dimensional space", who, (long long)l, (long long)p);
    MG_REQUIRE_AS(n < ((int64_t)1 << 24) && p < ((int64_t)1 << 24) && ((n + 15) / 16) * ((p + 15) / 16) < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED,
                  "%s: table too large", who);
    return MG_OK;
}

extern "C" int mg_pca_project(mg_context *ctx, const double *x_dev, const double *vt_dev, int64_t n, int64_t p, int64_t l, double *low_dev) {
    const int rc = fp_check_project("mg_pca_project", ctx, x_dev, vt_dev, low_dev, n, p, l);
    if (rc != MG_OK || n == 0) return rc;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    const int rg = fp_gemm(ctx, x_dev, vt_dev, nullptr, low_dev, 1, 0, 0, 0, n, l, p, p, 1, p, l);
    if (rg != MG_OK) return rg;
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

extern "C" int mg_pca_backproject(mg_context *ctx, const double *low_dev, const double *vt_dev, const double *mean_dev, int64_t n, int64_t p,
                                  int64_t l, double *high_dev) {
    const int rc = fp_check_project("mg_pca_backproject", ctx, low_dev, vt_dev, high_dev, n, p, l);
    if (rc != MG_OK || n == 0) return rc;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    const int rg = fp_gemm(ctx, low_dev, vt_dev, mean_dev, high_dev, 1, 0, 0, 0, n, p, l, l, p, 1, p);
    if (rg != MG_OK) return rg;
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

// ---- centring: mean[j] = (sum of the rows in row order) / n, as NumPy's mean(axis = 0) adds them --------------------------
__global__ __launch_bounds__(FP_BLOCK) void fpca_mean_kernel(const double *__restrict__ A, int64_t n, int64_t p, double *__restrict__ mean) {
    const int64_t j = (int64_t)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= p) return;
    double s = 0.0;
    for (int64_t i = 0; i < n; i++) s = s + A[i * p + j];
    mean[j] = s / (double)n;
}

// centred (n, p) = A - mean; work = the same rows (transpose 0) or the columns as rows (transpose 1: work (p, n))
__global__ __launch_bounds__(FP_BLOCK) void fpca_centre_kernel(const double *__restrict__ A, const double *__restrict__ mean, int64_t n, int64_t p,
                                                               double *__restrict__ centred, double *__restrict__ work, int transpose) {
    const int64_t e = (int64_t)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (e >= n * p) return;
    const int64_t i = e / p, j = e % p;
    const double v = A[e] - mean[j];
    centred[e] = v;
    work[transpose ? j * n + i : e] = v;
}

__global__ __launch_bounds__(FP_BLOCK) void fpca_identity_kernel(double *__restrict__ G, int64_t m) {
    const int64_t e = (int64_t)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (e < m * m) G[e] = (e / m == e % m) ? 1.0 : 0.0;
}

// ---- one round of the round-robin schedule: workgroup k orthogonalises its pair of rows ----------------------------------
__global__ __launch_bounds__(FP_BLOCK) void fpca_jacobi_round_kernel(double *__restrict__ W, double *__restrict__ G, int32_t m, int32_t mp, int64_t L,
                                                                     int32_t round, double tol, int32_t *__restrict__ counter) {
    __shared__ double red[3][FP_BLOCK];
    const int tid = threadIdx.x, k = blockIdx.x, n1 = mp - 1;
    // the circle method: player mp - 1 stays, the others turn by one seat per round
    const int p = k == 0 ? n1 : (round + k) % n1;
    const int q = k == 0 ? round : (round - k + n1) % n1;
    const int i = p < q ? p : q, j = p < q ? q : p;
    if (j >= m) return;   // the bye of an odd m (whole workgroup)
    double *wi = W + (int64_t)i * L, *wj = W + (int64_t)j * L;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t e = tid; e < L; e += FP_BLOCK) {
        const double x = wi[e], y = wj[e];
        a = a + x * x;
        b = b + y * y;
        c = c + x * y;
    }
    red[0][tid] = a, red[1][tid] = b, red[2][tid] = c;
    __syncthreads();
    for (int s = FP_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
            red[2][tid] += red[2][tid + s];
        }
        __syncthreads();
    }
    a = red[0][0], b = red[1][0], c = red[2][0];
    if (!(a > 0.0) || !(b > 0.0) || !(fabs(c) > tol * sqrt(a * b))) return;   // uniform over the workgroup
    const double zeta = (b - a) / (2.0 * c);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
    for (int64_t e = tid; e < L; e += FP_BLOCK) {
        const double x = wi[e], y = wj[e];
        wi[e] = cs * x - sn * y;
        wj[e] = sn * x + cs * y;
    }
    if (G) {
        double *gi = G + (int64_t)i * m, *gj = G + (int64_t)j * m;
        for (int e = tid; e < m; e += FP_BLOCK) {
            const double x = gi[e], y = gj[e];
            gi[e] = cs * x - sn * y;
            gj[e] = sn * x + cs * y;
        }
    }
    if (tid == 0) atomicAdd(counter, 1);
}

// G <- G - (Y - G) / 2 with Y = (G G^T) G: Y - G is the small correction, subtracted from G in one rounding
__global__ __launch_bounds__(FP_BLOCK) void fpca_polish_kernel(double *__restrict__ G, const double *__restrict__ Y, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (e < count) G[e] = G[e] - 0.5 * (Y[e] - G[e]);
}

// sum of squares of a row on the host, in blocks of 64 (an order fixed by the length alone)
static double fp_row_norm2(const double *w, int64_t L) {
    double total = 0.0;
    for (int64_t e0 = 0; e0 < L; e0 += 64) {
        double s = 0.0;
        const int64_t e1 = std::min<int64_t>(L, e0 + 64);
        for (int64_t e = e0; e < e1; e++) s = s + w[e] * w[e];
        total = total + s;
    }
    return total;
}

// The device's part of mg_pca_fit: centring, the Jacobi sweeps and the polish in one device block, then the rotated rows (hW),
// the companion (hG, n > p only) and the mean to the host.  The block is freed on return, before the host's part runs.
static int fp_jacobi_device(mg_context *ctx, const double *a_dev, int64_t n, int64_t p, int32_t centre, double *centred_dev, double *mean,
                            std::vector<double> &hW, std::vector<double> &hG, int32_t *n_sweeps, int32_t *status) {
    const int64_t m = std::min(n, p), L = std::max(n, p);
    const bool wide = n <= p;           // rotate the rows of the centred matrix itself
    mg_workspace ws(ctx, "mg_pca_fit");
    const size_t g1 = wide ? 0 : mg_workspace::align((size_t)m * m * 8);   // G, G G^T, (G G^T) G
    const size_t o_w = ws.carve((size_t)n * p * 8), o_mean = ws.carve((size_t)p * 8), o_g = ws.carve(3 * g1), o_cnt = ws.carve(256);
    const int ra = ws.alloc();
    if (ra != MG_OK) return ra;
    double *W = ws.at<double>(o_w), *d_mean = ws.at<double>(o_mean), *G = wide ? nullptr : ws.at<double>(o_g);
    int32_t *d_cnt = ws.at<int32_t>(o_cnt);
    const int32_t mp = (int32_t)(m + (m & 1));
    int32_t sweeps = 0, st = 2;
    MG_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 256, ctx->stream));
    if (centre)
        hipLaunchKernelGGL(fpca_mean_kernel, dim3((unsigned)((p + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, ctx->stream, a_dev, n, p, d_mean);
    else
        MG_HIP_CHECK(hipMemsetAsync(d_mean, 0, (size_t)p * 8, ctx->stream));   // a - 0.0 is a
    hipLaunchKernelGGL(fpca_centre_kernel, dim3((unsigned)((n * p + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, ctx->stream, a_dev, d_mean, n, p,
                       centred_dev, W, wide ? 0 : 1);
    if (G) hipLaunchKernelGGL(fpca_identity_kernel, dim3((unsigned)((m * m + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, ctx->stream, G, m);
    MG_HIP_CHECK(hipGetLastError());
    const double tol = DBL_EPSILON * std::sqrt((double)L);
    if (m >= 2) {
        for (sweeps = 0; sweeps < FP_MAX_SWEEPS;) {
            for (int32_t r = 0; r < mp - 1; r++)
                hipLaunchKernelGGL(fpca_jacobi_round_kernel, dim3((unsigned)(mp / 2)), dim3(FP_BLOCK), 0, ctx->stream, W, G, (int32_t)m, mp, L, r, tol,
                                   d_cnt + sweeps);
            MG_HIP_CHECK(hipGetLastError());
            int32_t rotations = 0;
            MG_HIP_CHECK(hipMemcpyAsync(&rotations, d_cnt + sweeps, 4, hipMemcpyDeviceToHost, ctx->stream));
            MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            sweeps++;
            if (rotations == 0) {
                st = 1;
                break;
            }
        }
        if (G) {
            double *T = (double *)((char *)G + g1), *Y = (double *)((char *)G + 2 * g1);
            int rc = fp_gemm(ctx, G, G, nullptr, T, 1, 0, 0, 0, m, m, m, m, 1, m, m);                     // T = G G^T
            if (rc == MG_OK) rc = fp_gemm(ctx, T, G, nullptr, Y, 1, 0, 0, 0, m, m, m, m, m, 1, m);        // Y = T G
            if (rc != MG_OK) return rc;
            hipLaunchKernelGGL(fpca_polish_kernel, dim3((unsigned)((m * m + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, ctx->stream, G, Y, m * m);
            MG_HIP_CHECK(hipGetLastError());
        }
    } else {
        st = 1;
    }
    try {
        hW.resize((size_t)m * L);
        if (G) hG.resize((size_t)m * m);
    } catch (const std::bad_alloc &) {
        mg_set_error("mg_pca_fit: cannot allocate the host copy of a %lld x %lld matrix", (long long)m, (long long)L);
        return MG_ERR_OUT_OF_MEMORY;
    }
    MG_HIP_CHECK(hipMemcpyAsync(hW.data(), W, (size_t)m * L * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (G) MG_HIP_CHECK(hipMemcpyAsync(hG.data(), G, (size_t)m * m * 8, hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipMemcpyAsync(mean, d_mean, (size_t)p * 8, hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *n_sweeps = sweeps;
    *status = st;
    return MG_OK;
}

extern "C" int mg_pca_fit(mg_context *ctx, const double *a_dev, int64_t n, int64_t p, int32_t centre, double *centred_dev, double *mean,
                          double *singular_values, double *vt, int32_t *n_sweeps, int32_t *status) {
    MG_REQUIRE_AS(ctx && a_dev && centred_dev && mean && singular_values && vt && n_sweeps && status, MG_ERR_INVALID_ARGUMENT, "mg_pca_fit: NULL argument");
    MG_REQUIRE_AS(n >= 1 && p >= 1, MG_ERR_INVALID_ARGUMENT, "mg_pca_fit: matrix %lld x %lld", (long long)n, (long long)p);
    const int64_t m = std::min(n, p), L = std::max(n, p);
    MG_REQUIRE_AS(m <= FP_MAX_SHORT, MG_ERR_UNSUPPORTED, "mg_pca_fit: min(n, p) = %lld, at most %d", (long long)m, FP_MAX_SHORT);
    MG_REQUIRE_AS(L <= FP_MAX_LONG, MG_ERR_UNSUPPORTED, "mg_pca_fit: max(n, p) = %lld, at most %lld", (long long)L, (long long)FP_MAX_LONG);
    const bool wide = n <= p;
    std::vector<double> hW, hG;
    int32_t sweeps = 0, st = 2;
    const int rc = fp_jacobi_device(ctx, a_dev, n, p, centre, centred_dev, mean, hW, hG, &sweeps, &st);
    if (rc != MG_OK) return rc;
    // ---- the host's part: norms, descending order (stable), normalisation, null rows, the sign rule ----
    std::vector<double> sig(m);
    for (int64_t r = 0; r < m; r++) sig[r] = std::sqrt(fp_row_norm2(hW.data() + r * L, L));
    for (int64_t r = 0; r < m; r++)
        MG_REQUIRE_AS(std::isfinite(sig[r]), MG_ERR_INVALID_ARGUMENT, "mg_pca_fit: the matrix holds non-finite values (or its norms overflow)");
    std::vector<int64_t> order(m);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return sig[x] > sig[y]; });
    const double smax = sig[order[0]];
    const double null_below = smax * DBL_EPSILON * (double)L;     // the rank tolerance of numpy.linalg.matrix_rank
    std::vector<char> null_row(m, 0);
    for (int64_t r = 0; r < m; r++) {
        const int64_t src = order[r];
        singular_values[r] = sig[src];
        double *out = vt + r * p;
        if (!wide) {
            for (int64_t e = 0; e < p; e++) out[e] = hG[src * m + e];
        } else if (sig[src] > null_below) {
            for (int64_t e = 0; e < p; e++) out[e] = hW[src * L + e] / sig[src];
        } else {
            null_row[r] = 1;
        }
    }
    // A row without a direction of its own (singular value at round-off level; after centring the last of n <= p rows always is):
    // the unit vector that the rows set so far leave the longest (the first on ties), after two Gram-Schmidt passes against them.
    std::vector<char> done(m, 0);
    for (int64_t r = 0; r < m; r++) done[r] = !null_row[r];
    std::vector<double> left(p);
    for (int64_t r = 0; r < m; r++) {
        if (!null_row[r]) continue;
        double *out = vt + r * p;
        std::fill(left.begin(), left.end(), 1.0);
        for (int64_t s = 0; s < m; s++)
            if (done[s])
                for (int64_t e = 0; e < p; e++) left[e] = left[e] - vt[s * p + e] * vt[s * p + e];
        int64_t unit = 0;
        for (int64_t e = 1; e < p; e++)
            if (left[e] > left[unit]) unit = e;
        for (int64_t e = 0; e < p; e++) out[e] = e == unit ? 1.0 : 0.0;
        for (int pass = 0; pass < 2; pass++)
            for (int64_t s = 0; s < m; s++) {
                if (!done[s]) continue;
                const double *v = vt + s * p;
                double dot = 0.0;
                for (int64_t e = 0; e < p; e++) dot = dot + v[e] * out[e];
                for (int64_t e = 0; e < p; e++) out[e] = out[e] - dot * v[e];
            }
        const double nn = std::sqrt(fp_row_norm2(out, p));
        if (nn > 0.0)
            for (int64_t e = 0; e < p; e++) out[e] = out[e] / nn;
        done[r] = 1;
    }
    // sign rule: the entry of largest magnitude is positive, the first one on ties
    for (int64_t r = 0; r < m; r++) {
        double *out = vt + r * p;
        int64_t best = 0;
        for (int64_t e = 1; e < p; e++)
            if (std::fabs(out[e]) > std::fabs(out[best])) best = e;
        if (out[best] < 0.0)
            for (int64_t e = 0; e < p; e++) out[e] = -out[e];
    }
    *n_sweeps = sweeps;
    *status = st;
    return MG_OK;
}

// ---- mg_pca_fit_leading: the leading principal components of a matrix beyond Jacobi's short-side limit -------------------------------
// Blocked subspace iteration on the Gram form Xc^T Xc with a block Q (b, p) of orthonormal rows:
//   Y = Xc Q^T (n, b)      fpca_gemm_kernel, as mg_pca_project runs it
//   Z = Y^T Xc (b, p)      fpca_gemm_ta_kernel below: row i of Z is (Xc^T Xc) q_i
//   the host reads Z: lambda_i = q_i . z_i (the Rayleigh quotient, s_i^2), residual_i = |z_i - lambda_i q_i|, the component count
//   Q <- the right singular vectors of Z by mg_pca_fit(Z, centre = 0): Jacobi on a short side of b, ordered, with its sign rule
// until every kept component's residual is at most tol lambda_1, or the cap.  The block starts at FP_LEAD_START rows and doubles
// (the rows it has, plus new start rows, re-orthonormalised by mg_pca_fit) while it captures no more than `fraction` of the variance
// or keeps fewer than FP_LEAD_SPARE rows beyond the kept ones.  The start rows are a counter-based hash of (row, column): the same
// for every call.  Every sum -- the column sums of squares in row order, the host's sums in index order, the MFMA's k order -- is fixed
// by the shape alone.
#define FP_LEAD_START 12
#define FP_LEAD_SPARE 4
#define FP_LEAD_MAX_ITERATIONS 100

// C (M, Nc) = A^T . B with A (K, M) and B (K, Nc) row-major: one wave per 16 x 16 tile like fpca_gemm_kernel, lane l supplies
// A^T[row l & 15][k l >> 4] = A[k][row] and B[k][col l & 15]; the k-tail and the edge tiles by a select on a clamped address.
struct fp_gemm_ta_args {
    const double *A, *B;
    double *C;
    int64_t lda, ldb, ldc;
    int32_t M, Nc, K, tiles_n, n_tiles;
};

__global__ __launch_bounds__(FP_BLOCK) void fpca_gemm_ta_kernel(fp_gemm_ta_args g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * (FP_BLOCK / 64) + wave;
    if (tile >= g.n_tiles) return;   // whole wave
    const int ti = tile / g.tiles_n, tj = tile % g.tiles_n;
    const int cl = lane & 15, q = lane >> 4;
    const int row = ti * 16 + cl, col = tj * 16 + cl;
    const bool rok = row < g.M, cok = col < g.Nc;
    const double *a = g.A + (rok ? row : g.M - 1);
    const double *b = g.B + (cok ? col : g.Nc - 1);
    fp_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < g.K; k0 += 4) {
        const int k = k0 + q;
        const bool kok = k < g.K;
        const int kc = kok ? k : g.K - 1;
        const double av = a[(int64_t)kc * g.lda], bv = b[(int64_t)kc * g.ldb];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((rok && kok) ? av : 0.0, (cok && kok) ? bv : 0.0, acc, 0, 0, 0);
    }
    if (!cok) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int orow = ti * 16 + q + 4 * r;
        if (orow < g.M) g.C[(int64_t)orow * g.ldc + col] = acc[r];
    }
}

static int fp_gemm_ta(mg_context *ctx, const double *A, const double *B, double *C, int64_t M, int64_t Nc, int64_t K, int64_t lda, int64_t ldb, int64_t ldc) {
    fp_gemm_ta_args g;
    g.A = A, g.B = B, g.C = C, g.lda = lda, g.ldb = ldb, g.ldc = ldc;
    g.M = (int32_t)M, g.Nc = (int32_t)Nc, g.K = (int32_t)K;
    const int64_t tn = (Nc + 15) / 16, tiles = ((M + 15) / 16) * tn;
    g.tiles_n = (int32_t)tn, g.n_tiles = (int32_t)tiles;
    hipLaunchKernelGGL(fpca_gemm_ta_kernel, dim3((unsigned)((tiles + FP_BLOCK / 64 - 1) / (FP_BLOCK / 64))), dim3(FP_BLOCK), 0, ctx->stream, g);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

// ss[j] = the sum of squares of column j, the rows added in row order
__global__ __launch_bounds__(FP_BLOCK) void fpca_column_squares_kernel(const double *__restrict__ A, int64_t n, int64_t p, double *__restrict__ ss) {
    const int64_t j = (int64_t)blockIdx.x * FP_BLOCK + threadIdx.x;
    if (j >= p) return;
    double s = 0.0;
    for (int64_t i = 0; i < n; i++) { const double v = A[i * p + j]; s = s + v * v; }
    ss[j] = s;
}

// start row r of the block: uniform in [-1, 1) from a hash of (r, column) (splitmix64's finaliser)
static void fp_lead_start_row(int64_t r, int64_t p, double *out) {
    for (int64_t e = 0; e < p; e++) {
        uint64_t z = ((uint64_t)r << 32) + (uint64_t)e + 0x9e3779b97f4a7c15ull;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z = z ^ (z >> 31);
        out[e] = (double)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;   // 53 bits / 2^52 - 1
    }
}

extern "C" int mg_pca_fit_leading(mg_context *ctx, const double *a_dev, int64_t n, int64_t p, double fraction, double tol, int32_t max_iterations,
                                  double *centred_dev, double *mean, int32_t k_cap, int32_t *k_out, double *singular_values, double *vt, double *ratios,
                                  int32_t *iterations, int32_t *status) {
    const char *who = "mg_pca_fit_leading";
    MG_REQUIRE_AS(ctx && a_dev && centred_dev && mean && k_out && singular_values && vt && ratios && iterations && status, MG_ERR_INVALID_ARGUMENT,
                  "%s: NULL argument", who);
    MG_REQUIRE_AS(n >= 2 && p >= 1 && k_cap >= 1, MG_ERR_INVALID_ARGUMENT, "%s: matrix %lld x %lld, room for %d components", who, (long long)n, (long long)p, k_cap);
    MG_REQUIRE_AS(fraction > 0.0 && fraction < 1.0, MG_ERR_INVALID_ARGUMENT, "%s: fraction %g outside (0, 1)", who, fraction);
    MG_REQUIRE_AS(n < ((int64_t)1 << 24) && p <= FP_MAX_LONG && ((n + 15) / 16) * ((p + 15) / 16) < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED,
                  "%s: table too large (n below 2^24, p at most 2^20, fewer than 2^31 tiles of 16 x 16)", who);
    const int64_t m = std::min(n, p), b_max = std::min<int64_t>(m, FP_MAX_SHORT);
    if (!(tol > 0.0)) tol = 64.0 * DBL_EPSILON * std::sqrt((double)std::max(n, p));
    const int32_t cap = max_iterations > 0 ? max_iterations : FP_LEAD_MAX_ITERATIONS;
    *k_out = 0, *iterations = 0, *status = 2;
    MG_HIP_CHECK(hipSetDevice(ctx->device));

    // centring and the total variance
    std::vector<double> colss;
    try { colss.resize((size_t)p); } catch (const std::bad_alloc &) { return MG_ERR_OUT_OF_MEMORY; }
    {
        mg_workspace ws(ctx, who);
        const size_t o_mean = ws.carve((size_t)p * 8), o_ss = ws.carve((size_t)p * 8);
        const int ra = ws.alloc();
        if (ra != MG_OK) return ra;
        double *d_mean = ws.at<double>(o_mean), *d_ss = ws.at<double>(o_ss);
        const unsigned gp = (unsigned)((p + FP_BLOCK - 1) / FP_BLOCK);
        hipLaunchKernelGGL(fpca_mean_kernel, dim3(gp), dim3(FP_BLOCK), 0, ctx->stream, a_dev, n, p, d_mean);
        hipLaunchKernelGGL(fpca_centre_kernel, dim3((unsigned)((n * p + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, ctx->stream, a_dev, (const double *)d_mean, n, p,
                           centred_dev, centred_dev, 0);
        hipLaunchKernelGGL(fpca_column_squares_kernel, dim3(gp), dim3(FP_BLOCK), 0, ctx->stream, (const double *)centred_dev, n, p, d_ss);
        MG_HIP_CHECK(hipGetLastError());
        MG_HIP_CHECK(hipMemcpyAsync(mean, d_mean, (size_t)p * 8, hipMemcpyDeviceToHost, ctx->stream));
        MG_HIP_CHECK(hipMemcpyAsync(colss.data(), d_ss, (size_t)p * 8, hipMemcpyDeviceToHost, ctx->stream));
        MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    double total = 0.0;      // |Xc|_F^2 = (n - 1) x the total variance, the columns added in blocks of 64
    for (int64_t e0 = 0; e0 < p; e0 += 64) {
        double s = 0.0;
        for (int64_t e = e0; e < std::min<int64_t>(p, e0 + 64); e++) s = s + colss[(size_t)e];
        total = total + s;
    }
    MG_REQUIRE_AS(std::isfinite(total), MG_ERR_INVALID_ARGUMENT, "%s: the matrix holds non-finite values (or its norms overflow)", who);
    MG_REQUIRE_AS(total > 0.0, MG_ERR_INVALID_ARGUMENT, "%s: the matrix has no variance", who);

    int64_t b = std::min<int64_t>(b_max, FP_LEAD_START);
    std::vector<double> hQ, hZ, lam, resid, sv_tmp, mean_tmp;
    int32_t iters = 0, in_block = 0, st = 2, k = 0;
    bool q_ready = false;    // hQ holds orthonormal rows and the device has them
    for (;;) {
        try {
            hQ.resize((size_t)b * p); hZ.resize((size_t)b * p); lam.resize((size_t)b); resid.resize((size_t)b); sv_tmp.resize((size_t)b); mean_tmp.resize((size_t)p);
        } catch (const std::bad_alloc &) {
            mg_set_error("%s: cannot allocate the host copies of a %lld x %lld block", who, (long long)b, (long long)p);
            return MG_ERR_OUT_OF_MEMORY;
        }
        mg_workspace ws(ctx, who);
        const size_t o_q = ws.carve((size_t)b * p * 8), o_z = ws.carve((size_t)b * p * 8), o_c = ws.carve((size_t)b * p * 8), o_y = ws.carve((size_t)n * b * 8);
        const int ra = ws.alloc();
        if (ra != MG_OK) return ra;
        double *Q = ws.at<double>(o_q), *Z = ws.at<double>(o_z), *Cz = ws.at<double>(o_c), *Y = ws.at<double>(o_y);
        int32_t sweeps = 0, jst = 0;
        if (!q_ready) {
            // rows the caller of this block left in hQ (the first `k` of them, 0 at the start), then start rows; orthonormalised by Jacobi
            for (int64_t r = k; r < b; r++) fp_lead_start_row(r, p, hQ.data() + (size_t)r * p);
            MG_HIP_CHECK(hipMemcpyAsync(Z, hQ.data(), (size_t)b * p * 8, hipMemcpyHostToDevice, ctx->stream));
            const int rc = mg_pca_fit(ctx, Z, b, p, 0, Cz, mean_tmp.data(), sv_tmp.data(), hQ.data(), &sweeps, &jst);
            if (rc != MG_OK) return rc;
            MG_HIP_CHECK(hipMemcpyAsync(Q, hQ.data(), (size_t)b * p * 8, hipMemcpyHostToDevice, ctx->stream));
            q_ready = true;
            in_block = 0;
        }
        bool grow = false;
        for (;;) {
            int rc = fp_gemm(ctx, centred_dev, Q, nullptr, Y, 1, 0, 0, 0, n, b, p, p, 1, p, b);            // Y = Xc Q^T
            if (rc == MG_OK) rc = fp_gemm_ta(ctx, Y, centred_dev, Z, b, p, n, b, p, p);                      // Z = Y^T Xc
            if (rc != MG_OK) return rc;
            MG_HIP_CHECK(hipMemcpyAsync(hZ.data(), Z, (size_t)b * p * 8, hipMemcpyDeviceToHost, ctx->stream));
            MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            iters++, in_block++;
            double lam_max = 0.0;
            for (int64_t i = 0; i < b; i++) {
                const double *q = hQ.data() + (size_t)i * p, *z = hZ.data() + (size_t)i * p;
                double dot = 0.0, r2 = 0.0;
                for (int64_t e = 0; e < p; e++) dot = dot + q[e] * z[e];
                for (int64_t e = 0; e < p; e++) { const double d = z[e] - dot * q[e]; r2 = r2 + d * d; }
                lam[(size_t)i] = dot > 0.0 ? dot : 0.0;
                resid[(size_t)i] = std::sqrt(r2);
                lam_max = std::max(lam_max, lam[(size_t)i]);
            }
            // sklearn's count for a float n_components: searchsorted(cumsum(ratio), fraction, side = "right") + 1
            double cum = 0.0;
            int64_t below = 0;
            for (int64_t i = 0; i < b; i++) { cum = cum + lam[(size_t)i] / total; if (cum <= fraction) below++; }
            const bool captured = below < b;
            k = (int32_t)std::min<int64_t>(below + 1, b);
            const bool small_block = b < b_max && (!captured || k + FP_LEAD_SPARE > b);
            bool converged = captured && !small_block;
            for (int64_t i = 0; i < k && converged; i++) converged = resid[(size_t)i] <= tol * lam_max;
            if (converged) { st = 1; break; }
            if (iters >= cap) { st = 2; break; }
            if (b == b_max && b < m && !captured && in_block >= 8) {
                // (the quotients rise towards the eigenvalues: eight rounds in, a block of Jacobi's limit that still captures too little will not)
                mg_set_error("%s: more than %lld components are needed for %g of the variance", who, (long long)b_max, fraction);
                return MG_ERR_UNSUPPORTED;
            }
            if (small_block && in_block >= 2) { grow = true; break; }
            rc = mg_pca_fit(ctx, Z, b, p, 0, Cz, mean_tmp.data(), sv_tmp.data(), hQ.data(), &sweeps, &jst);
            if (rc != MG_OK) return rc;
            MG_HIP_CHECK(hipMemcpyAsync(Q, hQ.data(), (size_t)b * p * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        if (!grow) break;
        // the block doubles: its rows stay (as (Xc^T Xc) q_i, one more step), new start rows join them
        const int64_t b2 = std::min<int64_t>(b_max, 2 * b);
        try { hZ.resize((size_t)b2 * p); } catch (const std::bad_alloc &) { return MG_ERR_OUT_OF_MEMORY; }
        hQ.swap(hZ);
        k = (int32_t)b;      // rows kept
        b = b2;
        q_ready = false;
    }
    *k_out = k;          // (what a caller with too little room asks again with)
    MG_REQUIRE_AS(k <= k_cap, MG_ERR_INVALID_ARGUMENT, "%s: %d components kept, room for %d", who, k, k_cap);
    for (int32_t i = 0; i < k; i++) {
        singular_values[i] = std::sqrt(lam[(size_t)i]);
        ratios[i] = lam[(size_t)i] / total;
        memcpy(vt + (size_t)i * p, hQ.data() + (size_t)i * p, (size_t)p * 8);
    }
    *k_out = k, *iterations = iters, *status = st;
    return MG_OK;
}
