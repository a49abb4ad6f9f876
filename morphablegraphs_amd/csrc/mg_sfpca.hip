// Scaled functional PCA (reference construction/fpca/scaled_fpca.py: ScaledFunctionalPCA; objective_functions.py: sfpca_objective_func),
// float64: the joint-space error of the rank-k PCA reconstruction of feature-weighted spline coefficients, for a batch of weight vectors.
//
// With X (n, p) the coefficient rows, Xc = X - mean and Dw the diagonal of spread weights, sklearn's reconstruction of X Dw divided by Dw
// again is mean + U_k U_k^T Xc, U the left singular vectors of Xc Dw: the eigenvectors of Xc Dw^2 Xc^T = sum_g w_g^2 G_g, with
// G_g = Xc[:, group g] Xc[:, group g]^T the (n, n) Gram matrix of group g's columns (3 root channels, then one group of four per joint).
// The G_g do not depend on w.  Spline evaluation is linear too: with Bf the design rows at the sampled frames, Ybar = Bf mean and
// Yc = Bf Xc, the reconstructed frames of sample i are Ybar + U_k[i, :] . Z, Z = U_k^T Yc (k, F' D).  
//
//   mg_sfpca_create      once per data set: mean, Xc, the group Grams (sfpca_gram_kernel: one wave per upper-triangle 16 x 16 tile and
//                        group, v_mfma_f64_16x16x4_f64 over the group's columns, mirrored), Ybar, Yc and the originals' frames on
//                        fpca_gemm_kernel, the originals' joint positions by mg_joint_positions' kernel
//   mg_sfpca_errors      per chunk of weight vectors (batch index in grid.y / grid.z):
//     sfpca_combine_kernel   A_w = sum_g w_g^2 G_g, g ascending, one fma each
//     sfpca_jacobi_round_kernel   one-sided Jacobi on the rows of every A_w: mg_pca_fit's round-robin schedule, rotation test
//                        (tol = eps sqrt(n)) and cap; one rotation counter per matrix and sweep, read by the host once per sweep.  The
//                        rows end as lambda_i u_i^T: for a symmetric matrix the singular vectors are the eigenvectors
//     sfpca_norms_kernel, sfpca_gather_kernel   row norms, the stable descending order, the k leading rows made unit under the sign rule,
//                        their means taken out (ones is the centring's exact null vector)
//     fpca_gemm_kernel, sfpca_polish_kernel   one Newton-Schulz step on the kept rows: U_k U_k^T a projector to rounding level
//     fpca_gemm_kernel   Z = U_k^T Yc
//     sfpca_fused_kernel a workgroup owns (weight vector, 16 samples, one sampled frame): U_k[16, k] . Z[k, D at f] on f64 MFMAs (column
//                        tiles padded by a select on a clamped address), + Ybar into LDS, one (sample, joint) per thread walks its chain
//                        (the statements of mg_joint_positions_kernel), squared distance to the stored original, fixed tree over the
//                        workgroup, one partial per workgroup in its own slot
//     sfpca_finish_kernel    the partials of a weight vector added in slot order, divided by the count
// No float atomics, no grid barrier; every sum's order is fixed by the shapes alone, and no kernel's arithmetic for one weight vector
// depends on the others in its batch.
#include "mg_construct.h"
#include "mg_joint_plan.h"
#include "mg_score_device.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <new>
#include <vector>

#define SF_BLOCK 256
#define SF_MAX_N 1024
#define SF_MAX_BASIS 64
#define SF_MAX_JOINTS 64
#define SF_MAX_FRAMES 1024
#define SF_MAX_JOINTS_OUT 256
#define SF_MAX_SWEEPS 30
#define SF_CHUNK_DOUBLES ((int64_t)1 << 27)   // A_w of one chunk of weight vectors: at most 1 GiB

typedef double sf_f64x4 __attribute__((ext_vector_type(4)));

struct mg_sfpca {
    mg_context *ctx = nullptr;
    int32_t n = 0, nb = 0, D = 0, J = 0, G = 0, Fs = 0, JO = 0, RS = 0;
    int64_t p = 0;
    char *base = nullptr;
    double *d_xc = nullptr, *d_gram = nullptr, *d_ybar = nullptr, *d_yc = nullptr, *d_orig = nullptr, *d_rec = nullptr;
};

// ---- once per data set ------------------------------------------------------------------------------------------------------------
// mean[j] = (sum of the rows in row order) / n, xc = x - mean
__global__ __launch_bounds__(SF_BLOCK) void sfpca_centre_kernel(const double *__restrict__ x, int n, int64_t p, double *__restrict__ mean,
                                                                double *__restrict__ xc) {
    const int64_t j = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (j >= p) return;
    double s = 0.0;
    for (int i = 0; i < n; i++) s = s + x[(int64_t)i * p + j];
    const double mu = s / (double)n;
    mean[j] = mu;
    for (int i = 0; i < n; i++) xc[(int64_t)i * p + j] = x[(int64_t)i * p + j] - mu;
}

// G_g (n, n) for every group g = blockIdx.y: one wave per tile (ti <= tj) of the upper triangle; k runs over the group's columns
// (control point c, channel d0 + e: k = c * w + e), the tail and the edge rows by a select on a clamped address
__global__ __launch_bounds__(SF_BLOCK) void sfpca_gram_kernel(const double *__restrict__ xc, double *__restrict__ gram, int n, int nb, int D, int64_t p,
                                                              int tiles, int n_pairs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pair = blockIdx.x * (SF_BLOCK / 64) + wave;
    if (pair >= n_pairs) return;   // whole wave
    int ti = 0;
    while (pair >= tiles - ti) { pair -= tiles - ti; ti++; }
    const int tj = ti + pair;
    const int g = blockIdx.y, d0 = g < 3 ? g : 3 + 4 * (g - 3), w = g < 3 ? 1 : 4, K = nb * w;
    const int cl = lane & 15, q = lane >> 4;
    const int ra = ti * 16 + cl, rb = tj * 16 + cl;
    const bool aok = ra < n, bok = rb < n;
    const double *a = xc + (int64_t)(aok ? ra : n - 1) * p, *b = xc + (int64_t)(bok ? rb : n - 1) * p;
    sf_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + q;
        const bool kok = k < K;
        const int kc = kok ? k : K - 1, c = kc / w, col = c * D + d0 + (kc - c * w);
        const double av = a[col], bv = b[col];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((aok && kok) ? av : 0.0, (bok && kok) ? bv : 0.0, acc, 0, 0, 0);
    }
    double *out = gram + (int64_t)g * n * n;
    const int ocol = tj * 16 + cl;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int orow = ti * 16 + q + 4 * r;
        if (orow < n && ocol < n && ocol >= orow) {
            out[(int64_t)orow * n + ocol] = acc[r];
            out[(int64_t)ocol * n + orow] = acc[r];
        }
    }
}

// ---- per weight vector ------------------------------------------------------------------------------------------------------------
// A[b] = sum_g w[b][g]^2 G_g: g ascending, one fma per group
__global__ __launch_bounds__(SF_BLOCK) void sfpca_combine_kernel(const double *__restrict__ gram, const double *__restrict__ w, int G, int64_t nn,
                                                                 double *__restrict__ A) {
    const int64_t e = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (e >= nn) return;
    const double *wb = w + (int64_t)blockIdx.y * G;
    double acc = 0.0;
    for (int g = 0; g < G; g++) {
        const double wg = wb[g];
        acc = fma(wg * wg, gram[(int64_t)g * nn + e], acc);
    }
    A[(int64_t)blockIdx.y * nn + e] = acc;
}

// One round of the round-robin schedule for every matrix (blockIdx.y): workgroup k orthogonalises its pair of rows, as
// fpca_jacobi_round_kernel does for one matrix; counter: one per matrix
__global__ __launch_bounds__(SF_BLOCK) void sfpca_jacobi_round_kernel(double *__restrict__ W, int32_t m, int32_t mp, int32_t round, double tol,
                                                                      int32_t *__restrict__ counter) {
    __shared__ double red[3][SF_BLOCK];
    const int tid = threadIdx.x, k = blockIdx.x, n1 = mp - 1;
    const int p = k == 0 ? n1 : (round + k) % n1;
    const int q = k == 0 ? round : (round - k + n1) % n1;
    const int i = p < q ? p : q, j = p < q ? q : p;
    if (j >= m) return;   // the bye of an odd m (whole workgroup)
    double *base = W + (int64_t)blockIdx.y * m * m;
    double *wi = base + (int64_t)i * m, *wj = base + (int64_t)j * m;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int e = tid; e < m; e += SF_BLOCK) {
        const double x = wi[e], y = wj[e];
        a = a + x * x;
        b = b + y * y;
        c = c + x * y;
    }
    red[0][tid] = a, red[1][tid] = b, red[2][tid] = c;
    __syncthreads();
    for (int s = SF_BLOCK / 2; s > 0; s >>= 1) {
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
    for (int e = tid; e < m; e += SF_BLOCK) {
        const double x = wi[e], y = wj[e];
        wi[e] = cs * x - sn * y;
        wj[e] = sn * x + cs * y;
    }
    if (tid == 0) atomicAdd(counter + blockIdx.y, 1);
}

// row i = blockIdx.x of matrix blockIdx.y: its sum of squares (fixed tree) and whether its entry of largest magnitude (the first on ties) is negative
__global__ __launch_bounds__(SF_BLOCK) void sfpca_norms_kernel(const double *__restrict__ W, int32_t m, double *__restrict__ norm2, int32_t *__restrict__ negative) {
    __shared__ double red[SF_BLOCK];
    __shared__ double bestv[SF_BLOCK];
    __shared__ int32_t besti[SF_BLOCK];
    const int tid = threadIdx.x;
    const double *w = W + ((int64_t)blockIdx.y * m + blockIdx.x) * m;
    double s = 0.0, bv = -1.0;
    int bi = 0x7fffffff;
    for (int e = tid; e < m; e += SF_BLOCK) {
        const double x = w[e];
        s = s + x * x;
        if (fabs(x) > bv) { bv = fabs(x); bi = e; }
    }
    const double total = mg_block_sum<SF_BLOCK>(s, red);
    bestv[tid] = bv, besti[tid] = bi;
    __syncthreads();
    for (int st = SF_BLOCK / 2; st > 0; st >>= 1) {
        if (tid < st) {
            const double ov = bestv[tid + st];
            const int oi = besti[tid + st];
            if (ov > bestv[tid] || (ov == bestv[tid] && oi < besti[tid])) { bestv[tid] = ov; besti[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o = (int64_t)blockIdx.y * m + blockIdx.x;
        const int best = besti[0] < m ? besti[0] : 0;   // (a row of NaNs names no entry)
        norm2[o] = total;
        negative[o] = w[best] < 0.0 ? 1 : 0;
    }
}

// Ut[b][r] (r = blockIdx.x < k, b = blockIdx.y): the row of rank r in the stable descending order of the norms, divided by its norm
// (the eigenvalue), under the sign rule; zero where the eigenvalue is at most eps m times the largest
__global__ __launch_bounds__(SF_BLOCK) void sfpca_gather_kernel(const double *__restrict__ W, const double *__restrict__ norm2, const int32_t *__restrict__ negative,
                                                                int32_t m, int32_t k, double *__restrict__ Ut) {
    __shared__ double s2[SF_MAX_N];
    __shared__ double red[SF_BLOCK];
    __shared__ int32_t sel;
    const int tid = threadIdx.x, r = blockIdx.x;
    const double *n2 = norm2 + (int64_t)blockIdx.y * m;
    double mx = 0.0;
    if (tid == 0) sel = 0;   // (norms that are not numbers have no order: some row is taken, none outside the matrix)
    for (int i = tid; i < m; i += SF_BLOCK) {
        s2[i] = n2[i];
        mx = fmax(mx, n2[i]);
    }
    red[tid] = mx;
    __syncthreads();
    for (int st = SF_BLOCK / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] = fmax(red[tid], red[tid + st]);
        __syncthreads();
    }
    const double smax = sqrt(red[0]);
    for (int i = tid; i < m; i += SF_BLOCK) {
        const double v = s2[i];
        int rank = 0;
        for (int j = 0; j < m; j++) rank += (s2[j] > v || (s2[j] == v && j < i)) ? 1 : 0;
        if (rank == r) sel = i;
    }
    __syncthreads();
    const int src = sel;
    const double sig = sqrt(s2[src]);
    const bool null_row = !(sig > smax * DBL_EPSILON * (double)m);
    const bool neg = negative[(int64_t)blockIdx.y * m + src] != 0;
    const double *w = W + ((int64_t)blockIdx.y * m + src) * m;
    double *out = Ut + ((int64_t)blockIdx.y * k + r) * m;
    // The data are centred, so the vector of ones is an eigenvector of every A_w with eigenvalue 0 and every other eigenvector sums
    // to zero.  A row of a small eigenvalue holds that direction only to eps lambda_1 / lambda_i: its mean is taken out (fixed tree).
    double part = 0.0;
    for (int e = tid; e < m; e += SF_BLOCK) part = part + (null_row ? 0.0 : w[e] / sig);
    __syncthreads();   // (red is read above)
    const double mu = mg_block_sum<SF_BLOCK>(part, red) / (double)m;
    for (int e = tid; e < m; e += SF_BLOCK) {
        const double v = null_row ? 0.0 : w[e] / sig - mu;
        out[e] = neg ? -v : v;
    }
}

// Ut <- Ut - (Y - Ut) / 2 with Y = (Ut Ut^T) Ut: one Newton-Schulz step, as mg_pca_fit's polish of its companion
__global__ __launch_bounds__(SF_BLOCK) void sfpca_polish_kernel(double *__restrict__ Ut, const double *__restrict__ Y, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (e < count) Ut[e] = Ut[e] - 0.5 * (Y[e] - Ut[e]);
}

struct sf_fused_args {
    const double *Ut, *Z, *ybar, *orig, *rec;
    double *partial;
    int32_t n, k, D, Fs, JO, RS, PS, CT, tiles;
};

// KK > 0: that many k-steps, unrolled (mg_dispatch.h); 0: (k + 3) / 4 of them in a loop
template <int KK>
__global__ __launch_bounds__(SF_BLOCK) void sfpca_fused_kernel(const sf_fused_args a) {
    extern __shared__ __attribute__((aligned(16))) double sf_lds[];
    double *pose = sf_lds, *red = sf_lds + 16 * a.PS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, q = lane >> 4;
    const int f = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
    const int n = a.n, k = a.k, D = a.D;
    const int64_t FD = (int64_t)a.Fs * D;
    const int row = t * 16 + cl;
    const bool rok = row < n;
    const double *ut = a.Ut + (int64_t)b * k * n + (rok ? row : n - 1);
    const int steps = KK > 0 ? KK : (k + 3) / 4;
    for (int ct = wave; ct < a.CT; ct += SF_BLOCK / 64) {
        const int col = ct * 16 + cl;
        const bool cok = col < D;
        const double *z = a.Z + (int64_t)b * k * FD + (int64_t)f * D + (cok ? col : D - 1);
        sf_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        auto step = [&](int s) {
            const int kx = 4 * s + q;
            const bool kok = kx < k;
            const int kc = kok ? kx : k - 1;
            const double av = ut[(int64_t)kc * n], bv = z[(int64_t)kc * FD];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((rok && kok) ? av : 0.0, (cok && kok) ? bv : 0.0, acc, 0, 0, 0);
        };
        if constexpr (KK > 0) {
#pragma unroll
            for (int s = 0; s < KK; s++) step(s);
        } else {
            for (int s = 0; s < steps; s++) step(s);
        }
        if (cok) {
            const double yb = a.ybar[(int64_t)f * D + col];
#pragma unroll
            for (int r = 0; r < 4; r++) pose[(q + 4 * r) * a.PS + col] = acc[r] + yb;
        }
    }
    __syncthreads();
    double v = 0.0;
    for (int e = tid; e < 16 * a.JO; e += SF_BLOCK) {
        const int s = e / a.JO, j = e - s * a.JO, i = t * 16 + s;
        if (i >= n) continue;
        const double *fr = pose + s * a.PS, *rec = a.rec + (int64_t)j * a.RS;
        const int m = (int)rec[0];
        double p[3] = {fr[0], fr[1], fr[2]}, o[4] = {1.0, 0.0, 0.0, 0.0};
        for (int l = 0; l < m; l++) {
            const int ch = (int)rec[1 + 4 * l];
            if (ch >= 0) mg_quat_accumulate(o, fr[ch], fr[ch + 1], fr[ch + 2], fr[ch + 3]);
            mg_fk_link(o, rec[2 + 4 * l], rec[3 + 4 * l], rec[4 + 4 * l], p);
        }
        const double *g = a.orig + (((int64_t)i * a.Fs + f) * a.JO + j) * 3;
        const double dx = p[0] - g[0], dy = p[1] - g[1], dz = p[2] - g[2];
        v = v + (dx * dx + dy * dy + dz * dz);
    }
    const double total = mg_block_sum<SF_BLOCK>(v, red);
    if (tid == 0) a.partial[((int64_t)b * a.tiles + t) * a.Fs + f] = total;
}

// errors[b] = (the partials of b in slot order) / count
__global__ __launch_bounds__(64) void sfpca_finish_kernel(const double *__restrict__ partial, int32_t mc, int64_t slots, double count, double *__restrict__ errors) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= mc) return;
    const double *p = partial + (int64_t)b * slots;
    double s = 0.0;
    for (int64_t e = 0; e < slots; e++) s = s + p[e];
    errors[b] = s / count;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static bool sf_all_finite(const double *v, size_t count) {
    for (size_t e = 0; e < count; e++)
        if (!std::isfinite(v[e])) return false;
    return true;
}

extern "C" void mg_sfpca_destroy(mg_sfpca *h) {
    if (!h) return;
    if (h->base) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        (void)hipFree(h->base);
        (void)hipGetLastError();
    }
    delete h;
}

extern "C" int mg_sfpca_create(mg_context *ctx, const double *coeffs_dev, int32_t n, int32_t n_basis, int32_t n_dims, const mg_skeleton_desc *sk,
                               const int32_t *joints, int32_t n_joints_out, const double *design, int32_t n_sampled_frames, mg_sfpca **handle) {
    const char *who = "mg_sfpca_create";
    MG_REQUIRE(ctx && coeffs_dev && sk && joints && design && handle, "%s: NULL argument", who);
    *handle = nullptr;
    MG_REQUIRE(n >= 1 && n_basis >= 1 && n_dims >= 3 && (n_dims - 3) % 4 == 0 && n_joints_out >= 1 && n_sampled_frames >= 1,
               "%s: n = %d, n_basis = %d, n_dims = %d (3 + 4 J), %d joints, %d sampled frames", who, n, n_basis, n_dims, n_joints_out, n_sampled_frames);
    const int J = (n_dims - 3) / 4;
    MG_REQUIRE_AS(n >= 2 && n <= SF_MAX_N && n_basis <= SF_MAX_BASIS && J <= SF_MAX_JOINTS && n_sampled_frames <= SF_MAX_FRAMES && n_joints_out <= SF_MAX_JOINTS_OUT,
                  MG_ERR_UNSUPPORTED, "%s: n = %d (2 .. %d), n_basis = %d (at most %d), J = %d (at most %d), %d sampled frames (at most %d), %d joints (at most %d)", who,
                  n, SF_MAX_N, n_basis, SF_MAX_BASIS, J, SF_MAX_JOINTS, n_sampled_frames, SF_MAX_FRAMES, n_joints_out, SF_MAX_JOINTS_OUT);
    MG_REQUIRE(mg_skeleton_complete(sk), "%s: incomplete skeleton", who);
    mg_joint_plan plan;
    const mg_plan_failure f = plan.build(sk, joints, n_joints_out, n_dims, true);
    MG_REQUIRE(!f.of_skeleton(), "%s: joint %d%s", who, f.joint, mg_chain_why(f.kind));
    MG_REQUIRE_AS(f.kind != MG_PLAN_TOO_LONG, MG_ERR_UNSUPPORTED, "%s: chain of %d joints exceeds %d", who, f.length, MG_MAX_CHAIN);
    MG_REQUIRE(f.kind != MG_PLAN_CHANNEL_OUTSIDE, "%s: quaternion channel %d outside n_dims = %d", who, f.channel, n_dims);
    const int Fs = n_sampled_frames, JO = n_joints_out, D = n_dims, nb = n_basis, G = 3 + J;
    const int64_t p = (int64_t)nb * D, FD = (int64_t)Fs * D, nn = (int64_t)n * n;
    MG_REQUIRE(sf_all_finite(design, (size_t)Fs * nb), "%s: the design matrix holds non-finite values", who);
    std::vector<double> rec, table, host;
    const int RS = plan.records(1, 0, rec);                    // the fused kernel's: as long as the longest chain
    plan.records(1, 1 + 4 * MG_MAX_CHAIN, table);              // mg_joint_positions_kernel's
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    // the coefficients' host copy: non-finite values are refused before anything is launched
    try { host.resize((size_t)n * p); } catch (const std::bad_alloc &) {
        mg_set_error("%s: cannot allocate the host copy of a %d x %lld matrix", who, n, (long long)p);
        return MG_ERR_OUT_OF_MEMORY;
    }
    MG_HIP_CHECK(hipMemcpyAsync(host.data(), coeffs_dev, (size_t)n * p * 8, hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MG_REQUIRE(sf_all_finite(host.data(), host.size()), "%s: the coefficients hold non-finite values", who);
    std::vector<double>().swap(host);

    mg_sfpca *h = new (std::nothrow) mg_sfpca;
    MG_REQUIRE_AS(h, MG_ERR_OUT_OF_MEMORY, "%s: out of memory", who);
    h->ctx = ctx; h->n = n; h->nb = nb; h->D = D; h->J = J; h->G = G; h->Fs = Fs; h->JO = JO; h->RS = RS; h->p = p;
    auto al = [](size_t b) { return mg_workspace::align(b); };
    const size_t b_xc = al((size_t)n * p * 8), b_gram = al((size_t)G * nn * 8), b_ybar = al((size_t)FD * 8), b_yc = al((size_t)n * FD * 8),
                 b_orig = al((size_t)n * Fs * JO * 3 * 8), b_rec = al(rec.size() * 8);
    const size_t total = b_xc + b_gram + b_ybar + b_yc + b_orig + b_rec;
    if (hipMalloc(&h->base, total) != hipSuccess) {
        (void)hipGetLastError();
        h->base = nullptr;
        delete h;
        mg_set_error("%s: cannot allocate %zu bytes of device memory", who, total);
        return MG_ERR_OUT_OF_MEMORY;
    }
    char *at = h->base;
    h->d_xc = (double *)at; at += b_xc;
    h->d_gram = (double *)at; at += b_gram;
    h->d_ybar = (double *)at; at += b_ybar;
    h->d_yc = (double *)at; at += b_yc;
    h->d_orig = (double *)at; at += b_orig;
    h->d_rec = (double *)at;
    auto run = [&]() -> int {
        mg_workspace ws(ctx, who);     // what only this call needs: the mean, the design rows, the originals' frames, the long chain records
        const mg_staged s_design = ws.in(design, (size_t)Fs * nb * 8), s_table = ws.in(table.data(), table.size() * 8), s_rec = ws.in(rec.data(), rec.size() * 8);
        const mg_staged s_mean = ws.room((size_t)p * 8), s_frames = ws.room((size_t)n * FD * 8);
        int rc = ws.upload();
        if (rc != MG_OK) return rc;
        const double *d_design = s_design.dev<double>();
        double *d_mean = s_mean.dev<double>(), *d_frames = s_frames.dev<double>();
        MG_HIP_CHECK(hipMemcpyAsync(h->d_rec, s_rec.dev<double>(), rec.size() * 8, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(sfpca_centre_kernel, dim3((unsigned)((p + SF_BLOCK - 1) / SF_BLOCK)), dim3(SF_BLOCK), 0, ctx->stream, coeffs_dev, n, p, d_mean, h->d_xc);
        const int tiles = (n + 15) / 16, n_pairs = tiles * (tiles + 1) / 2;
        hipLaunchKernelGGL(sfpca_gram_kernel, dim3((unsigned)((n_pairs + SF_BLOCK / 64 - 1) / (SF_BLOCK / 64)), (unsigned)G), dim3(SF_BLOCK), 0, ctx->stream,
                           (const double *)h->d_xc, h->d_gram, n, nb, D, p, tiles, n_pairs);
        MG_HIP_CHECK(hipGetLastError());
        // Ybar = Bf mean; Yc[i] = Bf Xc[i]; the originals' frames Bf X[i]: control points as (n_basis, D) matrices
        rc = mg_fpca_gemm(ctx, d_design, d_mean, nullptr, h->d_ybar, 1, 0, 0, 0, Fs, D, nb, nb, D, 1, D);
        if (rc == MG_OK) rc = mg_fpca_gemm(ctx, d_design, h->d_xc, nullptr, h->d_yc, n, 0, p, FD, Fs, D, nb, nb, D, 1, D);
        if (rc == MG_OK) rc = mg_fpca_gemm(ctx, d_design, coeffs_dev, nullptr, d_frames, n, 0, p, FD, Fs, D, nb, nb, D, 1, D);
        if (rc == MG_OK) rc = mg_launch_joint_positions(ctx, d_frames, s_table.dev<double>(), (int64_t)n * Fs, D, JO, h->d_orig);
        if (rc != MG_OK) return rc;
        MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MG_OK;
    };
    const int rc = run();
    if (rc != MG_OK) {
        mg_sfpca_destroy(h);
        return rc;
    }
    *handle = h;
    return MG_OK;
}

static int sf_check_weights(const char *who, const mg_sfpca *h, const double *weights, int32_t m, int32_t n_weights, int32_t npc) {
    MG_REQUIRE(n_weights == h->G, "%s: weight vectors of %d entries, the data has 3 + %d", who, n_weights, h->J);
    MG_REQUIRE(npc >= 1 && npc <= h->n - 1, "%s: %d components of %d samples (1 .. %d)", who, npc, h->n, h->n - 1);
    for (int64_t e = 0; e < (int64_t)m * n_weights; e++)
        MG_REQUIRE(weights[e] > 0.0 && std::isfinite(weights[e]), "%s: weight %lld of vector %lld is %g (positive and finite)", who, (long long)(e % n_weights),
                   (long long)(e / n_weights), weights[e]);
    return MG_OK;
}

// The leading k eigenvectors of sum_g w_g^2 G_g for the mc weight vectors at d_w, as rows: Ut (mc, k, n).  A, norm2, negative, counters:
// the call's regions (A: mc n n doubles; polish: mc k (k + n) doubles for the polish's two products); statuses (host, mc).  Synchronises
// once per sweep.
static int sf_eigenvectors(const mg_sfpca *h, const double *d_w, int32_t mc, int32_t k, double *A, double *norm2, int32_t *negative, int32_t *counters, double *Ut,
                           double *polish, std::vector<int32_t> &rotations, int32_t *statuses) {
    mg_context *ctx = h->ctx;
    const int32_t n = h->n, mp = n + (n & 1);
    const int64_t nn = (int64_t)n * n;
    hipLaunchKernelGGL(sfpca_combine_kernel, dim3((unsigned)((nn + SF_BLOCK - 1) / SF_BLOCK), (unsigned)mc), dim3(SF_BLOCK), 0, ctx->stream,
                       (const double *)h->d_gram, d_w, h->G, nn, A);
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipMemsetAsync(counters, 0, (size_t)SF_MAX_SWEEPS * mc * 4, ctx->stream));
    const double tol = DBL_EPSILON * std::sqrt((double)n);
    for (int32_t b = 0; b < mc; b++) statuses[b] = 2;
    rotations.resize((size_t)mc);
    for (int32_t sweep = 0; sweep < SF_MAX_SWEEPS; sweep++) {
        for (int32_t r = 0; r < mp - 1; r++)
            hipLaunchKernelGGL(sfpca_jacobi_round_kernel, dim3((unsigned)(mp / 2), (unsigned)mc), dim3(SF_BLOCK), 0, ctx->stream, A, n, mp, r, tol,
                               counters + (int64_t)sweep * mc);
        MG_HIP_CHECK(hipGetLastError());
        MG_HIP_CHECK(hipMemcpyAsync(rotations.data(), counters + (int64_t)sweep * mc, (size_t)mc * 4, hipMemcpyDeviceToHost, ctx->stream));
        MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        bool all = true;
        for (int32_t b = 0; b < mc; b++) {
            if (rotations[(size_t)b] == 0) statuses[b] = 1;   // (a matrix at rest stays at rest: later sweeps rotate nothing in it)
            all = all && statuses[b] == 1;
        }
        if (all) break;
    }
    hipLaunchKernelGGL(sfpca_norms_kernel, dim3((unsigned)n, (unsigned)mc), dim3(SF_BLOCK), 0, ctx->stream, (const double *)A, n, norm2, negative);
    hipLaunchKernelGGL(sfpca_gather_kernel, dim3((unsigned)k, (unsigned)mc), dim3(SF_BLOCK), 0, ctx->stream, (const double *)A, (const double *)norm2,
                       (const int32_t *)negative, n, k, Ut);
    MG_HIP_CHECK(hipGetLastError());
    // the kept rows are orthonormal as far as the last sweep's test saw them (and the null vector has just been taken out of them): one
    // Newton-Schulz step brings Ut Ut^T back to rounding level, so that U_k U_k^T is a projector to rounding level as well
    double *T = polish, *Y = polish + (int64_t)mc * k * k;    // (mc, k, k), (mc, k, n)
    int rc = mg_fpca_gemm(h->ctx, Ut, Ut, nullptr, T, mc, (int64_t)k * n, (int64_t)k * n, (int64_t)k * k, k, k, n, n, 1, n, k);               // T = Ut Ut^T
    if (rc == MG_OK) rc = mg_fpca_gemm(h->ctx, T, Ut, nullptr, Y, mc, (int64_t)k * k, (int64_t)k * n, (int64_t)k * n, k, n, k, k, n, 1, n);   // Y = T Ut
    if (rc != MG_OK) return rc;
    const int64_t count = (int64_t)mc * k * n;
    hipLaunchKernelGGL(sfpca_polish_kernel, dim3((unsigned)((count + SF_BLOCK - 1) / SF_BLOCK)), dim3(SF_BLOCK), 0, ctx->stream, Ut, (const double *)Y, count);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

// weight vectors per chunk: A_w of a chunk within SF_CHUNK_DOUBLES, the batch index within a grid's y and z
static int32_t sf_chunk(const mg_sfpca *h, int32_t m) {
    const int64_t nn = (int64_t)h->n * h->n;
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(m, 65535), SF_CHUNK_DOUBLES / nn));
}

extern "C" int mg_sfpca_errors(mg_sfpca *h, const double *weights, int32_t m, int32_t n_weights, int32_t npc, double *errors, int32_t *statuses) {
    const char *who = "mg_sfpca_errors";
    MG_REQUIRE(h && weights && errors && statuses && m >= 0, "%s: NULL argument or m = %d", who, m);
    int rc = sf_check_weights(who, h, weights, m, n_weights, npc);
    if (rc != MG_OK || m == 0) return rc;
    mg_context *ctx = h->ctx;
    const int32_t n = h->n, k = npc, D = h->D, Fs = h->Fs, tiles = (n + 15) / 16;
    const int64_t nn = (int64_t)n * n, FD = (int64_t)Fs * D, slots = (int64_t)tiles * Fs;
    const int32_t chunk = sf_chunk(h, m);
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_workspace ws(ctx, who);
    const mg_staged s_w = ws.in(weights, (size_t)m * n_weights * 8), s_err = ws.out(errors, (size_t)m * 8);
    const mg_staged s_A = ws.room((size_t)chunk * nn * 8), s_n2 = ws.room((size_t)chunk * n * 8), s_neg = ws.room((size_t)chunk * n * 4),
                    s_cnt = ws.room((size_t)SF_MAX_SWEEPS * chunk * 4), s_ut = ws.room((size_t)chunk * k * n * 8), s_z = ws.room((size_t)chunk * k * FD * 8),
                    s_part = ws.room((size_t)chunk * slots * 8), s_pol = ws.room((size_t)chunk * k * ((size_t)k + n) * 8);
    if ((rc = ws.upload()) != MG_OK) return rc;
    sf_fused_args a;
    a.ybar = h->d_ybar, a.orig = h->d_orig, a.rec = h->d_rec;
    a.n = n, a.k = k, a.D = D, a.Fs = Fs, a.JO = h->JO, a.RS = h->RS, a.PS = D | 1, a.CT = (D + 15) / 16, a.tiles = tiles;
    const size_t lds = (size_t)(16 * a.PS + SF_BLOCK) * 8;
    const int steps = (k + 3) / 4, kk = steps + (steps & 1);
    std::vector<int32_t> rotations;
    for (int32_t b0 = 0; b0 < m; b0 += chunk) {
        const int32_t mc = std::min(chunk, m - b0);
        double *Ut = s_ut.dev<double>(), *Z = s_z.dev<double>(), *partial = s_part.dev<double>();
        rc = sf_eigenvectors(h, s_w.dev<double>() + (int64_t)b0 * n_weights, mc, k, s_A.dev<double>(), s_n2.dev<double>(), s_neg.dev<int32_t>(),
                             s_cnt.dev<int32_t>(), Ut, s_pol.dev<double>(), rotations, statuses + b0);
        if (rc != MG_OK) return rc;
        // Z[b] (k, F' D) = Ut[b] (k, n) . Yc (n, F' D)
        if ((rc = mg_fpca_gemm(ctx, Ut, h->d_yc, nullptr, Z, mc, (int64_t)k * n, 0, (int64_t)k * FD, k, FD, n, n, FD, 1, FD)) != MG_OK) return rc;
        a.Ut = Ut, a.Z = Z, a.partial = partial;
        const dim3 grid((unsigned)Fs, (unsigned)tiles, (unsigned)mc);
        const int launched = mg_dispatch_kk(kk, 0, [&](auto KK) {
            hipLaunchKernelGGL(sfpca_fused_kernel<decltype(KK)::value>, grid, dim3(SF_BLOCK), lds, ctx->stream, a);
            return 1;
        });
        if (!launched) hipLaunchKernelGGL(sfpca_fused_kernel<0>, grid, dim3(SF_BLOCK), lds, ctx->stream, a);
        hipLaunchKernelGGL(sfpca_finish_kernel, dim3((unsigned)((mc + 63) / 64)), dim3(64), 0, ctx->stream, (const double *)partial, mc, slots,
                           (double)n * (double)Fs * (double)h->JO, s_err.dev<double>() + b0);
        MG_HIP_CHECK(hipGetLastError());
    }
    return ws.download();
}

extern "C" int mg_sfpca_projector(mg_sfpca *h, const double *weights, int32_t n_weights, int32_t npc, double *u_k, int32_t *status) {
    const char *who = "mg_sfpca_projector";
    MG_REQUIRE(h && weights && u_k && status, "%s: NULL argument", who);
    int rc = sf_check_weights(who, h, weights, 1, n_weights, npc);
    if (rc != MG_OK) return rc;
    mg_context *ctx = h->ctx;
    const int32_t n = h->n, k = npc;
    std::vector<double> ut;
    try { ut.resize((size_t)k * n); } catch (const std::bad_alloc &) { return MG_ERR_OUT_OF_MEMORY; }
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_workspace ws(ctx, who);
    const mg_staged s_w = ws.in(weights, (size_t)n_weights * 8), s_ut = ws.out(ut.data(), (size_t)k * n * 8);
    const mg_staged s_A = ws.room((size_t)n * n * 8), s_n2 = ws.room((size_t)n * 8), s_neg = ws.room((size_t)n * 4), s_cnt = ws.room((size_t)SF_MAX_SWEEPS * 4),
                    s_pol = ws.room((size_t)k * ((size_t)k + n) * 8);
    if ((rc = ws.upload()) != MG_OK) return rc;
    std::vector<int32_t> rotations;
    rc = sf_eigenvectors(h, s_w.dev<double>(), 1, k, s_A.dev<double>(), s_n2.dev<double>(), s_neg.dev<int32_t>(), s_cnt.dev<int32_t>(), s_ut.dev<double>(),
                         s_pol.dev<double>(), rotations, status);
    if (rc != MG_OK || (rc = ws.download()) != MG_OK) return rc;
    for (int32_t i = 0; i < n; i++)
        for (int32_t r = 0; r < k; r++) u_k[(size_t)i * k + r] = ut[(size_t)r * n + i];
    return MG_OK;
}
