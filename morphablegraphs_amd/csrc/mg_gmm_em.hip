// Batched EM of full-covariance Gaussian mixtures: the fits of GMMTrainer's AIC sweep (reference construction/
// motion_primitive/gmm_trainer.py, sklearn GaussianMixture(covariance_type='full') per K) over one device points table.
//
// Semantics are sklearn 1.7's GaussianMixture with init_params='kmeans' and n_init=1, statement for statement, float64:
//   init      resp one-hot from the caller's labels; nk = resp.sum(0) + 10 eps, means = resp.T X / nk, covariances in the
//             two-pass form sum_r r (x - mu)(x - mu)^T / nk + reg_covar I, weights = nk / n, precision Cholesky L^-T;
//   iteration E-step (log N through the precision Cholesky, y = X P - mu P; logsumexp as scipy: the first maximum held out,
//             log1p(sum exp(a - max) / m) + log m + max); lower bound = mean log_prob_norm; M-step always applied,
//             weights = nk / sum nk; stop when |lb - lb_prev| < tol or after max_iter iterations;
//   after     one E-step with the final parameters: score = mean(score_samples(X)) and each row's label (argmax log_resp).
// A non-positive or non-finite Cholesky pivot ends that fit only (state ILL_DEFINED).
//
// Shape of the work: per iteration five launches over the unfinished fits -- E-step (workgroup = 256 rows of one fit, all
// its components), the sums r and r x (workgroup = one slot of rows of one component), the covariance sums (same grid; it
// finishes the means from the slots itself), Cholesky and precision Cholesky (one wave per component), and a per-fit state
// pass (lower bound, weights, convergence).  Every component has EM_NSLOT partial slots whatever n is; rows are split into
// slots by n alone and every sum runs in a fixed order, so a fit gives the same bits in any batch and on any device size.
// No float atomics, no grid barriers: each kernel combines what an earlier launch of the stream wrote.
#include "mg_construct.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#define EM_BLOCK 256        // rows per E-step workgroup
#define EM_NSLOT 16         // partial-sum slots per component
#define EM_TILE 32          // rows per covariance tile in LDS
#define EM_MAX_D 64
#define EM_MAX_K 64
#define EM_LDP (EM_MAX_D + 1)

enum { EM_RUN = 0, EM_CONVERGED = 1, EM_MAX_ITER = 2, EM_ILL_DEFINED = 3 };
enum { EM_STATE_INIT = 0, EM_STATE_ITER = 1, EM_STATE_SCORE = 2 };

struct em_args {
    const double *X;                // [n][d]
    int64_t n;
    int32_t d, dt, nblk, chunk, max_iter;
    double tol, reg, dl2p;          // dl2p = d * log(2 pi), from the host
    const int32_t *K, *co, *fit_of; // per fit: components, first component; per component: its fit
    const int32_t *fits, *comps;    // the launch's fits / components
    double *resp;                   // [C][n]: weighted log prob, then responsibilities
    double *nk, *w, *logw, *means, *cov, *prec, *cvec, *logdet;
    double *psum;                   // [C][EM_NSLOT][d + 1]: sum r x, sum r
    double *pcov;                   // [C][EM_NSLOT][dt]: upper triangle of sum (r (x - mu)) (x - mu)^T
    double *blk;                    // [F][nblk]: per E-step workgroup, the sum of log_prob_norm
    double *lb;                     // [F][max_iter]
    double *score;
    int32_t *state, *n_iter, *fail, *labels;   // labels [F][n]
};

// ---- initial responsibilities: one-hot from the labels -------------------------------------------------------------
__global__ __launch_bounds__(EM_BLOCK) void em_onehot_kernel(em_args a, const int32_t *lab_in) {
    const int f = a.fits[blockIdx.y];
    const int64_t row = (int64_t)blockIdx.x * EM_BLOCK + threadIdx.x;
    if (row >= a.n) return;
    const int K = a.K[f], c0 = a.co[f];
    const int L = lab_in[(size_t)f * a.n + row];
    for (int k = 0; k < K; k++) a.resp[(size_t)(c0 + k) * a.n + row] = k == L ? 1.0 : 0.0;
}

// ---- E-step: weighted log prob of every component, logsumexp, responsibilities; the block's sum of log_prob_norm --------
// final: the scoring pass after the loop (labels instead of responsibilities) for the fits that ended without failure.
template <int DP>
__global__ __launch_bounds__(EM_BLOCK) void em_estep_kernel(em_args a, int final) {
    __shared__ double P[DP * DP];
    __shared__ double cv[DP];
    __shared__ double red[EM_BLOCK];
    const int f = a.fits[blockIdx.y];
    const int st = a.state[f];
    if (final ? st == EM_ILL_DEFINED : st != EM_RUN) return;
    const int d = a.d, K = a.K[f], c0 = a.co[f], tid = threadIdx.x;
    const int64_t n = a.n, row = (int64_t)blockIdx.x * EM_BLOCK + tid;
    const bool have = row < n;
    double x[DP];
#pragma unroll
    for (int i = 0; i < DP; i++) x[i] = (have && i < d) ? a.X[row * d + i] : 0.0;
    for (int k = 0; k < K; k++) {
        const int c = c0 + k;
        __syncthreads();
        for (int e = tid; e < d * d; e += EM_BLOCK) P[(e / d) * DP + e % d] = a.prec[(size_t)c * d * d + e];
        if (tid < d) cv[tid] = a.cvec[(size_t)c * d + tid];
        __syncthreads();
        if (have) {
            double lp = 0.0;
#pragma unroll
            for (int j = 0; j < DP; j++) {
                if (j < d) {
                    double acc = 0.0;
#pragma unroll
                    for (int i = 0; i <= j; i++) acc = acc + x[i] * P[i * DP + j];
                    const double y = acc - cv[j];
                    lp = lp + y * y;
                }
            }
            a.resp[(size_t)c * n + row] = (-0.5 * (a.dl2p + lp) + a.logdet[c]) + a.logw[c];
        }
    }
    double lpn = 0.0;
    if (have) {
        double amax = -INFINITY;
        for (int k = 0; k < K; k++) amax = fmax(amax, a.resp[(size_t)(c0 + k) * n + row]);
        double s = 0.0, m = 0.0;
        for (int k = 0; k < K; k++) {
            const double v = a.resp[(size_t)(c0 + k) * n + row];
            if (v == amax) m += 1.0;
            else s += exp(v - amax);
        }
        if (s != 0.0) s = s / m;
        lpn = (log1p(s) + log(m)) + amax;
        if (final) {
            int best = 0;
            double bv = a.resp[(size_t)c0 * n + row] - lpn;
            for (int k = 1; k < K; k++) {
                const double v = a.resp[(size_t)(c0 + k) * n + row] - lpn;
                if (v > bv) { bv = v; best = k; }
            }
            a.labels[(size_t)f * n + row] = best;
        } else {
            for (int k = 0; k < K; k++) {
                double *p = a.resp + (size_t)(c0 + k) * n + row;
                *p = exp(*p - lpn);
            }
        }
    }
    const double s = mg_block_sum<EM_BLOCK>(lpn, red);
    if (tid == 0) a.blk[(size_t)f * a.nblk + blockIdx.x] = s;
}

// ---- M-step, part 1: per slot the sums of r and r x (one lane per column) -----------------------------------------------
__global__ __launch_bounds__(64) void em_msum_kernel(em_args a) {
    const int c = a.comps[blockIdx.y];
    if (a.state[a.fit_of[c]] != EM_RUN) return;
    const int d = a.d, t = threadIdx.x, s = blockIdx.x;
    const int64_t r0 = (int64_t)s * a.chunk, r1 = min(a.n, r0 + a.chunk);
    const double *resp = a.resp + (size_t)c * a.n;
    double acc = 0.0, accn = 0.0;
    const int col = t < d ? t : 0;
    for (int64_t r = r0; r < r1; r++) {
        const double rr = resp[r];
        acc = acc + rr * a.X[r * d + col];
        accn = accn + rr;
    }
    double *slot = a.psum + ((size_t)c * EM_NSLOT + s) * (d + 1);
    if (t < d) slot[t] = acc;
    if (t == 0) slot[d] = accn;
}

// ---- M-step, part 2: the means (from the slots, in slot order), then per slot the covariance sums about them --------------
__global__ __launch_bounds__(EM_BLOCK) void em_mcov_kernel(em_args a) {
    __shared__ double mu[EM_MAX_D + 1];
    __shared__ double A[EM_TILE][EM_MAX_D], B[EM_TILE][EM_MAX_D];
    const int c = a.comps[blockIdx.y];
    if (a.state[a.fit_of[c]] != EM_RUN) return;
    const int d = a.d, dt = a.dt, tid = threadIdx.x, s = blockIdx.x;
    if (tid <= d) {
        double v = 0.0;
        for (int q = 0; q < EM_NSLOT; q++) v += a.psum[((size_t)c * EM_NSLOT + q) * (d + 1) + tid];
        mu[tid] = tid == d ? v + 10.0 * DBL_EPSILON : v;
    }
    __syncthreads();
    const double nk = mu[d];
    __syncthreads();
    if (tid < d) mu[tid] = mu[tid] / nk;
    __syncthreads();
    if (s == 0) {
        if (tid < d) a.means[(size_t)c * d + tid] = mu[tid];
        if (tid == 0) a.nk[c] = nk;
    }
    // the entries this thread owns: e = tid + EM_BLOCK q of the row-major upper triangle
    constexpr int NE = (EM_MAX_D * (EM_MAX_D + 1) / 2 + EM_BLOCK - 1) / EM_BLOCK;
    int ei[NE], ej[NE];
    double acc[NE];
#pragma unroll
    for (int q = 0; q < NE; q++) {
        int e = tid + EM_BLOCK * q, i = 0;
        acc[q] = 0.0;
        ei[q] = ej[q] = -1;
        if (e < dt) {
            while (e >= d - i) { e -= d - i; i++; }
            ei[q] = i;
            ej[q] = i + e;
        }
    }
    const int64_t r0 = (int64_t)s * a.chunk, r1 = min(a.n, r0 + a.chunk);
    const double *resp = a.resp + (size_t)c * a.n;
    for (int64_t t0 = r0; t0 < r1; t0 += EM_TILE) {
        const int nt = (int)min((int64_t)EM_TILE, r1 - t0);
        for (int idx = tid; idx < nt * d; idx += EM_BLOCK) {
            const int r = idx / d, i = idx - r * d;
            const double diff = a.X[(t0 + r) * d + i] - mu[i];
            A[r][i] = resp[t0 + r] * diff;
            B[r][i] = diff;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NE; q++)
            if (ei[q] >= 0)
                for (int r = 0; r < nt; r++) acc[q] = acc[q] + A[r][ei[q]] * B[r][ej[q]];
        __syncthreads();
    }
    double *slot = a.pcov + ((size_t)c * EM_NSLOT + s) * dt;
#pragma unroll
    for (int q = 0; q < NE; q++)
        if (ei[q] >= 0) slot[tid + EM_BLOCK * q] = acc[q];
}

// ---- M-step, part 3: covariance, Cholesky, precision Cholesky, log det, mu P (one wave per component) -----------------
__global__ __launch_bounds__(64) void em_mchol_kernel(em_args a) {
    __shared__ double L[EM_MAX_D][EM_LDP], M[EM_MAX_D][EM_LDP];
    __shared__ int bad;
    const int c = a.comps[blockIdx.x];
    const int f = a.fit_of[c];
    if (a.state[f] != EM_RUN) return;
    const int d = a.d, dt = a.dt, t = threadIdx.x;
    const double nk = a.nk[c];
    if (t == 0) bad = 0;
    for (int e0 = t; e0 < dt; e0 += 64) {
        int e = e0, i = 0;
        while (e >= d - i) { e -= d - i; i++; }
        const int j = i + e;
        double v = 0.0;
        for (int q = 0; q < EM_NSLOT; q++) v += a.pcov[((size_t)c * EM_NSLOT + q) * dt + e0];
        v = v / nk;
        if (i == j) v = v + a.reg;
        M[i][j] = v;
        M[j][i] = v;
    }
    __syncthreads();
    double *cov = a.cov + (size_t)c * d * d;
    for (int e = t; e < d * d; e += 64) cov[e] = M[e / d][e % d];
    // lower Cholesky, column by column: pivot, then the column below it scaled by the pivot's reciprocal
    for (int j = 0; j < d; j++) {
        if (t == 0) {
            double s = M[j][j];
            for (int p = 0; p < j; p++) s = s - L[j][p] * L[j][p];
            if (!(s > 0.0) || !isfinite(s)) bad = 1;
            else L[j][j] = sqrt(s);
        }
        __syncthreads();
        if (bad) break;
        if (t > j && t < d) {
            double s = M[t][j];
            for (int p = 0; p < j; p++) s = s - L[t][p] * L[j][p];
            L[t][j] = s * (1.0 / L[j][j]);
        }
        __syncthreads();
    }
    if (bad) {
        if (t == 0) a.fail[f] = 1;
        return;
    }
    // L^-1 by forward substitution, lane col owns column col (into M)
    if (t < d) {
        const int col = t;
        M[col][col] = 1.0 / L[col][col];
        for (int i = col + 1; i < d; i++) {
            double s = 0.0;
            for (int p = col; p < i; p++) s = s + L[i][p] * M[p][col];
            M[i][col] = -s / L[i][i];
        }
    }
    __syncthreads();
    // precision Cholesky P = (L^-1)^T (upper); log det = sum log diag P; mu P
    double *prec = a.prec + (size_t)c * d * d;
    for (int e = t; e < d * d; e += 64) {
        const int i = e / d, j = e % d;
        prec[e] = i <= j ? M[j][i] : 0.0;
    }
    const double *mu = a.means + (size_t)c * d;
    if (t < d) {
        const int j = t;
        double s = 0.0;
        for (int i = 0; i <= j; i++) s = s + mu[i] * M[j][i];
        a.cvec[(size_t)c * d + j] = s;
    }
    if (t == 0) {
        double s = 0.0;
        for (int j = 0; j < d; j++) s = s + log(M[j][j]);
        a.logdet[c] = s;
    }
}

// ---- per fit: weights, lower bound, convergence; or the score -------------------------------------------------------
__global__ __launch_bounds__(64) void em_state_kernel(em_args a, int mode) {
    const int f = a.fits[blockIdx.x];
    if (threadIdx.x != 0) return;
    const int st = a.state[f];
    const int K = a.K[f], c0 = a.co[f];
    if (mode == EM_STATE_SCORE) {
        if (st == EM_ILL_DEFINED) return;
        double s = 0.0;
        for (int b = 0; b < a.nblk; b++) s += a.blk[(size_t)f * a.nblk + b];
        a.score[f] = s / (double)a.n;
        return;
    }
    if (st != EM_RUN) return;
    if (a.fail[f]) {
        a.state[f] = EM_ILL_DEFINED;
        return;
    }
    double tot = (double)a.n;
    if (mode == EM_STATE_ITER) {
        tot = 0.0;
        for (int k = 0; k < K; k++) tot += a.nk[c0 + k];
    }
    for (int k = 0; k < K; k++) {
        const double w = a.nk[c0 + k] / tot;
        a.w[c0 + k] = w;
        a.logw[c0 + k] = log(w);
    }
    if (mode == EM_STATE_INIT) return;
    double s = 0.0;
    for (int b = 0; b < a.nblk; b++) s += a.blk[(size_t)f * a.nblk + b];
    const double lb = s / (double)a.n;
    const int it = a.n_iter[f] + 1;
    a.lb[(size_t)f * a.max_iter + it - 1] = lb;
    const double prev = it > 1 ? a.lb[(size_t)f * a.max_iter + it - 2] : -INFINITY;
    a.n_iter[f] = it;
    if (fabs(lb - prev) < a.tol) a.state[f] = EM_CONVERGED;
    else if (it >= a.max_iter) a.state[f] = EM_MAX_ITER;
}

extern "C" int mg_gmm_em_fit(mg_context *ctx, const double *points_dev, int64_t n, int32_t dim, int32_t n_fits, const int32_t *n_comp,
                             const int32_t *labels_in, double tol, double reg_covar, int32_t max_iter, double *weights, double *means,
                             double *covariances, double *precisions_chol, double *lower_bounds, int32_t *n_iter, int32_t *status,
                             double *score, int32_t *labels_out) {
    const int BAD = MG_ERR_INVALID_ARGUMENT, UNS = MG_ERR_UNSUPPORTED;
    MG_REQUIRE_AS(ctx && points_dev, BAD, "mg_gmm_em_fit: NULL context or points");
    MG_REQUIRE_AS(dim >= 1 && dim <= EM_MAX_D, UNS, "mg_gmm_em_fit: dim = %d outside [1, %d]", dim, EM_MAX_D);
    MG_REQUIRE_AS(n_fits >= 0 && max_iter >= 1 && tol >= 0.0 && reg_covar >= 0.0, BAD,
                  "mg_gmm_em_fit: n_fits = %d, max_iter = %d, tol = %g, reg_covar = %g", n_fits, max_iter, tol, reg_covar);
    if (n_fits == 0) return MG_OK;
    MG_REQUIRE_AS(n_comp && labels_in && weights && means && covariances && precisions_chol && lower_bounds && n_iter && status && score && labels_out,
                  BAD, "mg_gmm_em_fit: NULL argument");
    MG_REQUIRE_AS(n >= 1 && n < ((int64_t)1 << 40), BAD, "mg_gmm_em_fit: n = %lld", (long long)n);
    std::vector<int32_t> co(n_fits + 1, 0);
    for (int32_t f = 0; f < n_fits; f++) {
        MG_REQUIRE_AS(n_comp[f] >= 1 && n_comp[f] <= EM_MAX_K, UNS, "mg_gmm_em_fit: fit %d has %d components, outside [1, %d]", f, n_comp[f], EM_MAX_K);
        MG_REQUIRE_AS(n_comp[f] <= n, BAD, "mg_gmm_em_fit: fit %d has %d components and %lld samples", f, n_comp[f], (long long)n);
        co[f + 1] = co[f] + n_comp[f];
    }
    for (int32_t f = 0; f < n_fits; f++)
        for (int64_t r = 0; r < n; r++)
            MG_REQUIRE_AS(labels_in[(size_t)f * n + r] >= 0 && labels_in[(size_t)f * n + r] < n_comp[f], BAD,
                          "mg_gmm_em_fit: fit %d, row %lld: label %d outside [0, %d)", f, (long long)r, labels_in[(size_t)f * n + r], n_comp[f]);
    const int32_t C = co[n_fits], d = dim, dt = d * (d + 1) / 2;
    const int64_t nblk = (n + EM_BLOCK - 1) / EM_BLOCK, chunk = (n + EM_NSLOT - 1) / EM_NSLOT;
    MG_REQUIRE_AS(nblk < ((int64_t)1 << 31) && chunk < ((int64_t)1 << 31), UNS, "mg_gmm_em_fit: n = %lld too large", (long long)n);
    std::vector<int32_t> fit_of(C);
    for (int32_t f = 0; f < n_fits; f++)
        for (int32_t k = 0; k < n_comp[f]; k++) fit_of[co[f] + k] = f;
    std::vector<int32_t> fits(n_fits), comps(C), state(n_fits, EM_RUN);
    // one device block for everything the call needs; declared after the host buffers its copies touch: it drains the stream first
    mg_workspace ws(ctx, "mg_gmm_em_fit");
    auto carve = [&](size_t bytes) { return ws.carve(bytes); };
    const size_t o_K = carve(n_fits * 4), o_co = carve(n_fits * 4), o_fitof = carve(C * 4), o_fits = carve(n_fits * 4), o_comps = carve(C * 4);
    const size_t o_lin = carve((size_t)n_fits * n * 4), o_lout = carve((size_t)n_fits * n * 4);
    const size_t o_resp = carve((size_t)C * n * 8);
    const size_t o_nk = carve(C * 8), o_w = carve(C * 8), o_logw = carve(C * 8), o_means = carve((size_t)C * d * 8);
    const size_t o_cov = carve((size_t)C * d * d * 8), o_prec = carve((size_t)C * d * d * 8), o_cvec = carve((size_t)C * d * 8), o_ld = carve(C * 8);
    const size_t o_psum = carve((size_t)C * EM_NSLOT * (d + 1) * 8), o_pcov = carve((size_t)C * EM_NSLOT * dt * 8);
    const size_t o_blk = carve((size_t)n_fits * nblk * 8), o_lb = carve((size_t)n_fits * max_iter * 8), o_score = carve(n_fits * 8);
    const size_t o_state = carve(n_fits * 4), o_iter = carve(n_fits * 4), o_fail = carve(n_fits * 4), o_end = ws.bytes;
    const int ra = ws.alloc();
    if (ra != MG_OK) return ra;
    char *const base = ws.base;
    hipStream_t st = ctx->stream;
    em_args a;
    a.X = points_dev;
    a.n = n; a.d = d; a.dt = dt; a.nblk = (int32_t)nblk; a.chunk = (int32_t)chunk; a.max_iter = max_iter;
    a.tol = tol; a.reg = reg_covar; a.dl2p = d * std::log(2.0 * M_PI);
    a.K = (const int32_t *)(base + o_K); a.co = (const int32_t *)(base + o_co); a.fit_of = (const int32_t *)(base + o_fitof);
    a.fits = (const int32_t *)(base + o_fits); a.comps = (const int32_t *)(base + o_comps);
    a.resp = (double *)(base + o_resp);
    a.nk = (double *)(base + o_nk); a.w = (double *)(base + o_w); a.logw = (double *)(base + o_logw); a.means = (double *)(base + o_means);
    a.cov = (double *)(base + o_cov); a.prec = (double *)(base + o_prec); a.cvec = (double *)(base + o_cvec); a.logdet = (double *)(base + o_ld);
    a.psum = (double *)(base + o_psum); a.pcov = (double *)(base + o_pcov);
    a.blk = (double *)(base + o_blk); a.lb = (double *)(base + o_lb); a.score = (double *)(base + o_score);
    a.state = (int32_t *)(base + o_state); a.n_iter = (int32_t *)(base + o_iter); a.fail = (int32_t *)(base + o_fail);
    a.labels = (int32_t *)(base + o_lout);
    for (int32_t f = 0; f < n_fits; f++) fits[f] = f;
    for (int32_t c = 0; c < C; c++) comps[c] = c;
    int32_t nf = n_fits, nc = C;
    void (*estep)(em_args, int) = d <= 8 ? em_estep_kernel<8> : d <= 16 ? em_estep_kernel<16> : d <= 32 ? em_estep_kernel<32> : em_estep_kernel<64>;
    int next_check = 1;
    auto mstep = [&]() {
        hipLaunchKernelGGL(em_msum_kernel, dim3(EM_NSLOT, nc), dim3(64), 0, st, a);
        hipLaunchKernelGGL(em_mcov_kernel, dim3(EM_NSLOT, nc), dim3(EM_BLOCK), 0, st, a);
        hipLaunchKernelGGL(em_mchol_kernel, dim3(nc), dim3(64), 0, st, a);
        return hipGetLastError();
    };
    MG_HIP_CHECK(hipMemcpyAsync(base + o_K, n_comp, n_fits * 4, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_co, co.data(), n_fits * 4, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_fitof, fit_of.data(), C * 4, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_fits, fits.data(), n_fits * 4, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_comps, comps.data(), C * 4, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_lin, labels_in, (size_t)n_fits * n * 4, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemsetAsync(base + o_lb, 0, o_end - o_lb, st));     // lower bounds, scores, states (EM_RUN), n_iter, fail flags
    hipLaunchKernelGGL(em_onehot_kernel, dim3((unsigned)nblk, nf), dim3(EM_BLOCK), 0, st, a, (const int32_t *)(base + o_lin));
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(mstep());
    hipLaunchKernelGGL(em_state_kernel, dim3(nf), dim3(64), 0, st, a, (int)EM_STATE_INIT);
    MG_HIP_CHECK(hipGetLastError());
    for (int it = 1; it <= max_iter && nf > 0; it++) {
        hipLaunchKernelGGL(estep, dim3((unsigned)nblk, nf), dim3(EM_BLOCK), 0, st, a, 0);
        MG_HIP_CHECK(hipGetLastError());
        MG_HIP_CHECK(mstep());
        hipLaunchKernelGGL(em_state_kernel, dim3(nf), dim3(64), 0, st, a, (int)EM_STATE_ITER);
        MG_HIP_CHECK(hipGetLastError());
        if (it == next_check && it < max_iter) {    // drop the finished fits from the launches
            next_check = it < 8 ? it * 2 : it + 8;
            MG_HIP_CHECK(hipMemcpyAsync(state.data(), a.state, n_fits * 4, hipMemcpyDeviceToHost, st));
            MG_HIP_CHECK(hipStreamSynchronize(st));
            nf = nc = 0;
            for (int32_t f = 0; f < n_fits; f++)
                if (state[f] == EM_RUN) {
                    fits[nf++] = f;
                    for (int32_t k = 0; k < n_comp[f]; k++) comps[nc++] = co[f] + k;
                }
            if (nf > 0) {
                MG_HIP_CHECK(hipMemcpyAsync(base + o_fits, fits.data(), nf * 4, hipMemcpyHostToDevice, st));
                MG_HIP_CHECK(hipMemcpyAsync(base + o_comps, comps.data(), nc * 4, hipMemcpyHostToDevice, st));
                MG_HIP_CHECK(hipStreamSynchronize(st));    // the host lists are rewritten at the next check
            }
        }
    }
    // the scoring pass over every fit that did not fail
    for (int32_t f = 0; f < n_fits; f++) fits[f] = f;
    MG_HIP_CHECK(hipMemcpyAsync(base + o_fits, fits.data(), n_fits * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(estep, dim3((unsigned)nblk, n_fits), dim3(EM_BLOCK), 0, st, a, 1);
    hipLaunchKernelGGL(em_state_kernel, dim3(n_fits), dim3(64), 0, st, a, (int)EM_STATE_SCORE);
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipMemcpyAsync(weights, a.w, C * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(means, a.means, (size_t)C * d * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(covariances, a.cov, (size_t)C * d * d * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(precisions_chol, a.prec, (size_t)C * d * d * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(lower_bounds, a.lb, (size_t)n_fits * max_iter * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(n_iter, a.n_iter, n_fits * 4, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(status, a.state, n_fits * 4, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(score, a.score, n_fits * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(labels_out, a.labels, (size_t)n_fits * n * 4, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipStreamSynchronize(st));
    return MG_OK;
}
