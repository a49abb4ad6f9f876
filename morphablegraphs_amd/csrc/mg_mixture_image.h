// The image of a feature mixture (mg_feature_mixture, include/mg_hip.h) and the statements that score a target against it, as plain
// code: standard headers, the C ABI and mg_hostdefs.h only, no HIP call, so that a stand-alone program compiles this file without the
// library.  mg_mixture_scores.hip uploads the image as it stands; its kernel and its host twin run the statements below.  Compiled
// with -ffp-contract=off like the rest of the host code: every fma is spelled out.
//
// The image, float64, one block of mg_mix_stride(dim) doubles per component:
//   [0, tri)          the upper triangle of P = inv(chol_lower(C))^T by columns: P[i][j], i <= j, at j (j + 1) / 2 + i, so that the
//                     entries one y_j reads are consecutive
//   [tri, tri + dim)  m = mu . P
//   [tri + dim]       c = (-0.5 dim log(2 pi) + sum_j log P[j][j]) + log w
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "mg_hostdefs.h"

#if defined(__HIPCC__)
#define MG_MIX_HD __host__ __device__ __forceinline__
#else
#define MG_MIX_HD inline
#endif

#define MG_MIX_LOG_2PI 1.8378770664093453      // log(2 pi) to the nearest double, written out so that every build and the NumPy statement agree
#define MG_MIX_ILL_DEFINED                                                                                                               \
    "Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by singleton " \
    "or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data."

MG_MIX_HD int mg_mix_tri(int dim) { return dim * (dim + 1) / 2; }
MG_MIX_HD int mg_mix_stride(int dim) { return mg_mix_tri(dim) + dim + 1; }

struct mg_mixture_image {
    int32_t K = 0, dim = 0;
    double threshold = 0.0;
    std::vector<double> blocks;          // [K][mg_mix_stride(dim)]
};

// wlp_k of one target: comp: the component's block, x(i): the target's coordinate i.  Every operation rounded on its own:
// y_j = (x_0 P[0][j], then fma(x_i, P[i][j], .), i ascending) - m_j; q = y_0 y_0, then fma(y_j, y_j, .); fma(-0.5, q, c)
template <class X>
MG_MIX_HD double mg_mix_wlp(const double *comp, int dim, X x) {
#pragma clang fp contract(off)
    const double *m = comp + mg_mix_tri(dim);
    double q = 0.0;
    for (int j = 0; j < dim; j++) {
        const double *col = comp + j * (j + 1) / 2;
        double acc = x(0) * col[0];
        for (int i = 1; i <= j; i++) acc = fma(x(i), col[i], acc);
        const double y = acc - m[j];
        q = j == 0 ? y * y : fma(y, y, q);
    }
    return fma(-0.5, q, m[dim]);
}

// ... the same statement with the loops unrolled to DMAX >= dim, for a target whose coordinates live in registers
template <int DMAX, class X>
MG_MIX_HD double mg_mix_wlp_unrolled(const double *comp, int dim, X x) {
#pragma clang fp contract(off)
    const double *m = comp + mg_mix_tri(dim);
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < DMAX; j++) {
        if (j < dim) {
            const double *col = comp + j * (j + 1) / 2;
            double acc = x(0) * col[0];
#pragma unroll
            for (int i = 1; i <= j; i++) acc = fma(x(i), col[i], acc);
            const double y = acc - m[j];
            q = j == 0 ? y * y : fma(y, y, q);
        }
    }
    return fma(-0.5, q, m[dim]);
}

// logp of one target from its wlp(k), k = 0 .. K - 1: max + log(exp(wlp_0 - max) + exp(wlp_1 - max) + ..); -inf where all are -inf
template <class W>
MG_MIX_HD double mg_mix_logp(int K, W wlp) {
#pragma clang fp contract(off)
    double mx = wlp(0);
    for (int k = 1; k < K; k++) {
        const double w = wlp(k);
        if (w > mx) mx = w;
    }
    if (mx == -INFINITY) return -INFINITY;
    double s = exp(wlp(0) - mx);
    for (int k = 1; k < K; k++) s = s + exp(wlp(k) - mx);
    return mx + log(s);
}

// the reference's `if score < threshold: False else: True`
MG_MIX_HD int32_t mg_mix_reachable(double logp, double threshold) { return logp < threshold ? 0 : 1; }

// The argument checks of mg_feature_mixture_create and the whole image; nothing is allocated before this returns MG_OK.
inline int mg_mixture_image_build(const char *who, int32_t K, int32_t dim, const double *weights, const double *means, const double *covars, double threshold,
                                  mg_mixture_image &img) {
    MG_REQUIRE(weights && means && covars, "%s: NULL weights, means or covars", who);
    MG_REQUIRE_AS(dim >= 1 && dim <= MG_FEATURE_MIXTURE_MAX_DIM, MG_ERR_UNSUPPORTED, "%s: %d dimensions (1 .. %d supported)", who, dim, MG_FEATURE_MIXTURE_MAX_DIM);
    MG_REQUIRE_AS(K >= 1 && K <= MG_FEATURE_MIXTURE_MAX_COMPONENTS, MG_ERR_UNSUPPORTED, "%s: %d components (1 .. %d supported)", who, K,
                  MG_FEATURE_MIXTURE_MAX_COMPONENTS);
    MG_REQUIRE(!std::isnan(threshold), "%s: the threshold is NaN", who);
    for (int k = 0; k < K; k++) {
        MG_REQUIRE(std::isfinite(weights[k]) && weights[k] >= 0.0, "%s: weight %d is %g", who, k, weights[k]);
        for (int i = 0; i < dim; i++) MG_REQUIRE(std::isfinite(means[(size_t)k * dim + i]), "%s: mean %d of component %d is not finite", who, i, k);
    }
    const int tri = mg_mix_tri(dim), stride = mg_mix_stride(dim);
    img.K = K; img.dim = dim; img.threshold = threshold;
    img.blocks.assign((size_t)K * stride, 0.0);
    std::vector<double> Lo((size_t)dim * dim), X((size_t)dim * dim);
    for (int k = 0; k < K; k++) {
        const double *C = covars + (size_t)k * dim * dim, *mu = means + (size_t)k * dim;
        double *P = img.blocks.data() + (size_t)k * stride, *m = P + tri;
        // chol_lower(C), row by row, from C's lower triangle
        for (int i = 0; i < dim; i++)
            for (int j = 0; j <= i; j++) {
                double s = C[(size_t)i * dim + j];
                for (int p = 0; p < j; p++) s = s - Lo[(size_t)i * dim + p] * Lo[(size_t)j * dim + p];
                if (i == j) {
                    MG_REQUIRE(std::isfinite(s) && s > 0.0, "%s: component %d: %s", who, k, MG_MIX_ILL_DEFINED);
                    Lo[(size_t)i * dim + i] = sqrt(s);
                } else {
                    Lo[(size_t)i * dim + j] = s / Lo[(size_t)j * dim + j];
                }
            }
        // X = inv(chol) by forward substitution, column by column; P[i][j] = X[j][i]
        for (int c = 0; c < dim; c++)
            for (int r = c; r < dim; r++) {
                double s = r == c ? 1.0 : 0.0;
                for (int p = c; p < r; p++) s = s - Lo[(size_t)r * dim + p] * X[(size_t)p * dim + c];
                X[(size_t)r * dim + c] = s / Lo[(size_t)r * dim + r];
            }
        double logdet = 0.0;
        for (int j = 0; j < dim; j++) {
            double *col = P + j * (j + 1) / 2;
            for (int i = 0; i <= j; i++) col[i] = X[(size_t)j * dim + i];
            double acc = mu[0] * col[0];
            for (int i = 1; i <= j; i++) acc = fma(mu[i], col[i], acc);
            m[j] = acc;
            MG_REQUIRE(std::isfinite(col[j]) && col[j] > 0.0, "%s: component %d: %s", who, k, MG_MIX_ILL_DEFINED);
            logdet = j == 0 ? log(col[0]) : logdet + log(col[j]);
        }
        m[dim] = (-0.5 * dim * MG_MIX_LOG_2PI + logdet) + (weights[k] > 0.0 ? log(weights[k]) : -INFINITY);
    }
    return MG_OK;
}

// ---- the kernel's shape, for the entry point's cut and the tests' edges ----------------------------------------------------------
#define MG_MIX_TILE 64              // targets per workgroup: one wave, one target per lane
#define MG_MIX_XS 65                // doubles between two coordinates of the staged targets: 65 = 1 mod 64 banks' worth of doubles keeps both the
                                    // staging writes (lane = coordinate) and the reads (lane = target) off each other's banks
enum { MG_MIX_ROUTE_REG4 = 0, MG_MIX_ROUTE_REG8 = 1, MG_MIX_ROUTE_STREAM = 2 };
// dim <= 4 and dim <= 8: the target in registers, the whole mixture in LDS; above: the targets in LDS, the factors streamed from L2
inline int mg_mix_route_of(int dim) { return dim <= 4 ? MG_MIX_ROUTE_REG4 : dim <= 8 ? MG_MIX_ROUTE_REG8 : MG_MIX_ROUTE_STREAM; }
// dynamic LDS of a workgroup, bytes: the mixture's blocks, or the tile's targets [dim][MG_MIX_XS] and its wlp [K][MG_MIX_TILE]
inline int mg_mix_lds_of(int K, int dim) {
    return mg_mix_route_of(dim) == MG_MIX_ROUTE_STREAM ? (dim * MG_MIX_XS + K * MG_MIX_TILE) * 8 : K * mg_mix_stride(dim) * 8;
}
