// The device image of a motion primitive and of its time grids, built as plain host code (standard headers, the C ABI, mg_hostdefs.h
// and mg_pack.h only, no HIP call: tests/native/primitive_image_check.cpp compiles this file alone and decodes what it writes).  The
// layouts are the ones mg_primitive and mg_time_grid (mg_internal.h) document and the kernels read; mg_host.hip uploads the vectors as
// they stand.  A descriptor is checked and its whole image built before anything is allocated.  Compiled with -ffp-contract=off like
// the rest of the host code: every fma below is spelled out.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mg_hostdefs.h"
#include "mg_pack.h"

// What a primitive keeps on the host: its shape, the scalars derived from it and the float64 copies (mg_primitive derives from this)
struct mg_primitive_model {
    int32_t NB = 0, D = 0, L = 0, F = 0, K = 0, R = 0;
    int32_t nroot = 0;  // min(3, D): root-translation channels (float64 pipeline or mean/delta split)
    bool root_split = false;      // the accuracy gate allows the mean/delta split (mg_primitive_root_mode)
    double root_split_est = 0.0;  // its error estimate
    int32_t KK = 0;     // MFMA k-steps (even), 0 when L > 64
    int32_t Lg = 0;     // dimension of the mixture (>= L: spatial + time latents)
    int32_t KKg = 0;    // MFMA k-steps of the mixture kernels (even), 0 when Lg > 64
    int32_t Lt = 0, NBt = 0;         // time model: components, basis functions
    int32_t RT = 0;     // 16-row tiles of the padded-row space NB*Dp
    int32_t RRT = 0;    // 16-row tiles of the root-row space
    int32_t Dp = 0;     // row pitch of the padded coefficient rows (multiple of 4)
    int32_t cshift = 0; // column of channel d in a padded row is d + cshift
    // host float64 copies (already scaled by translation_maxima)
    std::vector<double> Es;    // (R, L)
    std::vector<double> means_;  // mean' (R)
    std::vector<double> knots;
    std::vector<double> gw, gm, gc, gp;  // weights (K), means (K,L), covars (K,L,L), prec chol (K,L,L)
};
// ... and what is only uploaded (the tables mg_primitive's d_ pointers document; means_, knots and gm are tables as well), plus the
// times of the two grids a primitive owns
struct mg_primitive_image : mg_primitive_model {
    std::vector<float> Et32, mean32, Epack;
    std::vector<double> Et64, Erpack, meanroot;
    std::vector<double> gcholpack, gmeanpad, gPpack, gPTpack, gmPpad, gP, gmP, gconst, gchol;
    std::vector<double> tphi, tmean;
    std::vector<double> canonical_times;                 // np.linspace(0, F, F)
    std::vector<double> identity_times, identity_w;      // the identity grid: row i selects coefficient i
    std::vector<int32_t> identity_i0;
};

// What a time grid keeps: its samples' basis rows and the chunk plan that selects the frames kernel (mg_time_grid derives from this)
struct mg_grid_plan {
    int32_t T = 0;
    std::vector<double> times;
    std::vector<int32_t> i0;
    std::vector<double> w;  // (T,4)
    std::vector<mg_chunk> chunks;
    int32_t n_chunks = 0;
    int32_t stride = 0;      // floats per candidate in the LDS coefficient image
    int32_t max_wi = 0;
    int32_t max_nt = 16;        // samples of the longest chunk, rounded up to 16: sizes the per-slot tables in LDS
    int32_t lds_bytes = 0;   // dynamic LDS of the MFMA kernel for this grid
    int32_t nbuf = 2;        // LDS ring depth of the MFMA kernel (3 when it fits)
    bool mfma_ok = false;
    int32_t max_tiles = 0;   // row tiles of the widest chunk window
    int32_t cs_lds_bytes = 0;   // dynamic LDS of the chunk-stationary kernel (without the fused mixture's buffers)
    bool cs_ok = false;      // the chunk-stationary kernel covers this grid (window fits the row producers' registers, LDS fits)
};
// ... and what is only uploaded; i0, w and chunks are tables as well
struct mg_grid_image : mg_grid_plan {
    std::vector<float> w32, rootm;
    std::vector<double> wtap;
};

// lower Cholesky factor; returns false if not positive definite
inline bool mg_cholesky_lower(const double *S, int L, double *c) {
    std::fill(c, c + (size_t)L * L, 0.0);
    for (int j = 0; j < L; j++) {
        double sum = S[j * L + j];
        for (int p = 0; p < j; p++) sum -= c[j * L + p] * c[j * L + p];
        if (!(sum > 0.0) || !std::isfinite(sum)) return false;
        c[j * L + j] = std::sqrt(sum);
        for (int i = j + 1; i < L; i++) {
            double s2 = S[i * L + j];
            for (int p = 0; p < j; p++) s2 -= c[i * L + p] * c[j * L + p];
            c[i * L + j] = s2 / c[j * L + j];
        }
    }
    return true;
}

// a knot vector of n knots: finite and non-decreasing (t[0] is held by the comparison alone, as ever)
inline bool mg_knots_ok(const double *t, int n) {
    for (int i = 0; i + 1 < n; i++)
        if (!(t[i] <= t[i + 1]) || !std::isfinite(t[i + 1])) return false;
    return true;
}

// a cubic spline's value from a basis row: w0 m0, fma(w1, m1, .), fma(w2, m2, .), fma(w3, m3, .) with m_j = m[j * stride]
inline double mg_tap4(const double *w, const double *m, size_t stride) {
    double v = w[0] * m[0];
    for (int j = 1; j < 4; j++) v = std::fma(w[j], m[j * stride], v);
    return v;
}

// The fragments of at(i, k) over `tiles` row tiles (mg_pack.h) twice, one copy directly behind the other: the k-steps in groups of Ga
// per lane, then in groups of Gb (1: the plain image [tile][KK][lane])
template <class T, class At>
inline std::vector<T> mg_pack_twice(int tiles, int KK, At at, int Ga, int Gb) {
    const size_t n1 = (size_t)tiles * KK * 64;
    std::vector<T> plain(n1), out(2 * n1);
    mg_pack_fragments(plain.data(), tiles, KK, at);
    for (int h = 0; h < 2; h++) {
        if ((h ? Gb : Ga) == 1) std::copy(plain.begin(), plain.end(), out.begin() + h * n1);
        else mg_pack_regroup(plain.data(), out.data() + h * n1, tiles, KK, h ? Gb : Ga);
    }
    return out;
}

// The parts of mg_primitive_image_build below, in its order.  First the shape's checks, the derived scalars, E', mean' and the knots
inline int mg_primitive_image_model(const mg_primitive_desc *d, mg_primitive_image *p) {
    MG_REQUIRE(d->n_basis >= 4, "mg_primitive_create: n_basis = %d, a cubic spline needs >= 4", d->n_basis);
    MG_REQUIRE(d->n_dim >= 1 && d->n_components >= 1 && d->n_canonical_frames >= 1,
               "mg_primitive_create: n_dim/n_components/n_canonical_frames must be >= 1");
    MG_REQUIRE(d->n_gmm >= 0, "mg_primitive_create: n_gmm < 0");
    MG_REQUIRE(d->eigen_vectors && d->mean_vector && d->knots, "mg_primitive_create: eigen_vectors/mean_vector/knots are required");
    MG_REQUIRE(d->n_gmm == 0 || (d->gmm_weights && d->gmm_means && d->gmm_covars),
               "mg_primitive_create: gmm arrays are required when n_gmm > 0");
    MG_REQUIRE((int64_t)d->n_basis * d->n_dim < (1 << 24), "mg_primitive_create: n_basis*n_dim too large");
    const int NB = d->n_basis, D = d->n_dim, L = d->n_components, K = d->n_gmm, R = NB * D;
    const int Lg = d->n_gmm_dims > 0 ? d->n_gmm_dims : L;   // the mixture spans the spatial AND the time latents
    MG_REQUIRE(Lg >= L, "mg_primitive_create: n_gmm_dims = %d < n_components = %d", Lg, L);
    const int Lt = d->n_time_components, NBt = d->n_basis_time;
    MG_REQUIRE(Lt >= 0 && (Lt == 0 || (NBt >= 4 && d->eigen_vectors_time && d->mean_time_vector && d->knots_time)),
               "mg_primitive_create: a time model needs n_basis_time >= 4, eigen_vectors_time, mean_time_vector and knots_time");
    MG_REQUIRE(mg_knots_ok(d->knots, NB + 4), "mg_primitive_create: knots must be finite and non-decreasing");
    MG_REQUIRE(d->knots[3] < d->knots[NB], "mg_primitive_create: knot vector has an empty domain");

    *p = mg_primitive_image();
    p->NB = NB; p->D = D; p->L = L; p->F = d->n_canonical_frames; p->K = K; p->R = R;
    p->nroot = std::min(3, D);
    p->KK = (L <= 4 * MG_MAX_KK) ? (((L + 3) / 4 + 1) / 2) * 2 : 0;
    p->Lg = Lg;
    p->KKg = (Lg <= 4 * MG_MAX_KK) ? (((Lg + 3) / 4 + 1) / 2) * 2 : 0;
    p->Lt = Lt; p->NBt = NBt;
    // padded coefficient rows: column = d + cshift so that the first non-root channel sits on a
    // 16-byte boundary (quads of channels start at d = nroot), pitch a multiple of 4
    p->cshift = (4 - p->nroot) & 3;
    p->Dp = (D + p->cshift + 3) & ~3;
    p->RT = (NB * p->Dp + 15) / 16;
    p->knots.assign(d->knots, d->knots + NB + 4);
    double tm[3] = {1.0, 1.0, 1.0};
    if (d->translation_maxima)
        for (int i = 0; i < 3; i++) tm[i] = d->translation_maxima[i];

    // E' = E * scale_d, mean' = mean * scale_d (float64 products): the reference applies
    // translation_maxima after adding the mean (motion_primitive.py:251-255), which is
    // the same linear map.
    p->Es.resize((size_t)R * L);
    p->means_.resize(R);
    for (int r = 0; r < R; r++) {
        double sc = (r % D < 3) ? tm[r % D] : 1.0;
        for (int k = 0; k < L; k++) {
            double e = d->eigen_is_transposed ? d->eigen_vectors[(size_t)r * L + k] : d->eigen_vectors[(size_t)k * R + r];
            p->Es[(size_t)r * L + k] = e * sc;
        }
        p->means_[r] = d->mean_vector[r] * sc;
    }
    return MG_OK;
}

// device images of E' and mean'
inline void mg_primitive_image_spatial(mg_primitive_image *p) {
    const int NB = p->NB, D = p->D, L = p->L, R = p->R;
    p->Et32.resize((size_t)L * R);
    p->Et64.resize((size_t)L * R);
    for (int r = 0; r < R; r++)
        for (int k = 0; k < L; k++) {
            p->Et64[(size_t)k * R + r] = p->Es[(size_t)r * L + k];
            p->Et32[(size_t)k * R + r] = (float)p->Es[(size_t)r * L + k];
        }
    p->mean32.assign((size_t)p->RT * 16, 0.0f);
    for (int i = 0; i < NB; i++)
        for (int dd = p->nroot; dd < D; dd++)   // the root rows' C-in is zero: they hold E'.s alone (the split's delta)
            p->mean32[(size_t)i * p->Dp + dd + p->cshift] = (float)p->means_[(size_t)i * D + dd];
    if (p->KK > 0) {
        // the root rows (row = i*nroot + d) of E' (mg_pack.h)
        const int KK = p->KK, nr = p->nroot, RR = NB * nr, Dp = p->Dp;
        p->RRT = (RR + 15) / 16;
        p->Erpack.resize((size_t)p->RRT * KK * 64);
        p->meanroot.assign((size_t)p->RRT * 16, 0.0);
        for (int rr = 0; rr < RR; rr++) p->meanroot[rr] = p->means_[(size_t)(rr / nr) * D + rr % nr];
        mg_pack_fragments(p->Erpack.data(), p->RRT, KK, [&](int rr, int k) { return rr < RR && k < L ? p->Es[((size_t)(rr / nr) * D + rr % nr) * L + k] : 0.0; });
        // the padded coefficient rows r' = i*Dp + d + cshift of E' in float32 (zero rows elsewhere), k-steps in pairs per lane (mg_pack.h),
        // followed by a second copy for the chunk-stationary kernel's one-time fragment loads, k-steps in quads per lane: 16-byte loads, 3 instead
        // of 5 instructions per tile at KK = 10 through a CU's address unit while the whole chip fetches its windows at once (csrc/mg_frames_cs.hip,
        // mg_cs_load_fragments)
        p->Epack = mg_pack_twice<float>(p->RT, KK, [&](int rp, int k) {
            const int i = rp / Dp, dd = rp - i * Dp - p->cshift;
            return (i < NB && dd >= 0 && dd < D && k < L) ? (float)p->Es[((size_t)i * D + dd) * L + k] : 0.0f;
        }, 2, 4);
    }
}

// the mixture: host copies, precision Cholesky factors in six layouts, per-component constants
inline int mg_primitive_image_mixture(const mg_primitive_desc *d, mg_primitive_image *p) {
    const int K = p->K, Lg = p->Lg;
    if (K > 0) {
        p->gw.assign(d->gmm_weights, d->gmm_weights + K);
        p->gm.assign(d->gmm_means, d->gmm_means + (size_t)K * Lg);
        p->gc.assign(d->gmm_covars, d->gmm_covars + (size_t)K * Lg * Lg);
        p->gp.assign((size_t)K * Lg * Lg, 0.0);
        std::vector<double> inv((size_t)Lg * Lg);
        std::vector<double> &chol = p->gchol, &gP = p->gP, &gmP = p->gmP, &gconst = p->gconst;
        chol.resize((size_t)K * Lg * Lg);
        gP.assign((size_t)K * Lg * Lg, 0.0);
        gmP.resize((size_t)K * Lg);
        gconst.resize(K);
        const double log2pi = std::log(2.0 * M_PI);
        for (int k = 0; k < K; k++) {
            double *c = &chol[(size_t)k * Lg * Lg];
            MG_REQUIRE(p->gw[k] >= 0.0 && std::isfinite(p->gw[k]), "mg_primitive_create: gmm_weights[%d] is negative or not finite", k);
            MG_REQUIRE_AS(mg_cholesky_lower(&p->gc[(size_t)k * Lg * Lg], Lg, c), MG_ERR_NOT_POSITIVE_DEFINITE,
                          "mg_primitive_create: gmm_covars[%d] is not positive definite", k);
            // sklearn _compute_precision_cholesky: P = solve_triangular(chol, I, lower=True).T
            std::fill(inv.begin(), inv.end(), 0.0);
            for (int col = 0; col < Lg; col++)
                for (int r = col; r < Lg; r++) {
                    double s = (r == col) ? 1.0 : 0.0;
                    for (int q = col; q < r; q++) s -= c[r * Lg + q] * inv[(size_t)q * Lg + col];
                    inv[(size_t)r * Lg + col] = s / c[r * Lg + r];
                }
            double *P = &p->gp[(size_t)k * Lg * Lg];
            double logdet = 0.0;
            for (int i = 0; i < Lg; i++) {
                for (int j = 0; j < Lg; j++) P[i * Lg + j] = inv[(size_t)j * Lg + i];
                logdet += std::log(P[i * Lg + i]);
            }
            for (int j = 0; j < Lg; j++) {
                double acc = 0.0;
                for (int i = 0; i <= j; i++) {
                    gP[((size_t)k * Lg + j) * Lg + i] = P[i * Lg + j];
                    acc += p->gm[(size_t)k * Lg + i] * P[i * Lg + j];
                }
                gmP[(size_t)k * Lg + j] = acc;
            }
            gconst[k] = std::log(p->gw[k]) + logdet - 0.5 * (double)Lg * log2pi;
        }
        if (p->KKg > 0) {
            // images [component][tile][k-step][lane] (mg_pack.h), (i16, k) = (16-wide index, reduction index); a row of the K * JT tiles
            // is (component, 16-wide index) = (row / JL, row % JL).  Inside this block L is the mixture's dimension.
            const int KK = p->KKg, JT = (Lg + 15) / 16, JL = JT * 16, L = Lg;
            p->gmPpad.assign((size_t)K * JL, 0.0);
            p->gmeanpad.assign((size_t)K * JL, 0.0);
            for (int k = 0; k < K; k++) {
                for (int j = 0; j < L; j++) p->gmPpad[(size_t)k * JL + j] = gmP[(size_t)k * L + j];
                for (int i = 0; i < L; i++) p->gmeanpad[(size_t)k * JL + i] = p->gm[(size_t)k * L + i];
            }
            auto upper = [&](int k, int i, int j) { return i < L && j < L && i <= j ? p->gp[((size_t)k * L + i) * L + j] : 0.0; };   // P_k[i][j]
            // the precision factor P_k[i][j], upper triangular, reduced over i; behind it the same fragments with the k-steps in pairs per lane (the
            // fused step's staged tail and its start-up half: half the load instructions through a CU's address unit, csrc/mg_gmm_device.h) ...
            p->gPpack = mg_pack_twice<double>(K * JT, KK, [&](int row, int i) { return upper(row / JL, i, row % JL); }, 1, 2);
            // ... its transpose for z = y P_k^T (log_likelihood_jac), reduced over j ...
            p->gPTpack.resize((size_t)K * JT * KK * 64);
            mg_pack_fragments(p->gPTpack.data(), K * JT, KK, [&](int row, int j) { return upper(row / JL, row % JL, j); });
            // ... and the sampler's x = mu + z L^T: L_k[i][j], lower triangular, reduced over j; behind it the pairs per lane: 16-byte loads in
            // the planner step's sampler
            p->gcholpack = mg_pack_twice<double>(K * JT, KK, [&](int row, int j) {
                const int k = row / JL, i = row % JL;
                return i < L && j < L && j <= i ? chol[((size_t)k * L + i) * L + j] : 0.0;
            }, 1, 2);
        }
    }
    return MG_OK;
}

// the mean/delta split's accuracy gate (mg_primitive_root_mode)
inline void mg_primitive_image_root_gate(mg_primitive_image *p) {
    const int NB = p->NB, D = p->D, L = p->L, K = p->K, Lg = p->Lg;
    std::vector<double> m2(L, 1.0);
    double wsum = 0.0;
    for (int j = 0; j < K; j++) wsum += p->gw[j];
    if (K > 0)
        for (int k = 0; k < L; k++) {
            double acc = 0.0;
            for (int j = 0; j < K; j++) {
                const double mu = p->gm[(size_t)j * Lg + k];
                acc += p->gw[j] * (mu * mu + p->gc[(size_t)j * Lg * Lg + (size_t)k * Lg + k]);
            }
            m2[k] = acc / wsum;
        }
    double worst = 0.0;
    for (int i = 0; i < NB; i++)
        for (int dd = 0; dd < p->nroot; dd++) {
            const double *e = &p->Es[((size_t)i * D + dd) * L];
            double ss = 0.0;
            for (int k = 0; k < L; k++) ss += e[k] * e[k] * m2[k];
            worst = std::max(worst, std::sqrt(ss));
        }
    p->root_split_est = (double)(L + 8) * 0x1p-24 * worst;
    p->root_split = std::isfinite(p->root_split_est) && p->root_split_est <= MG_ROOT_SPLIT_MAX_EST;
}

// the time model's tables, then the times of the two grids a primitive owns
inline int mg_primitive_image_time(const mg_primitive_desc *d, mg_primitive_image *p) {
    const int NB = p->NB, F = p->F, Lt = p->Lt, NBt = p->NBt;
    if (Lt > 0) {
        // mean time spline and harmonics at the canonical frames 0 .. F-1 (reference motion_primitive.py:258-268,293-296:
        // si.splev(canonical_time_range, (knots_t, coefficients, 3)); column l of eigen_vectors_time = coefficients of harmonic l)
        MG_REQUIRE(mg_knots_ok(d->knots_time, NBt + 4), "mg_primitive_create: knots_time must be finite and non-decreasing");
        p->tphi.resize((size_t)F * Lt);
        p->tmean.resize(F);
        for (int f = 0; f < F; f++) {
            int32_t i0;
            double w[4];
            mg_basis_row(d->knots_time, NBt + 4, (double)f, &i0, w);
            p->tmean[f] = mg_tap4(w, &d->mean_time_vector[i0], 1);
            for (int l = 0; l < Lt; l++) p->tphi[(size_t)f * Lt + l] = mg_tap4(w, &d->eigen_vectors_time[(size_t)i0 * Lt + l], (size_t)Lt);
        }
    }
    // canonical grid: np.linspace(0, F, int(F * 1.0))  (reference motion_primitive.py:233)
    p->canonical_times.resize(F);
    if (F == 1) {
        p->canonical_times[0] = 0.0;
    } else {
        double step = (double)F / (double)(F - 1);
        for (int f = 0; f < F; f++) p->canonical_times[f] = (double)f * step;
        p->canonical_times[F - 1] = (double)F;
    }
    // identity grid: row i selects coefficient i, so "frames" are the coefficients
    p->identity_times.assign(NB, 0.0);
    p->identity_w.assign((size_t)NB * 4, 0.0);
    p->identity_i0.resize(NB);
    for (int i = 0; i < NB; i++) {
        int base = std::min(i, NB - 4);
        p->identity_i0[i] = base;
        p->identity_w[4 * i + (i - base)] = 1.0;
        p->identity_times[i] = (double)i;
    }
    return MG_OK;
}

// The image of descriptor d.  MG_OK, or the refusal with its text set; `im` is then not to be read.
inline int mg_primitive_image_build(const mg_primitive_desc *d, mg_primitive_image &im) {
    int rc = mg_primitive_image_model(d, &im);
    if (rc != MG_OK) return rc;
    mg_primitive_image_spatial(&im);
    if ((rc = mg_primitive_image_mixture(d, &im)) != MG_OK) return rc;
    mg_primitive_image_root_gate(&im);
    return mg_primitive_image_time(d, &im);
}

// ---- time grids: the chunk plan ---------------------------------------------------------------------------------------------------
inline int mg_round_stride(int nlocal) {
    // floats per candidate in the LDS coefficient image: == 4 (mod 32) makes the
    // 16-candidate ds_write_b128 of an MFMA accumulator tile conflict-free.
    int s = nlocal;
    while (s % 32 != 4) s++;
    return s;
}

// LDS per ring slot of both frames kernels (coefficient image + float32 root outputs) and of their float64 root image
inline int mg_lds_slot_bytes(int stride, int max_nt) {
    int buf = (MG_NCAND * stride * 4 + 255) / 256 * 256;
    int rout = MG_RO_BYTES_N(max_nt);
    return buf + rout;
}
inline int mg_lds_root_bytes(int nroot, int wi) { return MG_NCAND * (wi * nroot + 1) * 8; }

// LDS of the persistent kernel: nbuf slots, each with a per-sample table set, and the float64 root image
inline int mg_lds_bytes(int nroot, int stride, int wi, int nbuf = 2, int max_nt = MG_MAX_NT) {
    int tabs = max_nt * 16 + max_nt * 4;
    return nbuf * (mg_lds_slot_bytes(stride, max_nt) + tabs) + mg_lds_root_bytes(nroot, wi) + 128;
}

// One chunk's run of samples: from sample a on, at most `cap` of them while their window stays within w basis functions.  Returns the
// end b of the run, [imin, imax] = the first basis functions of its samples.
inline int mg_grow_chunk(const std::vector<int32_t> &i0, int a, int cap, int w, int &imin, int &imax) {
    const int T = (int)i0.size();
    imin = i0[a]; imax = i0[a];
    int b = a + 1;
    while (b < T && b - a < cap) {
        int lo = std::min(imin, i0[b]), hi = std::max(imax, i0[b]);
        if (hi - lo + 4 > w) break;
        imin = lo; imax = hi;
        b++;
    }
    return b;
}

// Split the grid g (T, i0 set) of primitive p into chunks (runs of consecutive time samples) whose coefficient window fits the LDS
// budget.  opt_*: MG_OPT_CHUNK_SAMPLES, MG_OPT_CHUNK_WINDOW, MG_OPT_RING_SLOTS (0: default); cs_max_tiles: mg_cs_max_tiles(p.KK).
inline void mg_plan_chunks(const mg_primitive_model &p, mg_grid_plan &g, int opt_samples, int opt_window, int opt_ring, int cs_max_tiles) {
    const int Dp = p.Dp, T = g.T;
    g.chunks.clear();
    g.mfma_ok = false;
    if (p.KK == 0 || T == 0 || (p.D - p.nroot + 3) / 4 + 1 > 64) return;   // one row group must fit a wave
    // widest window (<= 8 basis functions) whose double-buffered image fits one CU's 160 KiB of LDS
    const int budget1 = 160 * 1024;
    auto fits = [&](int wi, int budget) {
        int nlocal = ((wi * Dp + 15) / 16 + 1) * 16;
        return mg_lds_bytes(p.nroot, mg_round_stride(nlocal), wi) <= budget;
    };
    int max_nt = MG_MAX_NT;
    if (const int o = opt_samples) max_nt = std::max(1, std::min(MG_MAX_NT, o));
    auto count_chunks = [&](int w) {   // greedy split under a window of w basis functions
        int n = 0, imin, imax;
        for (int a0 = 0; a0 < T; n++) a0 = mg_grow_chunk(g.i0, a0, max_nt, w, imin, imax);
        return n;
    };
    // Fewer, longer chunks win (each unit has fixed costs -- measured: 6 -> 4 chunks of the 'walk' grid -3 %, while a
    // two-slot ring instead of three costs 0.5 %): the narrowest window that reaches the smallest chunk count among
    // the windows whose two-slot ring fits LDS.
    int W = 0, best_n = 0;
    for (int w = MG_MAX_WI; w >= 4; w--) {
        if (!fits(w, budget1)) continue;
        const int n = count_chunks(w);
        if (W == 0 || n <= best_n) { W = w; best_n = n; }
    }
    if (W == 0) return;  // n_dim too large for the LDS-staged kernel
    if (const int o = opt_window) W = std::max(4, std::min(W, o));
    // the chunk count of the greedy split, evened out
    const int n_greedy = count_chunks(W);
    int a = 0;
    int max_stride = 0, max_wi = 0, longest = 0;
    while (a < T) {
        int imin, imax;
        const int left = std::max(1, n_greedy - (int)g.chunks.size());
        const int target = std::min(max_nt, (T - a + left - 1) / left);
        const int b = mg_grow_chunk(g.i0, a, target, W, imin, imax);
        mg_chunk c;
        memset(&c, 0, sizeof(c));
        c.t0 = a;
        c.nT = b - a;
        c.imin = imin;
        c.wi = imax - imin + 4;
        c.rt0 = (imin * Dp) / 16;
        int rt1 = ((imin + c.wi) * Dp + 15) / 16;
        c.ntiles = rt1 - c.rt0;
        c.rrt0 = (imin * p.nroot) / 16;
        c.nrt = ((imin + c.wi) * p.nroot + 15) / 16 - c.rrt0;
        g.chunks.push_back(c);
        max_stride = std::max(max_stride, mg_round_stride(c.ntiles * 16));
        max_wi = std::max(max_wi, c.wi);
        longest = std::max(longest, c.nT);
        a = b;
    }
    g.stride = max_stride;
    g.max_wi = max_wi;
    g.max_nt = (longest + 15) / 16 * 16;
    // a third ring slot lets the producers run a full unit ahead of the slowest consumer wave
    g.nbuf = mg_lds_bytes(p.nroot, max_stride, max_wi, 3, g.max_nt) <= budget1 ? 3 : 2;
    if (opt_ring == 2) g.nbuf = 2;
    g.lds_bytes = mg_lds_bytes(p.nroot, max_stride, max_wi, g.nbuf, g.max_nt);
    g.n_chunks = (int32_t)g.chunks.size();
    g.mfma_ok = g.lds_bytes <= budget1;
    // the chunk-stationary kernel: two ring slots, ONE table set, the window's mean' rows; its row producers hold the
    // window's eigenvector fragments in registers
    g.max_tiles = 0;
    for (const mg_chunk &c : g.chunks) g.max_tiles = std::max(g.max_tiles, c.ntiles);
    g.cs_lds_bytes = 2 * mg_lds_slot_bytes(max_stride, g.max_nt) + g.max_nt * 20 + mg_lds_root_bytes(p.nroot, max_wi) + g.max_tiles * 64 +
                     MG_TAP_FT * MG_TAP_KS * 64 * 8 + 512 + 2 * p.KK * 64 * 4 + 256;   // + tap weights, root means, two latent tiles, 64 counters
    g.cs_ok = g.mfma_ok && g.max_tiles <= cs_max_tiles && g.cs_lds_bytes <= budget1 && (int)g.chunks.size() <= MG_ARG_CHUNKS;
}

// The image of a grid of T samples on primitive p: the basis rows of `times` on p's knots, or (i0, w) as given; then the plan
// (mg_plan_chunks' arguments) and the per-sample and per-chunk tables
inline void mg_grid_image_build(const mg_primitive_model &p, const double *times, int32_t T, const int32_t *i0_override, const double *w_override,
                                int opt_samples, int opt_window, int opt_ring, int cs_max_tiles, mg_grid_image &im) {
    im = mg_grid_image();
    mg_grid_image *g = &im;
    g->T = T;
    g->times.assign(times, times + T);
    g->i0.resize(T);
    g->w.resize((size_t)T * 4);
    for (int f = 0; f < T; f++) {
        if (i0_override) {
            g->i0[f] = i0_override[f];
            for (int j = 0; j < 4; j++) g->w[4 * f + j] = w_override[4 * f + j];
        } else {
            mg_basis_row(p.knots.data(), (int)p.knots.size(), times[f], &g->i0[f], &g->w[4 * f]);
        }
    }
    mg_plan_chunks(p, im, opt_samples, opt_window, opt_ring, cs_max_tiles);
    g->w32.resize(g->w.size());
    for (size_t q = 0; q < g->w.size(); q++) g->w32[q] = (float)g->w[q];
    // the root channels' mean part (mean/delta split, mg_primitive_root_mode): M[f][d] = mg_tap4 in float64 with
    // m_j = mean'[(i0[f] + j) D + d]; Mhi = (float)M, Mlo = (float)(M - Mhi)
    g->rootm.assign((size_t)std::max(T, 1) * 8, 0.0f);
    for (int f = 0; f < T; f++)
        for (int d = 0; d < p.nroot; d++) {
            const double M = mg_tap4(&g->w[4 * (size_t)f], &p.means_[(size_t)g->i0[f] * p.D + d], (size_t)p.D);
            const float hi = (float)M;
            g->rootm[8 * (size_t)f + d] = hi;                              // {Mhi[0..2], Mlo[0], Mlo[1], Mlo[2], 0, 0}: the sweep reads
            g->rootm[8 * (size_t)f + 3 + d] = (float)(M - (double)hi);    // a float4 and a float2 per sample, every element used
        }
    // banded tap weights of every chunk (mg_pack.h): W[f][m] = w[f][m - (i0[f] - imin)] inside the band
    g->wtap.assign(std::max<size_t>(g->chunks.size(), 1) * MG_TAP_FT * MG_TAP_KS * 64, 0.0);
    for (size_t c = 0; c < g->chunks.size(); c++) {
        const mg_chunk &ck = g->chunks[c];
        mg_pack_fragments(&g->wtap[c * MG_TAP_FT * MG_TAP_KS * 64], MG_TAP_FT, MG_TAP_KS, [&](int f, int m) {
            const int j = f < ck.nT ? m - (g->i0[ck.t0 + f] - ck.imin) : -1;
            return j >= 0 && j < 4 ? g->w[4 * (size_t)(ck.t0 + f) + j] : 0.0;
        });
    }
}
