// What the primitive's and the time grids' images of csrc/mg_primitive_image.h must contain, checked by DECODING them: every packed
// image through mg_pack.h's own index functions back to the plain matrix it claims, the padded and root rows, the transposes, the
// regrouped copies behind the plain ones, the mean/delta pairs and the tap band, at the smallest shapes at which each index expression
// can go wrong; the chunk planner against a restatement written here (the algorithm of plan_chunks in tests/test_gpu_frame_shapes.py)
// over a dense sweep; every refusal with its full text, code and precedence.  Numeric content (the Cholesky factors, gconst, tphi) has
// no tolerance here: the GPU parity tests pin it against the reference's goldens.  Plain host code with its own main (test
// infrastructure, never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_primitive_image.h"

#include <cstdarg>
#include <cstdio>
#include <limits>
#include <string>

static long failures = 0, checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { if (failures++ < 30) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static char g_err[1024] = "";
void mg_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

// ---- a descriptor by formula: no two elements alike, a few negative zeros ---------------------------------------------------------
struct Desc {
    std::vector<double> ev, mean, knots, tm, gw, gm, gc, evt, mt, kt;
    mg_primitive_desc d;
    Desc(int NB, int D, int L, int F, int K, int Lg_in, int Lt, int NBt, bool transposed, bool with_tm) {
        std::memset(&d, 0, sizeof(d));
        const int R = NB * D, Lg = Lg_in > 0 ? Lg_in : L;
        ev.resize((size_t)R * L);
        for (int r = 0; r < R; r++)
            for (int k = 0; k < L; k++) (transposed ? ev[(size_t)r * L + k] : ev[(size_t)k * R + r]) = (r % 7 == 3 && k == 2) ? -0.0 : 1.0 / (1.0 + r + 0.37 * k) - 0.01 * k - 0.001 * r;
        for (int r = 0; r < R; r++) mean.push_back(r == 4 ? -0.0 : 0.25 * r - 7.0 + 1.0 / (r + 3.0));
        knots = clamped(NB);
        tm = {1.5, 2.0, 0.5};
        for (int k = 0; k < K; k++) {
            gw.push_back((k + 1.0) / (K * (K + 1) / 2.0));
            for (int i = 0; i < Lg; i++) gm.push_back(0.1 * i - 0.3 * k + 0.017);
            for (int i = 0; i < Lg; i++)   // diagonally dominant, symmetric, every off-diagonal element its own value
                for (int j = 0; j < Lg; j++) gc.push_back(i == j ? 2.0 + 0.1 * i + k : 1.0 / (8.0 + 3.0 * std::min(i, j) + std::max(i, j) + k) / Lg);
        }
        for (int i = 0; i < NBt; i++) {
            mt.push_back(0.05 * i - 0.1);
            for (int l = 0; l < Lt; l++) evt.push_back(0.04 / (1.0 + i + 2.0 * l) - 0.01);
        }
        kt = clamped(std::max(NBt, 4));
        d.n_basis = NB; d.n_dim = D; d.n_components = L; d.n_canonical_frames = F; d.n_gmm = K; d.n_gmm_dims = Lg_in;
        d.eigen_is_transposed = transposed; d.eigen_vectors = ev.data(); d.mean_vector = mean.data(); d.knots = knots.data();
        d.translation_maxima = with_tm ? tm.data() : nullptr;
        if (K > 0) { d.gmm_weights = gw.data(); d.gmm_means = gm.data(); d.gmm_covars = gc.data(); }
        d.n_time_components = Lt; d.n_basis_time = NBt;
        if (Lt > 0) { d.eigen_vectors_time = evt.data(); d.mean_time_vector = mt.data(); d.knots_time = kt.data(); }
    }
    static std::vector<double> clamped(int nb) {   // nb + 4 knots on [0, nb - 3]
        std::vector<double> t;
        for (int i = 0; i < nb + 4; i++) t.push_back(i < 4 ? 0.0 : (i >= nb ? nb - 3.0 : i - 3.0));
        return t;
    }
    double E(int r, int k) const { return d.eigen_is_transposed ? ev[(size_t)r * d.n_components + k] : ev[(size_t)k * d.n_basis * d.n_dim + r]; }
};

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool samef(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
static bool bytes_equal(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 8) == 0); }

// (row, k) of every element of an operand image, by mg_pack.h's own statements: the image of at(i, k) = i * 1024 + k, regrouped as asked
static std::vector<int> index_image(int tiles, int KK, int G) {
    std::vector<int> plain((size_t)tiles * KK * 64), out(plain.size());
    mg_pack_fragments(plain.data(), tiles, KK, [](int i, int k) { return i * 1024 + k; });
    if (G == 1) return plain;
    mg_pack_regroup(plain.data(), out.data(), tiles, KK, G);
    return out;
}
template <class T, class At>
static void decode(const char *what, const T *image, int tiles, int KK, int G, At expect) {
    const std::vector<int> idx = index_image(tiles, KK, G);
    long bad = 0;
    for (size_t q = 0; q < idx.size(); q++) {
        const T want = expect(idx[q] / 1024, idx[q] % 1024);
        if (std::memcmp(&image[q], &want, sizeof(T)) != 0) bad++;
    }
    CHECK(bad == 0, "%s: %ld of %zu elements differ (G = %d)", what, bad, idx.size(), G);
}

static int cs_max_tiles(int KK) {   // mg_cs_cfg<KK>::MAX_TILES (csrc/mg_frames_cs.hip), restated
    if (KK == 0) return 0;
    return 3 * std::min(120 / KK, 17) + 4 * std::min(std::max(40 / KK, 1), 5);
}

static void check_grid(const char *name, const mg_primitive_model &p, const mg_grid_image &g) {
    const int T = g.T;
    CHECK((int)g.i0.size() == T && (int)g.w.size() == 4 * T && g.w32.size() == g.w.size() && (int)g.times.size() == T, "%s: sizes", name);
    for (size_t q = 0; q < g.w.size(); q++) CHECK(samef(g.w32[q], (float)g.w[q]), "%s: w32[%zu]", name, q);
    CHECK(g.rootm.size() == (size_t)std::max(T, 1) * 8, "%s: rootm holds %zu floats", name, g.rootm.size());
    if (T == 0) for (float v : g.rootm) CHECK(samef(v, 0.0f), "%s: rootm of an empty grid", name);
    for (int f = 0; f < T; f++) {
        const float *r = &g.rootm[8 * (size_t)f];
        CHECK(samef(r[6], 0.0f) && samef(r[7], 0.0f), "%s: rootm[%d][6..7]", name, f);
        for (int d = 0; d < 3; d++) {
            if (d >= p.nroot) { CHECK(samef(r[d], 0.0f) && samef(r[3 + d], 0.0f), "%s: rootm[%d] channel %d beyond the root", name, f, d); continue; }
            long double M = 0.0L, mag = 0.0L;   // the float64 value, summed wider; hi + lo holds it to float32-pair precision (2 x 24 bits)
            for (int j = 0; j < 4; j++) {
                const long double t = (long double)g.w[4 * (size_t)f + j] * p.means_[(size_t)(g.i0[f] + j) * p.D + d];
                M += t; mag += std::fabs((double)t);
            }
            CHECK(r[d] == (float)(double)((long double)r[d] + r[3 + d]) && std::fabs((double)(((long double)r[d] + r[3 + d]) - M)) <= (double)(mag * 0x1p-45L) + 1e-44,
                  "%s: rootm[%d][%d] = %g + %g against %Lg", name, f, d, (double)r[d], (double)r[3 + d], M);
        }
    }
    // chunks: runs of consecutive samples that cover the grid, windows that hold their samples
    CHECK(g.n_chunks == (int)g.chunks.size() || !g.mfma_ok, "%s: n_chunks", name);
    int next = 0;
    for (const mg_chunk &c : g.chunks) {
        CHECK(c.t0 == next && c.nT >= 1 && c.nT <= MG_MAX_NT && c.wi >= 4 && (c.wi <= MG_MAX_WI), "%s: chunk at %d", name, c.t0);
        for (int f = c.t0; f < c.t0 + c.nT; f++) CHECK(g.i0[f] >= c.imin && g.i0[f] + 4 <= c.imin + c.wi, "%s: sample %d outside its window", name, f);
        CHECK(c.rt0 * 16 <= c.imin * p.Dp && (c.rt0 + c.ntiles) * 16 >= (c.imin + c.wi) * p.Dp && c.rrt0 * 16 <= c.imin * p.nroot &&
              (c.rrt0 + c.nrt) * 16 >= (c.imin + c.wi) * p.nroot, "%s: chunk at %d: tiles do not cover the window", name, c.t0);
        next = c.t0 + c.nT;
    }
    CHECK(g.chunks.empty() || next == T, "%s: chunks cover %d of %d samples", name, next, T);
    // the tap band: W[f][m] = w[f][m - (i0[f] - imin)] inside the band of four, zero elsewhere and beyond the chunk's samples
    const size_t per = (size_t)MG_TAP_FT * MG_TAP_KS * 64;
    CHECK(g.wtap.size() == std::max<size_t>(g.chunks.size(), 1) * per, "%s: wtap holds %zu doubles", name, g.wtap.size());
    if (g.chunks.empty()) for (double v : g.wtap) CHECK(same(v, 0.0), "%s: wtap without chunks", name);
    for (size_t c = 0; c < g.chunks.size(); c++) {
        const mg_chunk &ck = g.chunks[c];
        decode(name, &g.wtap[c * per], MG_TAP_FT, MG_TAP_KS, 1, [&](int f, int m) {
            const int j = f < ck.nT ? m - (g.i0[ck.t0 + f] - ck.imin) : -1;
            return j >= 0 && j < 4 ? g.w[4 * (size_t)(ck.t0 + f) + j] : 0.0;
        });
    }
}

static long shapes_checked = 0;
static void check_shape(int NB, int D, int L, int F, int K, int Lg_in, int Lt, int NBt, bool transposed, bool with_tm) {
    Desc ds(NB, D, L, F, K, Lg_in, Lt, NBt, transposed, with_tm);
    char name[160];
    std::snprintf(name, sizeof(name), "NB %d D %d L %d F %d K %d Lg %d Lt %d %s%s", NB, D, L, F, K, Lg_in, Lt, transposed ? "T" : "N", with_tm ? " tm" : "");
    mg_primitive_image im;
    const int rc = mg_primitive_image_build(&ds.d, im);
    CHECK(rc == MG_OK, "%s: refused (%d, %s)", name, rc, g_err);
    if (rc != MG_OK) return;
    shapes_checked++;
    const int R = NB * D, Lg = Lg_in > 0 ? Lg_in : L, nroot = std::min(3, D), cshift = (4 - nroot) % 4, Dp = (D + cshift + 3) / 4 * 4;
    const int KK = L <= 64 ? (L + 7) / 8 * 2 : 0, KKg = Lg <= 64 ? (Lg + 7) / 8 * 2 : 0, RT = (NB * Dp + 15) / 16;
    CHECK(im.NB == NB && im.D == D && im.L == L && im.F == F && im.K == K && im.R == R && im.Lg == Lg && im.Lt == Lt && im.NBt == NBt, "%s: shape", name);
    CHECK(im.nroot == nroot && im.cshift == cshift && im.Dp == Dp && im.RT == RT && im.KK == KK && im.KKg == KKg, "%s: derived scalars (KK %d, KKg %d, Dp %d)", name, im.KK, im.KKg, im.Dp);
    // E', mean', the transposes
    CHECK(im.Es.size() == (size_t)R * L && im.means_.size() == (size_t)R && im.Et64.size() == im.Es.size() && im.Et32.size() == im.Es.size(), "%s: sizes", name);
    for (int r = 0; r < R; r++) {
        const double sc = with_tm && r % D < 3 ? ds.tm[r % D] : 1.0;
        CHECK(same(im.means_[r], ds.mean[r] * sc), "%s: mean'[%d]", name, r);
        for (int k = 0; k < L; k++) {
            const double e = ds.E(r, k) * sc;
            CHECK(same(im.Es[(size_t)r * L + k], e) && same(im.Et64[(size_t)k * R + r], e) && samef(im.Et32[(size_t)k * R + r], (float)e), "%s: E'[%d][%d]", name, r, k);
        }
    }
    CHECK(bytes_equal(im.knots, ds.knots), "%s: knots", name);
    // mean32: padded rows, zero on the root rows and on the padding
    CHECK(im.mean32.size() == (size_t)RT * 16, "%s: mean32 holds %zu", name, im.mean32.size());
    for (size_t q = 0; q < im.mean32.size(); q++) {
        const int i = (int)q / Dp, d = (int)q % Dp - cshift;
        CHECK(samef(im.mean32[q], (i < NB && d >= nroot && d < D) ? (float)im.means_[(size_t)i * D + d] : 0.0f), "%s: mean32[%zu]", name, q);
    }
    if (KK == 0) {
        CHECK(im.Erpack.empty() && im.meanroot.empty() && im.Epack.empty() && im.RRT == 0, "%s: packs without k-steps", name);
    } else {
        const int RR = NB * nroot, RRT = (RR + 15) / 16;
        CHECK(im.RRT == RRT && im.Erpack.size() == (size_t)RRT * KK * 64 && im.meanroot.size() == (size_t)RRT * 16 && im.Epack.size() == 2 * (size_t)RT * KK * 64, "%s: pack sizes", name);
        for (int rr = 0; rr < RRT * 16; rr++) CHECK(same(im.meanroot[rr], rr < RR ? im.means_[(size_t)(rr / nroot) * D + rr % nroot] : 0.0), "%s: meanroot[%d]", name, rr);
        decode(name, im.Erpack.data(), RRT, KK, 1, [&](int rr, int k) { return rr < RR && k < L ? im.Es[((size_t)(rr / nroot) * D + rr % nroot) * L + k] : 0.0; });
        auto padded = [&](int rp, int k) {   // rows r' = i * Dp + d + cshift, zero rows and columns elsewhere
            const int i = rp / Dp, d = rp % Dp - cshift;
            return (i < NB && d >= 0 && d < D && k < L) ? (float)im.Es[((size_t)i * D + d) * L + k] : 0.0f;
        };
        decode(name, im.Epack.data(), RT, KK, 2, padded);
        decode(name, im.Epack.data() + (size_t)RT * KK * 64, RT, KK, 4, padded);   // the quads directly behind the pairs
    }
    // the mixture
    if (K == 0) {
        CHECK(im.gw.empty() && im.gm.empty() && im.gc.empty() && im.gp.empty() && im.gP.empty() && im.gmP.empty() && im.gconst.empty() && im.gchol.empty() &&
              im.gPpack.empty() && im.gPTpack.empty() && im.gcholpack.empty() && im.gmPpad.empty() && im.gmeanpad.empty(), "%s: mixture tables without a mixture", name);
    } else {
        const size_t LL = (size_t)Lg * Lg;
        CHECK(bytes_equal(im.gw, ds.gw) && bytes_equal(im.gm, ds.gm) && bytes_equal(im.gc, ds.gc), "%s: mixture host copies", name);
        CHECK(im.gp.size() == K * LL && im.gP.size() == K * LL && im.gchol.size() == K * LL && im.gmP.size() == (size_t)K * Lg && im.gconst.size() == (size_t)K, "%s: mixture sizes", name);
        for (int k = 0; k < K; k++)
            for (int i = 0; i < Lg; i++)
                for (int j = 0; j < Lg; j++) {
                    const double P = im.gp[k * LL + (size_t)i * Lg + j], C = im.gchol[k * LL + (size_t)i * Lg + j];
                    CHECK((i <= j || same(P, 0.0)) && (j <= i || same(C, 0.0)) && (i != j || (P > 0.0 && C > 0.0)), "%s: triangles of component %d at (%d, %d)", name, k, i, j);
                    CHECK(same(im.gP[k * LL + (size_t)j * Lg + i], i <= j ? P : 0.0), "%s: gP of component %d: column %d, element %d", name, k, j, i);   // column j contiguous over i
                }
        if (KKg == 0) {
            CHECK(im.gPpack.empty() && im.gPTpack.empty() && im.gcholpack.empty() && im.gmPpad.empty() && im.gmeanpad.empty(), "%s: mixture packs without k-steps", name);
        } else {
            const int JT = (Lg + 15) / 16, JL = JT * 16;
            const size_t n1 = (size_t)K * JT * KKg * 64;
            CHECK(im.gPpack.size() == 2 * n1 && im.gcholpack.size() == 2 * n1 && im.gPTpack.size() == n1 && im.gmPpad.size() == (size_t)K * JL && im.gmeanpad.size() == (size_t)K * JL,
                  "%s: mixture pack sizes", name);
            for (int k = 0; k < K; k++)
                for (int j = 0; j < JL; j++)
                    CHECK(same(im.gmPpad[(size_t)k * JL + j], j < Lg ? im.gmP[(size_t)k * Lg + j] : 0.0) && same(im.gmeanpad[(size_t)k * JL + j], j < Lg ? im.gm[(size_t)k * Lg + j] : 0.0),
                          "%s: padded rows of component %d at %d", name, k, j);
            auto P = [&](int k, int i, int j) { return i < Lg && j < Lg && i <= j ? im.gp[k * LL + (size_t)i * Lg + j] : 0.0; };
            auto C = [&](int k, int i, int j) { return i < Lg && j < Lg && j <= i ? im.gchol[k * LL + (size_t)i * Lg + j] : 0.0; };
            for (int h = 0; h < 2; h++) {   // the pairs directly behind the plain image
                decode(name, im.gPpack.data() + h * n1, K * JT, KKg, h ? 2 : 1, [&](int row, int i) { return P(row / JL, i, row % JL); });       // 16-wide j, reduced over i
                decode(name, im.gcholpack.data() + h * n1, K * JT, KKg, h ? 2 : 1, [&](int row, int j) { return C(row / JL, row % JL, j); });    // 16-wide i, reduced over j
            }
            decode(name, im.gPTpack.data(), K * JT, KKg, 1, [&](int row, int j) { return P(row / JL, row % JL, j); });
        }
    }
    CHECK(Lt > 0 ? (im.tphi.size() == (size_t)F * Lt && im.tmean.size() == (size_t)F) : (im.tphi.empty() && im.tmean.empty()), "%s: time tables", name);
    // the two grids' times, the identity grid's rows
    CHECK((int)im.canonical_times.size() == F && same(im.canonical_times[0], 0.0) && (F == 1 || same(im.canonical_times[F - 1], (double)F)), "%s: canonical times", name);
    for (int f = 1; f + 1 < F; f++) CHECK(same(im.canonical_times[f], (double)f * ((double)F / (double)(F - 1))), "%s: canonical time %d", name, f);
    CHECK((int)im.identity_i0.size() == NB && (int)im.identity_w.size() == 4 * NB && (int)im.identity_times.size() == NB, "%s: identity grid sizes", name);
    for (int i = 0; i < NB; i++)
        for (int j = 0; j < 4; j++)
            CHECK(im.identity_i0[i] == std::min(i, NB - 4) && same(im.identity_w[4 * i + j], im.identity_i0[i] + j == i ? 1.0 : 0.0), "%s: identity row %d", name, i);
    // the grids a primitive owns and a user's: empty, fractional, repeated, backwards, out of range
    mg_grid_image g;
    mg_grid_image_build(im, im.canonical_times.data(), F, nullptr, nullptr, 0, 0, 0, cs_max_tiles(KK), g);
    check_grid(name, im, g);
    mg_grid_image_build(im, im.identity_times.data(), NB, im.identity_i0.data(), im.identity_w.data(), 0, 0, 0, cs_max_tiles(KK), g);
    check_grid(name, im, g);
    for (int i = 0; i < NB; i++) CHECK(g.i0[i] == im.identity_i0[i] && same(g.w[4 * i + 3], im.identity_w[4 * i + 3]), "%s: identity grid row %d", name, i);
    const double top = NB - 3.0;
    const std::vector<double> times = {0.0, 0.25, 0.25, top / 3.0 + 0.5, top, top - 0.5, 0.7, 0.1, -3.0, top + 4.0, 0.5 * top};
    mg_grid_image_build(im, times.data(), (int)times.size(), nullptr, nullptr, 3, 5, 2, cs_max_tiles(KK), g);
    check_grid(name, im, g);
    mg_grid_image_build(im, times.data(), 0, nullptr, nullptr, 0, 0, 0, cs_max_tiles(KK), g);
    check_grid(name, im, g);
}

// ---- the planner, restated (plan_chunks of tests/test_gpu_frame_shapes.py) ---------------------------------------------------------
struct Plan {
    bool mfma_ok = false, cs_ok = false;
    int n_chunks = 0, lds_bytes = 0, cs_lds_bytes = 0, max_wi = 0, max_nt = 16, nbuf = 2, max_tiles = 0, stride = 0;
    std::vector<mg_chunk> chunks;
};
static int r_round_stride(int s) { while (s % 32 != 4) s++; return s; }
static int r_ro_bytes(int nt) { return 16 * (nt * 4 + 8) * 4; }
static int r_image_bytes(int stride) { return (16 * stride * 4 + 255) / 256 * 256; }
static int r_lds_bytes(int nroot, int stride, int wi, int nbuf, int nt) { return nbuf * (r_image_bytes(stride) + r_ro_bytes(nt) + nt * 20) + 16 * (wi * nroot + 1) * 8 + 128; }
static Plan restated_plan(int D, int KK, const std::vector<int32_t> &i0, int window, int samples, int ring, int cs_tiles) {
    const int T = (int)i0.size(), nroot = std::min(3, D), Dp = (D + ((4 - nroot) & 3) + 3) & ~3, budget = 160 * 1024;
    Plan plan;
    if (KK == 0 || T == 0 || (D - nroot + 3) / 4 + 1 > 64) return plan;
    const int max_nt = samples ? std::max(1, std::min(48, samples)) : 48;
    auto grow = [&](int a, int cap, int w, int &lo, int &hi) {
        lo = hi = i0[a];
        int b = a + 1;
        for (; b < T && b - a < cap; b++) {
            const int l2 = std::min(lo, (int)i0[b]), h2 = std::max(hi, (int)i0[b]);
            if (h2 - l2 + 4 > w) break;
            lo = l2; hi = h2;
        }
        return b;
    };
    auto count = [&](int w) { int n = 0, lo, hi; for (int a = 0; a < T; n++) a = grow(a, max_nt, w, lo, hi); return n; };
    int W = 0, best = 0;
    for (int w = 11; w >= 4; w--) {
        if (r_lds_bytes(nroot, r_round_stride(((w * Dp + 15) / 16 + 1) * 16), w, 2, 48) > budget) continue;
        const int n = count(w);
        if (W == 0 || n <= best) { W = w; best = n; }
    }
    if (W == 0) return plan;
    if (window) W = std::max(4, std::min(W, window));
    const int n_greedy = count(W);
    int longest = 0;
    for (int a = 0; a < T;) {
        const int left = std::max(1, n_greedy - (int)plan.chunks.size());
        int lo, hi;
        const int b = grow(a, std::min(max_nt, (T - a + left - 1) / left), W, lo, hi);
        mg_chunk c;
        c.t0 = a; c.nT = b - a; c.imin = lo; c.wi = hi - lo + 4;
        c.rt0 = lo * Dp / 16; c.ntiles = ((lo + c.wi) * Dp + 15) / 16 - c.rt0;
        c.rrt0 = lo * nroot / 16; c.nrt = ((lo + c.wi) * nroot + 15) / 16 - c.rrt0;
        plan.chunks.push_back(c);
        plan.stride = std::max(plan.stride, r_round_stride(c.ntiles * 16));
        plan.max_wi = std::max(plan.max_wi, c.wi);
        plan.max_tiles = std::max(plan.max_tiles, c.ntiles);
        longest = std::max(longest, c.nT);
        a = b;
    }
    const int nt = (longest + 15) / 16 * 16;
    plan.max_nt = nt;
    plan.nbuf = (ring != 2 && r_lds_bytes(nroot, plan.stride, plan.max_wi, 3, nt) <= budget) ? 3 : 2;
    plan.lds_bytes = r_lds_bytes(nroot, plan.stride, plan.max_wi, plan.nbuf, nt);
    plan.n_chunks = (int)plan.chunks.size();
    plan.cs_lds_bytes = 2 * (r_image_bytes(plan.stride) + r_ro_bytes(nt)) + nt * 20 + 16 * (plan.max_wi * nroot + 1) * 8 + plan.max_tiles * 64 + 3 * 3 * 64 * 8 + 512 +
                        2 * KK * 64 * 4 + 256;
    plan.mfma_ok = plan.lds_bytes <= budget;
    plan.cs_ok = plan.mfma_ok && plan.max_tiles <= cs_tiles && plan.cs_lds_bytes <= budget && plan.n_chunks <= 8;
    return plan;
}

static long plans_checked = 0, plans_mfma = 0, plans_cs = 0;
static void check_plan(int D, int KK, const std::vector<int32_t> &i0, int window, int samples, int ring) {
    mg_primitive_model p;
    p.D = D; p.KK = KK; p.nroot = std::min(3, D); p.cshift = (4 - p.nroot) & 3; p.Dp = (D + p.cshift + 3) & ~3;
    mg_grid_plan g;
    g.T = (int32_t)i0.size();
    g.i0 = i0;
    mg_plan_chunks(p, g, samples, window, ring, 1 << 20);
    const int tiles = g.max_tiles;
    for (int cs_tiles : {tiles, tiles - 1}) {   // the chunk-stationary kernel's register bound at and one below the grid's widest window
        mg_plan_chunks(p, g, samples, window, ring, cs_tiles);
        const Plan r = restated_plan(D, KK, i0, window, samples, ring, cs_tiles);
        plans_checked++; plans_mfma += r.mfma_ok; plans_cs += r.cs_ok;
        bool ok = g.mfma_ok == r.mfma_ok && g.chunks.size() == r.chunks.size();
        if (ok && !r.chunks.empty())   // (a plan that stops early leaves the fields of the grid as they were: nothing reads them without mfma_ok ... and chunks)
            ok = g.cs_ok == r.cs_ok && g.n_chunks == r.n_chunks && g.lds_bytes == r.lds_bytes && g.cs_lds_bytes == r.cs_lds_bytes && g.max_wi == r.max_wi &&
                 g.max_nt == r.max_nt && g.nbuf == r.nbuf && g.max_tiles == r.max_tiles && g.stride == r.stride;
        for (size_t c = 0; ok && c < r.chunks.size(); c++) {
            const mg_chunk &a = g.chunks[c], &b = r.chunks[c];
            ok = a.t0 == b.t0 && a.nT == b.nT && a.rt0 == b.rt0 && a.ntiles == b.ntiles && a.imin == b.imin && a.wi == b.wi && a.rrt0 == b.rrt0 && a.nrt == b.nrt;
        }
        CHECK(ok, "plan D %d KK %d T %zu window %d samples %d ring %d cs_tiles %d: mfma %d/%d cs %d/%d chunks %zu/%zu lds %d/%d cs_lds %d/%d", D, KK, i0.size(), window,
              samples, ring, cs_tiles, g.mfma_ok, r.mfma_ok, g.cs_ok, r.cs_ok, g.chunks.size(), r.chunks.size(), g.lds_bytes, r.lds_bytes, g.cs_lds_bytes, r.cs_lds_bytes);
    }
}
static void check_planner() {
    // grids: 0, 1, 47, 48, 49 and 300 samples, i0 rising, repeated and backwards (a sample's i0 is any basis function of the primitive)
    std::vector<std::vector<int32_t>> grids;
    for (int T : {0, 1, 47, 48, 49, 300}) {
        std::vector<int32_t> rising(T), repeated(T), backwards(T);
        for (int f = 0; f < T; f++) {
            rising[f] = T > 1 ? f * 13 / (T - 1) : 2;
            repeated[f] = (f / 7) % 3 == 1 ? 5 : f * 9 / std::max(T - 1, 1);
            backwards[f] = (f % 11 == 10) ? 0 : 16 - f * 16 / std::max(T - 1, 1);
        }
        grids.push_back(rising);
        if (T > 1) { grids.push_back(repeated); grids.push_back(backwards); }
    }
    // every option combination where the channel count is at an edge of the planner (the root columns, each step of the widest window
    // that fits LDS, none fitting, both sides of the row group that must fit a wave); one combination per plan, all of them in turn, between
    const int edges[] = {1, 2, 3, 4, 5, 7, 8, 79, 80, 87, 88, 99, 100, 111, 112, 123, 124, 143, 144, 167, 168, 199, 200, 251, 252, 253, 254, 255, 256, 257, 300};
    const int windows[] = {0, 4, 5, 6, 7, 8, 9, 10, 11}, samples[] = {0, 1, 47, 48, 49}, rings[] = {0, 2};
    unsigned turn = 0;
    for (int D = 1; D <= 300; D++) {
        const bool edge = std::find(std::begin(edges), std::end(edges), D) != std::end(edges);
        for (int KK = 0; KK <= 16; KK += 2)
            for (const auto &i0 : grids) {
                if (edge && (KK == 2 || KK == 16)) {
                    for (int w : windows) for (int s : samples) for (int r : rings) check_plan(D, KK, i0, w, s, r);
                } else {
                    turn++;
                    check_plan(D, KK, i0, windows[turn % 9], samples[(turn / 9) % 5], rings[(turn / 45) % 2]);
                }
            }
    }
    CHECK(plans_mfma > 0 && plans_cs > 0 && plans_mfma < plans_checked && plans_cs < plans_mfma, "the sweep reaches %ld / %ld / %ld plans", plans_checked, plans_mfma, plans_cs);
}

// ---- refusals: status, exact text, precedence between neighbours ------------------------------------------------------------------
static long refusals_checked = 0;
template <class Edit>
static void refuse(int status, const char *text, Edit edit) {
    Desc ds(5, 7, 5, 3, 2, 6, 2, 4, false, true);
    edit(ds);
    mg_primitive_image im;   // a refused build leaves the image unused: nothing below reads it
    g_err[0] = 0;
    const int rc = mg_primitive_image_build(&ds.d, im);
    refusals_checked++;
    CHECK(rc == status && std::string(g_err) == text, "refusal: got %d '%s', expected %d '%s'", rc, g_err, status, text);
}
static void check_refusals() {
    const int INV = MG_ERR_INVALID_ARGUMENT;
    const char *t_basis = "mg_primitive_create: n_basis = 3, a cubic spline needs >= 4", *t_dims = "mg_primitive_create: n_dim/n_components/n_canonical_frames must be >= 1",
               *t_ngmm = "mg_primitive_create: n_gmm < 0", *t_ptr = "mg_primitive_create: eigen_vectors/mean_vector/knots are required",
               *t_gptr = "mg_primitive_create: gmm arrays are required when n_gmm > 0", *t_large = "mg_primitive_create: n_basis*n_dim too large",
               *t_lg = "mg_primitive_create: n_gmm_dims = 4 < n_components = 5",
               *t_time = "mg_primitive_create: a time model needs n_basis_time >= 4, eigen_vectors_time, mean_time_vector and knots_time",
               *t_knots = "mg_primitive_create: knots must be finite and non-decreasing", *t_domain = "mg_primitive_create: knot vector has an empty domain",
               *t_knots_time = "mg_primitive_create: knots_time must be finite and non-decreasing";
    // each refusal alone, at each of its conditions
    auto basis = [](Desc &s) { s.d.n_basis = 3; };
    auto dims = [](Desc &s) { s.d.n_components = 0; };
    auto ngmm = [](Desc &s) { s.d.n_gmm = -1; };
    auto ptr = [](Desc &s) { s.d.knots = nullptr; };
    auto gptr = [](Desc &s) { s.d.gmm_covars = nullptr; };
    auto large = [](Desc &s) { s.d.n_basis = 1 << 12; s.d.n_dim = 1 << 12; };   // (refused before any array is read)
    auto lg = [](Desc &s) { s.d.n_gmm_dims = 4; };
    auto timem = [](Desc &s) { s.d.n_basis_time = 3; };
    auto knots = [](Desc &s) { s.knots[5] = 0.5; };            // 0 0 0 0 1 0.5 ...
    auto domain = [](Desc &s) { for (double &t : s.knots) t = 2.0; };
    auto weight1 = [](Desc &s) { s.gw[1] = -0.25; };
    auto covar0 = [](Desc &s) { s.gc[0] = -1.0; };
    auto covar1 = [](Desc &s) { s.gc[36 + 7] = -1.0; };
    auto knots_time = [](Desc &s) { s.kt[6] = NaN; };
    refuse(INV, t_basis, basis);
    refuse(INV, t_dims, dims);
    refuse(INV, t_dims, [](Desc &s) { s.d.n_dim = 0; });
    refuse(INV, t_dims, [](Desc &s) { s.d.n_canonical_frames = 0; });
    refuse(INV, t_ngmm, ngmm);
    refuse(INV, t_ptr, ptr);
    refuse(INV, t_ptr, [](Desc &s) { s.d.eigen_vectors = nullptr; });
    refuse(INV, t_ptr, [](Desc &s) { s.d.mean_vector = nullptr; });
    refuse(INV, t_gptr, gptr);
    refuse(INV, t_gptr, [](Desc &s) { s.d.gmm_weights = nullptr; });
    refuse(INV, t_gptr, [](Desc &s) { s.d.gmm_means = nullptr; });
    refuse(INV, t_large, large);
    refuse(INV, t_lg, lg);
    refuse(INV, t_time, timem);
    refuse(INV, t_time, [](Desc &s) { s.d.n_time_components = -1; });
    refuse(INV, t_time, [](Desc &s) { s.d.eigen_vectors_time = nullptr; });
    refuse(INV, t_time, [](Desc &s) { s.d.mean_time_vector = nullptr; });
    refuse(INV, t_time, [](Desc &s) { s.d.knots_time = nullptr; });
    refuse(INV, t_knots, knots);
    refuse(INV, t_knots, [](Desc &s) { s.knots[8] = Inf; });
    refuse(INV, t_knots, [](Desc &s) { s.knots[0] = NaN; });
    refuse(INV, t_domain, domain);
    refuse(INV, "mg_primitive_create: gmm_weights[1] is negative or not finite", weight1);
    refuse(INV, "mg_primitive_create: gmm_weights[0] is negative or not finite", [](Desc &s) { s.gw[0] = Inf; });
    refuse(INV, "mg_primitive_create: gmm_weights[0] is negative or not finite", [](Desc &s) { s.gw[0] = NaN; });
    refuse(MG_ERR_NOT_POSITIVE_DEFINITE, "mg_primitive_create: gmm_covars[0] is not positive definite", covar0);
    refuse(MG_ERR_NOT_POSITIVE_DEFINITE, "mg_primitive_create: gmm_covars[1] is not positive definite", covar1);
    refuse(MG_ERR_NOT_POSITIVE_DEFINITE, "mg_primitive_create: gmm_covars[1] is not positive definite", [](Desc &s) { s.gc[36 + 14] = NaN; });
    refuse(MG_ERR_NOT_POSITIVE_DEFINITE, "mg_primitive_create: gmm_covars[0] is not positive definite", [](Desc &s) { for (int j = 0; j < 6; j++) s.gc[6 * j + 2] = s.gc[12 + j] = 0.0; });   // singular
    refuse(INV, t_knots_time, knots_time);
    refuse(INV, t_knots_time, [](Desc &s) { s.kt[5] = 0.25; });
    // precedence: of two neighbours the earlier one is reported
    refuse(INV, t_basis, [&](Desc &s) { basis(s); dims(s); });
    refuse(INV, t_dims, [&](Desc &s) { dims(s); ngmm(s); });
    refuse(INV, t_ngmm, [&](Desc &s) { ngmm(s); ptr(s); });
    refuse(INV, t_ptr, [&](Desc &s) { ptr(s); gptr(s); });
    refuse(INV, t_gptr, [&](Desc &s) { gptr(s); large(s); });
    refuse(INV, t_large, [&](Desc &s) { large(s); s.d.n_gmm_dims = 4; });
    refuse(INV, t_lg, [&](Desc &s) { lg(s); timem(s); });
    refuse(INV, t_time, [&](Desc &s) { timem(s); knots(s); });
    refuse(INV, t_knots, [&](Desc &s) { knots(s); s.knots[3] = s.knots[5]; weight1(s); });
    refuse(INV, t_domain, [&](Desc &s) { domain(s); weight1(s); covar0(s); });
    refuse(INV, "mg_primitive_create: gmm_weights[0] is negative or not finite", [&](Desc &s) { s.gw[0] = -1.0; covar0(s); });      // weight k before covariance k
    refuse(MG_ERR_NOT_POSITIVE_DEFINITE, "mg_primitive_create: gmm_covars[0] is not positive definite", [&](Desc &s) { weight1(s); covar0(s); });   // ... covariance 0 before weight 1
    refuse(INV, "mg_primitive_create: gmm_weights[1] is negative or not finite", [&](Desc &s) { weight1(s); covar1(s); knots_time(s); });
    refuse(MG_ERR_NOT_POSITIVE_DEFINITE, "mg_primitive_create: gmm_covars[1] is not positive definite", [&](Desc &s) { covar1(s); knots_time(s); });   // knots_time after both
}

int main() {
    // shapes: each axis through its edges against a small base, then the axes that meet in one index expression together
    for (int NB : {4, 5}) for (int D : {1, 2, 3, 4, 7, 8}) for (int transposed = 0; transposed < 2; transposed++) check_shape(NB, D, 5, 3, 1, 0, 0, 0, transposed != 0, D % 2 == 0);
    check_shape(5, 79, 9, 2, 1, 0, 0, 0, false, true);
    for (int L : {1, 4, 5, 8, 9, 64, 65}) check_shape(4, 7, L, 2, 0, 0, 0, 0, L % 2 == 0, true);
    for (int L : {1, 8, 9}) for (int K : {1, 3}) check_shape(5, 4, L, 3, K, 0, 4, 4, false, false);      // the mixture at n_gmm_dims = n_components
    for (int Lg : {16, 17, 64, 65}) for (int K : {1, 3}) check_shape(4, 3, 9, 1, K, Lg, 0, 0, true, K == 1);   // ... and above it: JT 1/2, KKg 0
    check_shape(4, 2, 16, 1, 1, 16, 0, 0, false, false);
    check_shape(4, 1, 64, 2, 1, 64, 0, 0, false, true);
    check_shape(4, 1, 65, 2, 1, 65, 0, 0, true, true);
    for (int F : {1, 2, 3}) for (int Lt : {0, 2}) check_shape(5, 7, 5, F, 1, Lt ? 7 : 0, Lt, 4, false, true);
    check_planner();
    check_refusals();
    std::printf("primitive_image_check: %ld shapes decoded, %ld plans (%ld LDS-staged, %ld chunk-stationary), %ld refusals, %ld checks, %ld failures\n", shapes_checked,
                plans_checked, plans_mfma, plans_cs, refusals_checked, checks, failures);
    return failures ? 1 : 0;
}
