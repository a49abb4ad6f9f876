// The host side of the one-launch cluster-tree search (mg_cluster_tree.hip) that needs no device: the LDS plans of its two
// kernels with the ladder a plan beyond the workgroup's LDS is retried by, the per-search trajectory lists flattened into what a
// workgroup reads, and the alignment record as the trajectory scorers normalise it (mg_trajectory.hip reads it from here too).
// Standard headers and the C ABI only, no HIP call; tests/native/tree_plan_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mg_hostdefs.h"

#define MG_TREE_CHUNK 64
#define MG_TREE_WAVES 4
#define MG_TREE_THREADS (MG_TREE_CHUNK * MG_TREE_WAVES)
// the dynamic LDS a plan may ask for: the workgroup's 160 KiB less the kernels' own few shared scalars (under 512 bytes), which come
// out of the same 160 KiB -- a kernel cannot opt in to more than that
#define MG_TREE_LDS_MAX (160 * 1024 - 512)
#define MG_KD_GROUP 32

// ---- the alignment record of the trajectory scorers ----
// mode 0: none, 1: previous frame (root node), 2: start pose.  al: heading (x, z) made unit or (cos, sin); landing (x, z); ref_dir (3)
// or, in start-pose mode, the height.
inline int mg_traj_align_record(const char *who, const mg_alignment_desc *al, int32_t *mode, double out[7]) {
    *mode = 0;
    for (int i = 0; i < 7; i++) out[i] = 0.0;
    if (!al) return MG_OK;
    const double hn = std::sqrt(al->heading[0] * al->heading[0] + al->heading[1] * al->heading[1]);
    if (!(hn > 0.0) || !std::isfinite(hn)) { mg_set_error("%s: heading is zero or not finite", who); return MG_ERR_INVALID_ARGUMENT; }
    if (al->joint != 0 && al->joint != MG_ALIGN_START_POSE) {
        mg_set_error("%s: only the root joint or a start pose can be the aligning reference here (joint %d)", who, al->joint);
        return MG_ERR_UNSUPPORTED;
    }
    *mode = al->joint == MG_ALIGN_START_POSE ? 2 : 1;
    out[0] = al->heading[0] / hn; out[1] = al->heading[1] / hn; out[2] = al->position[0]; out[3] = al->position[2];
    if (*mode == 2) out[4] = al->position[1];
    else { out[4] = al->ref_dir[0]; out[5] = al->ref_dir[1]; out[6] = al->ref_dir[2]; }
    return MG_OK;
}

// ---- a search's trajectory list as its workgroup reads it ----
struct mg_tree_traj_rec {
    const double *poly;   // [n_seg][4][3] + the last control point (mg_trajectory::d_poly)
    double min_u, weight;
    int32_t n_seg, G;
};
struct mg_tree_traj_desc {
    const double *E, *mean;   // the primitive's root coefficient rows, [3 NB + 4][L] and [3 NB + 4] (mg_trajectory::d_E, d_mean)
    const int32_t *i0;        // the canonical grid's basis rows: first tap [T] and weights [T][4]
    const double *w;
    double al[7];
    int32_t n, T, NB, align_mode;
    int32_t search, pad;      // 0: the reference's search, 1: the monotone walk (MG_OPT_TRAJECTORY_SEARCH)
    mg_tree_traj_rec t[MG_TREE_MAX_TRAJECTORIES];
};
// what the entry point took from a validated trajectory handle
struct mg_tree_traj_in {
    const double *poly;
    int32_t n_seg, granularity;
};

// The flat arrays' first entry of every search: off[s] .. off[s + 1] are search s's (counts NULL: no search has any).
inline int mg_tree_traj_offsets(const char *fn, int32_t n_searches, const int32_t *counts, std::vector<int64_t> &off) {
    off.assign((size_t)n_searches + 1, 0);
    for (int32_t s = 0; s < n_searches; s++) {
        const int32_t c = counts ? counts[s] : 0;
        MG_REQUIRE(c >= 0 && c <= MG_TREE_MAX_TRAJECTORIES, "%s: search %d: %d trajectories outside [0, %d]", fn, s, c, MG_TREE_MAX_TRAJECTORIES);
        off[(size_t)s + 1] = off[s] + c;
    }
    return MG_OK;
}

// Search s's records and alignment into d (E, mean, the grid, NB and search are the caller's: they come from device objects)
inline int mg_tree_traj_fill(const char *fn, int32_t s, int32_t count, const mg_tree_traj_in *in, const double *min_u, const double *weight,
                             const mg_alignment_desc *al, mg_tree_traj_desc *d) {
    MG_REQUIRE(count >= 0 && count <= MG_TREE_MAX_TRAJECTORIES, "%s: search %d: %d trajectories outside [0, %d]", fn, s, count, MG_TREE_MAX_TRAJECTORIES);
    d->n = count;
    for (int32_t i = 0; i < count; i++) {
        MG_REQUIRE(in[i].poly != nullptr && in[i].n_seg >= 1 && in[i].granularity >= 2, "%s: search %d: trajectory %d has no tables", fn, s, i);
        MG_REQUIRE(min_u[i] >= 0.0 && min_u[i] <= 1.0, "%s: search %d: trajectory %d: min_u outside [0, 1]", fn, s, i);
        MG_REQUIRE(std::isfinite(weight[i]), "%s: search %d: trajectory %d: weight not finite", fn, s, i);
        mg_tree_traj_rec &r = d->t[i];
        r.poly = in[i].poly; r.min_u = min_u[i]; r.weight = weight[i]; r.n_seg = in[i].n_seg; r.G = in[i].granularity;
    }
    return count > 0 ? mg_traj_align_record(fn, al, &d->align_mode, d->al) : MG_OK;
}

// ---- the LDS regions both kernels have ----
struct mg_tree_lds_shared {
    int n_cand, cap_local, cap_level, cap_res, wrows;
    // trajectories: the slots of the term buffer (the longest list of the call; 0: none), the root rows staged per chunk row (0: a
    // control point is formed from the latents at each tap) and the doubles of one staged polynomial table (0: read from memory)
    int traj, cp_rows, poly_doubles;
    size_t off_w, off_rs, off_cval, off_cp, off_poly, off_tv, off_cid, off_clast, off_frn, off_froff;
};

// what of a call's tables a plan keeps in LDS
struct mg_tree_staging {
    int wrows;         // rows of the set's W (0: W is read from memory)
    int cp_rows;       // root rows 3 NB + 4 of the widest primitive with trajectories
    int poly_doubles;  // 12 n_seg + 3 of the longest trajectory
};

// the heaps' bounds and the 8-byte regions a plan begins with: xs [64][L + 1] at 0, the set's W [rows][L] and bias [rows], rs, cval, then
// the trajectories' regions (root rows [cp_rows][64], polynomials [traj][poly_doubles], terms [traj][64]: nothing without trajectories).
// Returns the offset behind them.
inline size_t mg_tree_carve_head(mg_tree_lds_shared &p, int Lmax, int ncmax, int n_cand, int max_children, int max_depth, int traj, const mg_tree_staging &st) {
    p.wrows = st.wrows;
    p.n_cand = n_cand;
    p.cap_local = std::max(max_children, 1);
    p.cap_level = n_cand * std::min(n_cand, p.cap_local);
    p.cap_res = n_cand * (max_depth + 1);
    p.traj = traj;
    p.cp_rows = traj > 0 ? st.cp_rows : 0;
    p.poly_doubles = traj > 0 ? st.poly_doubles : 0;
    size_t o = (size_t)MG_TREE_CHUNK * (Lmax + 1) * 8;
    p.off_w = o;    o += (size_t)st.wrows * (Lmax + 1) * 8;
    p.off_rs = o;   o += (size_t)std::max(ncmax, 1) * MG_TREE_CHUNK * 8;
    p.off_cval = o; o += MG_TREE_CHUNK * 8;
    p.off_cp = o;   o += (size_t)p.cp_rows * MG_TREE_CHUNK * 8;
    p.off_poly = o; o += (size_t)traj * p.poly_doubles * 8;
    p.off_tv = o;   o += (size_t)traj * MG_TREE_CHUNK * 8;
    return o;
}

// the shared 4-byte regions (behind every 8-byte one): cid, clast, fr_n, fr_off
inline size_t mg_tree_carve_ints(mg_tree_lds_shared &p, size_t o) {
    p.off_cid = o;   o += MG_TREE_CHUNK * 4;
    p.off_clast = o; o += MG_TREE_CHUNK * 4;
    p.off_frn = o;   o += (size_t)p.n_cand * 4;
    p.off_froff = o; o += (size_t)(p.n_cand + 1) * 4;
    return o;
}

// ---- the FeatureClusterTree's plan: (value, node) heaps kept as two arrays ----
struct mg_tree_lds_plan {
    mg_tree_lds_shared s;
    size_t off_frv, off_lvv, off_lov, off_rev, off_lvn, off_lon, off_ren, bytes;
};

inline mg_tree_lds_plan mg_tree_plan(int Lmax, int ncmax, int n_cand, int max_children, int max_depth, int traj, const mg_tree_staging &st) {
    mg_tree_lds_plan p;
    size_t o = mg_tree_carve_head(p.s, Lmax, ncmax, n_cand, max_children, max_depth, traj, st);
    p.off_frv = o; o += (size_t)n_cand * 8;
    p.off_lvv = o; o += (size_t)p.s.cap_level * 8;
    p.off_lov = o; o += (size_t)p.s.cap_local * 8;
    p.off_rev = o; o += (size_t)p.s.cap_res * 8;
    o = mg_tree_carve_ints(p.s, o);
    p.off_lvn = o; o += (size_t)p.s.cap_level * 4;
    p.off_lon = o; o += (size_t)p.s.cap_local * 4;
    p.off_ren = o; o += (size_t)p.s.cap_res * 4;
    p.bytes = (o + 15) & ~(size_t)15;
    return p;
}

// ---- the k-means / KD ClusterTree's plan: entries of 24 bytes (value, three ints) and the KD descents' (cost, depth) ----
#define MG_TREE_HENT_BYTES 24
#define MG_TREE_KENT_BYTES 16
struct mg_kd_lds_plan {
    mg_tree_lds_shared s;
    int cap_leaf, kcap, kd_depth;
    size_t off_lo, off_lv, off_re, off_lf, off_kh, off_resv, off_kev, off_cci, off_dsoff, off_resrow, off_dfr, off_dlast, bytes;
};

inline mg_kd_lds_plan mg_kd_plan(int Lmax, int ncmax, int n_cand, int max_children, int max_depth, int max_kd_children, int kd_depth, int traj,
                                 const mg_tree_staging &st) {
    mg_kd_lds_plan p;
    p.cap_leaf = std::max(max_kd_children, 1);
    p.kd_depth = kd_depth;
    p.kcap = kd_depth + 1;
    size_t o = mg_tree_carve_head(p.s, Lmax, ncmax, n_cand, max_children, max_depth, traj, st);
    p.off_lo = o;     o += (size_t)p.s.cap_local * MG_TREE_HENT_BYTES;
    p.off_lv = o;     o += (size_t)p.s.cap_level * MG_TREE_HENT_BYTES;
    p.off_re = o;     o += (size_t)p.s.cap_res * MG_TREE_HENT_BYTES;
    p.off_lf = o;     o += (size_t)p.cap_leaf * MG_TREE_HENT_BYTES;
    p.off_kh = o;     o += (size_t)MG_KD_GROUP * p.kcap * MG_TREE_KENT_BYTES;
    p.off_resv = o;   o += MG_KD_GROUP * 8;
    p.off_kev = o;    o += (size_t)MG_KD_GROUP * p.kcap * 4;
    o = mg_tree_carve_ints(p.s, o);
    p.off_cci = o;    o += MG_TREE_CHUNK * 4;
    p.off_dsoff = o;  o += (size_t)(n_cand + 1) * 4;
    p.off_resrow = o; o += MG_KD_GROUP * 4;
    p.off_dfr = o;    o += MG_KD_GROUP * 4;
    p.off_dlast = o;  o += MG_KD_GROUP * 4;
    p.bytes = (o + 15) & ~(size_t)15;
    return p;
}

// ---- the ladder ----
// A plan beyond the workgroup's LDS is tried again with one more table read from memory, the cheapest loss first: the set's W (a
// few fma chains per row), the trajectories' polynomials (every evaluation of the closest-point search looks its segment up), the
// root rows (each tap then forms its control point from the latents: 12 chains over the latents per frame).  Without trajectories
// the ladder is the two steps it always was.  plan(staging): the kernel's plan; returns the first that fits, or the last one tried.
template <class PlanFn>
inline auto mg_tree_plan_fit(const mg_tree_staging &want, int traj, PlanFn plan) -> decltype(plan(want)) {
    mg_tree_staging st = want;
    auto lp = plan(st);
    if (lp.bytes > MG_TREE_LDS_MAX && st.wrows > 0) { st.wrows = 0; lp = plan(st); }
    if (traj > 0) {
        if (lp.bytes > MG_TREE_LDS_MAX && st.poly_doubles > 0) { st.poly_doubles = 0; lp = plan(st); }
        if (lp.bytes > MG_TREE_LDS_MAX && st.cp_rows > 0) { st.cp_rows = 0; lp = plan(st); }
    }
    return lp;
}

// ---- per-frame constraint lists inside the search (mg_cluster_tree_search_frames) ----
// A search with a list forms, per chunk, its children's joint tracks: MG_TREE_TRACK_GROUP children at a time have the control points
// of the channels the joints' chains read in LDS, [group][ncp] (ncp = NB x kept channels), with their aligning transforms [group][8];
// the tracks go to the search's slab in device memory (mg_tree_frames_scratch).  The lists' trajectory tables (local trajectories,
// trajectory sets, joint trajectories) stand in LDS behind them where they fit.  These regions lie BEHIND the kernel's own plan, so a
// call without lists has the plan, to the byte, that it always had.
#define MG_TREE_TRACK_GROUP 4
#define MG_TREE_SCRATCH_MAX ((int64_t)256 << 20)   // the slabs of one call; beyond it the call is refused
struct mg_tree_frames_want {
    int ncp;              // the most control points one child keeps, over the searches with a list (0: no search has one)
    size_t table_bytes;   // the most LDS one search's tables take (0: no tables, or tables the scorers' own bound keeps in memory)
};
struct mg_tree_frames_lds {
    int group, ncp, tables_lds;     // group 0: no lists in this call
    size_t table_bytes;
    size_t off_cp, off_al, off_tab, bytes;   // bytes: the launch's dynamic LDS, the kernel's own plan included
};

inline mg_tree_frames_lds mg_tree_frames_carve(size_t plan_bytes, int ncp, int group, size_t table_bytes) {
    mg_tree_frames_lds f;
    f.ncp = ncp;
    f.group = ncp > 0 ? group : 0;
    f.table_bytes = ncp > 0 ? table_bytes : 0;
    f.tables_lds = f.table_bytes > 0 ? 1 : 0;
    size_t o = plan_bytes;          // (a multiple of 16)
    f.off_cp = o;  o += (size_t)f.group * ncp * 8;
    f.off_al = o;  o += (size_t)f.group * 8 * 8;
    f.off_tab = o; o += f.table_bytes;
    f.bytes = (o + 15) & ~(size_t)15;
    return f;
}

// The ladder with lists: the steps there always were, in their order (W, the polynomials, the root rows), then the lists' tables read
// from memory (every look-up of the arc-length walks then waits for L2), then the track group halved down to one child (more
// barriers per chunk).  *fl: the lists' regions on the rung taken; returns the kernel's plan there.  fl->bytes > MG_TREE_LDS_MAX: refused.
template <class PlanFn>
inline auto mg_tree_frames_fit(const mg_tree_staging &want, int traj, const mg_tree_frames_want &fw, PlanFn plan, mg_tree_frames_lds *fl) -> decltype(plan(want)) {
    mg_tree_staging st = want;
    int group = MG_TREE_TRACK_GROUP;
    size_t tables = fw.table_bytes;
    auto lp = plan(st);
    auto carve = [&]() { lp = plan(st); *fl = mg_tree_frames_carve(lp.bytes, fw.ncp, group, tables); return fl->bytes; };
    if (carve() > MG_TREE_LDS_MAX && st.wrows > 0) { st.wrows = 0; carve(); }
    if (traj > 0) {
        if (fl->bytes > MG_TREE_LDS_MAX && st.poly_doubles > 0) { st.poly_doubles = 0; carve(); }
        if (fl->bytes > MG_TREE_LDS_MAX && st.cp_rows > 0) { st.cp_rows = 0; carve(); }
    }
    if (fl->bytes > MG_TREE_LDS_MAX && tables > 0) { tables = 0; carve(); }
    while (fl->bytes > MG_TREE_LDS_MAX && fw.ncp > 0 && group > 1) { group /= 2; carve(); }
    return lp;
}

// A search's slab: its chunk's tracks, request after request [64][T][joints][3], then one frame row [64][D] per joint-rotation
// constraint; doubles, rounded up to 256 bytes.
inline int64_t mg_tree_frames_scratch(int n_requests, const int32_t *T, const int32_t *joints, int n_rotations, int D) {
    int64_t doubles = 0;
    for (int q = 0; q < n_requests; q++) doubles += (int64_t)MG_TREE_CHUNK * T[q] * joints[q] * 3;
    doubles += (int64_t)MG_TREE_CHUNK * n_rotations * D;
    return (doubles * 8 + 255) & ~(int64_t)255;
}
