// The reference's cluster-tree descent (space_partitioning/feature_cluster_tree.py:129-187,
// find_best_example_excluding_search_candidates) on gfx950: one workgroup per search, the whole descent in one launch.
//
// Per level the frontier's children are scored in chunks of 64 (a lane per child, the constraints dealt over the four
// waves, summed in constraint order by the child's lane: the statements of mg_score_kernel, so a child's value has the
// bits mg_score_constraints gives for its mean).  Lane 0 keeps the three heaps in LDS and restates heapq's _siftdown /
// _siftup literally; a comparison of two equal values (where the reference's tuples fall through to comparing tree nodes
// and raise TypeError) sets MG_TREE_TIE.
//
// The k-means / KD ClusterTree's search (below) runs the same level loop.  The two kernels share the chunk scorer, the staging of
// the set's W in LDS, the mapping of a chunk's lanes to frontier nodes, heapq's push and pop, and the LDS regions all of these use.
#include "mg_internal.h"

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <vector>

#include "mg_score_device.h"
#include "mg_spline_device.h"
#include "mg_traj_device.h"
#include "mg_frame_device.h"   // the per-frame chain scorers and the joint tracks' statements (mg_cluster_tree_search_frames)
#include "mg_tree_plan.h"  // the chunk's size, the LDS plans and their ladder, the trajectory lists as a workgroup reads them

struct mg_cluster_tree {
    mg_context *ctx = nullptr;
    int32_t kind = 0;                 // 0: a FeatureClusterTree (mg_cluster_tree_create), 1: a k-means/KD ClusterTree (_create_kd)
    int32_t n_nodes = 0, dim = 0, depth = 0, max_children = 0;
    int64_t n_rows = 0;
    // the rows the search scores, [.][dim].  kind 0: every node's mean.  kind 1: the KD nodes' points, then every cluster node's mean
    double *d_points = nullptr;
    int32_t *d_child_begin = nullptr; // [n_nodes + 1]
    int32_t *d_children = nullptr;    // [n_nodes - 1] (at least one entry allocated)
    int64_t *d_first = nullptr;       // kind 0: [n_nodes]
    // kind 1: the leaf flags, the KD roots per cluster node (CSR) and the KD nodes' left / right / inner
    int32_t n_kd = 0, max_kd_children = 0, kd_depth = 0;
    int32_t *d_leaf = nullptr, *d_kd_begin = nullptr, *d_kd_roots = nullptr, *d_kd_left = nullptr, *d_kd_right = nullptr, *d_kd_inner = nullptr;
};

// what a workgroup reads of its search (one table per launch, in device memory); a feature tree leaves the KD fields NULL
struct mg_tree_search_desc {
    mg_score_args a;
    const double *points;
    const int32_t *child_begin, *children;
    const int64_t *first;
    const int32_t *leaf, *kd_begin, *kd_roots, *kd_left, *kd_right, *kd_inner;
    int32_t dim, rows, n_kd, pad;   // rows: the set's rows of W (0: not known, W is read from global memory)
    mg_tree_traj_desc tr;           // the root trajectory constraints scored behind the set (tr.n = 0: none)
};

// ---- heapq on LDS, for any entry type and tuple comparison ----
// A heap is an array of entries, or (value, node) entries kept as two arrays (12 bytes an entry).
template <class T>
__device__ __forceinline__ T mg_heap_get(const T *h, int i) { return h[i]; }
template <class T>
__device__ __forceinline__ void mg_heap_set(T *h, int i, const T &x) { h[i] = x; }
struct mg_vn {
    double v;
    int32_t n;
};
struct mg_heap_vn {
    double *v;
    int32_t *n;
};
__device__ __forceinline__ mg_vn mg_heap_get(const mg_heap_vn &h, int i) { return mg_vn{h.v[i], h.n[i]}; }
__device__ __forceinline__ void mg_heap_set(const mg_heap_vn &h, int i, const mg_vn &x) { h.v[i] = x.v; h.n[i] = x.n; }

// heapq._siftdown(heap, 0, pos) with x the entry to place
template <class H, class T, class Lt>
__device__ __forceinline__ void mg_heap_siftdown(H h, int pos, const T &x, Lt lt) {
    while (pos > 0) {
        const int parent = (pos - 1) >> 1;
        if (!lt(x, mg_heap_get(h, parent))) break;
        mg_heap_set(h, pos, mg_heap_get(h, parent));
        pos = parent;
    }
    mg_heap_set(h, pos, x);
}

// heapq.heappush: append, then _siftdown(heap, 0, len - 1)
template <class H, class T, class Lt>
__device__ __forceinline__ void mg_heappush(H h, int &len, int cap, const T &x, Lt lt, int &flags) {
    if (len >= cap) { flags |= MG_TREE_OVERFLOW; return; }
    mg_heap_siftdown(h, len++, x, lt);
}

// The comparisons of heapq.heappop (the last entry to the root, _siftup, _siftdown) for what lt records of them (a tie): the
// answer is the root read before.
template <class H, class Lt>
__device__ __forceinline__ void mg_heappop_compares(H h, int len, Lt lt) {
    if (len <= 1) return;
    const int end = len - 1;
    const auto x = mg_heap_get(h, end);
    int pos = 0, child = 1;
    while (child < end) {
        const int right = child + 1;
        if (right < end && !lt(mg_heap_get(h, child), mg_heap_get(h, right))) child = right;
        mg_heap_set(h, pos, mg_heap_get(h, child));
        pos = child;
        child = 2 * pos + 1;
    }
    mg_heap_siftdown(h, pos, x, lt);
}

// ---- the LDS regions (mg_tree_plan.h), and the routines on them, that both kernels have ----
struct mg_tree_lds {
    double *xs, *rs, *cval;   // the scorer's: the chunk's rows, the residuals [constraint][lane], the values
    int32_t *cid;             // the chunk's rows of the points table
    const double *Wm, *Bm;   // the set's W and bias as the scorer reads them
};

// The shared regions of a workgroup, with the set's keyframe matrices staged in LDS where the plan has room for them: a level
// scores a handful of children, one wave per constraint, and every step of the scorer's fma chains would otherwise wait for a
// load from memory.  Same values, same order: the same bits.  (The caller's first __syncthreads publishes them.)
__device__ __forceinline__ mg_tree_lds mg_tree_lds_of(unsigned char *smem, const mg_tree_lds_shared &p, const mg_score_args &a, int rows, int tid) {
    mg_tree_lds s;
    s.xs = (double *)smem;
    s.rs = (double *)(smem + p.off_rs);
    s.cval = (double *)(smem + p.off_cval);
    s.cid = (int32_t *)(smem + p.off_cid);
    s.Wm = a.W;
    s.Bm = a.bias;
    if (p.wrows > 0 && rows > 0) {
        double *wl = (double *)(smem + p.off_w), *bl = wl + (size_t)p.wrows * a.L;
        for (int i = tid; i < rows * a.L; i += MG_TREE_THREADS) wl[i] = a.W[i];
        for (int i = tid; i < rows; i += MG_TREE_THREADS) bl[i] = a.bias[i];
        s.Wm = wl;
        s.Bm = bl;
    }
    return s;
}

// Entry e of a list that frontier node f's entries fill from off[f] to off[f + 1] (n nodes): its f, and whether e is f's last
__device__ __forceinline__ int mg_tree_owner(const int32_t *off, int n, int e, int32_t &last) {
    int f = 0;
    while (f + 1 < n && off[f + 1] <= e) f++;
    last = (e == off[f + 1] - 1);
    return f;
}

// cval[j] = the objective of row cid[j] of P for j < cnt (a row < 0 scores zeros, and its value is not used): a lane per row,
// the constraints dealt over the four waves, summed in constraint order by the row's lane.  The statements of mg_score_kernel, so
// a value has the bits mg_score_constraints gives for that row.  Called by every thread of the workgroup, cid published.
__device__ void mg_tree_score_chunk(const mg_score_args &a, const mg_tree_lds &s, const double *__restrict__ P, int dim, int cnt, int tid, int lane,
                                    int wave) {
    const int L = a.L, xs_stride = L + 1;
    for (int e = tid; e < MG_TREE_CHUNK * L; e += MG_TREE_THREADS) {
        const int c = e / L, i = e - c * L;
        s.xs[c * xs_stride + i] = (c < cnt && s.cid[c] >= 0) ? P[(size_t)s.cid[c] * dim + i] : 0.0;
    }
    __syncthreads();
    const double *x = s.xs + lane * xs_stride;
    for (int c = wave; c < a.n; c += MG_TREE_WAVES) {
        auto channel = [&](int row) {   // mg_score_kernel's fma chain over k from the bias
            const double *wr = s.Wm + (size_t)row * L;
            double acc = s.Bm[row];
            for (int k = 0; k < L; k++) acc = fma(wr[k], x[k], acc);
            return acc;
        };
        s.rs[c * MG_TREE_CHUNK + lane] = mg_constraint_residual(a, c, channel, 0);
    }
    __syncthreads();
    if (tid < cnt) {
        double err = 0.0;
        for (int c = 0; c < a.n; c++) err += s.rs[c * MG_TREE_CHUNK + tid];
        s.cval[tid] = err;
    }
    __syncthreads();
}

// ---- root trajectory constraints behind the set (mg_cluster_tree_search_trajectories) ----
struct mg_tree_traj_lds {
    double *cp;           // the chunk's root coefficient rows [3 NB + 4][64], or NULL: formed from the latents at each tap
    const double *poly;   // the search's polynomial tables staged one behind the other, or NULL: read from memory
    int poly_stride;
    double *tv;           // the terms [trajectory][lane]
};

// A workgroup's trajectory regions, the polynomial tables staged where the plan has room for them: every evaluation of the
// closest-point search looks its segment up, a chain of dependent reads.  (The caller's first __syncthreads publishes them.)
__device__ __forceinline__ mg_tree_traj_lds mg_tree_traj_lds_of(unsigned char *smem, const mg_tree_lds_shared &p, const mg_tree_traj_desc *__restrict__ tr, int tid) {
    mg_tree_traj_lds t;
    t.cp = p.cp_rows > 0 ? (double *)(smem + p.off_cp) : nullptr;
    t.tv = (double *)(smem + p.off_tv);
    t.poly = nullptr;
    t.poly_stride = p.poly_doubles;
    if (p.poly_doubles > 0) {
        double *pl = (double *)(smem + p.off_poly);
        for (int i = 0; i < tr->n; i++) {
            const double *src = tr->t[i].poly;
            const int m = tr->t[i].n_seg * 12 + 3;
            for (int e = tid; e < m; e += MG_TREE_THREADS) pl[(size_t)i * p.poly_doubles + e] = src[e];
        }
        t.poly = pl;
    }
    return t;
}

// cval[j] += weight x the average distance of row j's root path from each of the search's trajectories, in list order: what
// mg_score_trajectory(..., accumulate = 1) adds to mg_score_constraints' value, statement for statement (mg_trajectory.hip) --
// the root's coefficient rows as fma chains over the row's latents from the means, four taps per channel and frame on the
// canonical grid, the aligning transform from the first control point, the closest-point search of mg_traj_device.h with the
// bound carried from frame to frame, the sum over the frames in frame order, one division.  A lane per row; the root rows (the
// same for every trajectory: they are the primitive's) are formed once per chunk by all four waves, then wave i walks trajectory i.
// Lanes without a row walk zeros in the monotone search (its wave-wide help wants every lane) and nothing in the reference's.
// Called by every thread of the workgroup behind mg_tree_score_chunk, whose xs it reads.
__device__ void mg_tree_score_chunk_trajectories(const mg_tree_traj_desc *__restrict__ tr, const mg_tree_lds &s, const mg_tree_traj_lds &t, int L, int cnt,
                                                 int tid, int lane, int wave) {
    const int xs_stride = L + 1, NB = tr->NB, T = tr->T, n = tr->n, align_mode = tr->align_mode;
    const double *__restrict__ E = tr->E;
    const double *__restrict__ mean = tr->mean;
    const double *x = s.xs + lane * xs_stride;
    auto row = [&](int r) { return mg_control_point(mean[r], E + (size_t)r * L, 1, L, [&](int k) { return x[k]; }); };
    if (t.cp) {
        const int rows = NB * 3 + 4;
        for (int r = wave; r < rows; r += MG_TREE_WAVES) t.cp[r * MG_TREE_CHUNK + lane] = row(r);
        __syncthreads();
    }
    for (int i = wave; i < n; i += MG_TREE_WAVES) {   // (uniform over the wave)
        const double *poly = t.poly ? t.poly + (size_t)i * t.poly_stride : tr->t[i].poly;
        const int n_seg = tr->t[i].n_seg, G = tr->t[i].G;
        const double min_u0 = tr->t[i].min_u, weight = tr->t[i].weight;
        auto root = [&](int r) { return t.cp ? t.cp[r * MG_TREE_CHUNK + lane] : row(r); };
        const mg_align2d al = mg_traj_alignment_of(align_mode, tr->al, NB, nullptr, root);
        auto position = [&](int f, double *q) {        // the row's root position in frame f, aligned
            const int i0 = tr->i0[f];
            const double *w = tr->w + 4 * (size_t)f;
            if (t.cp) {
#pragma unroll
                for (int d = 0; d < 3; d++) q[d] = mg_taps4(w, t.cp + (i0 * 3 + d) * MG_TREE_CHUNK + lane, 3 * MG_TREE_CHUNK);
            } else {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const double c[4] = {row(i0 * 3 + d), row((i0 + 1) * 3 + d), row((i0 + 2) * 3 + d), row((i0 + 3) * 3 + d)};
                    q[d] = mg_taps4(w, c, 1);
                }
            }
            if (align_mode != 0) mg_align_position(al, q[0], q[1], q[2]);
        };
        const bool valid = lane < cnt && s.cid[lane] >= 0;
        double sum = 0.0;
        if (tr->search == 0) {
            mg_traj_chain(poly, n_seg, valid ? T : 0, min_u0, position, [&](int f, double dist, double u, int trips) { sum += dist; });
        } else {
            const double invG = 1.0 / (double)G;
            double min_u = min_u0;
            for (int f = 0; f < T; f++) {
                double q[3];
                position(f, q);
                sum += mg_traj_closest_dist<true>(poly, n_seg, G, invG, &min_u, q);   // (every lane of the wave is here: the help is legal)
            }
        }
        t.tv[i * MG_TREE_CHUNK + lane] = weight * (T > 0 ? sum / (double)T : 0.0);
    }
    __syncthreads();
    if (tid < cnt) {
        double err = s.cval[tid];
        for (int i = 0; i < n; i++) err = err + t.tv[i * MG_TREE_CHUNK + tid];
        s.cval[tid] = err;
    }
    __syncthreads();
}

// ---- per-frame constraint lists behind the set and the trajectories (mg_cluster_tree_search_frames) ----
// what a workgroup reads of its search's list (a second table of the launch, in device memory)
struct mg_tree_frames_desc {
    mg_track_args tk;                            // the tracks: out[q] = request q's part of the search's slab (no latents: the chunk's rows are in LDS)
    int32_t n, pad;                              // constraints in the list (0: the search has none)
    mg_fc_args c[MG_FRAME_LIST_MAX];             // the chain scorers' arguments, their tracks in the slab, B = the chunk
    const int32_t *rot_i0[MG_FRAME_LIST_MAX];    // MG_FRAME_JOINT_ROTATION: the basis row of its frame index (a one-sample grid), else NULL
    const double *rot_w[MG_FRAME_LIST_MAX];
    double *rot_out[MG_FRAME_LIST_MAX];          // ... and its frame rows [64][D] in the slab (the quaternion's four channels are written)
};
// a launch's view of the lists: this workgroup's entry, the lists' LDS regions, the dynamic LDS
struct mg_tree_frames_ctx {
    const mg_tree_frames_desc *fd;
    mg_tree_frames_lds fl;
    unsigned char *smem;
};

// cval[j] += the search's per-frame constraints for row j, in list order: what mg_joint_tracks + mg_score_frame_constraints (or, for a
// joint rotation, mg_back_project_frames_f64 + mg_align_frames + mg_score_frame_constraint) add behind mg_score_constraints and
// mg_score_trajectory in candidate_scoring.errors_of_samples, with their statements (mg_frame_device.h).
//   1. the chunk's tracks, fl.group children at a time: the control points of the kept channels as fma chains over the child's latents
//      from the mean, its aligning transform from the first of them, then per (time, joint) four taps per channel and the chain --
//      into the search's slab; a joint rotation's quaternion at its frame index likewise (sixteen chains per child).
//   2. behind a barrier a lane per child runs the chain scorers over its tracks and adds the weighted errors to its value.
// Every loop is bounded by what the entry point validated: cnt <= 64, the grids' T, the plan's joints and chain lengths, the list's n,
// the tables' n_seg and granularity.  Called by every thread of the workgroup behind mg_tree_score_chunk[_trajectories], whose xs it reads.
__device__ void mg_tree_score_chunk_frames(const mg_tree_frames_ctx &fx, const mg_tree_lds &s, int L, int cnt, int tid) {
    const mg_tree_frames_desc *__restrict__ fd = fx.fd;
    const mg_track_args &a = fd->tk;
    const int xs_stride = L + 1, nc = a.n_chan, ncp = a.NB * nc, D = a.D, G = fx.fl.group, n = fd->n;
    const size_t R = (size_t)a.R;
    double *cp_all = (double *)(fx.smem + fx.fl.off_cp), *al_all = (double *)(fx.smem + fx.fl.off_al);
    const double *tables = (const double *)(fx.smem + fx.fl.off_tab);
    const int32_t *__restrict__ slot = a.slot;
    auto slot_of = [&](int ch) { return slot[ch]; };
    const bool aligned = a.align_mode != 0;
    for (int g0 = 0; g0 < cnt; g0 += G) {
        const int n_here = min(G, cnt - g0);
        for (int e = tid; e < n_here * ncp; e += MG_TREE_THREADS) {
            const int c = e / ncp, r = e - c * ncp, i = r / nc, q = r - i * nc;
            const int row = i * D + a.chan[q];
            const double *x = s.xs + (g0 + c) * xs_stride;
            cp_all[e] = mg_control_point(a.mean[row], a.Et64 + row, R, L, [&](int k) { return x[k]; });
        }
        __syncthreads();
        if (tid < n_here && aligned) mg_track_alignment(a, cp_all + (size_t)tid * ncp, slot_of, al_all + tid * 8);
        __syncthreads();
        for (int rq = 0; rq < a.n_requests; rq++) {
            const int T = a.T[rq], j0 = a.req_joint0[rq], J = a.req_joint0[rq + 1] - j0;
            const int32_t *i0 = a.i0[rq];
            const double *w = a.w[rq];
            for (int ce = tid; ce < n_here * T * J; ce += MG_TREE_THREADS) {
                const int c = ce / (T * J), e = ce - c * (T * J), f = e / J, j = e - f * J;
                double *out = a.out[rq] + (size_t)(g0 + c) * T * J * 3;
                double p[3];
                mg_track_point(cp_all + (size_t)c * ncp, nc, slot_of, i0[f], w + 4 * (size_t)f, a.records + (size_t)(j0 + j) * MG_TRACK_REC, aligned,
                               al_all + c * 8, D, p);
                out[(size_t)e * 3] = p[0]; out[(size_t)e * 3 + 1] = p[1]; out[(size_t)e * 3 + 2] = p[2];
            }
        }
        for (int e = tid; e < n_here * n; e += MG_TREE_THREADS) {   // the joint rotations' quaternions, from the latents
            const int c = e / n, i = e - c * n;
            if (!fd->rot_i0[i]) continue;
            const int qc = fd->c[i].quat_channel, i0 = fd->rot_i0[i][0];
            const double *x = s.xs + (g0 + c) * xs_stride, *al = al_all + c * 8;
            double q[4];
            for (int k = 0; k < 4; k++) {
                double v[4];
                for (int t = 0; t < 4; t++) {
                    const size_t row = (size_t)(i0 + t) * D + qc + k;
                    v[t] = mg_control_point(a.mean[row], a.Et64 + row, R, L, [&](int kk) { return x[kk]; });
                }
                q[k] = mg_taps4(fd->rot_w[i], v, 1);
            }
            if (aligned && qc == 3 && D >= 7) mg_align_root_quat(al[5], al[6], q[0], q[1], q[2], q[3]);
            double *row = fd->rot_out[i] + (size_t)(g0 + c) * D + qc;
            row[0] = q[0]; row[1] = q[1]; row[2] = q[2]; row[3] = q[3];
        }
        __syncthreads();   // the group's control points are read: the next group overwrites them; the slab's rows are written
    }
    if (tid < cnt && s.cid[tid] >= 0) {
        double err = s.cval[tid];
        for (int i = 0; i < n; i++)
            err = err + (fx.fl.tables_lds ? mg_fc_evaluate<true>(fd->c[i], tid, tables) : mg_fc_evaluate<false>(fd->c[i], tid, nullptr));
        s.cval[tid] = err;
    }
    __syncthreads();
}

// the lists' trajectory tables into LDS where the plan has room for them (the caller's first __syncthreads publishes them)
__device__ __forceinline__ void mg_tree_stage_frame_tables(const mg_tree_frames_ctx &fx, int tid) {
    if (!fx.fl.tables_lds) return;
    double *tables = (double *)(fx.smem + fx.fl.off_tab);
    for (int i = 0; i < fx.fd->n; i++) mg_fc_stage_tables(fx.fd->c[i], tables, tid, MG_TREE_THREADS);
}

// The chunk scorer of both kernels: the set's value, then (a launch with trajectories, TRAJ) the search's trajectory terms, then (a
// launch with per-frame lists, FRAMES) the search's list.  Without either this is mg_tree_score_chunk alone: the kernels a call
// without trajectories always launched.
template <bool TRAJ, bool FRAMES>
__device__ __forceinline__ void mg_tree_score(const mg_tree_search_desc *__restrict__ d, const mg_score_args &a, const mg_tree_lds &s, const mg_tree_traj_lds &t,
                                              const mg_tree_frames_ctx &fx, const double *__restrict__ P, int dim, int cnt, int tid, int lane, int wave) {
    mg_tree_score_chunk(a, s, P, dim, cnt, tid, lane, wave);
    if constexpr (TRAJ) {
        if (d->tr.n > 0) mg_tree_score_chunk_trajectories(&d->tr, s, t, a.L, cnt, tid, lane, wave);   // (uniform over the workgroup)
    }
    if constexpr (FRAMES) {
        if (fx.fd->n > 0) mg_tree_score_chunk_frames(fx, s, a.L, cnt, tid);                           // (uniform over the workgroup)
    }
}

// ---- the FeatureClusterTree's search ----
// (the body of the kernels below: mg_tree_search_kernel<TRAJ> is the launch there always was, mg_tree_search_frames_kernel adds the lists)
template <bool TRAJ, bool FRAMES>
__device__ __forceinline__ void mg_tree_search_body(const mg_tree_search_desc *__restrict__ tab, const mg_tree_lds_plan &lp, mg_tree_search_record *__restrict__ rec,
                                                    const mg_tree_frames_desc *__restrict__ ftab, const mg_tree_frames_lds &fl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_fr_len, s_total;
    __shared__ long long s_evals;
    const mg_tree_search_desc *d = tab + blockIdx.x;
    const mg_score_args a = d->a;
    const double *__restrict__ means = d->points;
    const int32_t *__restrict__ cb = d->child_begin;
    const int32_t *__restrict__ ch = d->children;
    const int dim = d->dim, n_cand = lp.s.n_cand;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const mg_tree_lds s = mg_tree_lds_of(smem, lp.s, a, d->rows, tid);
    mg_tree_traj_lds tl = {};
    if constexpr (TRAJ) tl = mg_tree_traj_lds_of(smem, lp.s, &d->tr, tid);
    mg_tree_frames_ctx fx = {};
    if constexpr (FRAMES) { fx = mg_tree_frames_ctx{ftab + blockIdx.x, fl, smem}; mg_tree_stage_frame_tables(fx, tid); }
    // (cid from the plan, not s.cid: read back out of the struct it costs the KD kernel two VGPRs)
    int32_t *cid = (int32_t *)(smem + lp.s.off_cid), *clast = (int32_t *)(smem + lp.s.off_clast);
    int32_t *fr_n = (int32_t *)(smem + lp.s.off_frn), *fr_off = (int32_t *)(smem + lp.s.off_froff);
    double *fr_v = (double *)(smem + lp.off_frv);
    const mg_heap_vn lv = {(double *)(smem + lp.off_lvv), (int32_t *)(smem + lp.off_lvn)};   // the level's new_candidates
    const mg_heap_vn lo = {(double *)(smem + lp.off_lov), (int32_t *)(smem + lp.off_lon)};   // a node's result_queue
    const mg_heap_vn re = {(double *)(smem + lp.off_rev), (int32_t *)(smem + lp.off_ren)};   // results
    // lane 0's heap state (only thread 0 touches the heaps)
    int flags = 0, lv_len = 0, lo_len = 0, res_len = 0;
    // heapq's comparison of (value, node) tuples whose values differ: value < value.  Equal values would compare the nodes.
    auto lt = [&flags](const mg_vn &x, const mg_vn &y) {
        if (x.v == y.v) flags |= MG_TREE_TIE;
        return x.v < y.v;
    };
    if (tid == 0) {
        s_fr_len = 1; fr_v[0] = INFINITY; fr_n[0] = 0;   // candidates = [(np.inf, self)]
        s_evals = 0;
    }
    __syncthreads();
    // a validated tree ends after depth + 1 levels; the bound only keeps a wave from spinning on anything else
    for (int level = 0; level <= MG_TREE_MAX_DEPTH + 1; level++) {
        const int fr_len = s_fr_len;
        if (fr_len == 0) break;
        if (tid == 0) {
            int tot = 0;
            for (int f = 0; f < fr_len; f++) {
                const int node = fr_n[f];
                const int nc = cb[node + 1] - cb[node];
                fr_off[f] = tot;
                if (nc == 0) mg_heappush(re, res_len, lp.s.cap_res, mg_vn{fr_v[f], node}, lt, flags);   // a leaf: onto results
                tot += nc;
            }
            fr_off[fr_len] = tot;
            s_total = tot;
            s_evals += tot;
            lv_len = 0;
            lo_len = 0;
        }
        __syncthreads();
        const int tot = s_total;
        for (int c0 = 0; c0 < tot; c0 += MG_TREE_CHUNK) {
            const int cnt = min(MG_TREE_CHUNK, tot - c0);
            if (tid < cnt) {   // entry e of the level's list: child k of frontier node f
                const int e = c0 + tid;
                const int f = mg_tree_owner(fr_off, fr_len, e, clast[tid]);
                cid[tid] = ch[cb[fr_n[f]] + (e - fr_off[f])];
            }
            __syncthreads();
            mg_tree_score<TRAJ, FRAMES>(d, a, s, tl, fx, means, dim, cnt, tid, lane, wave);
            if (tid == 0) {
                for (int j = 0; j < cnt; j++) {
                    mg_heappush(lo, lo_len, lp.s.cap_local, mg_vn{s.cval[j], cid[j]}, lt, flags);   // _find_best_cluster_candidates
                    if (clast[j]) {   // the node's children are all in: result_queue[:n_candidates] onto the level's heap
                        const int m = min(n_cand, lo_len);
                        for (int i = 0; i < m; i++) mg_heappush(lv, lv_len, lp.s.cap_level, mg_heap_get(lo, i), lt, flags);
                        lo_len = 0;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {   // candidates = new_candidates[:n_candidates]
            const int m = min(n_cand, lv_len);
            for (int i = 0; i < m; i++) { fr_v[i] = lv.v[i]; fr_n[i] = lv.n[i]; }
            s_fr_len = m;
        }
        __syncthreads();
    }
    if (tid == 0) {
        mg_tree_search_record r;
        if (s_fr_len != 0) flags |= MG_TREE_OVERFLOW;   // (the level bound ended the loop)
        if (res_len == 0) {
            flags |= MG_TREE_NO_RESULT;
            r.leaf = 0; r.value = INFINITY; r.row = d->first[0];
        } else {
            r.leaf = re.n[0]; r.value = re.v[0]; r.row = d->first[re.n[0]];
            mg_heappop_compares(re, res_len, lt);
        }
        r.flags = flags;
        r.evaluations = s_evals;
        rec[blockIdx.x] = r;
    }
}

template <bool TRAJ>
__global__ __launch_bounds__(MG_TREE_THREADS) void mg_tree_search_kernel(const mg_tree_search_desc *__restrict__ tab, mg_tree_lds_plan lp,
                                                                         mg_tree_search_record *__restrict__ rec) {
    mg_tree_search_body<TRAJ, false>(tab, lp, rec, nullptr, mg_tree_frames_lds{});
}
// ... with per-frame lists (and trajectories, where a search has them): ftab[search], the lists' regions behind the plan's
__global__ __launch_bounds__(MG_TREE_THREADS) void mg_tree_search_frames_kernel(const mg_tree_search_desc *__restrict__ tab,
                                                                                const mg_tree_frames_desc *__restrict__ ftab, mg_tree_lds_plan lp,
                                                                                mg_tree_frames_lds fl, mg_tree_search_record *__restrict__ rec) {
    mg_tree_search_body<true, true>(tab, lp, rec, ftab, fl);
}

// ---------------------------------------------------------------------------------------------------------------
// The k-means / KD ClusterTree (reference space_partitioning/cluster_tree.py:117-149, cluster_tree_node.py:63-79,113-138,
// kdtree.py:132-164,233-250): the same level loop, and after each level's k-means children every frontier leaf's
// KD descents, in the same launch.  The descents of a level run side by side in groups of MG_KD_GROUP, one lane per
// descent for its heap and two score slots per descent per step (right child, then left), so a step of the whole group
// is one chunk of 64 scores.  Every value is scored from the points table with mg_score_kernel's statements.
//
// The heaps compare tuples as the reference's do:
//   a node's children   (value, cluster_index, node)  cluster_index unique within the node: never raises
//   new_candidates      (value, idx, node)            equal value and idx compare nodes: MG_TREE_TIE (TypeError)
//   a leaf's KD results (value, point list)           lists compare lexicographically
//   results             (value, c_idx, point list)
//   a KD descent        (cost, depth)
// ---------------------------------------------------------------------------------------------------------------
struct mg_hent {   // a heap entry: value, then up to three ints (what each heap compares and carries)
    double v;
    int32_t a, b, c, pad;
};
struct mg_kent {   // a KD descent's (cost, depth)
    double v;
    int32_t d, pad;
};

static_assert(sizeof(mg_hent) == MG_TREE_HENT_BYTES && sizeof(mg_kent) == MG_TREE_KENT_BYTES, "mg_kd_plan sizes the heaps by these");

// Python's `list < list` of two rows of the points table: the first position whose items differ decides
__device__ bool mg_kd_rows_lt(const double *__restrict__ P, int dim, int r, int s) {
    const double *x = P + (size_t)r * dim, *y = P + (size_t)s * dim;
    for (int k = 0; k < dim; k++)
        if (!(x[k] == y[k])) return x[k] < y[k];
    return false;
}

template <bool TRAJ, bool FRAMES>
__device__ __forceinline__ void mg_kd_tree_search_body(const mg_tree_search_desc *__restrict__ tab, const mg_kd_lds_plan &lp, mg_tree_search_record *__restrict__ rec,
                                                       const mg_tree_frames_desc *__restrict__ ftab, const mg_tree_frames_lds &fl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_fr_len, s_eff, s_total, s_ndesc, s_stop, s_kflags;
    __shared__ long long s_evals;
    const mg_tree_search_desc *d = tab + blockIdx.x;
    const mg_score_args a = d->a;
    const double *__restrict__ P = d->points;
    const int32_t *__restrict__ cb = d->child_begin;
    const int32_t *__restrict__ ch = d->children;
    const int32_t *__restrict__ isleaf = d->leaf;
    const int32_t *__restrict__ kb = d->kd_begin;
    const int32_t *__restrict__ kr = d->kd_roots;
    const int32_t *__restrict__ kl = d->kd_left;
    const int32_t *__restrict__ krt = d->kd_right;
    const int32_t *__restrict__ kin = d->kd_inner;
    const int dim = d->dim, n_kd = d->n_kd, n_cand = lp.s.n_cand, kcap = lp.kcap;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const mg_tree_lds s = mg_tree_lds_of(smem, lp.s, a, d->rows, tid);
    mg_tree_traj_lds tl = {};
    if constexpr (TRAJ) tl = mg_tree_traj_lds_of(smem, lp.s, &d->tr, tid);
    mg_tree_frames_ctx fx = {};
    if constexpr (FRAMES) { fx = mg_tree_frames_ctx{ftab + blockIdx.x, fl, smem}; mg_tree_stage_frame_tables(fx, tid); }
    double *cval = s.cval;
    // (cid from the plan, not s.cid: read back out of the struct it costs the KD kernel two VGPRs)
    int32_t *cid = (int32_t *)(smem + lp.s.off_cid), *clast = (int32_t *)(smem + lp.s.off_clast);
    int32_t *fr_n = (int32_t *)(smem + lp.s.off_frn), *fr_off = (int32_t *)(smem + lp.s.off_froff);
    mg_hent *lo = (mg_hent *)(smem + lp.off_lo);
    mg_hent *lv = (mg_hent *)(smem + lp.off_lv);
    mg_hent *re = (mg_hent *)(smem + lp.off_re);
    mg_hent *lf = (mg_hent *)(smem + lp.off_lf);
    mg_kent *kh_all = (mg_kent *)(smem + lp.off_kh);
    double *res_v = (double *)(smem + lp.off_resv);
    int32_t *kev_all = (int32_t *)(smem + lp.off_kev);
    int32_t *cci = (int32_t *)(smem + lp.off_cci);
    int32_t *ds_off = (int32_t *)(smem + lp.off_dsoff);
    int32_t *res_row = (int32_t *)(smem + lp.off_resrow);
    int32_t *dfr = (int32_t *)(smem + lp.off_dfr);
    int32_t *dlast = (int32_t *)(smem + lp.off_dlast);
    // (value, cluster_index, node): the indices differ within a node
    auto lt_local = [](const mg_hent &x, const mg_hent &y) { return x.v == y.v ? x.a < y.a : x.v < y.v; };
    // thread 0's heap state
    int flags = 0, lv_len = 0, lo_len = 0, re_len = 0, lf_len = 0;
    auto lt_level = [&flags](const mg_hent &x, const mg_hent &y) {   // (value, idx, node): equal idx compare the nodes
        if (x.v == y.v) {
            if (x.a == y.a) { flags |= MG_TREE_TIE; return false; }
            return x.a < y.a;
        }
        return x.v < y.v;
    };
    auto lt_leaf = [&](const mg_hent &x, const mg_hent &y) { return x.v == y.v ? mg_kd_rows_lt(P, dim, x.b, y.b) : x.v < y.v; };
    auto lt_res = [&](const mg_hent &x, const mg_hent &y) {   // (value, c_idx, point list)
        if (x.v == y.v) return x.a == y.a ? mg_kd_rows_lt(P, dim, x.b, y.b) : x.a < y.a;
        return x.v < y.v;
    };
    auto lt_kd = [](const mg_kent &x, const mg_kent &y) { return x.v == y.v ? x.d < y.d : x.v < y.v; };
    if (tid == 0) {
        s_fr_len = 1; fr_n[0] = 0;   // candidates = [(np.inf, 0, self.root)]
        s_evals = 0; s_stop = 0; s_kflags = 0;
    }
    __syncthreads();
    for (int level = 0; level <= MG_TREE_MAX_DEPTH + 1; level++) {
        const int fr_len = s_fr_len;
        if (fr_len == 0) break;
        if (tid == 0) {
            int tot = 0, nd = 0, eff = fr_len, stop = 0;
            for (int f = 0; f < fr_len; f++) {
                const int node = fr_n[f];
                const int nk = kb[node + 1] - kb[node];
                fr_off[f] = tot;
                ds_off[f] = nd;
                if (!isleaf[node]) {
                    if (nk > 0) { stop = 1; eff = f; break; }   // KDTreeWrapper children have no .mean: AttributeError
                    tot += cb[node + 1] - cb[node];
                } else {
                    nd += nk > 0 ? nk : 1;                       // a leaf without children scores its mean
                }
            }
            fr_off[eff] = tot;
            ds_off[eff] = nd;
            s_eff = eff;
            s_total = tot;
            s_ndesc = stop ? 0 : nd;
            s_stop = stop;
            s_evals += tot;
            lv_len = 0;
            lo_len = 0;
        }
        __syncthreads();
        const int eff = s_eff, tot = s_total, nd = s_ndesc;
        // the k-means children of the frontier's inner nodes (find_best_cluster_candidates)
        for (int c0 = 0; c0 < tot; c0 += MG_TREE_CHUNK) {
            const int cnt = min(MG_TREE_CHUNK, tot - c0);
            if (tid < cnt) {
                const int e = c0 + tid;
                const int f = mg_tree_owner(fr_off, eff, e, clast[tid]);
                cci[tid] = e - fr_off[f];
                cid[tid] = n_kd + ch[cb[fr_n[f]] + (e - fr_off[f])];
            }
            __syncthreads();
            mg_tree_score<TRAJ, FRAMES>(d, a, s, tl, fx, P, dim, cnt, tid, lane, wave);
            if (tid == 0) {
                for (int j = 0; j < cnt; j++) {
                    mg_hent x;
                    x.v = cval[j]; x.a = cci[j]; x.b = 0; x.c = cid[j] - n_kd; x.pad = 0;
                    mg_heappush(lo, lo_len, lp.s.cap_local, x, lt_local, flags);
                    if (clast[j]) {   // result_queue[:n_candidates] onto new_candidates as (value, idx, node)
                        const int m = min(n_cand, lo_len);
                        for (int i = 0; i < m; i++) {
                            mg_hent y;   // (built field by field: a copy of the whole entry went through scratch)
                            y.v = lo[i].v; y.a = i; y.b = lo[i].b; y.c = lo[i].c; y.pad = 0;
                            mg_heappush(lv, lv_len, lp.s.cap_level, y, lt_level, flags);
                        }
                        lo_len = 0;
                    }
                }
            }
            __syncthreads();
        }
        if (s_stop) break;
        // the leaves' KD descents (find_best_example), MG_KD_GROUP at a time
        for (int g0 = 0; g0 < nd; g0 += MG_KD_GROUP) {
            const int gcnt = min(MG_KD_GROUP, nd - g0);
            const int slot = tid < MG_KD_GROUP ? tid : 0;   // (only lanes < gcnt touch their heap)
            mg_kent *kh = kh_all + (size_t)slot * kcap;
            int32_t *kev = kev_all + (size_t)slot * kcap;
            int cur = -1, klen = 0, depth = 0, kflags = 0;
            if (tid < gcnt) {
                const int e = g0 + tid;
                const int f = mg_tree_owner(ds_off, eff, e, dlast[tid]);
                const int node = fr_n[f];
                const int nk = kb[node + 1] - kb[node];
                const int start = nk > 0 ? kr[kb[node] + (e - ds_off[f])] : n_kd + node;
                cur = nk > 0 ? start : -1;
                cid[tid] = start;
                dfr[tid] = f;
            }
            __syncthreads();
            mg_tree_score<TRAJ, FRAMES>(d, a, s, tl, fx, P, dim, gcnt, tid, lane, wave);
            if (tid < gcnt) {   // the KD root's point (or the leaf's mean) at depth 0
                mg_kent x;
                x.v = cval[tid]; x.d = 0; x.pad = 0;
                mg_heappush(kh, klen, kcap, x, lt_kd, kflags);
                kev[0] = cid[tid];
            }
            if (tid == 0) s_evals += gcnt;
            __syncthreads();
            for (int step = 0; step <= lp.kd_depth; step++) {
                const bool active = tid < gcnt && cur >= 0 && kin[cur];
                if (tid < MG_KD_GROUP) {   // slot 2t: the right child, slot 2t + 1: the left (the order the reference scores them)
                    cid[2 * tid] = active ? krt[cur] : -1;
                    cid[2 * tid + 1] = active ? kl[cur] : -1;
                }
                if (!__syncthreads_or(active)) break;
                mg_tree_score<TRAJ, FRAMES>(d, a, s, tl, fx, P, dim, MG_TREE_CHUNK, tid, lane, wave);
                if (active) {   // _decide_direction_objective: left only if l < r
                    const int r = cid[2 * tid], l = cid[2 * tid + 1];
                    double cost = INFINITY;
                    if (l >= 0 && r >= 0) {
                        const double ld = cval[2 * tid + 1], rd = cval[2 * tid];
                        if (ld < rd) { cur = l; cost = ld; } else { cur = r; cost = rd; }
                    } else if (r >= 0) {
                        cur = r; cost = cval[2 * tid];
                    } else if (l >= 0) {
                        cur = l; cost = cval[2 * tid + 1];
                    } else {
                        cur = -1;
                    }
                    depth++;
                    if (cur >= 0 && depth < kcap) {
                        mg_kent x;
                        x.v = cost; x.d = depth; x.pad = 0;
                        mg_heappush(kh, klen, kcap, x, lt_kd, kflags);
                        kev[depth] = cur;
                    } else if (cur >= 0) {
                        kflags |= MG_TREE_OVERFLOW;
                        cur = -1;
                    }
                }
                if (tid == 0) {
                    int n = 0;
                    for (int j = 0; j < MG_TREE_CHUNK; j++) n += cid[j] >= 0;
                    s_evals += n;
                }
                __syncthreads();
            }
            if (tid < gcnt) {   // result_queue[0] with that depth's point
                res_v[tid] = kh[0].v;
                res_row[tid] = kev[kh[0].d];
                if (kflags) atomicOr(&s_kflags, kflags);
            }
            __syncthreads();
            if (tid == 0) {
                for (int j = 0; j < gcnt; j++) {
                    mg_hent x;
                    x.v = res_v[j]; x.a = 0; x.b = res_row[j]; x.c = 0; x.pad = 0;
                    mg_heappush(lf, lf_len, lp.cap_leaf, x, lt_leaf, flags);
                    if (dlast[j]) {   // heappop(result_queue) onto results as (v, c_idx, sample)
                        mg_hent y;
                        y.v = lf[0].v; y.a = dfr[j]; y.b = lf[0].b; y.c = fr_n[dfr[j]]; y.pad = 0;
                        mg_heappush(re, re_len, lp.s.cap_res, y, lt_res, flags);
                        lf_len = 0;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {   // candidates = new_candidates[:n_candidates]
            const int m = min(n_cand, lv_len);
            for (int i = 0; i < m; i++) fr_n[i] = lv[i].c;
            s_fr_len = m;
        }
        __syncthreads();
    }
    if (tid == 0) {
        mg_tree_search_record r;
        flags |= s_kflags;
        if (s_stop) {
            if (!(flags & MG_TREE_TIE)) flags |= MG_TREE_NO_MEAN;   // whichever the reference raised first
            r.leaf = -1; r.value = INFINITY; r.row = -1;
        } else {
            if (s_fr_len != 0) flags |= MG_TREE_OVERFLOW;
            if (re_len == 0) {
                flags |= MG_TREE_NO_RESULT;
                r.leaf = 0; r.value = INFINITY; r.row = n_kd;   // self.root.mean
            } else {
                r.leaf = re[0].c; r.value = re[0].v; r.row = re[0].b;
            }
        }
        r.flags = flags;
        r.evaluations = s_evals;
        rec[blockIdx.x] = r;
    }
}

template <bool TRAJ>
__global__ __launch_bounds__(MG_TREE_THREADS) void mg_kd_tree_search_kernel(const mg_tree_search_desc *__restrict__ tab, mg_kd_lds_plan lp,
                                                                            mg_tree_search_record *__restrict__ rec) {
    mg_kd_tree_search_body<TRAJ, false>(tab, lp, rec, nullptr, mg_tree_frames_lds{});
}
__global__ __launch_bounds__(MG_TREE_THREADS) void mg_kd_tree_search_frames_kernel(const mg_tree_search_desc *__restrict__ tab,
                                                                                   const mg_tree_frames_desc *__restrict__ ftab, mg_kd_lds_plan lp,
                                                                                   mg_tree_frames_lds fl, mg_tree_search_record *__restrict__ rec) {
    mg_kd_tree_search_body<true, true>(tab, lp, rec, ftab, fl);
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
#define MG_TREE_REQUIRE(cond, ...) MG_REQUIRE_AS(cond, MG_ERR_INVALID_ARGUMENT, __VA_ARGS__)

static void mg_tree_free(mg_cluster_tree *t) {
    if (!t) return;
    for (void *q : {(void *)t->d_points, (void *)t->d_child_begin, (void *)t->d_children, (void *)t->d_first, (void *)t->d_leaf, (void *)t->d_kd_begin,
                    (void *)t->d_kd_roots, (void *)t->d_kd_left, (void *)t->d_kd_right, (void *)t->d_kd_inner})
        if (q) (void)hipFree(q);
    delete t;
}

// n elements of h on the device: at least one allocated, copied when there is something to copy.  A step of a chain: does
// nothing once e holds an error.
template <class T>
static void mg_tree_upload(hipError_t &e, T **d, const T *h, int64_t n) {
    if (e == hipSuccess) e = hipMalloc(d, (size_t)std::max<int64_t>(n, 1) * sizeof(T));
    if (e == hipSuccess && n > 0) e = hipMemcpy(*d, h, (size_t)n * sizeof(T), hipMemcpyHostToDevice);
}

// the end of both creators: the tree, or nothing partial left behind
static int mg_tree_uploaded(hipError_t e, const char *what, mg_cluster_tree *t, mg_cluster_tree **tree) {
    if (e != hipSuccess) {
        mg_tree_free(t);
        return mg_hip_fail(e, what);
    }
    *tree = t;
    return MG_OK;
}

// A CSR list over the cluster nodes (begin[0] = 0, checked by the caller together with its end): rows that do not decrease and
// hold at most MG_TREE_MAX_CHILDREN entries, so every row lies inside the list.  *widest: the longest row.
static int mg_tree_check_rows(const char *fn, const char *what, int32_t n_nodes, const int32_t *begin, int *widest) {
    *widest = 0;
    for (int32_t i = 0; i < n_nodes; i++) {
        const int32_t b = begin[i], e = begin[i + 1];
        MG_TREE_REQUIRE(b <= e, "%s: %s decreases at node %d", fn, what, i);
        MG_TREE_REQUIRE(e - b <= MG_TREE_MAX_CHILDREN, "%s: node %d has %d children (at most %d)", fn, i, e - b, MG_TREE_MAX_CHILDREN);
        *widest = std::max(*widest, e - b);
    }
    return MG_OK;
}

// The cluster nodes' children (child_begin, children): n_nodes - 1 edges, every child in [1, n_nodes).  kids[i]: node i's.
static int mg_tree_check_children(const char *fn, int32_t n_nodes, const int32_t *child_begin, const int32_t *children,
                                  std::vector<std::vector<int32_t>> &kids, int *max_children) {
    const int64_t n_edges = (int64_t)n_nodes - 1;
    MG_TREE_REQUIRE(child_begin[0] == 0 && child_begin[n_nodes] == n_edges,
                    "%s: child_begin must run from 0 to n_nodes - 1 = %lld (every node but the root has one parent)", fn, (long long)n_edges);
    MG_TREE_REQUIRE(n_edges == 0 || children != nullptr, "%s: children is NULL", fn);
    int rc = mg_tree_check_rows(fn, "child_begin", n_nodes, child_begin, max_children);
    if (rc != MG_OK) return rc;
    kids.assign(n_nodes, std::vector<int32_t>());
    for (int32_t i = 0; i < n_nodes; i++)
        for (int32_t k = child_begin[i]; k < child_begin[i + 1]; k++) {
            MG_TREE_REQUIRE(children[k] >= 1 && children[k] < n_nodes, "%s: child %d of node %d out of range (the root is nobody's child)", fn, children[k], i);
            kids[i].push_back(children[k]);
        }
    return MG_OK;
}

// one parent per node, reachable from `roots` (BFS by levels), at most max_depth edges deep: MG_OK, or the error set
static int mg_tree_check_forest(const char *fn, const char *what, int32_t n, const std::vector<int32_t> &roots,
                                const std::vector<std::vector<int32_t>> &kids, int max_depth, int *depth_out) {
    std::vector<char> seen(n, 0);
    std::vector<int32_t> level, next;
    for (int32_t r : roots) {
        MG_TREE_REQUIRE(r >= 0 && r < n, "%s: %s root %d out of range [0, %d)", fn, what, r, n);
        MG_TREE_REQUIRE(!seen[r], "%s: %s node %d has more than one parent", fn, what, r);
        seen[r] = 1;
        level.push_back(r);
    }
    int64_t reached = (int64_t)level.size();
    int depth = 0;
    while (true) {
        next.clear();
        for (int32_t v : level)
            for (int32_t c : kids[v]) {
                MG_TREE_REQUIRE(c >= 0 && c < n && !seen[c], "%s: %s node %d out of range or with more than one parent", fn, what, c);
                seen[c] = 1;
                next.push_back(c);
            }
        if (next.empty()) break;
        depth++;
        reached += (int64_t)next.size();
        MG_TREE_REQUIRE(depth <= max_depth, "%s: %s depth beyond %d or a cycle", fn, what, max_depth);
        level.swap(next);
    }
    MG_TREE_REQUIRE(reached == n, "%s: %lld of %d %s nodes reachable (a cycle)", fn, (long long)reached, n, what);
    *depth_out = depth;
    return MG_OK;
}

extern "C" int mg_cluster_tree_create(mg_primitive *prim, int32_t n_nodes, int32_t dim, const double *means, const int32_t *child_begin,
                                      const int32_t *children, const int64_t *first_index, int64_t n_rows, mg_cluster_tree **tree) {
    const char *fn = "mg_cluster_tree_create";
    MG_TREE_REQUIRE(tree != nullptr, "%s: tree is NULL", fn);
    *tree = nullptr;
    MG_TREE_REQUIRE(prim && means && child_begin && first_index, "%s: NULL argument", fn);
    MG_TREE_REQUIRE(n_nodes >= 1, "%s: n_nodes = %d", fn, n_nodes);
    MG_TREE_REQUIRE(n_rows >= 1, "%s: n_rows = %lld", fn, (long long)n_rows);
    MG_TREE_REQUIRE(dim >= prim->L, "%s: mean width %d < the primitive's %d spatial components", fn, dim, prim->L);
    std::vector<std::vector<int32_t>> kids;
    int max_children = 0, depth = 0;
    int rc = mg_tree_check_children(fn, n_nodes, child_begin, children, kids, &max_children);
    if (rc == MG_OK) rc = mg_tree_check_forest(fn, "cluster", n_nodes, std::vector<int32_t>(1, 0), kids, MG_TREE_MAX_DEPTH, &depth);
    if (rc != MG_OK) return rc;
    for (int32_t i = 0; i < n_nodes; i++) {
        const int64_t fi = first_index[i];
        MG_TREE_REQUIRE(fi >= -1 && fi < n_rows, "%s: node %d: index %lld out of range [0, %lld)", fn, i, (long long)fi, (long long)n_rows);
        MG_TREE_REQUIRE(!(kids[i].empty() && i != 0 && fi < 0), "%s: leaf %d has no index", fn, i);
    }
    mg_context *ctx = prim->ctx;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_cluster_tree *t = new mg_cluster_tree;
    t->ctx = ctx; t->n_nodes = n_nodes; t->dim = dim; t->depth = depth; t->max_children = max_children; t->n_rows = n_rows;
    hipError_t e = hipSuccess;
    mg_tree_upload(e, &t->d_points, means, (int64_t)n_nodes * dim);
    mg_tree_upload(e, &t->d_child_begin, child_begin, (int64_t)n_nodes + 1);
    mg_tree_upload(e, &t->d_children, children, (int64_t)n_nodes - 1);
    mg_tree_upload(e, &t->d_first, first_index, n_nodes);
    return mg_tree_uploaded(e, "mg_cluster_tree_create: upload", t, tree);
}

extern "C" int mg_cluster_tree_create_kd(mg_primitive *prim, int32_t n_nodes, int32_t n_kd, int32_t dim, const double *points, const int32_t *child_begin,
                                         const int32_t *children, const int32_t *leaf, const int32_t *kd_begin, const int32_t *kd_roots,
                                         const int32_t *kd_left, const int32_t *kd_right, const int32_t *kd_inner, mg_cluster_tree **tree) {
    const char *fn = "mg_cluster_tree_create_kd";
    MG_TREE_REQUIRE(tree != nullptr, "%s: tree is NULL", fn);
    *tree = nullptr;
    MG_TREE_REQUIRE(prim && points && child_begin && leaf && kd_begin, "%s: NULL argument", fn);
    MG_TREE_REQUIRE(n_nodes >= 1 && n_kd >= 0, "%s: n_nodes = %d, n_kd = %d", fn, n_nodes, n_kd);
    MG_TREE_REQUIRE(dim >= prim->L, "%s: point width %d < the primitive's %d spatial components", fn, dim, prim->L);
    MG_TREE_REQUIRE(n_kd == 0 || (kd_left && kd_right && kd_inner), "%s: NULL KD table", fn);
    std::vector<std::vector<int32_t>> kids, kkids(n_kd);
    int max_children = 0, max_kd = 0, depth = 0, kd_depth = 0;
    int rc = mg_tree_check_children(fn, n_nodes, child_begin, children, kids, &max_children);
    if (rc != MG_OK) return rc;
    const int32_t n_roots = kd_begin[n_nodes];
    MG_TREE_REQUIRE(kd_begin[0] == 0 && n_roots >= 0 && n_roots <= n_kd, "%s: kd_begin must run from 0 to at most n_kd", fn);
    MG_TREE_REQUIRE(n_roots == 0 || kd_roots != nullptr, "%s: kd_roots is NULL", fn);
    rc = mg_tree_check_rows(fn, "kd_begin", n_nodes, kd_begin, &max_kd);
    if (rc != MG_OK) return rc;
    for (int32_t i = 0; i < n_nodes; i++) {
        MG_TREE_REQUIRE(kids[i].empty() || kd_begin[i + 1] == kd_begin[i], "%s: node %d mixes cluster-node and KD-tree children", fn, i);
        MG_TREE_REQUIRE(!(leaf[i] && !kids[i].empty()), "%s: leaf %d has cluster-node children", fn, i);
    }
    rc = mg_tree_check_forest(fn, "cluster", n_nodes, std::vector<int32_t>(1, 0), kids, MG_TREE_MAX_DEPTH, &depth);
    if (rc != MG_OK) return rc;
    for (int32_t k = 0; k < n_kd; k++) {
        MG_TREE_REQUIRE(kd_left[k] >= -1 && kd_left[k] < n_kd && kd_right[k] >= -1 && kd_right[k] < n_kd, "%s: KD node %d: a child out of range", fn, k);
        if (kd_left[k] >= 0) kkids[k].push_back(kd_left[k]);
        if (kd_right[k] >= 0) kkids[k].push_back(kd_right[k]);
    }
    rc = mg_tree_check_forest(fn, "KD", n_kd, std::vector<int32_t>(kd_roots, kd_roots + n_roots), kkids, MG_KD_MAX_DEPTH, &kd_depth);
    if (rc != MG_OK) return rc;
    mg_context *ctx = prim->ctx;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_cluster_tree *t = new mg_cluster_tree;
    t->ctx = ctx; t->kind = 1; t->n_nodes = n_nodes; t->dim = dim; t->depth = depth; t->max_children = max_children; t->n_rows = (int64_t)n_kd + n_nodes;
    t->n_kd = n_kd; t->max_kd_children = max_kd; t->kd_depth = kd_depth;
    hipError_t e = hipSuccess;
    mg_tree_upload(e, &t->d_points, points, t->n_rows * dim);
    mg_tree_upload(e, &t->d_child_begin, child_begin, (int64_t)n_nodes + 1);
    mg_tree_upload(e, &t->d_children, children, (int64_t)n_nodes - 1);
    mg_tree_upload(e, &t->d_leaf, leaf, n_nodes);
    mg_tree_upload(e, &t->d_kd_begin, kd_begin, (int64_t)n_nodes + 1);
    mg_tree_upload(e, &t->d_kd_roots, kd_roots, n_roots);
    mg_tree_upload(e, &t->d_kd_left, kd_left, n_kd);
    mg_tree_upload(e, &t->d_kd_right, kd_right, n_kd);
    mg_tree_upload(e, &t->d_kd_inner, kd_inner, n_kd);
    return mg_tree_uploaded(e, "mg_cluster_tree_create_kd: upload", t, tree);
}

extern "C" void mg_cluster_tree_destroy(mg_cluster_tree *tree) {
    if (!tree) return;
    (void)hipSetDevice(tree->ctx->device);
    (void)hipStreamSynchronize(tree->ctx->stream);   // no search in flight reads the arrays
    mg_tree_free(tree);
}

// what a call's plan is sized by: the largest of each over its searches
struct mg_tree_maxima {
    int L = 1, nc = 1, children = 1, depth = 0, kd_children = 1, kd_depth = 0, wrows = 0;
    bool rows_known = true;
    int traj = 0, cp_rows = 0, poly_doubles = 0;   // the longest trajectory list, the most root rows and the longest polynomial table
};

// One launch for the table's searches with the plan the ladder settled on (mg_tree_planned).
template <class Plan, class Kernel>
static int mg_tree_launch(mg_context *ctx, const std::vector<mg_tree_search_desc> &tab, const mg_tree_maxima &m, int n_candidates, const Plan &lp, Kernel kernel,
                          mg_tree_search_record *records_dev) {
    if (lp.bytes > MG_TREE_LDS_MAX) {
        mg_set_error("mg_cluster_tree_search: %zu bytes of LDS (latents %d, constraints %d, candidates %d, children %d, depth %d, KD depth %d, trajectories %d) "
                     "beyond 160 KiB", lp.bytes, m.L, m.nc, n_candidates, m.children, m.depth, m.kd_depth, m.traj);
        return MG_ERR_UNSUPPORTED;
    }
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_device_table &dt = ctx->tab[MG_TABLE_TREE];
    int rc = dt.upload(ctx, "mg_cluster_tree_search", tab.data(), tab.size() * sizeof(mg_tree_search_desc));
    if (rc != MG_OK) return rc;
    if (lp.bytes > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in(MG_TREE_LDS_MAX, kernel));
    mg_prof_begin(ctx, MG_PROF_CLUSTER_TREE_SEARCH);
    hipLaunchKernelGGL(kernel, dim3((unsigned)tab.size()), dim3(MG_TREE_THREADS), lp.bytes, ctx->stream, (const mg_tree_search_desc *)dt.base(), lp,
                       records_dev);
    mg_prof_end(ctx, MG_PROF_CLUSTER_TREE_SEARCH);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

// a validated call: its context, its tree kind, the table its workgroups read and the maxima its plan is sized by
struct mg_tree_call {
    mg_context *ctx = nullptr;
    int kind = 0;
    std::vector<mg_tree_search_desc> tab;
    mg_tree_maxima m;
};

// The arguments of both entry points and of the plan query (the messages name the family), validated and gathered into c:
// trajectory_counts NULL is the call without trajectories.  n_searches >= 1.  Touches no device.
static int mg_tree_gather(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees, const mg_constraint_set *const *csets,
                          const int32_t *trajectory_counts, const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                          const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_call &c) {
    MG_TREE_REQUIRE(n_candidates >= 1 && n_candidates <= MG_TREE_MAX_CANDIDATES, "mg_cluster_tree_search: n_candidates = %d outside [1, %d]",
                    n_candidates, MG_TREE_MAX_CANDIDATES);
    MG_TREE_REQUIRE(prims[0] != nullptr, "mg_cluster_tree_search: primitive 0 is NULL");
    MG_TREE_REQUIRE(trees[0] != nullptr, "mg_cluster_tree_search: search 0: NULL primitive, tree or constraint set");
    const int kind = trees[0]->kind;
    for (int32_t s = 1; s < n_searches; s++)
        MG_TREE_REQUIRE(trees[s] == nullptr || trees[s]->kind == kind,
                        "mg_cluster_tree_search: search %d: a %s tree in a call of %s trees (one kind per call)", s,
                        trees[s]->kind ? "KD" : "feature", kind ? "KD" : "feature");
    mg_context *ctx = prims[0]->ctx;
    c.ctx = ctx;
    c.kind = kind;
    std::vector<int64_t> toff;
    { const int rc = mg_tree_traj_offsets("mg_cluster_tree_search", n_searches, trajectory_counts, toff); if (rc != MG_OK) return rc; }
    MG_TREE_REQUIRE(toff[n_searches] == 0 || (trajectories && min_u && weights), "mg_cluster_tree_search: NULL trajectory, min_u or weight array");
    std::vector<mg_tree_search_desc> &tab = c.tab;
    tab.resize(n_searches);
    mg_tree_maxima &m = c.m;
    for (int32_t s = 0; s < n_searches; s++) {
        mg_primitive *p = prims[s];
        const mg_cluster_tree *t = trees[s];
        const mg_constraint_set *cs = csets[s];
        MG_TREE_REQUIRE(p && t && cs, "mg_cluster_tree_search: search %d: NULL primitive, tree or constraint set", s);
        MG_TREE_REQUIRE(p->ctx == ctx, "mg_cluster_tree_search: search %d: the primitives live in different contexts", s);
        MG_TREE_REQUIRE(t->ctx == ctx, "mg_cluster_tree_search: search %d: the tree was uploaded to another context", s);
        MG_TREE_REQUIRE(cs->prim == p, "mg_cluster_tree_search: search %d: the constraint set belongs to another primitive", s);
        MG_TREE_REQUIRE(t->dim >= p->L, "mg_cluster_tree_search: search %d: tree %s of width %d < %d spatial components", s, kind ? "points" : "means",
                        t->dim, p->L);
        mg_tree_search_desc &d = tab[s];
        memset(&d, 0, sizeof(d));   // (the padding too: the table is compared with the last call's)
        d.a = mg_score_args_of(cs, p->L);
        d.points = t->d_points; d.child_begin = t->d_child_begin; d.children = t->d_children; d.first = t->d_first; d.leaf = t->d_leaf;
        d.kd_begin = t->d_kd_begin; d.kd_roots = t->d_kd_roots; d.kd_left = t->d_kd_left; d.kd_right = t->d_kd_right; d.kd_inner = t->d_kd_inner;
        d.dim = t->dim; d.rows = cs->rows; d.n_kd = t->n_kd;
        m.rows_known = m.rows_known && cs->rows > 0;
        m.wrows = std::max(m.wrows, (int)cs->rows);
        m.L = std::max(m.L, (int)p->L);
        m.nc = std::max(m.nc, (int)cs->n);
        m.children = std::max(m.children, (int)t->max_children);
        m.depth = std::max(m.depth, (int)t->depth);
        m.kd_children = std::max(m.kd_children, (int)t->max_kd_children);
        m.kd_depth = std::max(m.kd_depth, (int)t->kd_depth);
        // the search's trajectories: every one made for this primitive (its root rows are the primitive's), scored on the canonical grid
        const int32_t count = (int32_t)(toff[s + 1] - toff[s]);
        if (count == 0) continue;
        mg_tree_traj_in in[MG_TREE_MAX_TRAJECTORIES];
        for (int32_t i = 0; i < count; i++) {
            const mg_trajectory *tj = trajectories[toff[s] + i];
            MG_TREE_REQUIRE(tj != nullptr, "mg_cluster_tree_search: search %d: trajectory %d is NULL", s, i);
            MG_TREE_REQUIRE(tj->prim == p, "mg_cluster_tree_search: search %d: trajectory %d was made for another primitive or context", s, i);
            in[i] = mg_tree_traj_in{tj->d_poly, tj->n_seg, tj->granularity};
            m.poly_doubles = std::max(m.poly_doubles, (int)tj->n_seg * 12 + 3);
        }
        const int rc = mg_tree_traj_fill("mg_cluster_tree_search", s, count, in, min_u + toff[s], weights + toff[s], alignments ? alignments[s] : nullptr, &d.tr);
        if (rc != MG_OK) return rc;
        const mg_trajectory *t0 = trajectories[toff[s]];
        const mg_time_grid *g = p->canonical;
        d.tr.E = t0->d_E; d.tr.mean = t0->d_mean; d.tr.i0 = g->d_i0; d.tr.w = g->d_w;
        d.tr.T = g->T; d.tr.NB = p->NB; d.tr.search = ctx->opt[MG_OPT_TRAJECTORY_SEARCH] == 1 ? 1 : 0;
        m.traj = std::max(m.traj, (int)count);
        m.cp_rows = std::max(m.cp_rows, (int)t0->rows);
    }
    return MG_OK;
}

// The plan of a gathered call as the ladder settles it, and the kernel that goes with it: f(plan, kernel).  The searches launch
// through it and the plan query reads it, so the two cannot disagree.  (A call without trajectories has the kernels it always
// launched, with the plan it always had.)
template <class F>
static int mg_tree_planned(const mg_tree_call &c, int n_candidates, F f) {
    const mg_tree_maxima &m = c.m;
    const mg_tree_staging want{m.rows_known ? m.wrows : 0, m.cp_rows, m.poly_doubles};
    if (c.kind == 1) {
        const auto lp = mg_tree_plan_fit(want, m.traj, [&](const mg_tree_staging &st) {
            return mg_kd_plan(m.L, m.nc, n_candidates, m.children, m.depth, m.kd_children, m.kd_depth, m.traj, st);
        });
        return m.traj > 0 ? f(lp, mg_kd_tree_search_kernel<true>) : f(lp, mg_kd_tree_search_kernel<false>);
    }
    const auto lp = mg_tree_plan_fit(want, m.traj, [&](const mg_tree_staging &st) { return mg_tree_plan(m.L, m.nc, n_candidates, m.children, m.depth, m.traj, st); });
    return m.traj > 0 ? f(lp, mg_tree_search_kernel<true>) : f(lp, mg_tree_search_kernel<false>);
}

static int mg_tree_search(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees, const mg_constraint_set *const *csets,
                          const int32_t *trajectory_counts, const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                          const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_search_record *records_dev) {
    MG_TREE_REQUIRE(n_searches >= 0, "mg_cluster_tree_search: n_searches = %d", n_searches);
    if (n_searches == 0) return MG_OK;
    MG_TREE_REQUIRE(prims && trees && csets && records_dev, "mg_cluster_tree_search: NULL argument");
    mg_tree_call c;
    const int rc = mg_tree_gather(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, n_candidates, c);
    if (rc != MG_OK) return rc;
    return mg_tree_planned(c, n_candidates, [&](const auto &lp, auto kernel) { return mg_tree_launch(c.ctx, c.tab, c.m, n_candidates, lp, kernel, records_dev); });
}

extern "C" int mg_cluster_tree_search_plan(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                           const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                           const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                           const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_search_plan_info *out) {
    MG_TREE_REQUIRE(out != nullptr, "mg_cluster_tree_search_plan: out is NULL");
    memset(out, 0, sizeof(*out));
    MG_TREE_REQUIRE(n_searches >= 0, "mg_cluster_tree_search: n_searches = %d", n_searches);
    if (n_searches == 0) return MG_OK;
    MG_TREE_REQUIRE(prims && trees && csets, "mg_cluster_tree_search: NULL argument");
    mg_tree_call c;
    const int rc = mg_tree_gather(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, n_candidates, c);
    if (rc != MG_OK) return rc;
    return mg_tree_planned(c, n_candidates, [&](const auto &lp, auto) {
        out->lds_bytes = (int64_t)lp.bytes;
        out->w_rows = lp.s.wrows; out->root_rows = lp.s.cp_rows; out->poly_doubles = lp.s.poly_doubles; out->trajectory_slots = lp.s.traj;
        out->lds_opt_in = lp.bytes > 64 * 1024;
        out->refused = lp.bytes > MG_TREE_LDS_MAX;
        return MG_OK;
    });
}

extern "C" int mg_cluster_tree_search(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                      const mg_constraint_set *const *csets, int32_t n_candidates, mg_tree_search_record *records_dev) {
    return mg_tree_search(n_searches, prims, trees, csets, nullptr, nullptr, nullptr, nullptr, nullptr, n_candidates, records_dev);
}

extern "C" int mg_cluster_tree_search_trajectories(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                                   const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                                   const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                                   const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_search_record *records_dev) {
    return mg_tree_search(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, n_candidates, records_dev);
}

// the records read back: the launch, one copy, one wait
template <class Search>
static int mg_tree_search_to_host(int32_t n_searches, mg_primitive *const *prims, mg_tree_search_record *records, Search search) {
    MG_TREE_REQUIRE(n_searches >= 0 && (n_searches == 0 || (records && prims && prims[0])), "mg_cluster_tree_search_host: bad arguments");
    if (n_searches == 0) return MG_OK;
    mg_context *ctx = prims[0]->ctx;
    const int64_t bytes = (int64_t)n_searches * (int64_t)sizeof(mg_tree_search_record);
    void *d_rec = nullptr;
    int rc = mg_ctx_scratch(ctx, bytes, &d_rec);
    if (rc != MG_OK) return rc;
    rc = search((mg_tree_search_record *)d_rec);
    if (rc != MG_OK) return rc;
    MG_HIP_CHECK(hipMemcpyAsync(records, d_rec, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

extern "C" int mg_cluster_tree_search_host(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                           const mg_constraint_set *const *csets, int32_t n_candidates, mg_tree_search_record *records) {
    return mg_tree_search_to_host(n_searches, prims, records, [&](mg_tree_search_record *d_rec) {
        return mg_cluster_tree_search(n_searches, prims, trees, csets, n_candidates, d_rec);
    });
}

extern "C" int mg_cluster_tree_search_trajectories_host(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                                        const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                                        const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                                        const mg_alignment_desc *const *alignments, int32_t n_candidates, mg_tree_search_record *records) {
    return mg_tree_search_to_host(n_searches, prims, records, [&](mg_tree_search_record *d_rec) {
        return mg_cluster_tree_search_trajectories(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, n_candidates,
                                                   d_rec);
    });
}

// ---------------------------------------------------------------------------------------------------------------
// mg_cluster_tree_search_frames: the same launch with per-frame constraint lists in the objective
// ---------------------------------------------------------------------------------------------------------------
// the lists of a validated call: the table its workgroups read, what its plan is sized by, the slabs
struct mg_tree_frames_call {
    std::vector<mg_tree_frames_desc> ftab;
    mg_tree_frames_want want = {0, 0};
    bool tables_fit = true;     // no search holds tables that the scorers' own bound keeps in memory
    int64_t scratch_bytes = 0;  // the slabs of all searches, one behind the other
    int with_lists = 0;
};

// The lists' arguments validated and gathered into f (the searches themselves: mg_tree_gather, before).  slab: where the slabs
// begin (the plan query passes a place nothing is read from or written to).  Touches no device.
static int mg_tree_gather_frames(const char *fn, int32_t n_searches, mg_primitive *const *prims, const mg_alignment_desc *const *alignments,
                                 const mg_tree_frame_lists *lists, char *slab, mg_tree_frames_call &f) {
    f.ftab.resize(n_searches);
    for (int32_t s = 0; s < n_searches; s++) {
        mg_tree_frames_desc &d = f.ftab[s];
        memset(&d, 0, sizeof(d));
        mg_track_plan *pl = lists && lists->plans ? lists->plans[s] : nullptr;
        const int32_t n = lists && lists->n_constraints ? lists->n_constraints[s] : 0;
        MG_TREE_REQUIRE(n >= 0 && n <= MG_FRAME_LIST_MAX, "%s: search %d: %d per-frame constraints outside [0, %d]", fn, s, n, MG_FRAME_LIST_MAX);
        if (n == 0) continue;
        mg_primitive *p = prims[s];
        MG_TREE_REQUIRE(pl != nullptr && pl->prim == p, "%s: search %d has per-frame constraints but no track plan of its primitive", fn, s);
        MG_TREE_REQUIRE(lists->grids && lists->constraints && lists->request_of, "%s: NULL grids, constraints or request_of", fn);
        const mg_time_grid *const *grids = lists->grids + (size_t)s * MG_TRACK_MAX_REQUESTS;
        // the slab: the requests' tracks, then the joint rotations' frame rows
        int32_t T[MG_TRACK_MAX_REQUESTS], J[MG_TRACK_MAX_REQUESTS];
        double *outs[MG_TRACK_MAX_REQUESTS] = {nullptr, nullptr, nullptr, nullptr};
        char *at = slab + f.scratch_bytes;
        for (int q = 0; q < pl->n_requests; q++) {
            const mg_time_grid *g = grids[q] ? grids[q] : p->canonical;
            MG_TREE_REQUIRE(g->prim == p && g->T >= 1, "%s: search %d: grid %d is empty or belongs to another primitive", fn, s, q);
            T[q] = g->T; J[q] = pl->req_joint0[q + 1] - pl->req_joint0[q];
            outs[q] = (double *)at;
            at += (size_t)MG_TREE_CHUNK * T[q] * J[q] * 3 * 8;
        }
        size_t lds_unused = 0;
        int rc = mg_track_fill_args(fn, pl, nullptr, MG_F64, 0, p->L, alignments ? alignments[s] : nullptr, grids, outs, &d.tk, &lds_unused);
        if (rc != MG_OK) return rc;
        int n_rot = 0;
        for (int32_t i = 0; i < n; i++) {
            const mg_frame_constraint_desc *c = lists->constraints[(size_t)s * MG_FRAME_LIST_MAX + i];
            MG_TREE_REQUIRE(c != nullptr, "%s: search %d: constraint %d is NULL", fn, s, i);
            if (c->type == MG_FRAME_JOINT_ROTATION) {
                const mg_time_grid *g = lists->rotation_grids ? lists->rotation_grids[(size_t)s * MG_FRAME_LIST_MAX + i] : nullptr;
                MG_TREE_REQUIRE(g != nullptr && g->prim == p && g->T == 1, "%s: search %d: joint rotation %d needs a one-sample grid of its primitive at its frame index", fn, s, i);
                MG_TREE_REQUIRE(p->D >= 7, "%s: search %d: joint rotation %d on a primitive without quaternions", fn, s, i);
                d.rot_i0[i] = g->d_i0; d.rot_w[i] = g->d_w; d.rot_out[i] = (double *)at;
                rc = mg_fc_args_from_desc(fn, p, c, (const double *)at, MG_TREE_CHUNK, 1, (int32_t)p->D, nullptr, &d.c[i]);
                at += (size_t)MG_TREE_CHUNK * p->D * 8;
                n_rot++;
            } else {
                const int q = lists->request_of[(size_t)s * MG_FRAME_LIST_MAX + i];
                MG_TREE_REQUIRE(q >= 0 && q < pl->n_requests, "%s: search %d: constraint %d reads request %d of %d", fn, s, i, q, pl->n_requests);
                rc = mg_fc_args_from_desc(fn, p, c, outs[q], MG_TREE_CHUNK, T[q], J[q], nullptr, &d.c[i]);
            }
            if (rc != MG_OK) return rc;
        }
        d.n = n;
        f.scratch_bytes += mg_tree_frames_scratch(pl->n_requests, T, J, n_rot, (int)p->D);
        bool has_tables = false;
        const size_t tb = mg_fc_place_list_tables(d.c, n, &has_tables);
        if (has_tables && tb == 0) f.tables_fit = false;
        f.want.table_bytes = std::max(f.want.table_bytes, tb);
        f.want.ncp = std::max(f.want.ncp, (int)(p->NB * pl->n_chan));
        f.with_lists++;
    }
    if (!f.tables_fit) f.want.table_bytes = 0;
    if (f.scratch_bytes > MG_TREE_SCRATCH_MAX) {
        mg_set_error("%s: the searches' track slabs take %lld bytes (at most %lld)", fn, (long long)f.scratch_bytes, (long long)MG_TREE_SCRATCH_MAX);
        return MG_ERR_UNSUPPORTED;
    }
    return MG_OK;
}

// The plan of a gathered call with lists as its ladder settles it, and the kernel that goes with it: f(plan, lists' regions, kernel).
template <class F>
static int mg_tree_frames_planned(const mg_tree_call &c, const mg_tree_frames_call &fc, int n_candidates, F f) {
    const mg_tree_maxima &m = c.m;
    const mg_tree_staging want{m.rows_known ? m.wrows : 0, m.cp_rows, m.poly_doubles};
    mg_tree_frames_lds fl;
    if (c.kind == 1) {
        const auto lp = mg_tree_frames_fit(want, m.traj, fc.want, [&](const mg_tree_staging &st) {
            return mg_kd_plan(m.L, m.nc, n_candidates, m.children, m.depth, m.kd_children, m.kd_depth, m.traj, st);
        }, &fl);
        return f(lp, fl, mg_kd_tree_search_frames_kernel);
    }
    const auto lp = mg_tree_frames_fit(want, m.traj, fc.want, [&](const mg_tree_staging &st) { return mg_tree_plan(m.L, m.nc, n_candidates, m.children, m.depth, m.traj, st); }, &fl);
    return f(lp, fl, mg_tree_search_frames_kernel);
}

// gather + validate a frames call: the searches, then their lists
static int mg_tree_frames_gather_all(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees, const mg_constraint_set *const *csets,
                                     const int32_t *trajectory_counts, const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                     const mg_alignment_desc *const *alignments, const mg_tree_frame_lists *lists, int32_t n_candidates, char *slab,
                                     mg_tree_call &c, mg_tree_frames_call &fc) {
    MG_TREE_REQUIRE(prims && trees && csets, "mg_cluster_tree_search_frames: NULL argument");
    // (a search whose only constraints are per-frame ones is aligned through its plan's joint, which the trajectories' record refuses:
    // the trajectories see the records of the searches that have trajectories, as mg_cluster_tree_search_trajectories does)
    const int rc{mg_tree_gather(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, n_candidates, c)};
    if (rc != MG_OK) return rc;
    return mg_tree_gather_frames("mg_cluster_tree_search_frames", n_searches, prims, alignments, lists, slab, fc);
}

extern "C" int mg_cluster_tree_search_frames_plan(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                                  const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                                  const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                                  const mg_alignment_desc *const *alignments, const mg_tree_frame_lists *lists, int32_t n_candidates,
                                                  mg_tree_frames_plan_info *out) {
    MG_TREE_REQUIRE(out != nullptr, "mg_cluster_tree_search_frames_plan: out is NULL");
    memset(out, 0, sizeof(*out));
    MG_TREE_REQUIRE(n_searches >= 0, "mg_cluster_tree_search_frames: n_searches = %d", n_searches);
    if (n_searches == 0) return MG_OK;
    mg_tree_call c;
    mg_tree_frames_call fc;
    static char nowhere[256];
    const int rc = mg_tree_frames_gather_all(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, lists, n_candidates,
                                             nowhere, c, fc);
    if (rc != MG_OK) return rc;
    return mg_tree_frames_planned(c, fc, n_candidates, [&](const auto &lp, const mg_tree_frames_lds &fl, auto) {
        out->lds_bytes = (int64_t)fl.bytes;
        out->w_rows = lp.s.wrows; out->root_rows = lp.s.cp_rows; out->poly_doubles = lp.s.poly_doubles; out->trajectory_slots = lp.s.traj;
        out->lds_opt_in = fl.bytes > 64 * 1024;
        out->refused = fl.bytes > MG_TREE_LDS_MAX;
        out->track_group = fl.group; out->control_points = fl.ncp; out->tables_lds = fl.tables_lds; out->table_bytes = (int64_t)fl.table_bytes;
        out->scratch_bytes = fc.scratch_bytes;
        return MG_OK;
    });
}

extern "C" int mg_cluster_tree_search_frames(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                             const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                             const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                             const mg_alignment_desc *const *alignments, const mg_tree_frame_lists *lists, int32_t n_candidates,
                                             void *scratch_dev, int64_t scratch_bytes, mg_tree_search_record *records_dev) {
    MG_TREE_REQUIRE(n_searches >= 0, "mg_cluster_tree_search_frames: n_searches = %d", n_searches);
    if (n_searches == 0) return MG_OK;
    MG_TREE_REQUIRE(records_dev != nullptr, "mg_cluster_tree_search_frames: NULL argument");
    mg_tree_call c;
    mg_tree_frames_call fc;
    static char nowhere[256];
    const int rc = mg_tree_frames_gather_all(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, lists, n_candidates,
                                             scratch_dev ? (char *)scratch_dev : nowhere, c, fc);
    if (rc != MG_OK) return rc;
    if (fc.with_lists == 0)   // no lists anywhere: the launch without them, byte for byte
        return mg_tree_search(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, n_candidates, records_dev);
    MG_TREE_REQUIRE(scratch_dev != nullptr && scratch_bytes >= fc.scratch_bytes && ((size_t)scratch_dev & 15) == 0,
                    "mg_cluster_tree_search_frames: the track slabs need %lld bytes at a 16-byte boundary (mg_cluster_tree_search_frames_plan), %lld given",
                    (long long)fc.scratch_bytes, (long long)scratch_bytes);
    return mg_tree_frames_planned(c, fc, n_candidates, [&](const auto &lp, const mg_tree_frames_lds &fl, auto kernel) {
        if (fl.bytes > MG_TREE_LDS_MAX) {
            mg_set_error("mg_cluster_tree_search_frames: %zu bytes of LDS (latents %d, constraints %d, candidates %d, children %d, trajectories %d, control points %d) "
                         "beyond 160 KiB", fl.bytes, c.m.L, c.m.nc, n_candidates, c.m.children, c.m.traj, fl.ncp);
            return (int)MG_ERR_UNSUPPORTED;
        }
        if (!fl.tables_lds)
            for (auto &d : fc.ftab) mg_fc_unplace_tables(d.c, d.n);
        mg_context *ctx = c.ctx;
        MG_HIP_CHECK(hipSetDevice(ctx->device));
        // one table: the searches, then their lists
        const size_t sb = c.tab.size() * sizeof(mg_tree_search_desc), fb = fc.ftab.size() * sizeof(mg_tree_frames_desc);
        static_assert(sizeof(mg_tree_search_desc) % 8 == 0 && sizeof(mg_tree_frames_desc) % 8 == 0, "the lists' table follows the searches'");
        std::vector<unsigned char> both(sb + fb);
        memcpy(both.data(), c.tab.data(), sb);
        memcpy(both.data() + sb, fc.ftab.data(), fb);
        mg_device_table &dt = ctx->tab[MG_TABLE_TREE];
        const int rcu = dt.upload(ctx, "mg_cluster_tree_search_frames", both.data(), both.size());
        if (rcu != MG_OK) return rcu;
        if (fl.bytes > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in(MG_TREE_LDS_MAX, kernel));
        mg_prof_begin(ctx, MG_PROF_CLUSTER_TREE_SEARCH);
        hipLaunchKernelGGL(kernel, dim3((unsigned)c.tab.size()), dim3(MG_TREE_THREADS), fl.bytes, ctx->stream, (const mg_tree_search_desc *)dt.base(),
                           (const mg_tree_frames_desc *)(dt.base() + sb), lp, fl, records_dev);
        mg_prof_end(ctx, MG_PROF_CLUSTER_TREE_SEARCH);
        MG_HIP_CHECK(hipGetLastError());
        return (int)MG_OK;
    });
}

extern "C" int mg_cluster_tree_search_frames_host(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                                  const mg_constraint_set *const *csets, const int32_t *trajectory_counts,
                                                  const mg_trajectory *const *trajectories, const double *min_u, const double *weights,
                                                  const mg_alignment_desc *const *alignments, const mg_tree_frame_lists *lists, int32_t n_candidates,
                                                  void *scratch_dev, int64_t scratch_bytes, mg_tree_search_record *records) {
    return mg_tree_search_to_host(n_searches, prims, records, [&](mg_tree_search_record *d_rec) {
        return mg_cluster_tree_search_frames(n_searches, prims, trees, csets, trajectory_counts, trajectories, min_u, weights, alignments, lists, n_candidates,
                                             scratch_dev, scratch_bytes, d_rec);
    });
}
