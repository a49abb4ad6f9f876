// Batched k-means for the cluster-tree builders (reference space_partitioning/cluster_tree_node_builder.py:83-100 and
// clustering.py:69-129 call sklearn's KMeans once per tree node; here every node of a tree level is a SEGMENT of one
// row permutation over one device points table and all segments are clustered together).
//
// Semantics are sklearn's KMeans(algorithm="lloyd") per segment (and per run of n_init):
//   init      greedy k-means++ (_kmeans_plusplus): a uniformly drawn first centre, then 2 + int(ln k) D^2-sampled candidates
//             per centre, the one of least potential kept; uniforms from Philox4x32-10 with counter (draw, run, node id)
//             and key seed, so a segment's draws depend on its node id alone, not on how segments are batched -- or the
//             caller's initial centres;
//   iteration assignment by squared Euclidean distance in float64 (sequential over the dimensions), ties to the lowest
//             centre; the centres the means of their members (sum * (1 / count), as _average_centers); an empty cluster
//             takes the member farthest from its centre (_relocate_empty_clusters_dense); several empty clusters take the
//             farthest members in descending order of distance, the first position on equal distances, in ascending
//             cluster order;
//   stop      labels unchanged (strict), or summed squared centre shift <= tol * mean(var(X, axis=0)) of the segment, or
//             max_iter iterations; without strict convergence one assignment-only pass follows; the inertia is the
//             summed squared distance of every member to its centre.
// sklearn centres X on its column means before it clusters; this code does not, so distances and centres agree with
// sklearn's to rounding (a member whose two nearest centres are that close may be assigned differently).
//
// Shape of the work: a table of TILES of at most 256 positions of one (segment, run) UNIT; one launch per Lloyd iteration
// over all unfinished units.  Each workgroup assigns its tile and writes per-cluster partial sums, counts and the number
// of changed labels into its own slot; the last workgroup of a unit to arrive (an agent-scope release / relaxed counter /
// acquire hand-off, no co-residency assumed, no float atomics) combines the slots in slot order, moves the centres and
// decides the unit's state, which the next launch reads.  The host reads the states every few launches.  Everything is
// summed in a fixed order, so results are bit-reproducible.
#include "mg_construct.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mg_gmm_device.h"

#define MG_KM_BLOCK 256             // threads per workgroup = positions per tile
#define MG_KM_MAX_DIM 128
#define MG_KM_MAX_K 64
#define MG_KM_MAX_NINIT 16
#define MG_KM_MAX_TRIALS 8          // 2 + int(ln 64) = 6
#define MG_KM_ACC 8                 // centres whose distances one pass over a row accumulates

enum { MG_KM_ITER = 0, MG_KM_FINAL_STRICT = 1, MG_KM_FINAL_ASSIGN = 2, MG_KM_DONE = 3 };

struct mg_km_tile { int32_t unit, slot, begin, end; };     // positions [begin, end) of the unit's segment; slot within the unit
struct mg_km_unit { int32_t begin, end, ntiles, part0; };  // the segment's positions; its tiles' first partial slot

struct mg_km_args {
    const double *points;           // [n_rows][dim]
    const int64_t *rows;            // position -> row of points
    const mg_km_tile *tiles;
    const mg_km_unit *units;
    double *centres;                // [units][k][dim]
    int32_t *labels;                // [n_init][n_pos]
    double *dist;                   // [n_init][n_pos]: squared distance to the assigned (old) centre; k-means++: closest distance
    double *part;                   // [slots][pstride]
    int32_t *state, *n_iter;
    unsigned int *counter;
    double *tol_abs, *inertia;
    double tol;
    int32_t dim, k, n_init, max_iter, pstride, n_pos;
};

// ---- the hand-off of a unit's partial slots to its last-arriving workgroup ------------------------------------------
// Every wave drains its stores, the workgroup meets, lane 0 releases at agent scope and takes a ticket; the workgroup
// holding the last ticket acquires at agent scope before it reads any other workgroup's slot.
__device__ __forceinline__ bool mg_km_arrive(unsigned int *counter, int ntiles, int *flag_lds) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = ticket == (unsigned int)(ntiles - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag_lds = last;
    }
    __syncthreads();
    return *flag_lds != 0;
}

__device__ __forceinline__ double mg_km_sqdist(const double *x, const double *c, int dim) {
    double acc = 0.0;
    for (int d = 0; d < dim; d++) {
        const double t = x[d] - c[d];
        acc = acc + t * t;
    }
    return acc;
}

// argmin over the k centres (LDS), ties to the lowest index; per row the distances of MG_KM_ACC centres at a time, each
// summed over d in order (the bits of mg_km_sqdist)
__device__ __forceinline__ int mg_km_nearest(const double *x, const double *C, int k, int dim, double &dmin) {
    int best = 0;
    dmin = INFINITY;
    for (int j0 = 0; j0 < k; j0 += MG_KM_ACC) {
        double acc[MG_KM_ACC];
#pragma unroll
        for (int q = 0; q < MG_KM_ACC; q++) acc[q] = 0.0;
        const int nj = min(MG_KM_ACC, k - j0);
        for (int d = 0; d < dim; d++) {
            const double xd = x[d];
#pragma unroll
            for (int q = 0; q < MG_KM_ACC; q++)
                if (q < nj) {
                    const double t = xd - C[(j0 + q) * dim + d];
                    acc[q] = acc[q] + t * t;
                }
        }
#pragma unroll
        for (int q = 0; q < MG_KM_ACC; q++)
            if (q < nj && acc[q] < dmin) { dmin = acc[q]; best = j0 + q; }
    }
    return best;
}

// (value, position) larger distance first, then smaller position
__device__ __forceinline__ bool mg_km_farther(double v, int p, double bv, int bp) {
    return v > bv || (v == bv && p < bp);
}

// ---- one Lloyd iteration (or the final pass) of every unfinished unit --------------------------------------------------
__global__ __launch_bounds__(MG_KM_BLOCK) void mg_kmeans_lloyd_kernel(mg_km_args a) {
    extern __shared__ double lds[];
    const int k = a.k, dim = a.dim, kd = k * dim, tid = threadIdx.x;
    double *C = lds;                             // [k][dim] the unit's centres
    double *S = C + kd;                          // [k][dim] sums
    double *W = S + kd;                          // counts [k], changed, stats s1 [dim], s2 [dim]
    double *dm = W + k + 1 + 2 * dim;            // [256] the tile's distances
    int *lab = (int *)(dm + MG_KM_BLOCK);        // [256] the tile's labels
    int *flag = lab + MG_KM_BLOCK;               // [4 + MG_KM_MAX_K]: the last-arrival flag, the empty count, a pick, the empty clusters
    const mg_km_tile t = a.tiles[blockIdx.x];
    const int u = t.unit;
    const int st = a.state[u];
    if (st == MG_KM_DONE) return;
    const mg_km_unit un = a.units[u];
    const int run = u % a.n_init;
    const int iter = a.n_iter[u];
    for (int i = tid; i < kd; i += MG_KM_BLOCK) C[i] = a.centres[(size_t)u * kd + i];
    __syncthreads();
    const int p = t.begin + tid;
    const bool have = p < t.end;
    int L = -1, changed = 0;
    double dmin = 0.0;
    if (have) {
        const double *x = a.points + (size_t)a.rows[p] * dim;
        int32_t *lp = a.labels + (size_t)run * a.n_pos + p;
        if (st == MG_KM_FINAL_STRICT) {
            L = *lp;
            dmin = mg_km_sqdist(x, C + L * dim, dim);
        } else {
            L = mg_km_nearest(x, C, k, dim, dmin);
            if (st == MG_KM_ITER) {
                changed = L != *lp;
                a.dist[(size_t)run * a.n_pos + p] = dmin;
            }
            *lp = L;
        }
    }
    lab[tid] = L;
    dm[tid] = dmin;
    const int n_changed = __syncthreads_count(changed);
    const int nt = t.end - t.begin;
    double *slot = a.part + (size_t)(un.part0 + t.slot) * a.pstride;
    if (st == MG_KM_ITER) {
        // column d: its k sums (and at iteration 0 the column statistics about the segment's first row) over the tile's
        // rows in order; cluster j: its count
        if (tid < dim) {
            const int d = tid;
            for (int j = 0; j < k; j++) S[j * dim + d] = 0.0;
            const double x0 = a.points[(size_t)a.rows[un.begin] * dim + d];
            double s1 = 0.0, s2 = 0.0;
            for (int r = 0; r < nt; r++) {
                const double v = a.points[(size_t)a.rows[t.begin + r] * dim + d];
                S[lab[r] * dim + d] += v;
                const double c = v - x0;
                s1 += c;
                s2 += c * c;
            }
            slot[kd + k + 2 + d] = s1;
            slot[kd + k + 2 + dim + d] = s2;
        }
        if (tid < k) {
            int cnt = 0;
            for (int r = 0; r < nt; r++) cnt += lab[r] == tid;
            slot[kd + tid] = (double)cnt;
        }
        if (tid == 0) slot[kd + k] = (double)n_changed;
        __syncthreads();
        for (int i = tid; i < kd; i += MG_KM_BLOCK) slot[i] = S[i];
    } else if (tid == 0) {
        double s = 0.0;
        for (int r = 0; r < nt; r++) s += dm[r];
        slot[kd + k + 1] = s;
    }
    if (!mg_km_arrive(a.counter + u, un.ntiles, flag)) return;

    // ---- the unit's last workgroup: combine the slots in slot order -------------------------------------------------
    const double *part0 = a.part + (size_t)un.part0 * a.pstride;
    if (st != MG_KM_ITER) {
        if (tid == 0) {
            double s = 0.0;
            for (int q = 0; q < un.ntiles; q++) s += part0[(size_t)q * a.pstride + kd + k + 1];
            a.inertia[u] = s;
            a.state[u] = MG_KM_DONE;
            a.counter[u] = 0;
        }
        return;
    }
    const int nw = kd + k + 1 + 2 * dim;     // sums, counts, changed, (skip the inertia word) statistics
    for (int i = tid; i < nw; i += MG_KM_BLOCK) {
        const int off = i < kd + k + 1 ? i : i + 1;
        double s = 0.0;
        for (int q = 0; q < un.ntiles; q++) s += part0[(size_t)q * a.pstride + off];
        if (i < kd) S[i] = s; else W[i - kd] = s;
    }
    __syncthreads();
    double *cnt = W, *stat1 = W + k + 1, *stat2 = stat1 + dim;
    const int n = un.end - un.begin;
    if (tid == 0) {
        if (iter == 0) {    // tol * mean(var(X, axis=0)) of the segment
            double m = 0.0;
            for (int d = 0; d < dim; d++) {
                const double mu = stat1[d] / n;
                m += stat2[d] / n - mu * mu;
            }
            a.tol_abs[u] = a.tol * (m / dim);
        }
        int ne = 0;
        for (int j = 0; j < k; j++)
            if (cnt[j] == 0.0) flag[4 + ne++] = j;     // np.where(weight_in_clusters == 0): fixed before any relocation
        flag[1] = ne;
    }
    __syncthreads();
    // empty clusters: the farthest members (descending distance, first position on ties) in ascending cluster order
    const int n_empty = flag[1];
    if (n_empty > 0) {
        double *rv = dm;            // reduction scratch
        int *rp = lab;
        int *picked = flag + 2;     // flag[2]: the position picked in this round
        const double *dist = a.dist + (size_t)run * a.n_pos;
        const int32_t *labels = a.labels + (size_t)run * a.n_pos;
        int prev_p = -1;
        double prev_v = INFINITY;
        for (int e = 0; e < n_empty; e++) {
            const int j_new = flag[4 + e];
            // the next member after (prev_v, prev_p) in (descending value, ascending position) order
            double bv = -INFINITY;
            int bp = INT32_MAX;
            for (int q = un.begin + tid; q < un.end; q += MG_KM_BLOCK) {
                const double v = dist[q];
                const bool after = v < prev_v || (v == prev_v && q > prev_p);
                if (after && mg_km_farther(v, q, bv, bp)) { bv = v; bp = q; }
            }
            rv[tid] = bv;
            rp[tid] = bp;
            __syncthreads();
            for (int s = MG_KM_BLOCK / 2; s > 0; s >>= 1) {
                if (tid < s && mg_km_farther(rv[tid + s], rp[tid + s], rv[tid], rp[tid])) { rv[tid] = rv[tid + s]; rp[tid] = rp[tid + s]; }
                __syncthreads();
            }
            if (tid == 0) *picked = rp[0];
            prev_v = rv[0];
            __syncthreads();
            const int far = *picked;
            if (far < un.begin || far >= un.end) break;     // cannot happen: a segment has at least k members
            prev_p = far;
            const int j_old = labels[far];
            if (tid < dim) {
                const double v = a.points[(size_t)a.rows[far] * dim + tid];
                S[j_old * dim + tid] -= v;
                S[j_new * dim + tid] = v;
            }
            if (tid == 0) {
                cnt[j_new] = 1.0;
                cnt[j_old] -= 1.0;
            }
            __syncthreads();
        }
    }
    // the new centres, and the squared shift per element (into S, summed by thread 0 cluster by cluster)
    for (int i = tid; i < kd; i += MG_KM_BLOCK) {
        const double c = cnt[i / dim];
        const double v = c > 0.0 ? S[i] * (1.0 / c) : S[i];
        a.centres[(size_t)u * kd + i] = v;
        const double sh = v - C[i];
        S[i] = sh * sh;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int j = 0; j < k; j++) {
            double cj = 0.0;
            for (int d = 0; d < dim; d++) cj += S[j * dim + d];
            tot += cj;
        }
        const int it = iter + 1;
        a.n_iter[u] = it;
        if (W[k] == 0.0) a.state[u] = MG_KM_FINAL_STRICT;
        else if (tot <= a.tol_abs[u] || it >= a.max_iter) a.state[u] = MG_KM_FINAL_ASSIGN;
        a.counter[u] = 0;
    }
}

// ---- greedy k-means++ (sklearn _kmeans_plusplus), one workgroup per unit --------------------------------------------
__device__ __forceinline__ double mg_km_uniform(uint64_t seed, uint32_t draw, uint32_t run, uint64_t node) {
    uint32_t r[4];
    mg_philox4x32_10(draw, run, (uint32_t)node, (uint32_t)(node >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const uint64_t bits = ((uint64_t)r[0] << 21) ^ ((uint64_t)r[1] >> 11);
    return (double)(bits & ((1ull << 53) - 1)) * 0x1.0p-53;
}

__global__ __launch_bounds__(MG_KM_BLOCK) void mg_kmeans_pp_kernel(mg_km_args a, const uint64_t *node_ids, uint64_t seed, int trials) {
    __shared__ double red[MG_KM_BLOCK];
    __shared__ double scan[MG_KM_BLOCK];
    __shared__ double target[MG_KM_MAX_TRIALS], pot_t[MG_KM_MAX_TRIALS];
    __shared__ int cand[MG_KM_MAX_TRIALS];
    const int u = blockIdx.x, tid = threadIdx.x, dim = a.dim, k = a.k;
    const mg_km_unit un = a.units[u];
    const int run = u % a.n_init, seg = u / a.n_init;
    const uint64_t node = node_ids[seg];
    const int n = un.end - un.begin;
    double *closest = a.dist + (size_t)run * a.n_pos;
    double *centres = a.centres + (size_t)u * k * dim;
    uint32_t draw = 0;
    const int first = min((int)(mg_km_uniform(seed, draw++, run, node) * n), n - 1);
    const double *c0 = a.points + (size_t)a.rows[un.begin + first] * dim;
    for (int d = tid; d < dim; d += MG_KM_BLOCK) centres[d] = c0[d];
    double mine = 0.0;
    for (int q = un.begin + tid; q < un.end; q += MG_KM_BLOCK) {
        const double v = mg_km_sqdist(a.points + (size_t)a.rows[q] * dim, c0, dim);
        closest[q] = v;
        mine += v;
    }
    double pot = mg_block_sum<MG_KM_BLOCK>(mine, red);
    for (int c = 1; c < k; c++) {
        if (tid < trials) {
            target[tid] = mg_km_uniform(seed, draw + tid, run, node) * pot;
            cand[tid] = INT32_MAX;
        }
        draw += trials;
        __syncthreads();
        // searchsorted(cumsum(closest), target) (side "left"): the first position whose running sum reaches the target
        double running = 0.0;
        for (int base = 0; base < n; base += MG_KM_BLOCK) {
            const int q = base + tid;
            scan[tid] = q < n ? closest[un.begin + q] : 0.0;
            __syncthreads();
            for (int s = 1; s < MG_KM_BLOCK; s <<= 1) {     // inclusive scan (Hillis-Steele, fixed order)
                const double add = tid >= s ? scan[tid - s] : 0.0;
                __syncthreads();
                scan[tid] += add;
                __syncthreads();
            }
            const double cum = running + scan[tid];
            if (q < n)
                for (int tr = 0; tr < trials; tr++)
                    if (cum >= target[tr]) atomicMin(&cand[tr], q);
            running += scan[MG_KM_BLOCK - 1];
            __syncthreads();
        }
        if (tid < trials && cand[tid] == INT32_MAX) cand[tid] = n - 1;
        __syncthreads();
        // the potential of every candidate, in one pass over the rows
        double acc[MG_KM_MAX_TRIALS];
        for (int tr = 0; tr < MG_KM_MAX_TRIALS; tr++) acc[tr] = 0.0;
        for (int q = un.begin + tid; q < un.end; q += MG_KM_BLOCK) {
            const double *x = a.points + (size_t)a.rows[q] * dim;
            const double cl = closest[q];
            for (int tr = 0; tr < trials; tr++) {
                const double v = mg_km_sqdist(x, a.points + (size_t)a.rows[un.begin + cand[tr]] * dim, dim);
                acc[tr] += v < cl ? v : cl;
            }
        }
        for (int tr = 0; tr < trials; tr++) {
            const double s = mg_block_sum<MG_KM_BLOCK>(acc[tr], red);
            if (tid == 0) pot_t[tr] = s;
        }
        __syncthreads();
        int best = 0;
        for (int tr = 1; tr < trials; tr++)
            if (pot_t[tr] < pot_t[best]) best = tr;
        pot = pot_t[best];
        const double *cb = a.points + (size_t)a.rows[un.begin + cand[best]] * dim;
        for (int d = tid; d < dim; d += MG_KM_BLOCK) centres[c * dim + d] = cb[d];
        for (int q = un.begin + tid; q < un.end; q += MG_KM_BLOCK) {
            const double v = mg_km_sqdist(a.points + (size_t)a.rows[q] * dim, cb, dim);
            if (v < closest[q]) closest[q] = v;
        }
        __syncthreads();
    }
}

// ---- the best run of every segment (least inertia, the first on ties) to the outputs ---------------------------------
__global__ __launch_bounds__(MG_KM_BLOCK) void mg_kmeans_select_kernel(mg_km_args a, const mg_km_tile *seg_tiles, int32_t *labels_out,
                                                                       double *centres_out, double *inertia_out, int32_t *n_iter_out) {
    const mg_km_tile t = seg_tiles[blockIdx.x];
    const int s = t.unit, tid = threadIdx.x, kd = a.k * a.dim;
    int best = 0;
    for (int r = 1; r < a.n_init; r++)
        if (a.inertia[s * a.n_init + r] < a.inertia[s * a.n_init + best]) best = r;
    const int p = t.begin + tid;
    if (p < t.end) labels_out[p] = a.labels[(size_t)best * a.n_pos + p];
    if (t.slot == 0) {
        const int u = s * a.n_init + best;
        for (int i = tid; i < kd; i += MG_KM_BLOCK) centres_out[(size_t)s * kd + i] = a.centres[(size_t)u * kd + i];
        if (tid == 0) {
            inertia_out[s] = a.inertia[u];
            n_iter_out[s] = a.n_iter[u];
        }
    }
}

extern "C" int mg_kmeans_segments(mg_context *ctx, const double *points_dev, int64_t n_rows, int32_t dim, int32_t n_segments,
                                  const int64_t *seg_begin, const int64_t *rows, int32_t k, int32_t n_init, const double *init,
                                  const uint64_t *node_ids, uint64_t seed, int32_t max_iter, double tol, int32_t *labels, double *centres,
                                  double *inertia, int32_t *n_iter) {
    const int BAD = MG_ERR_INVALID_ARGUMENT, UNS = MG_ERR_UNSUPPORTED;
    MG_REQUIRE_AS(ctx && points_dev, BAD, "mg_kmeans_segments: NULL context or points");
    MG_REQUIRE_AS(dim >= 1 && dim <= MG_KM_MAX_DIM, UNS, "mg_kmeans_segments: dim = %d outside [1, %d]", dim, MG_KM_MAX_DIM);
    MG_REQUIRE_AS(k >= 2 && k <= MG_KM_MAX_K, UNS, "mg_kmeans_segments: k = %d outside [2, %d]", k, MG_KM_MAX_K);
    MG_REQUIRE_AS(n_init >= 1 && n_init <= MG_KM_MAX_NINIT, UNS, "mg_kmeans_segments: n_init = %d outside [1, %d]", n_init, MG_KM_MAX_NINIT);
    MG_REQUIRE_AS(init == nullptr || n_init == 1, BAD, "mg_kmeans_segments: initial centres given with n_init = %d (1 run per segment)", n_init);
    MG_REQUIRE_AS(n_segments >= 0 && n_rows >= 1 && max_iter >= 1 && tol >= 0.0, BAD,
                  "mg_kmeans_segments: n_segments = %d, n_rows = %lld, max_iter = %d, tol = %g", n_segments, (long long)n_rows, max_iter, tol);
    if (n_segments == 0) return MG_OK;
    MG_REQUIRE_AS(seg_begin && rows && labels && centres && inertia && n_iter, BAD, "mg_kmeans_segments: NULL argument");
    MG_REQUIRE_AS(seg_begin[0] == 0, BAD, "mg_kmeans_segments: seg_begin[0] = %lld, not 0", (long long)seg_begin[0]);
    for (int32_t s = 0; s < n_segments; s++)
        MG_REQUIRE_AS(seg_begin[s + 1] - seg_begin[s] >= k, BAD, "mg_kmeans_segments: segment %d has %lld rows, fewer than k = %d", s,
                      (long long)(seg_begin[s + 1] - seg_begin[s]), k);
    const int64_t n_pos = seg_begin[n_segments];
    MG_REQUIRE_AS(n_pos * n_init < ((int64_t)1 << 31), UNS, "mg_kmeans_segments: %lld positions x %d runs beyond 2^31", (long long)n_pos, n_init);
    for (int64_t p = 0; p < n_pos; p++)
        MG_REQUIRE_AS(rows[p] >= 0 && rows[p] < n_rows, BAD, "mg_kmeans_segments: rows[%lld] = %lld outside [0, %lld)", (long long)p,
                      (long long)rows[p], (long long)n_rows);
    const int U = n_segments * n_init, kd = k * dim;
    const int pstride = kd + k + 2 + 2 * dim;
    std::vector<mg_km_unit> units(U);
    std::vector<mg_km_tile> tiles, seg_tiles;
    int32_t slots = 0;
    for (int32_t s = 0; s < n_segments; s++) {
        const int32_t b = (int32_t)seg_begin[s], e = (int32_t)seg_begin[s + 1];
        const int32_t nt = (e - b + MG_KM_BLOCK - 1) / MG_KM_BLOCK;
        for (int32_t q = 0; q < nt; q++) seg_tiles.push_back({s, q, b + q * MG_KM_BLOCK, std::min(e, b + (q + 1) * MG_KM_BLOCK)});
        for (int32_t r = 0; r < n_init; r++) {
            const int32_t u = s * n_init + r;
            units[u] = {b, e, nt, slots};
            for (int32_t q = 0; q < nt; q++) tiles.push_back({u, q, b + q * MG_KM_BLOCK, std::min(e, b + (q + 1) * MG_KM_BLOCK)});
            slots += nt;
        }
    }
    std::vector<uint64_t> ids(n_segments);
    for (int32_t s = 0; s < n_segments; s++) ids[s] = node_ids ? node_ids[s] : (uint64_t)s;
    std::vector<int32_t> state(U);
    std::vector<mg_km_tile> active;
    // one device block for everything the call needs; declared after the host buffers its copies touch: it drains the stream first
    mg_workspace ws(ctx, "mg_kmeans_segments");
    auto carve = [&](size_t bytes) { return ws.carve(bytes); };
    const size_t o_rows = carve(n_pos * 8), o_tiles = carve(tiles.size() * sizeof(mg_km_tile)), o_segt = carve(seg_tiles.size() * sizeof(mg_km_tile));
    const size_t o_units = carve(U * sizeof(mg_km_unit)), o_ids = carve(n_segments * 8), o_cent = carve((size_t)U * kd * 8);
    const size_t o_lab = carve((size_t)n_init * n_pos * 4), o_dist = carve((size_t)n_init * n_pos * 8), o_part = carve((size_t)slots * pstride * 8);
    const size_t o_state = carve(U * 4), o_iter = carve(U * 4), o_cnt = carve(U * 4), o_tol = carve(U * 8), o_inert = carve(U * 8);
    const size_t o_lout = carve(n_pos * 4), o_cout = carve((size_t)n_segments * kd * 8), o_iout = carve(n_segments * 8), o_nout = carve(n_segments * 4);
    const int ra = ws.alloc();
    if (ra != MG_OK) return ra;
    char *const base = ws.base;
    hipStream_t st = ctx->stream;
    mg_km_args a;
    a.points = points_dev;
    a.rows = (const int64_t *)(base + o_rows);
    a.tiles = (const mg_km_tile *)(base + o_tiles);
    a.units = (const mg_km_unit *)(base + o_units);
    a.centres = (double *)(base + o_cent);
    a.labels = (int32_t *)(base + o_lab);
    a.dist = (double *)(base + o_dist);
    a.part = (double *)(base + o_part);
    a.state = (int32_t *)(base + o_state);
    a.n_iter = (int32_t *)(base + o_iter);
    a.counter = (unsigned int *)(base + o_cnt);
    a.tol_abs = (double *)(base + o_tol);
    a.inertia = (double *)(base + o_inert);
    a.tol = tol;
    a.dim = dim; a.k = k; a.n_init = n_init; a.max_iter = max_iter; a.pstride = pstride; a.n_pos = (int32_t)n_pos;
    const size_t lds = (size_t)(2 * kd + k + 1 + 2 * dim + MG_KM_BLOCK) * 8 + (MG_KM_BLOCK + 4 + MG_KM_MAX_K) * 4;
    const int trials = 2 + (int)std::log((double)k);
    int launches = 0, next_check = 1;
    MG_HIP_CHECK(hipMemcpyAsync(base + o_rows, rows, n_pos * 8, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_tiles, tiles.data(), tiles.size() * sizeof(mg_km_tile), hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_segt, seg_tiles.data(), seg_tiles.size() * sizeof(mg_km_tile), hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_units, units.data(), U * sizeof(mg_km_unit), hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemcpyAsync(base + o_ids, ids.data(), n_segments * 8, hipMemcpyHostToDevice, st));
    MG_HIP_CHECK(hipMemsetAsync(base + o_state, 0, o_tol - o_state, st));        // state, n_iter, counters
    if (init) {
        MG_HIP_CHECK(hipMemcpyAsync(a.centres, init, (size_t)U * kd * 8, hipMemcpyHostToDevice, st));
    } else {
        hipLaunchKernelGGL(mg_kmeans_pp_kernel, dim3(U), dim3(MG_KM_BLOCK), 0, st, a, (const uint64_t *)(base + o_ids), seed, trials);
        MG_HIP_CHECK(hipGetLastError());
    }
    MG_HIP_CHECK(hipMemsetAsync(a.labels, 0xFF, (size_t)n_init * n_pos * 4, st));   // label -1: every label of iteration 0 changes
    // what this call needs, not the whole 160 KiB: __syncthreads_count keeps a static word in the LDS, and static + dynamic past 160 KiB is refused
    if (lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in((int)lds, mg_kmeans_lloyd_kernel));
    active = tiles;
    // every unit needs at most max_iter iterations and one final pass
    while (launches < max_iter + 1 && !active.empty()) {
        hipLaunchKernelGGL(mg_kmeans_lloyd_kernel, dim3((unsigned)active.size()), dim3(MG_KM_BLOCK), lds, st, a);
        MG_HIP_CHECK(hipGetLastError());
        launches++;
        if (launches == next_check || launches == max_iter + 1) {
            next_check = launches < 8 ? launches * 2 : launches + 8;
            MG_HIP_CHECK(hipMemcpyAsync(state.data(), a.state, U * 4, hipMemcpyDeviceToHost, st));
            MG_HIP_CHECK(hipStreamSynchronize(st));
            std::vector<mg_km_tile> still;
            for (const mg_km_tile &t : tiles)
                if (state[t.unit] != MG_KM_DONE) still.push_back(t);
            if (still.size() != active.size() && !still.empty())
                MG_HIP_CHECK(hipMemcpyAsync(base + o_tiles, still.data(), still.size() * sizeof(mg_km_tile), hipMemcpyHostToDevice, st));
            active.swap(still);
        }
    }
    MG_REQUIRE_AS(active.empty(), MG_ERR_INVALID_ARGUMENT, "mg_kmeans_segments: a unit did not finish in %d launches", launches);
    hipLaunchKernelGGL(mg_kmeans_select_kernel, dim3((unsigned)seg_tiles.size()), dim3(MG_KM_BLOCK), 0, st, a,
                       (const mg_km_tile *)(base + o_segt), (int32_t *)(base + o_lout), (double *)(base + o_cout), (double *)(base + o_iout),
                       (int32_t *)(base + o_nout));
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipMemcpyAsync(labels, base + o_lout, n_pos * 4, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(centres, base + o_cout, (size_t)n_segments * kd * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(inertia, base + o_iout, n_segments * 8, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipMemcpyAsync(n_iter, base + o_nout, n_segments * 4, hipMemcpyDeviceToHost, st));
    MG_HIP_CHECK(hipStreamSynchronize(st));
    return MG_OK;
}
