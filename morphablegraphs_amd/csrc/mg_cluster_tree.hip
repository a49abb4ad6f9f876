// The reference's cluster-tree descent (space_partitioning/feature_cluster_tree.py:129-187,
// find_best_example_excluding_search_candidates) on gfx950: one workgroup per search, the whole descent in one launch.
//
// Per level the frontier's children are scored in chunks of 64 (a lane per child, the constraints dealt over the four
// waves, summed in constraint order by the child's lane: the statements of mg_score_kernel, so a child's value has the
// bits mg_score_constraints gives for its mean).  Lane 0 keeps the three heaps in LDS and restates heapq's _siftdown /
// _siftup literally; a comparison of two equal values (where the reference's tuples fall through to comparing tree nodes
// and raise TypeError) sets MG_TREE_TIE.
#include "mg_internal.h"

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <vector>

#include "mg_score_device.h"

struct mg_cluster_tree {
    mg_context *ctx = nullptr;
    int32_t n_nodes = 0, dim = 0, depth = 0, max_children = 0;
    int64_t n_rows = 0;
    double *d_means = nullptr;        // [n_nodes][dim]
    int32_t *d_child_begin = nullptr; // [n_nodes + 1]
    int32_t *d_children = nullptr;    // [n_nodes - 1] (at least one entry allocated)
    int64_t *d_first = nullptr;       // [n_nodes]
};

// what a workgroup reads of its search (one table per launch, in device memory)
struct mg_tree_search_desc {
    mg_score_args a;
    const double *means;
    const int32_t *child_begin, *children;
    const int64_t *first;
    int32_t dim, rows;   // rows: the set's rows of W (0: not known, W is read from global memory)
};

#define MG_TREE_CHUNK 64
#define MG_TREE_WAVES 4

// heapq's comparison of (value, node) tuples whose values differ: value < value.  Equal values would compare the nodes.
__device__ __forceinline__ bool mg_tree_lt(double a, double b, int &flags) {
    if (a == b) flags |= MG_TREE_TIE;
    return a < b;
}

// heapq.heappush: append, then _siftdown(heap, 0, len - 1)
__device__ void mg_tree_heappush(double *hv, int32_t *hn, int &len, int cap, double v, int32_t node, int &flags) {
    if (len >= cap) { flags |= MG_TREE_OVERFLOW; return; }
    int pos = len++;
    while (pos > 0) {
        const int parent = (pos - 1) >> 1;
        if (mg_tree_lt(v, hv[parent], flags)) {
            hv[pos] = hv[parent]; hn[pos] = hn[parent];
            pos = parent;
            continue;
        }
        break;
    }
    hv[pos] = v; hn[pos] = node;
}

// The comparisons of heapq.heappop (the last entry to the root, _siftup, _siftdown) for their tie flag alone: the
// answer is the root read before.
__device__ void mg_tree_heappop_compares(double *hv, int32_t *hn, int len, int &flags) {
    if (len <= 1) return;
    const int end = len - 1;
    const double v = hv[end];
    const int32_t nd = hn[end];
    int pos = 0, child = 1;
    while (child < end) {
        const int right = child + 1;
        if (right < end && !mg_tree_lt(hv[child], hv[right], flags)) child = right;
        hv[pos] = hv[child]; hn[pos] = hn[child];
        pos = child;
        child = 2 * pos + 1;
    }
    while (pos > 0) {
        const int parent = (pos - 1) >> 1;
        if (mg_tree_lt(v, hv[parent], flags)) {
            hv[pos] = hv[parent]; hn[pos] = hn[parent];
            pos = parent;
            continue;
        }
        break;
    }
    hv[pos] = v; hn[pos] = nd;
}

struct mg_tree_lds_plan {
    int Lmax, ncmax, n_cand, cap_local, cap_level, cap_res, wrows;
    size_t off_w, off_rs, off_cval, off_frv, off_lvv, off_lov, off_rev, off_frn, off_froff, off_lvn, off_lon, off_ren, off_cid, off_clast, bytes;
};

static mg_tree_lds_plan mg_tree_plan(int Lmax, int ncmax, int n_cand, int max_children, int max_depth, int wrows) {
    mg_tree_lds_plan p;
    p.wrows = wrows;
    p.Lmax = Lmax; p.ncmax = std::max(ncmax, 1); p.n_cand = n_cand;
    p.cap_local = std::max(max_children, 1);
    p.cap_level = n_cand * std::min(n_cand, p.cap_local);
    p.cap_res = n_cand * (max_depth + 1);
    size_t o = (size_t)MG_TREE_CHUNK * (Lmax + 1) * 8;   // xs [64][L+1]
    p.off_w = o;     o += (size_t)wrows * (Lmax + 1) * 8;  // the set's W [rows][L] and bias [rows]
    p.off_rs = o;    o += (size_t)p.ncmax * MG_TREE_CHUNK * 8;
    p.off_cval = o;  o += MG_TREE_CHUNK * 8;
    p.off_frv = o;   o += (size_t)n_cand * 8;
    p.off_lvv = o;   o += (size_t)p.cap_level * 8;
    p.off_lov = o;   o += (size_t)p.cap_local * 8;
    p.off_rev = o;   o += (size_t)p.cap_res * 8;
    p.off_frn = o;   o += (size_t)n_cand * 4;
    p.off_froff = o; o += (size_t)(n_cand + 1) * 4;
    p.off_lvn = o;   o += (size_t)p.cap_level * 4;
    p.off_lon = o;   o += (size_t)p.cap_local * 4;
    p.off_ren = o;   o += (size_t)p.cap_res * 4;
    p.off_cid = o;   o += MG_TREE_CHUNK * 4;
    p.off_clast = o; o += MG_TREE_CHUNK * 4;
    p.bytes = (o + 15) & ~(size_t)15;
    return p;
}

__global__ __launch_bounds__(MG_TREE_CHUNK *MG_TREE_WAVES) void mg_tree_search_kernel(const mg_tree_search_desc *__restrict__ tab, mg_tree_lds_plan lp,
                                                                                      mg_tree_search_record *__restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_fr_len, s_total;
    __shared__ long long s_evals;
    const mg_tree_search_desc *d = tab + blockIdx.x;
    const mg_score_args a = d->a;
    const double *__restrict__ means = d->means;
    const int32_t *__restrict__ cb = d->child_begin;
    const int32_t *__restrict__ ch = d->children;
    const int dim = d->dim, L = a.L, xs_stride = L + 1, n_cand = lp.n_cand;
    double *xs = (double *)smem;
    double *rs = (double *)(smem + lp.off_rs);
    double *cval = (double *)(smem + lp.off_cval);
    double *fr_v = (double *)(smem + lp.off_frv);
    double *lv_v = (double *)(smem + lp.off_lvv);
    double *lo_v = (double *)(smem + lp.off_lov);
    double *re_v = (double *)(smem + lp.off_rev);
    int32_t *fr_n = (int32_t *)(smem + lp.off_frn);
    int32_t *fr_off = (int32_t *)(smem + lp.off_froff);
    int32_t *lv_n = (int32_t *)(smem + lp.off_lvn);
    int32_t *lo_n = (int32_t *)(smem + lp.off_lon);
    int32_t *re_n = (int32_t *)(smem + lp.off_ren);
    int32_t *cid = (int32_t *)(smem + lp.off_cid);
    int32_t *clast = (int32_t *)(smem + lp.off_clast);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // The set's keyframe matrices in LDS: a level scores a handful of children, one wave per constraint, and every step of
    // the fma chains below would otherwise wait for a load from memory.  Same values, same order: the same bits.
    const double *Wm = a.W, *Bm = a.bias;
    if (lp.wrows > 0 && d->rows > 0) {
        double *wl = (double *)(smem + lp.off_w), *bl = wl + (size_t)lp.wrows * L;
        for (int i = tid; i < d->rows * L; i += MG_TREE_CHUNK * MG_TREE_WAVES) wl[i] = a.W[i];
        for (int i = tid; i < d->rows; i += MG_TREE_CHUNK * MG_TREE_WAVES) bl[i] = a.bias[i];
        Wm = wl;
        Bm = bl;
    }
    // lane 0's heap state (only thread 0 touches the heaps)
    int flags = 0, lv_len = 0, lo_len = 0, res_len = 0;
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
                if (nc == 0) mg_tree_heappush(re_v, re_n, res_len, lp.cap_res, fr_v[f], node, flags);   // a leaf: onto results
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
                int f = 0;
                while (f + 1 < fr_len && fr_off[f + 1] <= e) f++;
                const int node = fr_n[f];
                cid[tid] = ch[cb[node] + (e - fr_off[f])];
                clast[tid] = (e == fr_off[f + 1] - 1);
            }
            __syncthreads();
            for (int e = tid; e < MG_TREE_CHUNK * L; e += MG_TREE_CHUNK * MG_TREE_WAVES) {
                const int c = e / L, i = e - c * L;
                xs[c * xs_stride + i] = c < cnt ? means[(size_t)cid[c] * dim + i] : 0.0;
            }
            __syncthreads();
            const double *x = xs + lane * xs_stride;
            for (int c = wave; c < a.n; c += MG_TREE_WAVES) {
                auto channel = [&](int row) {   // mg_score_kernel's fma chain over k from the bias
                    const double *wr = Wm + (size_t)row * L;
                    double acc = Bm[row];
                    for (int k = 0; k < L; k++) acc = fma(wr[k], x[k], acc);
                    return acc;
                };
                rs[c * MG_TREE_CHUNK + lane] = mg_constraint_residual(a, c, channel, 0);
            }
            __syncthreads();
            if (tid < cnt) {
                double err = 0.0;
                for (int c = 0; c < a.n; c++) err += rs[c * MG_TREE_CHUNK + tid];
                cval[tid] = err;
            }
            __syncthreads();
            if (tid == 0) {
                for (int j = 0; j < cnt; j++) {
                    mg_tree_heappush(lo_v, lo_n, lo_len, lp.cap_local, cval[j], cid[j], flags);   // _find_best_cluster_candidates
                    if (clast[j]) {   // the node's children are all in: result_queue[:n_candidates] onto the level's heap
                        const int m = min(n_cand, lo_len);
                        for (int i = 0; i < m; i++) mg_tree_heappush(lv_v, lv_n, lv_len, lp.cap_level, lo_v[i], lo_n[i], flags);
                        lo_len = 0;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {   // candidates = new_candidates[:n_candidates]
            const int m = min(n_cand, lv_len);
            for (int i = 0; i < m; i++) { fr_v[i] = lv_v[i]; fr_n[i] = lv_n[i]; }
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
            r.leaf = re_n[0]; r.value = re_v[0]; r.row = d->first[re_n[0]];
            mg_tree_heappop_compares(re_v, re_n, res_len, flags);
        }
        r.flags = flags;
        r.evaluations = s_evals;
        rec[blockIdx.x] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
#define MG_TREE_REQUIRE(cond, ...)          \
    do {                                    \
        if (!(cond)) {                      \
            mg_set_error(__VA_ARGS__);      \
            return MG_ERR_INVALID_ARGUMENT; \
        }                                   \
    } while (0)

static void mg_tree_free(mg_cluster_tree *t) {
    if (!t) return;
    for (void *q : {(void *)t->d_means, (void *)t->d_child_begin, (void *)t->d_children, (void *)t->d_first})
        if (q) (void)hipFree(q);
    delete t;
}

extern "C" int mg_cluster_tree_create(mg_primitive *prim, int32_t n_nodes, int32_t dim, const double *means, const int32_t *child_begin,
                                      const int32_t *children, const int64_t *first_index, int64_t n_rows, mg_cluster_tree **tree) {
    MG_TREE_REQUIRE(tree != nullptr, "mg_cluster_tree_create: tree is NULL");
    *tree = nullptr;
    MG_TREE_REQUIRE(prim && means && child_begin && first_index, "mg_cluster_tree_create: NULL argument");
    MG_TREE_REQUIRE(n_nodes >= 1, "mg_cluster_tree_create: n_nodes = %d", n_nodes);
    MG_TREE_REQUIRE(n_rows >= 1, "mg_cluster_tree_create: n_rows = %lld", (long long)n_rows);
    MG_TREE_REQUIRE(dim >= prim->L, "mg_cluster_tree_create: mean width %d < the primitive's %d spatial components", dim, prim->L);
    const int64_t n_edges = (int64_t)n_nodes - 1;
    MG_TREE_REQUIRE(child_begin[0] == 0 && child_begin[n_nodes] == n_edges,
                    "mg_cluster_tree_create: child_begin must run from 0 to n_nodes - 1 = %lld (every node but the root has one parent)",
                    (long long)n_edges);
    MG_TREE_REQUIRE(n_edges == 0 || children != nullptr, "mg_cluster_tree_create: children is NULL");
    std::vector<int32_t> parents(n_nodes, -1);
    int max_children = 0;
    for (int32_t i = 0; i < n_nodes; i++) {
        const int32_t b = child_begin[i], e = child_begin[i + 1];
        MG_TREE_REQUIRE(b <= e, "mg_cluster_tree_create: child_begin decreases at node %d", i);
        MG_TREE_REQUIRE(e - b <= MG_TREE_MAX_CHILDREN, "mg_cluster_tree_create: node %d has %d children (at most %d)", i, e - b, MG_TREE_MAX_CHILDREN);
        max_children = std::max(max_children, e - b);
        for (int32_t k = b; k < e; k++) {
            const int32_t c = children[k];
            MG_TREE_REQUIRE(c >= 1 && c < n_nodes, "mg_cluster_tree_create: child %d of node %d out of range (the root is nobody's child)", c, i);
            MG_TREE_REQUIRE(parents[c] < 0, "mg_cluster_tree_create: node %d has more than one parent", c);
            parents[c] = i;
        }
        const int64_t fi = first_index[i];
        MG_TREE_REQUIRE(fi >= -1 && fi < n_rows, "mg_cluster_tree_create: node %d: index %lld out of range [0, %lld)", i, (long long)fi, (long long)n_rows);
        MG_TREE_REQUIRE(!(e == b && i != 0 && fi < 0), "mg_cluster_tree_create: leaf %d has no index", i);
    }
    // reachability from the root by levels: n - 1 edges, one parent each, all reached <=> a tree (no cycle)
    std::vector<int32_t> level(1, 0), next;
    int64_t reached = 1;
    int depth = 0;
    while (true) {
        next.clear();
        for (int32_t v : level)
            for (int32_t k = child_begin[v]; k < child_begin[v + 1]; k++) next.push_back(children[k]);
        if (next.empty()) break;
        depth++;
        reached += (int64_t)next.size();
        MG_TREE_REQUIRE(depth <= MG_TREE_MAX_DEPTH && reached <= n_nodes, "mg_cluster_tree_create: depth beyond %d or a cycle", MG_TREE_MAX_DEPTH);
        level.swap(next);
    }
    MG_TREE_REQUIRE(reached == n_nodes, "mg_cluster_tree_create: %lld of %d nodes reachable from the root (a cycle)", (long long)reached, n_nodes);
    mg_context *ctx = prim->ctx;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_cluster_tree *t = new mg_cluster_tree;
    t->ctx = ctx; t->n_nodes = n_nodes; t->dim = dim; t->depth = depth; t->max_children = max_children; t->n_rows = n_rows;
    const size_t mb = (size_t)n_nodes * dim * 8, cbb = (size_t)(n_nodes + 1) * 4, chb = (size_t)std::max<int64_t>(n_edges, 1) * 4, fb = (size_t)n_nodes * 8;
    hipError_t e = hipMalloc(&t->d_means, mb);
    if (e == hipSuccess) e = hipMalloc(&t->d_child_begin, cbb);
    if (e == hipSuccess) e = hipMalloc(&t->d_children, chb);
    if (e == hipSuccess) e = hipMalloc(&t->d_first, fb);
    if (e == hipSuccess) e = hipMemcpy(t->d_means, means, mb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_child_begin, child_begin, cbb, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_edges > 0) e = hipMemcpy(t->d_children, children, (size_t)n_edges * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_first, first_index, fb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        mg_tree_free(t);
        return mg_hip_fail(e, "mg_cluster_tree_create: upload");
    }
    *tree = t;
    return MG_OK;
}

extern "C" void mg_cluster_tree_destroy(mg_cluster_tree *tree) {
    if (!tree) return;
    (void)hipSetDevice(tree->ctx->device);
    (void)hipStreamSynchronize(tree->ctx->stream);   // no search in flight reads the arrays
    mg_tree_free(tree);
}

extern "C" int mg_cluster_tree_search(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                      const mg_constraint_set *const *csets, int32_t n_candidates, mg_tree_search_record *records_dev) {
    MG_TREE_REQUIRE(n_searches >= 0, "mg_cluster_tree_search: n_searches = %d", n_searches);
    if (n_searches == 0) return MG_OK;
    MG_TREE_REQUIRE(prims && trees && csets && records_dev, "mg_cluster_tree_search: NULL argument");
    MG_TREE_REQUIRE(n_candidates >= 1 && n_candidates <= MG_TREE_MAX_CANDIDATES, "mg_cluster_tree_search: n_candidates = %d outside [1, %d]",
                    n_candidates, MG_TREE_MAX_CANDIDATES);
    MG_TREE_REQUIRE(prims[0] != nullptr, "mg_cluster_tree_search: primitive 0 is NULL");
    mg_context *ctx = prims[0]->ctx;
    std::vector<mg_tree_search_desc> tab(n_searches);
    int Lmax = 1, ncmax = 1, maxch = 1, maxdepth = 0, wrows = 0;
    bool rows_known = true;
    for (int32_t s = 0; s < n_searches; s++) {
        mg_primitive *p = prims[s];
        const mg_cluster_tree *t = trees[s];
        const mg_constraint_set *cs = csets[s];
        MG_TREE_REQUIRE(p && t && cs, "mg_cluster_tree_search: search %d: NULL primitive, tree or constraint set", s);
        MG_TREE_REQUIRE(p->ctx == ctx, "mg_cluster_tree_search: search %d: the primitives live in different contexts", s);
        MG_TREE_REQUIRE(t->ctx == ctx, "mg_cluster_tree_search: search %d: the tree was uploaded to another context", s);
        MG_TREE_REQUIRE(cs->prim == p, "mg_cluster_tree_search: search %d: the constraint set belongs to another primitive", s);
        MG_TREE_REQUIRE(t->dim >= p->L, "mg_cluster_tree_search: search %d: tree means of width %d < %d spatial components", s, t->dim, p->L);
        mg_tree_search_desc &d = tab[s];
        memset(&d, 0, sizeof(d));
        d.a.W = cs->d_W; d.a.bias = cs->d_bias; d.a.par = cs->d_par; d.a.woff = cs->d_woff; d.a.chain = cs->d_chain; d.a.choff = cs->d_choff;
        d.a.pose = cs->d_pose; d.a.align = cs->d_align; d.a.align_cand = nullptr; d.a.lat = nullptr; d.a.out = nullptr; d.a.res = nullptr;
        d.a.B = 0; d.a.ld = 0; d.a.n = cs->n; d.a.nch = cs->nch; d.a.L = p->L;
        d.means = t->d_means; d.child_begin = t->d_child_begin; d.children = t->d_children; d.first = t->d_first; d.dim = t->dim;
        d.rows = cs->rows;
        rows_known = rows_known && cs->rows > 0;
        wrows = std::max(wrows, (int)cs->rows);
        Lmax = std::max(Lmax, (int)p->L);
        ncmax = std::max(ncmax, (int)cs->n);
        maxch = std::max(maxch, (int)t->max_children);
        maxdepth = std::max(maxdepth, (int)t->depth);
    }
    mg_tree_lds_plan lp = mg_tree_plan(Lmax, ncmax, n_candidates, maxch, maxdepth, rows_known ? wrows : 0);
    if (lp.bytes > 160 * 1024 && lp.wrows > 0) lp = mg_tree_plan(Lmax, ncmax, n_candidates, maxch, maxdepth, 0);   // W from memory
    if (lp.bytes > 160 * 1024) {
        mg_set_error("mg_cluster_tree_search: %zu bytes of LDS (latents %d, constraints %d, candidates %d, children %d, depth %d) beyond 160 KiB",
                     lp.bytes, Lmax, ncmax, n_candidates, maxch, maxdepth);
        return MG_ERR_UNSUPPORTED;
    }
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t tab_bytes = tab.size() * sizeof(mg_tree_search_desc);
    if (!ctx->tree_tab_dev || ctx->tree_tab_host.size() != tab_bytes || memcmp(ctx->tree_tab_host.data(), tab.data(), tab_bytes) != 0) {
        MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // no launch in flight reads the table being replaced
        if (ctx->tree_tab_cap < tab_bytes) {
            if (ctx->tree_tab_dev) { (void)hipFree(ctx->tree_tab_dev); ctx->tree_tab_dev = nullptr; ctx->tree_tab_cap = 0; }
            MG_HIP_CHECK(hipMalloc(&ctx->tree_tab_dev, tab_bytes));
            ctx->tree_tab_cap = tab_bytes;
        }
        MG_HIP_CHECK(hipMemcpy(ctx->tree_tab_dev, tab.data(), tab_bytes, hipMemcpyHostToDevice));
        ctx->tree_tab_host.assign((const unsigned char *)tab.data(), (const unsigned char *)tab.data() + tab_bytes);
    }
    if (lp.bytes > 64 * 1024)
        MG_HIP_CHECK(hipFuncSetAttribute((const void *)mg_tree_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    mg_prof_begin(ctx, 11);
    hipLaunchKernelGGL(mg_tree_search_kernel, dim3(n_searches), dim3(MG_TREE_CHUNK * MG_TREE_WAVES), lp.bytes, ctx->stream,
                       (const mg_tree_search_desc *)ctx->tree_tab_dev, lp, records_dev);
    mg_prof_end(ctx, 11);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

extern "C" int mg_cluster_tree_search_host(int32_t n_searches, mg_primitive *const *prims, mg_cluster_tree *const *trees,
                                           const mg_constraint_set *const *csets, int32_t n_candidates, mg_tree_search_record *records) {
    MG_TREE_REQUIRE(n_searches >= 0 && (n_searches == 0 || (records && prims && prims[0])), "mg_cluster_tree_search_host: bad arguments");
    if (n_searches == 0) return MG_OK;
    mg_context *ctx = prims[0]->ctx;
    const int64_t bytes = (int64_t)n_searches * (int64_t)sizeof(mg_tree_search_record);
    void *d_rec = nullptr;
    int rc = mg_ctx_scratch(ctx, bytes, &d_rec);
    if (rc != MG_OK) return rc;
    rc = mg_cluster_tree_search(n_searches, prims, trees, csets, n_candidates, (mg_tree_search_record *)d_rec);
    if (rc != MG_OK) return rc;
    MG_HIP_CHECK(hipMemcpyAsync(records, d_rec, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}
