// What csrc/mg_tree_plan.h promises the one-launch cluster-tree search: the LDS plans of both kernels against a restatement of their
// layout (regions in order, none overlapping, 8-byte regions aligned, a call without trajectories the plan it always had), the ladder
// a plan beyond the workgroup's LDS is retried by, the per-search trajectory lists flattened and refused, and the alignment record.
// Plain host code with its own main (test infrastructure, never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_tree_plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static char last_error[512];
void mg_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}

// the head of a plan, restated: bytes of every region in order
static size_t head_bytes(int L, int nc, int traj, const mg_tree_staging &st) {
    const size_t xs = 64 * (size_t)(L + 1) * 8, w = (size_t)st.wrows * (L + 1) * 8, rs = (size_t)(nc < 1 ? 1 : nc) * 64 * 8, cval = 64 * 8;
    const size_t cp = traj > 0 ? (size_t)st.cp_rows * 64 * 8 : 0, poly = traj > 0 ? (size_t)traj * st.poly_doubles * 8 : 0, tv = (size_t)traj * 64 * 8;
    return xs + w + rs + cval + cp + poly + tv;
}

static long plans = 0;

static void check_plans(int L, int nc, int n_cand, int children, int depth, int kd_children, int kd_depth, int traj, const mg_tree_staging &st) {
    const mg_tree_lds_plan p = mg_tree_plan(L, nc, n_cand, children, depth, traj, st);
    const mg_kd_lds_plan k = mg_kd_plan(L, nc, n_cand, children, depth, kd_children, kd_depth, traj, st);
    plans += 2;
    const size_t head = head_bytes(L, nc, traj, st);
    const int cap_local = children < 1 ? 1 : children, cap_level = n_cand * (n_cand < cap_local ? n_cand : cap_local), cap_res = n_cand * (depth + 1);
    CHECK(p.off_frv == head && k.off_lo == head, "the head ends at %zu / %zu, restated %zu", p.off_frv, k.off_lo, head);
    for (const mg_tree_lds_shared *s : {&p.s, &k.s}) {
        CHECK(s->off_w == 64 * (size_t)(L + 1) * 8 && s->off_rs >= s->off_w && s->off_cval > s->off_rs && s->off_cp == s->off_cval + 512 && s->off_poly >= s->off_cp &&
              s->off_tv >= s->off_poly, "regions out of order");
        CHECK(s->off_cp % 8 == 0 && s->off_poly % 8 == 0 && s->off_tv % 8 == 0 && s->off_cid % 4 == 0, "a region not aligned");
        CHECK(s->cap_local == cap_local && s->cap_level == cap_level && s->cap_res == cap_res && s->n_cand == n_cand, "heap bounds");
        CHECK(s->traj == traj && s->cp_rows == (traj > 0 ? st.cp_rows : 0) && s->poly_doubles == (traj > 0 ? st.poly_doubles : 0), "trajectory fields");
        CHECK(s->off_froff == s->off_frn + (size_t)n_cand * 4 && s->off_frn == s->off_clast + 256 && s->off_clast == s->off_cid + 256, "int regions");
    }
    const size_t tree_total = head + (size_t)n_cand * 8 + (size_t)(cap_level + cap_local + cap_res) * 12 + 512 + (size_t)(2 * n_cand + 1) * 4;
    CHECK(p.bytes == ((tree_total + 15) & ~(size_t)15), "feature plan %zu bytes, restated %zu", p.bytes, tree_total);
    const int kcap = kd_depth + 1, cap_leaf = kd_children < 1 ? 1 : kd_children;
    const size_t kd_total = head + (size_t)(cap_local + cap_level + cap_res + cap_leaf) * 24 + (size_t)32 * kcap * 16 + 32 * 8 + (size_t)32 * kcap * 4 + 512 +
                            (size_t)(2 * n_cand + 1) * 4 + 256 + (size_t)(n_cand + 1) * 4 + 3 * 32 * 4;
    CHECK(k.bytes == ((kd_total + 15) & ~(size_t)15), "KD plan %zu bytes, restated %zu", k.bytes, kd_total);
    if (traj == 0) {   // without trajectories nothing of a plan depends on the trajectory staging
        const mg_tree_lds_plan q = mg_tree_plan(L, nc, n_cand, children, depth, 0, mg_tree_staging{st.wrows, 0, 0});
        CHECK(q.bytes == p.bytes && q.off_frv == p.off_frv && q.s.off_cid == p.s.off_cid && q.off_ren == p.off_ren, "a call without trajectories has another plan");
    }
}

// The fitted plan of shapes given on the command line, twelve integers each (kind 0 feature / 1 KD, L, nc, n_cand, children, depth,
// kd_children, kd_depth, traj, wrows, cp_rows, poly_doubles): one line "bytes wrows cp_rows poly_doubles traj" per shape, as
// mg_cluster_tree_search_plan reports them.  tests/test_tree_search_shapes_host.py compares them with its restatement.
static int print_fitted(int argc, char **argv) {
    if ((argc - 1) % 12 != 0) { std::printf("usage: tree_plan_check [kind L nc n_cand children depth kd_children kd_depth traj wrows cp_rows poly]...\n"); return 2; }
    for (int a = 1; a + 12 <= argc; a += 12) {
        int v[12];
        for (int i = 0; i < 12; i++) v[i] = std::atoi(argv[a + i]);
        const mg_tree_staging want{v[9], v[10], v[11]};
        if (v[0] == 1) {
            const auto p = mg_tree_plan_fit(want, v[8], [&](const mg_tree_staging &st) { return mg_kd_plan(v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], st); });
            std::printf("%zu %d %d %d %d\n", p.bytes, p.s.wrows, p.s.cp_rows, p.s.poly_doubles, p.s.traj);
        } else {
            const auto p = mg_tree_plan_fit(want, v[8], [&](const mg_tree_staging &st) { return mg_tree_plan(v[1], v[2], v[3], v[4], v[5], v[8], st); });
            std::printf("%zu %d %d %d %d\n", p.bytes, p.s.wrows, p.s.cp_rows, p.s.poly_doubles, p.s.traj);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return print_fitted(argc, argv);
    // the plans over a grid of shapes, with and without trajectories and each staging
    for (int L : {1, 3, 40, 64, 68})
        for (int nc : {0, 1, 5, 33})
            for (int n_cand : {1, 2, 9, 64})
                for (int children : {0, 1, 8, 256})
                    for (int depth : {0, 3, 64})
                        for (int traj = 0; traj <= MG_TREE_MAX_TRAJECTORIES; traj++)
                            for (int wrows : {0, 7, 400})
                                for (int cp_rows : {0, 25, 97})
                                    for (int poly : {0, 63, 1203})
                                        check_plans(L, nc, n_cand, children, depth, children / 2, depth, traj, mg_tree_staging{wrows, cp_rows, poly});

    // the ladder: W first, then the polynomials, then the root rows; the first plan that fits is taken
    auto plan_of = [](int L, int n_cand, int traj) {
        return [=](const mg_tree_staging &st) { return mg_tree_plan(L, 2, n_cand, 8, 6, traj, st); };
    };
    {
        const mg_tree_staging all = {12, 97, 123};
        auto p = mg_tree_plan_fit(all, 1, plan_of(40, 2, 1));                        // the walk primitive: everything fits
        CHECK(p.bytes <= MG_TREE_LDS_MAX && p.s.wrows == 12 && p.s.cp_rows == 97 && p.s.poly_doubles == 123, "walk shape: %zu bytes", p.bytes);
        p = mg_tree_plan_fit(mg_tree_staging{3000, 97, 123}, 1, plan_of(40, 2, 1));   // W too large alone
        CHECK(p.bytes <= MG_TREE_LDS_MAX && p.s.wrows == 0 && p.s.cp_rows == 97 && p.s.poly_doubles == 123, "W leaves first");
        p = mg_tree_plan_fit(mg_tree_staging{3000, 97, 12003}, 2, plan_of(40, 2, 2));  // two tables of 96 KB
        CHECK(p.bytes <= MG_TREE_LDS_MAX && p.s.wrows == 0 && p.s.cp_rows == 97 && p.s.poly_doubles == 0, "the polynomials leave second");
        p = mg_tree_plan_fit(mg_tree_staging{3000, 400, 12003}, 2, plan_of(40, 2, 2)); // 400 root rows: 200 KB
        CHECK(p.bytes <= MG_TREE_LDS_MAX && p.s.wrows == 0 && p.s.cp_rows == 0 && p.s.poly_doubles == 0, "the root rows leave last");
        p = mg_tree_plan_fit(mg_tree_staging{12, 97, 123}, 1, plan_of(400, 2, 1));     // 64 x 401 latents: nothing helps
        CHECK(p.bytes > MG_TREE_LDS_MAX && p.s.wrows == 0 && p.s.cp_rows == 0 && p.s.poly_doubles == 0, "a plan that cannot fit comes back bare");
        p = mg_tree_plan_fit(mg_tree_staging{3000, 97, 123}, 0, plan_of(40, 2, 0));    // no trajectories: the two steps there always were
        CHECK(p.s.wrows == 0 && p.s.cp_rows == 0 && p.s.poly_doubles == 0 && p.s.traj == 0 && p.bytes == mg_tree_plan(40, 2, 2, 8, 6, 0, mg_tree_staging{0, 0, 0}).bytes,
              "no trajectories");
    }

    // the flattened lists
    {
        std::vector<int64_t> off;
        const int32_t counts[4] = {0, 2, MG_TREE_MAX_TRAJECTORIES, 1};
        CHECK(mg_tree_traj_offsets("t", 4, counts, off) == MG_OK && off.size() == 5 && off[0] == 0 && off[1] == 0 && off[2] == 2 && off[3] == 6 && off[4] == 7, "offsets");
        CHECK(mg_tree_traj_offsets("t", 3, nullptr, off) == MG_OK && off.size() == 4 && off[3] == 0, "no counts: no trajectories");
        CHECK(mg_tree_traj_offsets("t", 0, nullptr, off) == MG_OK && off.size() == 1, "no searches");
        const int32_t over[2] = {1, MG_TREE_MAX_TRAJECTORIES + 1}, under[1] = {-1};
        CHECK(mg_tree_traj_offsets("t", 2, over, off) == MG_ERR_INVALID_ARGUMENT && mg_tree_traj_offsets("t", 1, under, off) == MG_ERR_INVALID_ARGUMENT, "counts out of range");
    }
    {
        const double poly[15] = {0};
        mg_tree_traj_in in[MG_TREE_MAX_TRAJECTORIES];
        double min_u[MG_TREE_MAX_TRAJECTORIES], weight[MG_TREE_MAX_TRAJECTORIES];
        for (int i = 0; i < MG_TREE_MAX_TRAJECTORIES; i++) { in[i] = mg_tree_traj_in{poly, 1 + i, 1000}; min_u[i] = 0.1 * i; weight[i] = 1.0 + i; }
        mg_tree_traj_desc d = {};
        mg_alignment_desc al = {};
        al.joint = 0; al.position[0] = 5.0; al.position[1] = 6.0; al.position[2] = 7.0; al.heading[0] = 3.0; al.heading[1] = 4.0; al.ref_dir[2] = 1.0;
        CHECK(mg_tree_traj_fill("t", 0, MG_TREE_MAX_TRAJECTORIES, in, min_u, weight, &al, &d) == MG_OK, "a full list: %s", last_error);
        CHECK(d.n == MG_TREE_MAX_TRAJECTORIES && d.t[3].n_seg == 4 && d.t[3].G == 1000 && d.t[3].min_u == 0.1 * 3 && d.t[3].weight == 4.0 && d.t[0].poly == poly, "records");
        CHECK(d.align_mode == 1 && d.al[0] == 0.6 && d.al[1] == 0.8 && d.al[2] == 5.0 && d.al[3] == 7.0 && d.al[4] == 0.0 && d.al[6] == 1.0, "previous-frame record");
        al.joint = MG_ALIGN_START_POSE;
        CHECK(mg_tree_traj_fill("t", 0, 1, in, min_u, weight, &al, &d) == MG_OK && d.align_mode == 2 && d.al[4] == 6.0 && d.al[5] == 0.0, "start-pose record");
        CHECK(mg_tree_traj_fill("t", 0, 1, in, min_u, weight, nullptr, &d) == MG_OK && d.align_mode == 0 && d.al[0] == 0.0, "no record");
        al.joint = 2;
        CHECK(mg_tree_traj_fill("t", 0, 1, in, min_u, weight, &al, &d) == MG_ERR_UNSUPPORTED, "another aligning joint");
        d.align_mode = 7;
        CHECK(mg_tree_traj_fill("t", 0, 0, in, min_u, weight, &al, &d) == MG_OK && d.n == 0 && d.align_mode == 7, "a search without trajectories ignores its record");
        al.joint = 0; al.heading[0] = al.heading[1] = 0.0;
        CHECK(mg_tree_traj_fill("t", 0, 1, in, min_u, weight, &al, &d) == MG_ERR_INVALID_ARGUMENT, "a zero heading");
        CHECK(mg_tree_traj_fill("t", 0, MG_TREE_MAX_TRAJECTORIES + 1, in, min_u, weight, nullptr, &d) == MG_ERR_INVALID_ARGUMENT, "a fifth trajectory");
        min_u[0] = 1.5;
        CHECK(mg_tree_traj_fill("t", 0, 1, in, min_u, weight, nullptr, &d) == MG_ERR_INVALID_ARGUMENT, "min_u beyond 1");
        min_u[0] = 0.0; weight[0] = INFINITY;
        CHECK(mg_tree_traj_fill("t", 0, 1, in, min_u, weight, nullptr, &d) == MG_ERR_INVALID_ARGUMENT, "an infinite weight");
        weight[0] = 1.0; in[0].poly = nullptr;
        CHECK(mg_tree_traj_fill("t", 0, 1, in, min_u, weight, nullptr, &d) == MG_ERR_INVALID_ARGUMENT, "a trajectory without tables");
    }

    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("tree_plan_check: ok (%ld plans)\n", plans);
    return failures ? 1 : 0;
}
