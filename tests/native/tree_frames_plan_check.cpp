// What csrc/mg_tree_plan.h promises mg_cluster_tree_search_frames: the per-frame lists' LDS regions lie behind the kernel's own plan
// (a call without lists has the plan it always had, to the byte), the ladder's further rungs come after the ones there always were
// and in their order (the lists' tables to memory, then the track group halved down to one child), and the slab's size.
// Plain host code with its own main (test infrastructure, never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_tree_plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

void mg_set_error(const char *, ...) {}

// The fitted plan of shapes given on the command line, fourteen integers each (kind 0 feature / 1 KD, L, nc, n_cand, children, depth,
// kd_children, kd_depth, traj, wrows, cp_rows, poly_doubles, ncp, table_bytes): one line "bytes wrows cp_rows poly_doubles traj group
// tables_lds table_bytes" per shape, as mg_cluster_tree_search_frames_plan reports them.
static int print_fitted(int argc, char **argv) {
    if ((argc - 1) % 14 != 0) { std::printf("usage: tree_frames_plan_check [kind L nc n_cand children depth kd_children kd_depth traj wrows cp_rows poly ncp tables]...\n"); return 2; }
    for (int a = 1; a + 14 <= argc; a += 14) {
        long v[14];
        for (int i = 0; i < 14; i++) v[i] = std::atol(argv[a + i]);
        const mg_tree_staging want{(int)v[9], (int)v[10], (int)v[11]};
        const mg_tree_frames_want fw{(int)v[12], (size_t)v[13]};
        mg_tree_frames_lds fl;
        if (v[0] == 1) {
            const auto p = mg_tree_frames_fit(want, (int)v[8], fw, [&](const mg_tree_staging &st) { return mg_kd_plan(v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], st); }, &fl);
            std::printf("%zu %d %d %d %d %d %d %zu\n", fl.bytes, p.s.wrows, p.s.cp_rows, p.s.poly_doubles, p.s.traj, fl.group, fl.tables_lds, fl.table_bytes);
        } else {
            const auto p = mg_tree_frames_fit(want, (int)v[8], fw, [&](const mg_tree_staging &st) { return mg_tree_plan(v[1], v[2], v[3], v[4], v[5], v[8], st); }, &fl);
            std::printf("%zu %d %d %d %d %d %d %zu\n", fl.bytes, p.s.wrows, p.s.cp_rows, p.s.poly_doubles, p.s.traj, fl.group, fl.tables_lds, fl.table_bytes);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return print_fitted(argc, argv);
    long plans = 0;
    // the regions: behind the plan, in order, aligned, nothing without lists
    for (size_t base : {(size_t)0, (size_t)4096, (size_t)65536})
        for (int ncp : {0, 49, 105, 2449})
            for (int group : {1, 2, 4})
                for (size_t tables : {(size_t)0, (size_t)112, (size_t)56160}) {
                    const mg_tree_frames_lds f = mg_tree_frames_carve(base, ncp, group, tables);
                    plans++;
                    if (ncp == 0) {
                        CHECK(f.bytes == base && f.group == 0 && f.tables_lds == 0 && f.table_bytes == 0, "a call without lists has %zu bytes, its plan %zu", f.bytes, base);
                        continue;
                    }
                    CHECK(f.off_cp == base && f.off_al == base + (size_t)group * ncp * 8 && f.off_tab == f.off_al + (size_t)group * 64, "regions out of order");
                    CHECK(f.off_cp % 8 == 0 && f.off_al % 8 == 0 && f.off_tab % 8 == 0 && f.bytes % 16 == 0 && f.bytes >= f.off_tab + tables && f.bytes < f.off_tab + tables + 16,
                          "alignment or size");
                    CHECK(f.group == group && f.tables_lds == (tables > 0) && f.table_bytes == tables, "fields");
                }
    // the ladder
    auto plan_of = [](int L, int traj) { return [=](const mg_tree_staging &st) { return mg_tree_plan(L, 2, 2, 8, 6, traj, st); }; };
    mg_tree_frames_lds fl;
    {
        auto p = mg_tree_frames_fit(mg_tree_staging{12, 97, 123}, 1, mg_tree_frames_want{105, 16064}, plan_of(40, 1), &fl);    // everything fits
        CHECK(fl.bytes <= MG_TREE_LDS_MAX && p.s.wrows == 12 && p.s.cp_rows == 97 && p.s.poly_doubles == 123 && fl.group == 4 && fl.tables_lds == 1, "all staged");
        CHECK(fl.bytes == ((p.bytes + 4 * 105 * 8 + 4 * 64 + 16064 + 15) & ~(size_t)15), "bytes behind the plan");
        p = mg_tree_frames_fit(mg_tree_staging{12, 97, 123}, 1, mg_tree_frames_want{0, 0}, plan_of(40, 1), &fl);               // no lists: the old ladder, the old bytes
        const auto q = mg_tree_plan_fit(mg_tree_staging{12, 97, 123}, 1, plan_of(40, 1));
        CHECK(fl.bytes == q.bytes && p.bytes == q.bytes && p.s.wrows == q.s.wrows && fl.group == 0, "a call without lists has another plan");
        p = mg_tree_frames_fit(mg_tree_staging{3000, 97, 123}, 1, mg_tree_frames_want{105, 16064}, plan_of(40, 1), &fl);        // W leaves first, the tables stay
        CHECK(fl.bytes <= MG_TREE_LDS_MAX && p.s.wrows == 0 && p.s.cp_rows == 97 && fl.tables_lds == 1 && fl.group == 4, "W leaves before the lists' tables");
        p = mg_tree_frames_fit(mg_tree_staging{12, 25, 63}, 1, mg_tree_frames_want{105, 150000}, plan_of(40, 1), &fl);          // the tables alone are too much
        CHECK(fl.bytes <= MG_TREE_LDS_MAX && p.s.wrows == 0 && p.s.cp_rows == 0 && p.s.poly_doubles == 0 && fl.tables_lds == 0 && fl.table_bytes == 0 && fl.group == 4,
              "the lists' tables leave after the rungs there always were");
        p = mg_tree_frames_fit(mg_tree_staging{0, 0, 0}, 0, mg_tree_frames_want{3400, 0}, plan_of(40, 0), &fl);                 // 4 x 3400 control points: 106 KiB
        CHECK(fl.bytes <= MG_TREE_LDS_MAX && fl.group == 4, "four children's control points fit");
        p = mg_tree_frames_fit(mg_tree_staging{0, 0, 0}, 0, mg_tree_frames_want{6000, 0}, plan_of(40, 0), &fl);                 // 4 x 6000: 187 KiB; 2 x: 94 KiB
        CHECK(fl.bytes <= MG_TREE_LDS_MAX && fl.group == 2, "the group is halved: %d", fl.group);
        p = mg_tree_frames_fit(mg_tree_staging{0, 0, 0}, 0, mg_tree_frames_want{12000, 0}, plan_of(40, 0), &fl);
        CHECK(fl.bytes <= MG_TREE_LDS_MAX && fl.group == 1, "down to one child: %d", fl.group);
        p = mg_tree_frames_fit(mg_tree_staging{12, 25, 63}, 1, mg_tree_frames_want{30000, 4000}, plan_of(40, 1), &fl);          // one child's control points: 234 KiB
        CHECK(fl.bytes > MG_TREE_LDS_MAX && fl.group == 1 && fl.tables_lds == 0 && p.s.wrows == 0 && p.s.cp_rows == 0 && p.s.poly_doubles == 0, "a plan that cannot fit comes back bare");
        (void)p;
        plans += 9;
    }
    // the slab
    {
        const int32_t T[3] = {7, 12, 12}, J[3] = {1, 1, 2};
        CHECK(mg_tree_frames_scratch(3, T, J, 1, 15) == (((int64_t)64 * (7 * 3 + 12 * 3 + 12 * 6 + 15) * 8 + 255) & ~(int64_t)255), "slab of three requests and a rotation");
        CHECK(mg_tree_frames_scratch(0, T, J, 0, 15) == 0 && mg_tree_frames_scratch(1, T, J, 0, 7) == 10752, "slab sizes");
        CHECK(MG_TREE_TRACK_GROUP == 4 && MG_TREE_SCRATCH_MAX == ((int64_t)256 << 20), "constants");
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("tree_frames_plan_check: ok (%ld plans)\n", plans);
    return failures ? 1 : 0;
}
