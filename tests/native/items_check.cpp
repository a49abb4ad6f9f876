// What csrc/mg_items_cut.h promises the item-table entry points (mg_items.h): the cut of a call's items into launches against a
// direct restatement, the workgroup-to-item bisection on every launch it makes, which items share one copy of a latent matrix, and
// where an array lands behind a table.  What csrc/mg_feature_rows.h promises the feature-point entry points: the row plan of the
// host-planned frames against a literal statement of it.  What csrc/mg_step_length_layout.h gives the step-length kernel: its parts
// in order without overlap, and, called as `items_check slen L NB F [L NB F ...]`, the tile, the limit and every shape's total_bytes
// on a line each, for tests/test_step_length_shapes_host.py to compare its restatement with.
// The workgroup bound of a launch (2^31 - 1) is reached here with sample counts no GPU test can afford.  Plain host code with its
// own main (test infrastructure, never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_feature_rows.h"
#include "../../morphablegraphs_amd/csrc/mg_items_cut.h"
#include "../../morphablegraphs_amd/csrc/mg_step_length_layout.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int64_t BOUND = 0x7fffffff;

struct item { int64_t n; int lds; };
struct slot { int32_t wg0; };          // what the bisection reads of a kernel's item

// The rule, restated: launch_of[i] for every non-empty item by counting what the current launch already holds, then every launch's
// figures from its members alone.
static void check_cut(const char *name, const std::vector<item> &items, int tile, int max_items, int expect_launches) {
    std::vector<int32_t> wg0;
    const std::vector<mg_item_launch> got = mg_cut_items((int)items.size(), [&](int i) { return items[(size_t)i].n; }, [&](int i) { return items[(size_t)i].lds; },
                                                         tile, max_items, wg0);
    CHECK(wg0.size() == items.size(), "%s: %zu wg0 values for %zu items", name, wg0.size(), items.size());
    std::vector<int> launch_of(items.size(), -1);
    int n_launches = 0, held = 0;
    int64_t held_wgs = 0;
    for (size_t i = 0; i < items.size(); i++) {
        if (items[i].n == 0) continue;
        const int64_t wgs = items[i].n / tile + (items[i].n % tile ? 1 : 0);
        if (n_launches == 0 || held == max_items || held_wgs + wgs > BOUND) { n_launches++; held = 0; held_wgs = 0; }
        launch_of[i] = n_launches - 1;
        held++;
        held_wgs += wgs;
    }
    CHECK((int)got.size() == n_launches, "%s: %zu launches, the rule makes %d", name, got.size(), n_launches);
    if (expect_launches >= 0) CHECK((int)got.size() == expect_launches, "%s: %zu launches, the case was built for %d", name, got.size(), expect_launches);
    if ((int)got.size() != n_launches || wg0.size() != items.size()) return;
    size_t seen = 0;                    // non-empty items in front of the launch
    for (int l = 0; l < n_launches; l++) {
        std::vector<slot> slice;
        std::vector<int64_t> wgs_of;
        int64_t grid = 0;
        int lds = 0;
        for (size_t i = 0; i < items.size(); i++) {
            if (launch_of[i] != l) continue;
            CHECK(wg0[i] == grid, "%s: item %zu starts at workgroup %d, the items before it in launch %d take %lld", name, i, wg0[i], l, (long long)grid);
            CHECK(slice.empty() || wg0[i] > slice.back().wg0, "%s: item %zu: wg0 %d does not rise", name, i, wg0[i]);
            slice.push_back({wg0[i]});
            wgs_of.push_back((items[i].n + tile - 1) / tile);
            grid += wgs_of.back();
            if (items[i].lds > lds) lds = items[i].lds;
        }
        const mg_item_launch &g = got[(size_t)l];
        CHECK(g.first == seen && g.n_items == (int)slice.size() && g.grid == grid && g.lds == lds, "%s: launch %d is {%zu, %d, %lld, %d}, expected {%zu, %zu, %lld, %d}",
              name, l, g.first, g.n_items, (long long)g.grid, g.lds, seen, slice.size(), (long long)grid, lds);
        CHECK(g.n_items >= 1 && g.n_items <= max_items && g.grid >= 1 && g.grid <= BOUND, "%s: launch %d holds %d items, %lld workgroups", name, l, g.n_items,
              (long long)g.grid);
        CHECK(!slice.empty() && slice[0].wg0 == 0, "%s: launch %d does not start at workgroup 0", name, l);
        // the first and the last workgroup of every item find it
        for (size_t e = 0; e < slice.size(); e++) {
            const int64_t first = slice[e].wg0, last = first + wgs_of[e] - 1;
            const int a = mg_item_at(slice.data(), (int)slice.size(), (int)first), b = mg_item_at(slice.data(), (int)slice.size(), (int)last);
            CHECK(a == (int)e && b == (int)e, "%s: launch %d: workgroups %lld and %lld of item %zu found items %d and %d", name, l, (long long)first, (long long)last, e, a, b);
        }
        seen += slice.size();
    }
    for (size_t i = 0; i < items.size(); i++)
        if (items[i].n == 0) CHECK(wg0[i] == -1, "%s: the empty item %zu has wg0 %d", name, i, wg0[i]);
}

// `count` non-empty items of varying size and LDS, an empty one after every third
static std::vector<item> interleaved(int count) {
    std::vector<item> v;
    for (int i = 0; i < count; i++) {
        v.push_back({1 + (i * 7) % 40, 1000 + (i * 37) % 500});
        if (i % 3 == 2) v.push_back({0, 999999});
    }
    return v;
}

struct lat_item { const void *latents_dev; int64_t n_samples, ld; };

static void check_shared(const char *name, const std::vector<lat_item> &items, const std::vector<int> &expect) {
    const std::vector<int> got = mg_shared_latents(items.data(), (int)items.size());
    CHECK(got == expect, "%s: the shared-latents decision differs", name);
    if (got != expect)
        for (size_t i = 0; i < got.size() && i < expect.size(); i++) std::printf("  item %zu: %d, expected %d\n", i, got[i], expect[i]);
}

// The row plan, literally: sort and unique the slots' tap control points, find every slot's first among them, mark the (control
// point, channel) pairs some range wants, number the marked pairs in order.  Then what the kernels rely on: every wanted channel of
// every tap of a slot is found through tap[] and map[] at the row of E' it means, and nothing else is listed.
static void check_rows(const char *name, int D, const std::vector<int32_t> &first, const std::vector<mg_feature_range> &wanted) {
    const mg_feature_rows got = mg_feature_rows_of(D, first, wanted);
    std::vector<int32_t> cps;
    for (size_t s = 0; s < first.size(); s++)
        for (int j = 0; j < 4; j++) cps.push_back(first[s] + j);
    std::sort(cps.begin(), cps.end());
    cps.erase(std::unique(cps.begin(), cps.end()), cps.end());
    std::vector<int32_t> tap(first.size(), 0);
    for (size_t s = 0; s < first.size(); s++)
        while (cps[(size_t)tap[s]] != first[s]) tap[s]++;
    std::vector<char> need(cps.size() * D, 0);
    for (const mg_feature_range &w : wanted)
        for (int j = 0; j < 4; j++)
            for (int d = w.d0; d < w.d0 + w.count; d++) need[(size_t)(tap[(size_t)w.slot] + j) * D + d] = 1;
    std::vector<int32_t> map(cps.size() * D, -1), src;
    for (size_t c = 0; c < cps.size(); c++)
        for (int d = 0; d < D; d++)
            if (need[c * D + d]) {
                map[c * D + d] = (int32_t)src.size();
                src.push_back(cps[c] * D + d);
            }
    CHECK(got.NCP == (int32_t)cps.size() && got.NRS == (int32_t)src.size(), "%s: %d control points, %d rows; the statement lists %zu and %zu", name, got.NCP, got.NRS,
          cps.size(), src.size());
    CHECK(got.tap == tap, "%s: tap differs", name);
    CHECK(got.map == map, "%s: map differs", name);
    CHECK(got.src == src, "%s: src differs", name);
    if ((size_t)got.NCP != cps.size() || got.map.size() != map.size() || got.tap.size() != first.size()) return;
    size_t listed = 0;
    for (size_t c = 0; c < cps.size(); c++)
        for (int d = 0; d < D; d++) {
            const int32_t row = got.map[c * D + d];
            if (row < 0) continue;
            listed++;
            CHECK(row < got.NRS && (size_t)row < got.src.size() && got.src[(size_t)row] == cps[c] * D + d, "%s: map[%zu][%d] = %d does not name row %d of E'", name, c, d,
                  row, cps[c] * D + d);
        }
    CHECK(listed == got.src.size(), "%s: %zu map entries for %zu rows", name, listed, got.src.size());
    for (size_t e = 1; e < got.src.size(); e++) CHECK(got.src[e] > got.src[e - 1], "%s: src does not rise at %zu", name, e);
    for (const mg_feature_range &w : wanted)
        for (int j = 0; j < 4; j++)
            for (int d = w.d0; d < w.d0 + w.count; d++) {
                const size_t at = (size_t)(got.tap[(size_t)w.slot] + j) * D + d;
                CHECK(at < got.map.size() && got.map[at] >= 0 && got.src[(size_t)got.map[at]] == (first[(size_t)w.slot] + j) * D + d,
                      "%s: slot %d, tap %d, channel %d is not found at its row", name, w.slot, j, d);
            }
}

// the plain kernel's three slots (root xyz; root xyz and the quaternions at `quats`; the root's seven) and the time-warped kernel's two
static void check_plans(const char *name, int D, const std::vector<int32_t> &first, const std::vector<int> &quats) {
    std::vector<mg_feature_range> three = {{0, 0, 3}, {1, 0, 3}, {2, 0, 7}};
    for (const int qc : quats) three.push_back({1, qc, 4});
    check_rows(name, D, first, three);
    check_rows(name, D, {first[0], first[2]}, {{0, 0, 3}, {1, 0, 7}});
}

// the step-length workgroup's LDS: every part starts where the one before it ends, the int32 tail behind the doubles
static void check_slen_layout(int L, int NB, int F) {
    const mg_slen_layout y = mg_slen_layout_of(L, NB, F);
    const int T = MG_SLEN_TILE;
    CHECK(y.NR == 3 * NB && y.FS >= F && y.FS <= F + 1 && (y.FS & 1), "slen %d %d %d: NR %d, FS %d", L, NB, F, y.NR, y.FS);
    CHECK(y.E == 0 && y.mean - y.E == L * y.NR && y.w - y.mean == y.NR && y.lat - y.w == 4 * F && y.cp - y.lat == T * L && y.seg - y.cp == T * y.NR &&
              y.ints - y.seg == T * y.FS && y.total_bytes == y.ints * 8 + 4 * (F + T),
          "slen %d %d %d: the parts are not back to back", L, NB, F);
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "slen") == 0) {
        std::printf("tile %d\nlds_max %d\n", MG_SLEN_TILE, MG_SLEN_LDS_MAX);
        for (int a = 2; a + 2 < argc; a += 3) {
            const int L = std::atoi(argv[a]), NB = std::atoi(argv[a + 1]), F = std::atoi(argv[a + 2]);
            std::printf("%d %d %d %d\n", L, NB, F, mg_slen_layout_of(L, NB, F).total_bytes);
        }
        return 0;
    }
    for (const int L : {1, 3, 64, 65})
        for (const int NB : {4, 7, 64})
            for (const int F : {2, 3, 127, 128, 257}) check_slen_layout(L, NB, F);
    for (const int D : {7, 8, 79}) {
        const std::vector<std::vector<int>> quat_sets = {{}, {3}, {D - 4}, {3, D - 4, 3}};
        for (const std::vector<int> &quats : quat_sets) {
            check_plans("one frame", D, {0, 0, 0}, quats);
            check_plans("one frame, later", D, {5, 5, 5}, quats);
            check_plans("frame 0 as the mid frame", D, {0, 0, 9}, quats);
            check_plans("frame F - 1 as the mid frame", D, {0, 9, 9}, quats);
            for (int shared = 1; shared <= 3; shared++) {
                check_plans("mid window overlaps the first", D, {0, 4 - shared, 12}, quats);
                check_plans("mid window overlaps the last", D, {0, 8 + shared, 12}, quats);
                check_plans("all three overlap", D, {0, 4 - shared, 3}, quats);
            }
            check_plans("adjacent windows", D, {0, 4, 8}, quats);
            check_plans("disjoint windows", D, {2, 11, 40}, quats);
        }
    }
    // seeded random slot sets: one to four slots in any order, ranges anywhere in 0 .. D
    {
        uint32_t state = 12345u;
        auto draw = [&](int n) { state = state * 1664525u + 1013904223u; return (int)((state >> 8) % (uint32_t)n); };
        for (int round = 0; round < 4000; round++) {
            const int D = 7 + draw(6), slots = 1 + draw(4);
            std::vector<int32_t> first;
            for (int s = 0; s < slots; s++) first.push_back(draw(12));
            std::vector<mg_feature_range> wanted;
            for (int r = draw(8); r > 0; r--) {
                const int d0 = draw(D), count = draw(D - d0 + 1);
                wanted.push_back({draw(slots), d0, count});
            }
            check_rows("random", D, first, wanted);
        }
    }

    // an array behind a table: at the next multiple of 8, the gap zeroed, an empty array at its place too
    {
        std::vector<unsigned char> table(13, 0xff);
        const int32_t three[3] = {1, 2, 3};
        const size_t a = mg_table_append(table, three, sizeof(three)), b = mg_table_append(table, nullptr, 0), c = mg_table_append(table, three, 4);
        CHECK(a == 16 && b == 32 && c == 32 && table.size() == 36, "appends at %zu, %zu, %zu, %zu bytes in all", a, b, c, table.size());
        CHECK(table[12] == 0xff && table[13] == 0 && table[15] == 0 && table[16] == 1 && table[28] == 0 && table[32] == 1, "the appended bytes");
        const std::vector<int> of = mg_nonempty_items(5, [](int i) { return i % 2 ? 0 : 7; });
        CHECK(of == std::vector<int>({0, 2, 4}), "the non-empty items");
    }

    const int MAX = 8;
    check_cut("no items", {}, 16, MAX, 0);
    check_cut("all empty", {{0, 5}, {0, 7}, {0, 9}}, 16, MAX, 0);
    check_cut("one item", {{100, 4096}}, 16, MAX, 1);
    check_cut("max - 1 items", interleaved(MAX - 1), 16, MAX, 1);
    check_cut("max items", interleaved(MAX), 16, MAX, 1);
    check_cut("max + 1 items", interleaved(MAX + 1), 16, MAX, 2);
    check_cut("2 max + 1 items", interleaved(2 * MAX + 1), 16, MAX, 3);
    check_cut("the library's cap", interleaved(2 * 256 + 1), 16, 256, 3);
    check_cut("tile remainders", {{1, 10}, {15, 30}, {16, 20}, {17, 5}}, 16, MAX, 1);
    // the workgroup bound
    check_cut("workgroups sum to the bound", {{(BOUND - 5) * 16, 100}, {0, 1}, {5 * 16 - 3, 200}}, 16, MAX, 1);
    check_cut("one workgroup past the bound", {{(BOUND - 5) * 16, 100}, {0, 1}, {5 * 16 + 1, 200}, {40, 50}}, 16, MAX, 2);
    check_cut("one item of the bound", {{BOUND * 16, 100}}, 16, MAX, 1);
    check_cut("one item of the bound, then another", {{BOUND * 16 - 15, 100}, {1, 300}}, 16, MAX, 2);

    // the bisection where the last workgroup of a launch is the bound's
    {
        const slot two[2] = {{0}, {(int32_t)(BOUND - 5)}};
        CHECK(mg_item_at(two, 2, (int)(BOUND - 6)) == 0 && mg_item_at(two, 2, (int)(BOUND - 5)) == 1 && mg_item_at(two, 2, (int)(BOUND - 1)) == 1,
              "the bisection at the workgroup bound");
    }

    static const double A[4] = {0}, B[4] = {0};
    check_shared("three items on one matrix", {{A, 4, 1}, {A, 4, 1}, {A, 4, 1}}, {-1, 0, 0});
    check_shared("same pointer, other n_samples or ld", {{A, 4, 1}, {A, 2, 1}, {A, 4, 2}, {A, 2, 1}}, {-1, -1, -1, 1});
    check_shared("an empty item between two sharers", {{A, 4, 1}, {A, 0, 1}, {A, 4, 1}, {B, 4, 1}, {B, 4, 1}}, {-1, -1, 0, -1, 3});
    check_shared("empty items share nothing", {{A, 0, 1}, {A, 0, 1}}, {-1, -1});
    check_shared("no items", {}, {});

    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("items_check: ok\n");
    return failures ? 1 : 0;
}
