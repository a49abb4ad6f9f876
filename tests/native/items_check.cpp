// What csrc/mg_items_cut.h promises the item-table entry points (mg_items.h): the cut of a call's items into launches against a
// direct restatement, the workgroup-to-item bisection on every launch it makes, and which items share one copy of a latent matrix.
// The workgroup bound of a launch (2^31 - 1) is reached here with sample counts no GPU test can afford.  Plain host code with its
// own main (test infrastructure, never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_items_cut.h"

#include <cstdio>

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

int main() {
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
