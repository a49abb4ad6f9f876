// What the images of csrc/mg_pack.h must contain, checked by DECODING them: every element index of an image is taken apart into
// (tile, k-step, lane) and the value there compared with the source matrix; every source element must turn up exactly once.  Plain
// host code with its own main (test infrastructure, never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_pack.h"

#include <cstdio>
#include <functional>
#include <string>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the k-steps of a latent width L (mg_primitive_create): groups of four, an even number of them
static int kk_of(int L) { return (((L + 3) / 4 + 1) / 2) * 2; }

// one source: I x Kx values, inside(i, k) says which of them the matrix, the triangle or the band holds
static void check_fragments(const char *what, int I, int Kx, int KK, const std::function<bool(int, int)> &inside) {
    const int tiles = (I + 15) / 16;
    auto value = [&](int i, int k) { return 1.0 + (double)i * Kx + k; };   // no two alike, none zero
    std::vector<double> image((size_t)tiles * KK * 64, -1.0);
    mg_pack_fragments(image.data(), tiles, KK, [&](int i, int k) { return i < I && k < Kx && inside(i, k) ? value(i, k) : 0.0; });
    std::vector<int> seen((size_t)I * Kx, 0);
    for (size_t e = 0; e < image.size(); e++) {
        const int lane = (int)(e % 64), kk = (int)(e / 64 % KK), tile = (int)(e / 64 / KK);
        const int i = 16 * tile + (lane & 15), k = 4 * kk + (lane >> 4);
        const bool in = i < I && k < Kx;
        CHECK(image[e] == (in && inside(i, k) ? value(i, k) : 0.0), "%s I=%d Kx=%d KK=%d: element %zu (i=%d, k=%d) holds %g", what, I, Kx, KK, e, i, k, image[e]);
        if (in) seen[(size_t)i * Kx + k]++;
    }
    for (size_t s = 0; s < seen.size(); s++) CHECK(seen[s] == 1, "%s I=%d Kx=%d KK=%d: source element %zu appears %d times", what, I, Kx, KK, s, seen[s]);
}

static void check_regroup(int tiles, int KK, int G) {
    const size_t n = (size_t)tiles * KK * 64;
    std::vector<float> plain(n), out(n, -1.0f);
    for (size_t e = 0; e < n; e++) plain[e] = (float)(e + 1);   // exact in float32 at these sizes, no two alike
    mg_pack_regroup(plain.data(), out.data(), tiles, KK, G);
    std::vector<int> seen(n, 0);
    const size_t whole = (size_t)(KK / G) * 64 * G;   // a tile's elements that sit in whole groups; behind them the remaining pair
    for (size_t e = 0; e < n; e++) {
        const size_t tile = e / ((size_t)KK * 64), r = e % ((size_t)KK * 64);
        size_t kk, lane;
        if (r < whole) { kk = r / (64 * G) * G + r % G; lane = r / G % 64; }
        else { kk = (size_t)(KK / G) * G + (r - whole) % 2; lane = (r - whole) / 2; }
        CHECK(kk < (size_t)KK && lane < 64, "regroup KK=%d G=%d: element %zu decodes to k-step %zu, lane %zu", KK, G, e, kk, lane);
        if (kk >= (size_t)KK || lane >= 64) continue;
        const size_t src = (tile * KK + kk) * 64 + lane;
        CHECK(out[e] == plain[src], "regroup KK=%d G=%d: element %zu holds %g, plain[%zu] = %g", KK, G, e, out[e], src, plain[src]);
        seen[src]++;
    }
    for (size_t s = 0; s < n; s++) CHECK(seen[s] == 1, "regroup KK=%d G=%d: plain element %zu appears %d times", KK, G, s, seen[s]);
}

static void check_chains() {
    std::vector<int> ch;
    int bad = -7;
    const int32_t root[] = {-1};
    CHECK(mg_joint_chain(root, 1, 0, ch, &bad) == MG_CHAIN_OK && ch == std::vector<int>({0}), "the root alone");
    CHECK(mg_joint_chain(nullptr, 0, 0, ch) == MG_CHAIN_OK && ch == std::vector<int>({0}), "no skeleton: the root alone");
    CHECK(mg_joint_chain(nullptr, 0, 1, ch, &bad) == MG_CHAIN_NO_JOINT && bad == 1 && ch.empty(), "no skeleton: joint 1");
    //                       0   1  2  3  4  5  6
    const int32_t tree[] = {-1, 0, 1, 1, 3, 0, 5};
    CHECK(mg_joint_chain(tree, 7, 4, ch) == MG_CHAIN_OK && ch == std::vector<int>({0, 1, 3, 4}), "leaf 4 of the branching skeleton");
    CHECK(mg_joint_chain(tree, 7, 6, ch) == MG_CHAIN_OK && ch == std::vector<int>({0, 5, 6}), "leaf 6 of the branching skeleton");
    CHECK(mg_joint_chain(tree, 7, 7, ch, &bad) == MG_CHAIN_NO_JOINT && bad == 7 && ch.empty(), "joint 7 of 7");
    CHECK(mg_joint_chain(tree, 7, -1, ch, &bad) == MG_CHAIN_NO_JOINT && bad == -1 && ch.empty(), "joint -1");
    const int32_t loop[] = {-1, 0, 3, 2};   // 2 and 3 name each other
    CHECK(mg_joint_chain(loop, 4, 3, ch, &bad) == MG_CHAIN_ORDER && bad == 2 && ch.empty(), "a parent behind its child: bad = %d", bad);
    CHECK(std::string("joint 7") + mg_chain_why(MG_CHAIN_NO_JOINT) == "joint 7 out of range" &&
          std::string("joint 2") + mg_chain_why(MG_CHAIN_ORDER) == "joint 2: parents must precede their children", "the words of a failed chain");
    const int32_t self[] = {-1, 1};
    CHECK(mg_joint_chain(self, 2, 1, ch, &bad) == MG_CHAIN_ORDER && bad == 1 && ch.empty(), "a joint that is its own parent: bad = %d", bad);
    CHECK(mg_joint_chain(loop, 4, 1, ch) == MG_CHAIN_OK && ch == std::vector<int>({0, 1}), "the sound part of that skeleton");

    // links of root .. 4: {channel of 0, offset of 1}, {channel of 1, offset of 3}, {channel of 3, offset of 4}
    double offsets[7 * 3], rec[2 + 4 * 3];
    for (int q = 0; q < 7 * 3; q++) offsets[q] = 100.0 + q;
    for (double &v : rec) v = -9.0;
    const int channel[] = {3, -1, 7, 11, 15, 19, 23};
    mg_joint_chain(tree, 7, 4, ch);
    mg_chain_links(ch, offsets, [&](int j) { return channel[j]; }, rec + 1);
    const double want[] = {-9.0, 3.0, 103.0, 104.0, 105.0, -1.0, 109.0, 110.0, 111.0, 11.0, 112.0, 113.0, 114.0, -9.0};
    for (int q = 0; q < 14; q++) CHECK(rec[q] == want[q], "link record[%d] = %g, expected %g", q, rec[q], want[q]);
}

int main() {
    const int extents[] = {1, 15, 16, 17, 33}, widths[] = {1, 3, 4, 5, 8, 9, 40, 63, 64};
    bool tail = false, no_tail = false;
    for (int I : extents)
        for (int L : widths) {
            const int KK = kk_of(L);
            (KK % 4 == 2 ? tail : no_tail) = true;
            check_fragments("full", I, L, KK, [](int, int) { return true; });
            check_fragments("upper", I, L, KK, [](int i, int k) { return i <= k; });    // the precision factor, reduced over its column index
            check_fragments("lower", I, L, KK, [](int i, int k) { return k <= i; });    // the Cholesky factor (and the precision factor's other image)
            // four taps per row, the row's first tap at an offset of its own; the columns are all 4 KK of the k-steps
            const int Kx = 4 * KK;
            check_fragments("band", I, Kx, KK, [&](int i, int k) { const int j = k - (i * 5 + 2) % (Kx - 3); return j >= 0 && j < 4; });
            const int tiles = (I + 15) / 16;
            check_regroup(tiles, KK, 2);
            check_regroup(tiles, KK, 4);
        }
    CHECK(tail && no_tail, "the widths must give KK %% 4 == 0 and KK %% 4 == 2");
    check_chains();
    if (failures) std::printf("pack_check: %d checks failed\n", failures);
    return failures ? 1 : 0;
}
