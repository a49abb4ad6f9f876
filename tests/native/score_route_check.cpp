// What csrc/mg_score_route.h promises the keyframe scorers: mg_score_route_of against a restatement written the other way round (the
// candidate kernels in order of preference, each with the conditions under which it may take the call) over a dense grid of k-step
// counts, row tiles, constraint counts, batch sizes and options, and the named edges as numbers.  The workgroup bound (2^31 - 1) is
// reached here with batch sizes no GPU test can afford.  Plain host code with its own main (test infrastructure, never linked into
// the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_score_route.h"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int64_t BOUND = 0x7fffffff, KB = 1024;

struct expect { int status, kernel; int64_t lds, grid; bool opt_in; };

static int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b ? 1 : 0); }

// The rule, restated.  Bytes per double 8; a tile-kernel wave keeps 16 candidates x (16 RT + 1) channels and n x 16 residuals, a
// wide-kernel wave 64 x (16 RT + 1) channels, four waves each; the VALU workgroup 64 x (L + 1) latents and n x 64 residuals.
static expect restated(int KK, int L, int RT, int n, int64_t B, int opt, int force, bool wpack) {
    const int64_t nn = n < 1 ? 1 : n;
    const bool kk_ok = KK >= 2 && KK <= 16 && KK % 2 == 0;
    const int64_t wide_lds = 4 * 64 * (16 * (int64_t)RT + 1) * 8, tile_lds = 4 * (16 * (16 * (int64_t)RT + 1) + 16 * nn) * 8, valu_lds = 64 * ((int64_t)L + 1 + nn) * 8;
    const bool matrix_pipe = wpack && force == 0 && kk_ok;
    const bool wide_asked = opt == 2 || (opt == 0 && B >= 49152);
    const bool wide_fits = wide_lds <= 64 * KB;                 // RT == 1
    if (matrix_pipe && wide_asked && wide_fits && ceil_div(B, 256) <= BOUND) return {0, MG_SCORE_KERNEL_WIDE, wide_lds, ceil_div(B, 256), false};
    // (a wide launch that fits LDS and has too many workgroups goes to the VALU kernel, not to the tile kernel)
    const bool tile_allowed = matrix_pipe && !(wide_asked && wide_fits);
    if (tile_allowed && tile_lds <= 150 * KB && ceil_div(B, 64) <= BOUND) return {0, MG_SCORE_KERNEL_TILE, tile_lds, ceil_div(B, 64), tile_lds > 64 * KB};
    if (valu_lds > 150 * KB) return {MG_SCORE_REFUSED_LDS, MG_SCORE_KERNEL_VALU, valu_lds, ceil_div(B, 64), true};
    if (ceil_div(B, 64) > BOUND) return {MG_SCORE_REFUSED_SAMPLES, MG_SCORE_KERNEL_VALU, valu_lds, ceil_div(B, 64), valu_lds > 64 * KB};
    return {0, MG_SCORE_KERNEL_VALU, valu_lds, ceil_div(B, 64), valu_lds > 64 * KB};
}

static long checked = 0;
static int seen[3][2] = {{0, 0}, {0, 0}, {0, 0}}, refused[3] = {0, 0, 0};

static void check_one(int KK, int L, int RT, int n, int64_t B, int opt, int force, bool wpack) {
    mg_score_route r = {-1, 0, false, 0};
    const int status = mg_score_route_of(KK, L, RT, n, B, opt, force, wpack, &r);
    const expect e = restated(KK, L, RT, n, B, opt, force, wpack);
    checked++;
    CHECK(status == e.status, "KK %d L %d RT %d n %d B %lld opt %d force %d wpack %d: status %d, restated %d", KK, L, RT, n, (long long)B, opt, force, (int)wpack, status, e.status);
    if (status != e.status) return;
    refused[status]++;
    if (status != MG_SCORE_ROUTE_OK) return;
    CHECK(r.kernel == e.kernel && (int64_t)r.lds == e.lds && r.grid == e.grid && r.opt_in == e.opt_in,
          "KK %d L %d RT %d n %d B %lld opt %d force %d wpack %d: {%d, %zu, %d, %lld}, restated {%d, %lld, %d, %lld}", KK, L, RT, n, (long long)B, opt, force, (int)wpack,
          r.kernel, r.lds, (int)r.opt_in, (long long)r.grid, e.kernel, (long long)e.lds, (int)e.opt_in, (long long)e.grid);
    CHECK(r.grid >= 1 && r.grid <= BOUND && r.lds <= (size_t)(150 * KB) && (r.kernel != MG_SCORE_KERNEL_WIDE || (r.lds <= (size_t)(64 * KB) && !r.opt_in)), "a launch outside the limits");
    if (r.kernel >= 0 && r.kernel < 3) seen[r.kernel][r.opt_in ? 1 : 0]++;
}

static mg_score_route route(int KK, int L, int RT, int n, int64_t B, int opt, int force, bool wpack, int *status) {
    mg_score_route r = {-1, 0, false, 0};
    *status = mg_score_route_of(KK, L, RT, n, B, opt, force, wpack, &r);
    return r;
}

int main() {
    // the dense grid: every k-step count the primitives can have and their neighbours, row tiles through both tile-kernel thresholds
    // (RT = 31 / 32 at n = 1: 64 KiB; RT = 74 / 75: 150 KiB), constraint counts through the VALU kernel's (L = 8: n = 119 / 120 and 291 / 292)
    const std::vector<int64_t> batches = {1, 15, 16, 17, 48, 49, 63, 64, 65, 255, 256, 257, 4099, 49151, 49152, 49153, 65536,
                                          64 * BOUND - 1, 64 * BOUND, 64 * BOUND + 1, 256 * BOUND - 1, 256 * BOUND, 256 * BOUND + 1};
    const std::vector<int> ns = {0, 1, 3, 4, 5, 16, 31, 32, 33, 60, 61, 74, 75, 76, 110, 111, 119, 120, 121, 282, 283, 290, 291, 292, 293, 400};
    const std::vector<int> tiles = {0, 1, 2, 3, 4, 5, 6, 7, 14, 21, 30, 31, 32, 33, 60, 73, 74, 75, 76, 80};
    for (int KK = -1; KK <= 19; KK++)
        for (int RT : tiles)
            for (int n : ns)
                for (int64_t B : batches)
                    for (int opt = 0; opt <= 3; opt++)
                        for (int force = 0; force <= 2; force++)
                            for (int wpack = 0; wpack <= 1; wpack++) {
                                if (force == 2 && (RT % 7 || KK % 3)) continue;     // (any non-zero value forces; sampled thinly)
                                const int L = KK >= 2 && KK <= 16 ? std::min(64, 4 * KK - (RT % 4)) : 65 + RT;
                                check_one(KK, L, RT, n, B, opt, force, wpack != 0);
                            }
    CHECK(seen[MG_SCORE_KERNEL_WIDE][0] > 0 && seen[MG_SCORE_KERNEL_WIDE][1] == 0, "the wide kernel: %d launches, %d with the opt-in", seen[2][0], seen[2][1]);
    CHECK(seen[MG_SCORE_KERNEL_TILE][0] > 0 && seen[MG_SCORE_KERNEL_TILE][1] > 0 && seen[MG_SCORE_KERNEL_VALU][0] > 0 && seen[MG_SCORE_KERNEL_VALU][1] > 0, "a route the grid never took");
    CHECK(refused[MG_SCORE_REFUSED_LDS] > 0 && refused[MG_SCORE_REFUSED_SAMPLES] > 0, "a refusal the grid never met");

    // the named edges, as numbers
    int st = 0;
    mg_score_route r = route(2, 8, 1, 2, 65, 2, 0, true, &st);
    CHECK(st == 0 && r.kernel == MG_SCORE_KERNEL_WIDE && r.lds == 34816 && r.grid == 1, "16 rows under option 2");
    r = route(2, 8, 2, 3, 65, 2, 0, true, &st);
    CHECK(st == 0 && r.kernel == MG_SCORE_KERNEL_TILE && r.lds == 512u * (33 + 3) && r.grid == 2 && !r.opt_in, "17 rows under option 2 keep the tile kernel");
    CHECK(route(2, 8, 1, 2, 49151, 0, 0, true, &st).kernel == MG_SCORE_KERNEL_TILE && route(2, 8, 1, 2, 49152, 0, 0, true, &st).kernel == MG_SCORE_KERNEL_WIDE, "the automatic switch");
    CHECK(route(2, 8, 1, 2, 49152, 1, 0, true, &st).kernel == MG_SCORE_KERNEL_TILE && route(2, 8, 1, 2, 49152, 0, 1, true, &st).kernel == MG_SCORE_KERNEL_VALU, "options 1 and force");
    CHECK(route(2, 8, 1, 2, 256, 2, 0, true, &st).grid == 1 && route(2, 8, 1, 2, 257, 2, 0, true, &st).grid == 2, "the wide kernel's second workgroup");
    // tile LDS 512 (16 RT + 1 + n): three-row constraints, RT = ceil(3 n / 16)
    auto tile3 = [&](int n) { return route(2, 8, (3 * n + 15) / 16, n, 17, 0, 0, true, &st); };
    CHECK(tile3(31).lds == 512u * (97 + 31) && tile3(31).lds == 64u * KB && !tile3(31).opt_in && tile3(32).opt_in && tile3(32).kernel == MG_SCORE_KERNEL_TILE, "tile: 64 KiB between 31 and 32");
    CHECK(tile3(74).kernel == MG_SCORE_KERNEL_TILE && tile3(74).lds == 512u * (225 + 74) && tile3(75).kernel == MG_SCORE_KERNEL_VALU && tile3(75).lds == 512u * (9 + 75), "tile: 150 KiB between 74 and 75");
    // VALU LDS 512 (L + 1 + n)
    auto valu = [&](int L, int n) { return route(0, L, 0, n, 17, 0, 0, false, &st); };
    CHECK(!valu(65, 62).opt_in && valu(65, 62).lds == 64u * KB && valu(65, 63).opt_in, "VALU: 64 KiB between n = 62 and 63 at L = 65");
    r = valu(65, 234);
    CHECK(st == 0 && r.lds == 150u * KB, "VALU: n = 234 at L = 65 fills 150 KiB");
    (void)valu(65, 235);
    CHECK(st == MG_SCORE_REFUSED_LDS, "VALU: n = 235 at L = 65 is refused");
    r = valu(65, 0);
    CHECK(st == 0 && r.lds == 512u * 67, "n = 0 keeps one residual row");
    // the workgroup bound: wide past it goes to VALU, tile past it goes to VALU, VALU past it is refused
    CHECK(route(2, 8, 1, 2, 256 * BOUND, 2, 0, true, &st).kernel == MG_SCORE_KERNEL_WIDE && st == 0, "the largest wide batch");
    (void)route(2, 8, 1, 2, 256 * BOUND + 1, 2, 0, true, &st);
    CHECK(st == MG_SCORE_REFUSED_SAMPLES, "one candidate more");
    CHECK(route(2, 8, 2, 3, 64 * BOUND, 1, 0, true, &st).kernel == MG_SCORE_KERNEL_TILE && st == 0, "the largest tile batch");
    (void)route(2, 8, 2, 3, 64 * BOUND + 1, 1, 0, true, &st);
    CHECK(st == MG_SCORE_REFUSED_SAMPLES, "one candidate more, tile");

    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("score_route_check: ok (%ld routes)\n", checked);
    return failures ? 1 : 0;
}
