// What csrc/mg_dispatch.h promises its launchers: every k-step count reaches its own tag exactly once, any other value reaches
// none and comes back as `miss`, and the flag helpers reach each combination exactly once with the tags in argument order.  Plain
// host code with its own main (test infrastructure, never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_dispatch.h"

#include <climits>
#include <cstdio>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
    // calls[KK]: how often the tag KK was reached, over the whole run
    int calls[32] = {0};
    auto body = [&](auto kk) {
        static_assert(decltype(kk)::value >= 2 && decltype(kk)::value <= 16 && decltype(kk)::value % 2 == 0, "a k-step count outside 2, 4, ..., 16");
        calls[decltype(kk)::value]++;
        return 100 + decltype(kk)::value;
    };
    for (int kk = 2; kk <= 16; kk += 2) {
        const int r = mg_dispatch_kk(kk, -1, body);
        CHECK(r == 100 + kk, "kk=%d: returned %d", kk, r);
        for (int t = 0; t < 32; t++) CHECK(calls[t] == (t % 2 == 0 && t >= 2 && t <= kk ? 1 : 0), "after kk=%d: tag %d reached %d times", kk, t, calls[t]);
    }
    const int misses[] = {-2, 0, 1, 3, 15, 17, 18, INT_MAX};
    for (int kk : misses) {
        const int r = mg_dispatch_kk(kk, -7, body);
        CHECK(r == -7, "kk=%d: returned %d, not miss", kk, r);
    }
    for (int t = 0; t < 32; t++) CHECK(calls[t] == (t % 2 == 0 && t >= 2 && t <= 16 ? 1 : 0), "after the misses: tag %d reached %d times", t, calls[t]);

    // every k-step count, ascending, until a body returns something other than 0
    int order[8], n = 0;
    int rc = mg_each_kk([&](auto kk) { order[n++] = decltype(kk)::value; return 0; });
    CHECK(rc == 0 && n == 8, "mg_each_kk: rc %d after %d calls", rc, n);
    for (int i = 0; i < n; i++) CHECK(order[i] == 2 * (i + 1), "mg_each_kk: call %d had tag %d", i, order[i]);
    n = 0;
    rc = mg_each_kk([&](auto kk) { n++; return decltype(kk)::value == 6 ? -4 : 0; });
    CHECK(rc == -4 && n == 3, "mg_each_kk: rc %d after %d calls, expected -4 after 3", rc, n);

    // flags: combination (a, b, c) is counted in slot a * 4 + b * 2 + c as the TAGS say it, and returned as the ARGUMENTS say it
    int one[2] = {0}, two[4] = {0}, three[8] = {0};
    for (int m = 0; m < 8; m++) {
        const bool a = m & 4, b = m & 2, c = m & 1;
        if (m < 2) {
            const int r = mg_dispatch_flags(c, [&](auto C) { one[decltype(C)::value]++; return (int)decltype(C)::value; });
            CHECK(r == m, "one flag %d: the tag said %d", m, r);
        }
        if (m < 4) {
            const int r = mg_dispatch_flags(b, c, [&](auto B, auto C) {
                const int s = decltype(B)::value * 2 + decltype(C)::value;
                two[s]++;
                return s;
            });
            CHECK(r == m, "two flags %d: the tags said %d", m, r);
        }
        const int r = mg_dispatch_flags(a, b, c, [&](auto A, auto B, auto C) {
            const int s = decltype(A)::value * 4 + decltype(B)::value * 2 + decltype(C)::value;
            three[s]++;
            return s;
        });
        CHECK(r == m, "three flags %d: the tags said %d", m, r);
    }
    for (int s = 0; s < 2; s++) CHECK(one[s] == 1, "one flag: combination %d reached %d times", s, one[s]);
    for (int s = 0; s < 4; s++) CHECK(two[s] == 1, "two flags: combination %d reached %d times", s, two[s]);
    for (int s = 0; s < 8; s++) CHECK(three[s] == 1, "three flags: combination %d reached %d times", s, three[s]);

    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("dispatch_check: ok\n");
    return failures ? 1 : 0;
}
