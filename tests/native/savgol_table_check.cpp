// csrc/mg_savgol_table.h on its own (host compiler, no HIP, no Python): the 225 doubles of the Savitzky-Golay hat matrix, one per line as
// "row column %a", for tests/test_time_smoothing_host.py to compare with time_smoothing.savgol_hat_matrix(); before that the table's
// own properties in exact integer arithmetic -- symmetric, rows sum to the denominator (a constant is reproduced), idempotent
// (H H = H: a projection), row 7 the classic smoothing weights over 1105.  Any failure: a line on stderr and exit status 1.
#include <cstdint>
#include <cstdio>

#include "../../morphablegraphs_amd/csrc/mg_savgol_table.h"

int main() {
    int bad = 0;
    const int64_t den = MG_SAVGOL_DENOMINATOR;
    for (int i = 0; i < MG_SAVGOL_WINDOW; i++) {
        int64_t sum = 0;
        for (int j = 0; j < MG_SAVGOL_WINDOW; j++) {
            sum += mg_savgol_numerators[i][j];
            if (mg_savgol_numerators[i][j] != mg_savgol_numerators[j][i]) { std::fprintf(stderr, "not symmetric at %d %d\n", i, j); bad = 1; }
            int64_t dot = 0;
            for (int k = 0; k < MG_SAVGOL_WINDOW; k++) dot += (int64_t)mg_savgol_numerators[i][k] * mg_savgol_numerators[k][j];
            if (dot != den * mg_savgol_numerators[i][j]) { std::fprintf(stderr, "not idempotent at %d %d\n", i, j); bad = 1; }
        }
        if (sum != den) { std::fprintf(stderr, "row %d sums to %lld\n", i, (long long)sum); bad = 1; }
    }
    static const int classic[MG_SAVGOL_WINDOW] = {-78, -13, 42, 87, 122, 147, 162, 167, 162, 147, 122, 87, 42, -13, -78};
    for (int j = 0; j < MG_SAVGOL_WINDOW; j++)
        if ((int64_t)mg_savgol_numerators[MG_SAVGOL_HALF][j] * 1105 != den * classic[j]) { std::fprintf(stderr, "row 7, column %d\n", j); bad = 1; }
    double H[MG_SAVGOL_WINDOW * MG_SAVGOL_WINDOW];
    mg_savgol_hat_matrix(H);
    for (int i = 0; i < MG_SAVGOL_WINDOW; i++)
        for (int j = 0; j < MG_SAVGOL_WINDOW; j++) std::printf("%d %d %a\n", i, j, H[MG_SAVGOL_WINDOW * i + j]);
    return bad;
}
