// The Savitzky-Golay pass of the reference's smoothed time functions as ONE table (host-only, plain C++): scipy.signal.savgol_filter(t,
// 15, 3) in its default mode "interp" (motion_model/motion_primitive.py:321-331) is a fixed linear map with a 15-sample footprint.  With
// H = A (A^T A)^-1 A^T, A[i][k] = (i - 7)^k, the 15 x 15 hat matrix of the least-squares cubic on 15 equally spaced points, sample q of
// a row of T >= 15 samples is
//   q < 7        row q of H times the first 15 samples
//   q >= T - 7   row 15 - (T - q) of H times the last 15 samples
//   otherwise    row 7 of H times samples q - 7 .. q + 7 (row 7: (-78, -13, 42, 87, 122, 147, 162, 167, ...) / 1105)
// The entries are exact integers over one denominator (1105 * 252); a double is ONE division of two exactly representable integers,
// which is correctly rounded: the same 225 doubles as time_smoothing.savgol_hat_matrix(), which divides the same fractions.  The
// kernels read them from the context's cached device table (MG_TABLE_SAVGOL); the statements: mg_timewarp_device.h.
#pragma once
#include <cstdint>

#define MG_SAVGOL_WINDOW 15
#define MG_SAVGOL_HALF 7
#define MG_SAVGOL_DENOMINATOR 278460

static const int32_t mg_savgol_numerators[MG_SAVGOL_WINDOW][MG_SAVGOL_WINDOW] = {
    {187369, 104104, 44044, 4004, -19201, -28756, -27846, -19656, -7371, 5824, 16744, 22204, 19019, 4004, -26026},
    {104104, 75829, 52624, 34034, 19604, 8879, 1404, -3276, -5616, -6071, -5096, -3146, -676, 1859, 4004},
    {44044, 52624, 54709, 51524, 44294, 34244, 22599, 10584, -576, -9656, -15431, -16676, -12166, -676, 19019},
    {4004, 34034, 51524, 58504, 57004, 49054, 36684, 21924, 6804, -6646, -16396, -20416, -16676, -3146, 22204},
    {-19201, 19604, 44294, 57004, 59869, 55024, 44604, 30744, 15579, 1244, -10126, -16396, -15431, -5096, 16744},
    {-28756, 8879, 34244, 49054, 55024, 53869, 47304, 37044, 24804, 12299, 1244, -6646, -9656, -6071, 5824},
    {-27846, 1404, 22599, 36684, 44604, 47304, 45729, 40824, 33534, 24804, 15579, 6804, -576, -5616, -7371},
    {-19656, -3276, 10584, 21924, 30744, 37044, 40824, 42084, 40824, 37044, 30744, 21924, 10584, -3276, -19656},
    {-7371, -5616, -576, 6804, 15579, 24804, 33534, 40824, 45729, 47304, 44604, 36684, 22599, 1404, -27846},
    {5824, -6071, -9656, -6646, 1244, 12299, 24804, 37044, 47304, 53869, 55024, 49054, 34244, 8879, -28756},
    {16744, -5096, -15431, -16396, -10126, 1244, 15579, 30744, 44604, 55024, 59869, 57004, 44294, 19604, -19201},
    {22204, -3146, -16676, -20416, -16396, -6646, 6804, 21924, 36684, 49054, 57004, 58504, 51524, 34034, 4004},
    {19019, -676, -12166, -16676, -15431, -9656, -576, 10584, 22599, 34244, 44294, 51524, 54709, 52624, 44044},
    {4004, 1859, -676, -3146, -5096, -6071, -5616, -3276, 1404, 8879, 19604, 34034, 52624, 75829, 104104},
    {-26026, 4004, 19019, 22204, 16744, 5824, -7371, -19656, -27846, -28756, -19201, 4004, 44044, 104104, 187369},
};

// H as 225 doubles, row-major: H[15 * row + k]
static inline void mg_savgol_hat_matrix(double *H) {
    for (int r = 0; r < MG_SAVGOL_WINDOW; r++)
        for (int k = 0; k < MG_SAVGOL_WINDOW; k++) H[MG_SAVGOL_WINDOW * r + k] = (double)mg_savgol_numerators[r][k] / (double)MG_SAVGOL_DENOMINATOR;
}
