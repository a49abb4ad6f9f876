"""The Savitzky-Golay pass of a smoothed time function (smooth_time_parameters, reference motion_model/motion_primitive.py:284-285,
320-331: scipy.signal.savgol_filter(t, 15, 3)) as a table, on the host: the NumPy statement of what csrc/mg_timewarp_device.h states
for the kernels (mg_tw_smooth_window, mg_tw_smoothed) over the table of csrc/mg_savgol_table.h.

savgol_filter in its default mode "interp" is a fixed linear map with a 15-sample footprint.  With H = A (A^T A)^-1 A^T,
A[i][k] = (i - 7)^k, the hat matrix of the least-squares cubic on 15 equally spaced points, sample q of a row of T >= 15 samples is

    q < 7         row q of H times the first 15 samples
    q >= T - 7    row 15 - (T - q) of H times the last 15 samples
    otherwise     row 7 of H times samples q - 7 .. q + 7   (row 7: (-78, -13, 42, 87, 122, 147, 162, 167, ...) / 1105)

so a smoothed sample needs 15 unsmoothed ones and no row in memory.  Window 15 and order 3 are the reference's constants."""
from fractions import Fraction

import numpy as np

WINDOW = 15
HALF = 7
ORDER = 3


def _hat_matrix_fractions():
    """H in exact rationals: Gauss-Jordan on A^T A (4 x 4), then A (A^T A)^-1 A^T."""
    A = [[Fraction((i - HALF) ** k) for k in range(ORDER + 1)] for i in range(WINDOW)]
    n = ORDER + 1
    G = [[sum(A[i][r] * A[i][c] for i in range(WINDOW)) for c in range(n)] + [Fraction(int(r == c)) for c in range(n)] for r in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if G[r][c] != 0)
        G[c], G[p] = G[p], G[c]
        G[c] = [v / G[c][c] for v in G[c]]
        for r in range(n):
            if r != c and G[r][c] != 0:
                f = G[r][c]
                G[r] = [a - f * b for a, b in zip(G[r], G[c])]
    inv = [row[n:] for row in G]
    AG = [[sum(A[i][k] * inv[k][c] for k in range(n)) for c in range(n)] for i in range(WINDOW)]
    return [[sum(AG[i][k] * A[j][k] for k in range(n)) for j in range(WINDOW)] for i in range(WINDOW)]


_H = None


def savgol_hat_matrix():
    """The (15, 15) float64 hat matrix: every entry its Fraction rounded once (numerator / denominator of two exactly representable
    integers, one correctly rounded division) -- the 225 doubles of csrc/mg_savgol_table.h."""
    global _H
    if _H is None:
        _H = np.array([[v.numerator / v.denominator for v in row] for row in _hat_matrix_fractions()], dtype=np.float64)
        _H.setflags(write=False)
    return _H


def smooth_window(q, T):
    """(row of H, first unsmoothed sample) of smoothed sample q of a row of T >= 15 samples: mg_tw_smooth_window."""
    if q < HALF:
        return q, 0
    if q >= T - HALF:
        return WINDOW - (T - q), T - WINDOW
    return HALF, q - HALF


def smooth_time_row_host(row):
    """savgol_filter(row, 15, 3) as the kernels state it: per sample acc = H[r][0] u[0], then acc = acc + H[r][k] u[k] for
    k = 1 .. 14, every product and every sum rounded on its own.  ValueError, in scipy's words, for fewer than 15 samples."""
    row = np.asarray(row, dtype=np.float64)
    if row.ndim != 1:
        raise ValueError("one row of samples")
    T = len(row)
    if T < WINDOW:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    H = savgol_hat_matrix()
    rows, bases = np.empty(T, dtype=np.int64), np.empty(T, dtype=np.int64)
    for q in range(T):
        rows[q], bases[q] = smooth_window(q, T)
    acc = H[rows, 0] * row[bases]
    for k in range(1, WINDOW):
        acc = acc + H[rows, k] * row[bases + k]
    return acc


def smooth_time_rows_host(times, lengths):
    """Every row of `times` (n, t_cap) smoothed over its first lengths[b] samples; what lies behind a row's length stays.  Returns a
    new array.  A row of length 0 (no row) stays; ValueError naming the row for 0 < length < 15."""
    times = np.array(times, dtype=np.float64)
    for b, T in enumerate(np.asarray(lengths).ravel()):
        T = int(T)
        if T <= 0:
            continue
        if T < WINDOW:
            raise ValueError("row %d: %d samples: If mode is 'interp', window_length must be less than or equal to the size of x." % (b, T))
        times[b, :T] = smooth_time_row_host(times[b, :T])
    return times


def require_smoothing_window(lengths, name):
    """ValueError, in scipy.signal.savgol_filter's words, for the first row of 0 < T < 15 samples; name: a format of the row's index
    (of its indices, for a table of lengths with more than one axis)."""
    lengths = np.asarray(lengths)
    short = np.argwhere((lengths > 0) & (lengths < WINDOW))
    if len(short):
        at = tuple(int(v) for v in short[0])
        raise ValueError((name % at) + ": %d samples: If mode is 'interp', window_length must be less than or equal to the size of x." % int(lengths[at]))
