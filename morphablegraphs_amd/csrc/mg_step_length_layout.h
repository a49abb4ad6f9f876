// The LDS layout of a step-length workgroup (mg_step_length.hip), stated once for the kernel, for the entry point's checks and launch
// sizes, and for tests/native/items_check.cpp: standard headers only and no HIP call, so that the test compiles this file without the
// library and prints the layout's bytes for the shape sweep (tests/step_length_cases.py) to compare its restatement with.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MG_SLEN_HD __host__ __device__
#else
#define MG_SLEN_HD
#endif

#define MG_SLEN_TILE 16                  // candidates per workgroup
#define MG_SLEN_LDS_MAX (150 * 1024)

// LDS of a workgroup, in doubles, and where its parts start (host and device agree through this)
struct mg_slen_layout {
    int E, mean, w, lat, cp, seg, ints, total_bytes;
    int NR, FS;
};
MG_SLEN_HD static inline mg_slen_layout mg_slen_layout_of(int L, int NB, int F) {
    mg_slen_layout y;
    y.NR = 3 * NB;
    y.FS = F | 1;                        // odd: the lanes of phase 3 (one per candidate) read different banks
    y.E = 0;
    y.mean = y.E + L * y.NR;
    y.w = y.mean + y.NR;
    y.lat = y.w + 4 * F;
    y.cp = y.lat + MG_SLEN_TILE * L;
    y.seg = y.cp + MG_SLEN_TILE * y.NR;
    y.ints = y.seg + MG_SLEN_TILE * y.FS;   // then int32: i0[F], bad[MG_SLEN_TILE]
    y.total_bytes = y.ints * 8 + (F + MG_SLEN_TILE) * 4;
    return y;
}
