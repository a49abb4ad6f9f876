// Which rows of E' the host-planned frames of a feature-point item touch (mg_feature_points.hip), as plain code: standard headers
// only and no HIP call, so that tests/native/items_check.cpp compiles this file beside mg_items_cut.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include <algorithm>
#include <vector>

struct mg_feature_range {
    int slot, d0, count;                 // the channels d0 .. d0 + count - 1 (all below D) of a frame slot's four tap control points
};

struct mg_feature_rows {
    int32_t NCP = 0, NRS = 0;            // listed control points (at most four per slot); listed rows
    std::vector<int32_t> tap;            // [slots]: where a slot's first tap sits among the listed control points
    std::vector<int32_t> map;            // [NCP * D]: the listed row of (listed control point, channel), -1 where no slot wants it
    std::vector<int32_t> src;            // [NRS]: the row of E' behind a listed row, control point * D + channel
};

// first[s]: the first of the four control points frame slot s taps.  A control point two slots share is listed once; the rows are
// numbered control points ascending, channels ascending within one.
inline mg_feature_rows mg_feature_rows_of(int D, const std::vector<int32_t> &first, const std::vector<mg_feature_range> &wanted) {
    mg_feature_rows r;
    std::vector<int32_t> cps;
    for (const int32_t f : first)
        for (int j = 0; j < 4; j++) cps.push_back(f + j);
    std::sort(cps.begin(), cps.end());
    cps.erase(std::unique(cps.begin(), cps.end()), cps.end());
    r.NCP = (int32_t)cps.size();
    for (const int32_t f : first) r.tap.push_back((int32_t)(std::lower_bound(cps.begin(), cps.end(), f) - cps.begin()));
    std::vector<char> need((size_t)r.NCP * D, 0);
    for (const mg_feature_range &w : wanted)
        for (int j = 0; j < 4; j++)
            for (int d = w.d0; d < w.d0 + w.count; d++) need[(size_t)(r.tap[(size_t)w.slot] + j) * D + d] = 1;
    r.map.assign((size_t)r.NCP * D, -1);
    for (int c = 0; c < r.NCP; c++)
        for (int d = 0; d < D; d++)
            if (need[(size_t)c * D + d]) {
                r.map[(size_t)c * D + d] = (int32_t)r.src.size();
                r.src.push_back(cps[(size_t)c] * D + d);
            }
    r.NRS = (int32_t)r.src.size();
    return r;
}
