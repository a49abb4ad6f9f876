// The host decisions of the item-table entry points (mg_items.h) -- the cut into launches, the bisection, which items travel and
// where an array lands behind them, the shared latents -- as plain code: standard headers only and no HIP call, so that
// tests/native/items_check.cpp compiles this file without the library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define MG_ITEMS_HD __host__ __device__
#else
#define MG_ITEMS_HD
#endif

struct mg_item_launch {
    size_t first;        // its first item among the call's non-empty ones
    int32_t n_items;
    int64_t grid;        // workgroups
    int lds;             // bytes
};

// The cut of a call's items into launches.  A workgroup serves up to `tile` candidates of ONE item; empty items take no part.  A launch
// holds at most max_items items and at most 2^31 - 1 workgroups; wg0[i] is the first workgroup that serves item i, counted from 0 in
// every launch (-1 for an empty item); the launch's dynamic LDS is the largest of its items'.  samples_of(i), lds_of(i): item i's sample
// count and LDS bytes (lds_of is asked of non-empty items only).
template <class SamplesOf, class LdsOf>
inline std::vector<mg_item_launch> mg_cut_items(int n_items, SamplesOf samples_of, LdsOf lds_of, int tile, int max_items, std::vector<int32_t> &wg0) {
    std::vector<mg_item_launch> launches;
    size_t taken = 0;
    wg0.assign((size_t)n_items, -1);
    for (int i = 0; i < n_items; i++) {
        const int64_t n = samples_of(i);
        if (n == 0) continue;
        const int64_t wgs = (n + tile - 1) / tile;
        if (launches.empty() || launches.back().n_items == max_items || launches.back().grid + wgs > 0x7fffffff) launches.push_back({taken, 0, 0, 0});
        mg_item_launch &l = launches.back();
        wg0[(size_t)i] = (int32_t)l.grid;
        l.n_items++;
        l.grid += wgs;
        l.lds = std::max(l.lds, (int)lds_of(i));
        taken++;
    }
    return launches;
}

// the caller's index of every non-empty item, in order: the items of the device table
template <class SamplesOf>
inline std::vector<int> mg_nonempty_items(int n_items, SamplesOf samples_of) {
    std::vector<int> of;
    for (int i = 0; i < n_items; i++)
        if (samples_of(i) != 0) of.push_back(i);
    return of;
}

// `bytes` of data behind a device table, at the next multiple of 8 (the gap zeroed); returns where, in bytes from the table's base
inline size_t mg_table_append(std::vector<unsigned char> &table, const void *data, size_t bytes) {
    const size_t at = (table.size() + 7) & ~(size_t)7;
    table.resize(at + bytes, 0);
    if (bytes) std::memcpy(table.data() + at, data, bytes);
    return at;
}

// the item of workgroup wg in a launch's slice of the table: the last one whose wg0 is not past it (the kernels' bisection)
template <class Item>
MG_ITEMS_HD inline int mg_item_at(const Item *items, int n_items, int wg) {
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].wg0 <= wg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// lat_of[i]: the first earlier item that names the same latent matrix as item i (same pointer, rows and ld: the steps of a walk, the
// nodes of a graph over one matrix), whose copy item i reads in a _host twin; -1 where item i brings its own, and for an empty item.
template <class Item>
inline std::vector<int> mg_shared_latents(const Item *items, int n_items) {
    std::vector<int> lat_of((size_t)n_items, -1);
    for (int i = 0; i < n_items; i++)
        for (int j = 0; j < i && lat_of[(size_t)i] < 0 && items[i].n_samples != 0; j++)
            if (items[j].n_samples == items[i].n_samples && items[j].latents_dev == items[i].latents_dev && items[j].ld == items[i].ld) lat_of[(size_t)i] = j;
    return lat_of;
}
