// The two statements the model and constraint images are built from, once, as plain host code (standard headers only, no HIP call:
// tests/native/pack_check.cpp compiles this file alone and decodes what it writes).
//
// 1. The operand image of a 16x16x4 MFMA.  Both v_mfma_f32_16x16x4_f32 and v_mfma_f64_16x16x4_f64 take their A and their B operand
//    one value per lane, and in both lane l supplies X[i = l & 15][k = 4 * step + (l >> 4)]: i is the 16-wide index (A's row, B's
//    column), k the reduction index.  An image is [tile][k-step][lane]; every device-side loader reads it as such.
// 2. A joint's chain, root first, and its links: link k is the rotation of chain joint k and the offset of chain joint k + 1.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <vector>

// image[(tile * KK + kk) * 64 + lane] = at(16 * tile + (lane & 15), 4 * kk + (lane >> 4)); at(i, k) returns the element, or 0 outside
// the matrix, the band or the triangle
template <class T, class At>
inline void mg_pack_fragments(T *image, int tiles, int KK, At at) {
    for (int tile = 0; tile < tiles; tile++)
        for (int i = 0; i < 16; i++)        // (i outermost: what at() derives from i alone is derived once per row, and it reads along k)
            for (int kk = 0; kk < KK; kk++)
                for (int lane = i; lane < 64; lane += 16) image[((size_t)tile * KK + kk) * 64 + lane] = at(16 * tile + (lane & 15), 4 * kk + (lane >> 4));
}

// The same values with G k-steps side by side per lane, for 8- and 16-byte loads: G = 2 gives [tile][KK / 2][lane][2]; G = 4 gives
// [tile][q < KK / 4][lane][4], then the remaining pair [lane][2] where KK % 4 == 2.  KK is even; out does not overlap plain.
template <class T>
inline void mg_pack_regroup(const T *plain, T *out, int tiles, int KK, int G) {
    assert(KK % 2 == 0 && (G == 2 || G == 4));
    for (int tile = 0; tile < tiles; tile++) {
        const T *src = plain + (size_t)tile * KK * 64;
        T *dst = out + (size_t)tile * KK * 64;
        for (int kk = 0; kk < KK; kk += G) {
            const int g = std::min(G, KK - kk);   // G, or the remaining pair
            for (int h = 0; h < g; h++)
                for (int lane = 0; lane < 64; lane++) dst[lane * g + h] = src[(kk + h) * 64 + lane];
            dst += 64 * g;
        }
    }
}

// out = the joints from the root down to `joint`.  parents == NULL stands for a skeleton of the root alone.  Parents precede their
// children (parents[j] < j, negative at the root); *bad is the joint where that fails, or `joint` itself where it is out of range.
enum { MG_CHAIN_OK = 0, MG_CHAIN_NO_JOINT, MG_CHAIN_ORDER };
inline const char *mg_chain_why(int failed) { return failed == MG_CHAIN_NO_JOINT ? " out of range" : ": parents must precede their children"; }   // after "joint %d"
inline int mg_joint_chain(const int32_t *parents, int n_joints, int joint, std::vector<int> &out, int *bad = nullptr) {
    out.clear();
    if (bad) *bad = joint;
    if (joint < 0 || joint >= (parents ? n_joints : 1)) return MG_CHAIN_NO_JOINT;
    for (int j = joint; j >= 0; j = parents ? parents[j] : -1) {
        if (parents && parents[j] >= j) {
            if (bad) *bad = j;
            out.clear();
            return MG_CHAIN_ORDER;
        }
        out.push_back(j);
    }
    std::reverse(out.begin(), out.end());
    return MG_CHAIN_OK;
}

// The links of a chain, {quaternion channel or -1, offset xyz} each: rec[4 k] = channel(chain[k]), the channel the caller wants for that
// joint's rotation; rec[4 k + 1 .. 3] = offsets[chain[k + 1]]
template <class Channel>
inline void mg_chain_links(const std::vector<int> &chain, const double *offsets, Channel channel, double *rec) {
    for (size_t k = 0; k + 1 < chain.size(); k++) {
        rec[4 * k] = (double)channel(chain[k]);
        for (int e = 0; e < 3; e++) rec[4 * k + 1 + e] = offsets[(size_t)chain[k + 1] * 3 + e];
    }
}
