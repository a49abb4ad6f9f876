// What every entry point that walks a joint list makes of (a skeleton, a list of joints, a primitive's D channels) before it launches
// anything, once, as plain host code (standard headers, the C ABI and mg_pack.h only, no HIP call: tests/native/joint_plan_check.cpp
// compiles this file alone and compares what it writes with values written out):
//
//   chains     the root-to-joint chain of every listed joint (mg_joint_chain), each formed once
//   records    per joint [header ..., m, m x {quaternion channel or -1, offset xyz}] (mg_chain_links), zero behind the links
//   channels   the channels the chains read -- root xyz, every quaternion along them -- as chan[] and slot[D]
//   aligning   the quaternion channels of the chain root .. node, the node's own included
//
// Nothing here sets an error text or picks a status code: a refusal comes back as an mg_plan_failure, and the entry point gives it its own
// code and words ("Joint plans", has the table).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mg_hip.h"
#include "mg_pack.h"

// offsets: mg_walk_frames reads no positions and passes false
inline bool mg_skeleton_complete(const mg_skeleton_desc *sk, bool offsets = true) {
    return sk->n_joints > 0 && sk->parents && (sk->offsets || !offsets) && sk->quat_channel && sk->parents[0] < 0;
}

// NO_JOINT and ORDER are mg_joint_chain's and take mg_chain_why(kind)
enum { MG_PLAN_OK = MG_CHAIN_OK, MG_PLAN_NO_JOINT = MG_CHAIN_NO_JOINT, MG_PLAN_ORDER = MG_CHAIN_ORDER, MG_PLAN_TOO_LONG, MG_PLAN_CHANNEL_OUTSIDE };
struct mg_plan_failure {
    int kind = MG_PLAN_OK;
    int joint = -1;     // NO_JOINT: the listed joint; ORDER: the joint whose parent does not precede it; TOO_LONG: the listed joint; CHANNEL_OUTSIDE: the chain's joint
    int channel = -1;   // CHANNEL_OUTSIDE: the first of the joint's four channels (an aligning chain's TOO_LONG: the quaternion that is one too many)
    int length = 0;     // TOO_LONG: the chain's links (an aligning chain's: its quaternions)
    explicit operator bool() const { return kind != MG_PLAN_OK; }
    bool of_skeleton() const { return kind == MG_PLAN_NO_JOINT || kind == MG_PLAN_ORDER; }   // the joint list against the skeleton, not the kernels' limits
};

struct mg_joint_plan {
    const mg_skeleton_desc *sk = nullptr;
    std::vector<std::vector<int>> chains;   // root first, the listed joint last
    int longest = 0;                        // links of the longest chain
    std::vector<char> need;                 // [D]: a channel the chains read

    // Phase 1, the joints: the chain of every listed joint in list order, up to the first that is NO_JOINT or ORDER (the chains before
    // it are kept).  sk is complete (mg_skeleton_complete), or n == 0.
    mg_plan_failure check(const mg_skeleton_desc *skeleton, const int32_t *joints, int n) {
        sk = skeleton;
        chains.clear();
        for (int j = 0; j < n; j++) {
            std::vector<int> ch;
            mg_plan_failure f;
            f.kind = mg_joint_chain(sk->parents, sk->n_joints, joints[j], ch, &f.joint);
            if (f) return f;
            chains.push_back(std::move(ch));
        }
        return {};
    }

    // Phase 2, the formed chains against the kernels' limits, chain by chain: its links (at most MG_MAX_CHAIN), then the quaternion
    // channels of its links root first (inside D); sets longest and need.  root_xyz: channels 0 .. 2 are read whatever the chains are.
    mg_plan_failure measure(int D, bool root_xyz) {
        need.assign((size_t)std::max(D, 0), 0);
        longest = 0;
        for (int d = 0; root_xyz && d < 3 && d < D; d++) need[(size_t)d] = 1;
        for (const std::vector<int> &ch : chains) {
            const int m = (int)ch.size() - 1;
            mg_plan_failure f;
            if (m > MG_MAX_CHAIN) { f.kind = MG_PLAN_TOO_LONG; f.joint = ch.back(); f.length = m; return f; }
            longest = std::max(longest, m);
            for (int k = 0; k < m; k++)
                if (!want(sk->quat_channel[ch[(size_t)k]])) { f.kind = MG_PLAN_CHANNEL_OUTSIDE; f.joint = ch[(size_t)k]; f.channel = sk->quat_channel[f.joint]; return f; }
        }
        return {};
    }

    // Both phases for an entry point that refuses joint by joint (each joint's chain, then its length, then its channels): the first
    // failure in list order.  One that keeps the argument errors of all joints ahead of the limits calls check and measure itself.
    mg_plan_failure build(const mg_skeleton_desc *skeleton, const int32_t *joints, int n, int D, bool root_xyz) {
        const mg_plan_failure listed = check(skeleton, joints, n), limit = measure(D, root_xyz);   // (limit: of the chains ahead of the failing joint)
        return limit ? limit : listed;
    }

    // the quaternion qc .. qc + 3 is read (-1: not animated, nothing is); false: outside D
    bool want(int qc) {
        if (qc < 0) return true;
        if ((size_t)qc + 4 > need.size()) return false;
        for (int e = 0; e < 4; e++) need[(size_t)qc + e] = 1;
        return true;
    }

    // out = [joint][stride] doubles, zero but for the chain's links m at [header - 1] and the m links behind it; stride 0: that of the
    // longest chain, header + 4 * longest.  Returns the stride.
    int records(int header, int stride, std::vector<double> &out) const {
        if (stride == 0) stride = header + 4 * longest;
        out.assign(chains.size() * (size_t)stride, 0.0);
        for (size_t j = 0; j < chains.size(); j++) {
            double *r = &out[j * (size_t)stride];
            r[header - 1] = (double)(chains[j].size() - 1);
            mg_chain_links(chains[j], sk->offsets, [&](int joint) { return sk->quat_channel[joint]; }, r + header);
        }
        return stride;
    }

    // the needed channels ascending, and where each of the D channels sits among them (-1: not needed)
    void compact(std::vector<int32_t> &chan, std::vector<int32_t> &slot) const {
        chan.clear();
        slot.assign(need.size(), -1);
        for (size_t d = 0; d < need.size(); d++)
            if (need[d]) { slot[d] = (int32_t)chan.size(); chan.push_back((int32_t)d); }
    }
};

// The aligning node's global orientation is the product of the quaternions along root .. node: their channels, root first, the node's
// own included, joints that are not animated skipped; at most MG_MAX_CHAIN of them, each inside D.  sk is complete but for its offsets.
inline mg_plan_failure mg_aligning_quaternions(const mg_skeleton_desc *sk, int node, int D, std::vector<int32_t> &quats) {
    quats.clear();
    std::vector<int> ch;
    mg_plan_failure f;
    f.kind = mg_joint_chain(sk->parents, sk->n_joints, node, ch, &f.joint);
    if (f) return f;
    for (int j : ch) {
        const int qc = sk->quat_channel[j];
        if (qc < 0) continue;
        f.joint = j; f.channel = qc;
        if (qc + 4 > D) { f.kind = MG_PLAN_CHANNEL_OUTSIDE; return f; }
        if ((int)quats.size() >= MG_MAX_CHAIN) { f.kind = MG_PLAN_TOO_LONG; f.length = MG_MAX_CHAIN + 1; return f; }
        quats.push_back(qc);
    }
    return {};
}
