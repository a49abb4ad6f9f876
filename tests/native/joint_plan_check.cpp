// What csrc/mg_joint_plan.h makes of (a skeleton, a list of joints, D channels), compared value by value with what is written out
// here: the chains, the longest, the channels the chains read and their compaction, the records at the three (header, stride) pairs
// the entry points use, the aligning node's quaternions, every failure kind at its boundary and which of two failures comes first.
// The chains' own edge cases (mg_pack.h) are pack_check.cpp's, restated.  Plain host code with its own main (test infrastructure,
// never linked into the library); exit status 0 = every check held.
#include "../../morphablegraphs_amd/csrc/mg_joint_plan.h"
#include "../../morphablegraphs_amd/csrc/mg_pack.h"

#include <cstdio>
#include <string>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

typedef std::vector<int> ints;
typedef std::vector<int32_t> ints32;

static void check_chains() {
    std::vector<int> ch;
    int bad = -7;
    const int32_t root[] = {-1};
    CHECK(mg_joint_chain(root, 1, 0, ch, &bad) == MG_CHAIN_OK && ch == std::vector<int>({0}), "the root alone");
    CHECK(mg_joint_chain(nullptr, 0, 0, ch) == MG_CHAIN_OK && ch == std::vector<int>({0}), "no skeleton: the root alone");
    CHECK(mg_joint_chain(nullptr, 0, 1, ch, &bad) == MG_CHAIN_NO_JOINT && bad == 1 && ch.empty(), "no skeleton: joint 1");
    //                       0   1  2  3  4  5  6
    const int32_t tree[] = {-1, 0, 1, 1, 3, 0, 5};
    CHECK(mg_joint_chain(tree, 7, 4, ch) == MG_CHAIN_OK && ch == std::vector<int>({0, 1, 3, 4}), "leaf 4 of the branching skeleton");
    CHECK(mg_joint_chain(tree, 7, 6, ch) == MG_CHAIN_OK && ch == std::vector<int>({0, 5, 6}), "leaf 6 of the branching skeleton");
    CHECK(mg_joint_chain(tree, 7, 7, ch, &bad) == MG_CHAIN_NO_JOINT && bad == 7 && ch.empty(), "joint 7 of 7");
    CHECK(mg_joint_chain(tree, 7, -1, ch, &bad) == MG_CHAIN_NO_JOINT && bad == -1 && ch.empty(), "joint -1");
    const int32_t loop[] = {-1, 0, 3, 2};   // 2 and 3 name each other
    CHECK(mg_joint_chain(loop, 4, 3, ch, &bad) == MG_CHAIN_ORDER && bad == 2 && ch.empty(), "a parent behind its child: bad = %d", bad);
    CHECK(std::string("joint 7") + mg_chain_why(MG_CHAIN_NO_JOINT) == "joint 7 out of range" &&
          std::string("joint 2") + mg_chain_why(MG_CHAIN_ORDER) == "joint 2: parents must precede their children", "the words of a failed chain");
    const int32_t self[] = {-1, 1};
    CHECK(mg_joint_chain(self, 2, 1, ch, &bad) == MG_CHAIN_ORDER && bad == 1 && ch.empty(), "a joint that is its own parent: bad = %d", bad);
    CHECK(mg_joint_chain(loop, 4, 1, ch) == MG_CHAIN_OK && ch == std::vector<int>({0, 1}), "the sound part of that skeleton");

    // links of root .. 4: {channel of 0, offset of 1}, {channel of 1, offset of 3}, {channel of 3, offset of 4}
    double offsets[7 * 3], rec[2 + 4 * 3];
    for (int q = 0; q < 7 * 3; q++) offsets[q] = 100.0 + q;
    for (double &v : rec) v = -9.0;
    const int channel[] = {3, -1, 7, 11, 15, 19, 23};
    mg_joint_chain(tree, 7, 4, ch);
    mg_chain_links(ch, offsets, [&](int j) { return channel[j]; }, rec + 1);
    const double want[] = {-9.0, 3.0, 103.0, 104.0, 105.0, -1.0, 109.0, 110.0, 111.0, 11.0, 112.0, 113.0, 114.0, -9.0};
    for (int q = 0; q < 14; q++) CHECK(rec[q] == want[q], "link record[%d] = %g, expected %g", q, rec[q], want[q]);
}

static bool is(const mg_plan_failure &f, int kind, int joint, int channel, int length) {
    return f.kind == kind && f.joint == joint && f.channel == channel && f.length == length && (bool)f == (kind != MG_PLAN_OK) &&
           f.of_skeleton() == (kind == MG_PLAN_NO_JOINT || kind == MG_PLAN_ORDER);
}
#define CHECK_IS(failure, k_, j_, c_, l_, what) \
    do { const mg_plan_failure f_ = (failure); CHECK(is(f_, k_, j_, c_, l_), "%s: kind %d, joint %d, channel %d, length %d", what, f_.kind, f_.joint, f_.channel, f_.length); } while (0)

// a skeleton whose arrays live as long as it does
struct skeleton {
    ints32 parents, channel;
    std::vector<double> offsets;
    mg_skeleton_desc desc;
    skeleton(const ints32 &p, const ints32 &c) : parents(p), channel(c), offsets(p.size() * 3) {
        for (size_t q = 0; q < offsets.size(); q++) offsets[q] = 100.0 + (double)q;
        desc.n_joints = (int32_t)parents.size(); desc.reserved = 0;
        desc.parents = parents.data(); desc.offsets = offsets.data(); desc.quat_channel = channel.data();
    }
};
// joint j hangs below joint j - 1
static ints32 straight(int n) {
    ints32 p((size_t)n);
    for (int j = 0; j < n; j++) p[(size_t)j] = j - 1;
    return p;
}

// the records of `plan` at (header, stride or 0): the stride, and per joint zeros ahead of the length, the length, the links written
// out in `links`, zeros behind them
static void check_records(const char *what, const mg_joint_plan &plan, int header, int stride_or_0, int stride, const std::vector<std::vector<double>> &links) {
    std::vector<double> rec(7, -9.0);
    const int got = plan.records(header, stride_or_0, rec);
    CHECK(got == stride && rec.size() == links.size() * (size_t)stride, "%s, header %d: stride %d, %zu values", what, header, got, rec.size());
    if (got != stride || rec.size() != links.size() * (size_t)stride) return;
    for (size_t j = 0; j < links.size(); j++)
        for (int e = 0; e < stride; e++) {
            const int l = e - header;
            const double want = e == header - 1 ? (double)(links[j].size() / 4) : l >= 0 && l < (int)links[j].size() ? links[j][(size_t)l] : 0.0;
            CHECK(rec[j * (size_t)stride + e] == want, "%s, header %d, stride %d: record %zu[%d] = %g, expected %g", what, header, stride, j, e, rec[j * (size_t)stride + e], want);
        }
}

static void check_compaction(const char *what, const mg_joint_plan &plan, const ints &need, const ints32 &chan, const ints32 &slot) {
    CHECK(ints(plan.need.begin(), plan.need.end()) == need, "%s: the channels the chains read", what);
    ints32 c(3, -5), s(1, -5);
    plan.compact(c, s);
    CHECK(c == chan && s == slot, "%s: chan (%zu) and slot (%zu)", what, c.size(), s.size());
}

static void check_branching() {
    const int D = 27, FIXED = 1 + 4 * MG_MAX_CHAIN;
    //                  0   1  2  3   4   5   6
    const skeleton sk({-1, 0, 1, 1, 3, 0, 5}, {3, -1, 7, 11, 15, 19, 23});
    CHECK(mg_skeleton_complete(&sk.desc) && mg_skeleton_complete(&sk.desc, false), "the branching skeleton is complete");
    // {channel of the chain's joint k, offset of its joint k + 1}: joint 1 is not animated, the end joint's own channel is not read
    const std::vector<double> L4 = {3, 103, 104, 105, -1, 109, 110, 111, 11, 112, 113, 114}, L6 = {3, 115, 116, 117, 19, 118, 119, 120}, L0 = {};
    mg_joint_plan plan;
    {
        const int32_t list[] = {4};
        CHECK_IS(plan.build(&sk.desc, list, 1, D, true), MG_PLAN_OK, -1, -1, 0, "{4}");
        CHECK(plan.chains == std::vector<ints>({{0, 1, 3, 4}}) && plan.longest == 3, "{4}: chains, longest %d", plan.longest);
        check_compaction("{4}", plan, {1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14},
                         {0, 1, 2, 3, 4, 5, 6, -1, -1, -1, -1, 7, 8, 9, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1});
        check_records("{4}", plan, 1, FIXED, FIXED, {L4});
        check_records("{4}", plan, 1, 0, 13, {L4});
        check_records("{4}", plan, 5, 0, 17, {L4});
        // without the root position: what the chains alone read
        CHECK_IS(plan.build(&sk.desc, list, 1, D, false), MG_PLAN_OK, -1, -1, 0, "{4}, chains only");
        check_compaction("{4}, chains only", plan, {0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {3, 4, 5, 6, 11, 12, 13, 14},
                         {-1, -1, -1, 0, 1, 2, 3, -1, -1, -1, -1, 4, 5, 6, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1});
    }
    {
        const int32_t list[] = {4, 6};
        CHECK_IS(plan.build(&sk.desc, list, 2, D, true), MG_PLAN_OK, -1, -1, 0, "{4, 6}");
        CHECK(plan.chains == std::vector<ints>({{0, 1, 3, 4}, {0, 5, 6}}) && plan.longest == 3, "{4, 6}: chains, longest %d", plan.longest);
        check_compaction("{4, 6}", plan, {1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0},
                         {0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 19, 20, 21, 22},
                         {0, 1, 2, 3, 4, 5, 6, -1, -1, -1, -1, 7, 8, 9, 10, -1, -1, -1, -1, 11, 12, 13, 14, -1, -1, -1, -1});
        check_records("{4, 6}", plan, 1, FIXED, FIXED, {L4, L6});
        check_records("{4, 6}", plan, 1, 0, 13, {L4, L6});
        check_records("{4, 6}", plan, 5, 0, 17, {L4, L6});
    }
    {
        const int32_t list[] = {0};
        CHECK_IS(plan.build(&sk.desc, list, 1, D, true), MG_PLAN_OK, -1, -1, 0, "{0}");
        CHECK(plan.chains == std::vector<ints>({{0}}) && plan.longest == 0, "{0}: chains, longest %d", plan.longest);
        check_compaction("{0}", plan, {1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2},
                         {0, 1, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1});
        check_records("{0}", plan, 1, FIXED, FIXED, {L0});
        check_records("{0}", plan, 1, 0, 1, {L0});
        check_records("{0}", plan, 5, 0, 5, {L0});
    }
    {
        const int32_t list[] = {6, 6};
        CHECK_IS(plan.build(&sk.desc, list, 2, D, true), MG_PLAN_OK, -1, -1, 0, "{6, 6}");
        CHECK(plan.chains == std::vector<ints>({{0, 5, 6}, {0, 5, 6}}) && plan.longest == 2, "{6, 6}: chains, longest %d", plan.longest);
        check_compaction("{6, 6}", plan, {1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 19, 20, 21, 22},
                         {0, 1, 2, 3, 4, 5, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 7, 8, 9, 10, -1, -1, -1, -1});
        check_records("{6, 6}", plan, 1, FIXED, FIXED, {L6, L6});
        check_records("{6, 6}", plan, 1, 0, 9, {L6, L6});
        check_records("{6, 6}", plan, 5, 0, 13, {L6, L6});
    }
    {
        // no joints at all (a feature-point item without a points output): no skeleton is read
        CHECK_IS(plan.check(nullptr, nullptr, 0), MG_PLAN_OK, -1, -1, 0, "{}");
        CHECK_IS(plan.measure(D, false), MG_PLAN_OK, -1, -1, 0, "{}");
        CHECK(plan.chains.empty() && plan.longest == 0, "{}: chains, longest %d", plan.longest);
        check_compaction("{}", plan, ints(27, 0), {}, ints32(27, -1));
        check_records("{}", plan, 5, 0, 5, {});
    }
    // what makes a skeleton incomplete, and that mg_walk_frames' reading does without the offsets
    mg_skeleton_desc d = sk.desc;
    d.offsets = nullptr;
    CHECK(!mg_skeleton_complete(&d) && mg_skeleton_complete(&d, false), "a skeleton without offsets");
    d = sk.desc; d.n_joints = 0;
    CHECK(!mg_skeleton_complete(&d) && !mg_skeleton_complete(&d, false), "a skeleton without joints");
    d = sk.desc; d.parents = nullptr;
    CHECK(!mg_skeleton_complete(&d) && !mg_skeleton_complete(&d, false), "a skeleton without parents");
    d = sk.desc; d.quat_channel = nullptr;
    CHECK(!mg_skeleton_complete(&d) && !mg_skeleton_complete(&d, false), "a skeleton without channels");
    const skeleton rooted({0, 0}, {3, 7});
    CHECK(!mg_skeleton_complete(&rooted.desc) && !mg_skeleton_complete(&rooted.desc, false), "a root with a parent");
}

static void check_boundaries() {
    mg_joint_plan plan;
    // the channels against D: joint 2's chain reads the quaternions of joints 0 and 1, not its own
    const skeleton sk(straight(3), {3, 7, 11});
    const int32_t two[] = {2}, zero[] = {0};
    CHECK_IS(plan.build(&sk.desc, two, 1, 11, true), MG_PLAN_OK, -1, -1, 0, "qc + 4 == D");
    CHECK(plan.need == std::vector<char>({1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}), "qc + 4 == D: every channel is read");
    CHECK_IS(plan.build(&sk.desc, two, 1, 10, true), MG_PLAN_CHANNEL_OUTSIDE, 1, 7, 0, "qc + 4 == D + 1");
    CHECK_IS(plan.build(&sk.desc, two, 1, 6, true), MG_PLAN_CHANNEL_OUTSIDE, 0, 3, 0, "the root's quaternion outside D comes first");
    CHECK_IS(plan.build(&sk.desc, zero, 1, 3, true), MG_PLAN_OK, -1, -1, 0, "the root alone reads no quaternion");
    const skeleton still(straight(3), {-1, -1, -1});
    CHECK_IS(plan.build(&still.desc, zero, 1, 3, true), MG_PLAN_OK, -1, -1, 0, "D = 3, the root, nothing animated");
    CHECK(plan.need == std::vector<char>({1, 1, 1}) && plan.longest == 0, "D = 3: the root position");
    CHECK_IS(plan.build(&still.desc, two, 1, 3, true), MG_PLAN_OK, -1, -1, 0, "D = 3, joint 2, nothing animated");
    check_records("nothing animated", plan, 1, 0, 9, {{-1, 103, 104, 105, -1, 106, 107, 108}});

    // the chain's length: MG_MAX_CHAIN links fill a fixed-stride record to its last value
    const int M = MG_MAX_CHAIN;
    const skeleton full(straight(M + 1), ints32((size_t)M + 1, -1)), over(straight(M + 2), ints32((size_t)M + 2, -1));
    const int32_t last[] = {M}, beyond[] = {M + 1};
    CHECK_IS(plan.build(&full.desc, last, 1, 3, true), MG_PLAN_OK, -1, -1, 0, "a chain of MG_MAX_CHAIN links");
    CHECK(plan.chains.size() == 1 && (int)plan.chains[0].size() == M + 1 && plan.longest == M, "MG_MAX_CHAIN links: longest %d", plan.longest);
    std::vector<double> links;
    for (int k = 0; k < M; k++)
        for (double v : {-1.0, 100.0 + 3 * (k + 1), 101.0 + 3 * (k + 1), 102.0 + 3 * (k + 1)}) links.push_back(v);
    check_records("MG_MAX_CHAIN links", plan, 1, 1 + 4 * M, 1 + 4 * M, {links});
    check_records("MG_MAX_CHAIN links", plan, 5, 0, 5 + 4 * M, {links});
    CHECK_IS(plan.build(&over.desc, beyond, 1, 3, true), MG_PLAN_TOO_LONG, M + 1, -1, M + 1, "a chain of MG_MAX_CHAIN + 1 links");
    CHECK_IS(plan.build(&over.desc, last, 1, 3, true), MG_PLAN_OK, -1, -1, 0, "its parent in the same skeleton");

    // the joints against the skeleton
    const int32_t seven[] = {2, 3}, minus[] = {-1};
    CHECK_IS(plan.build(&sk.desc, seven, 2, 11, true), MG_PLAN_NO_JOINT, 3, -1, 0, "joint 3 of 3");
    CHECK_IS(plan.build(&sk.desc, minus, 1, 11, true), MG_PLAN_NO_JOINT, -1, -1, 0, "joint -1");
    const skeleton loop({-1, 0, 3, 2}, {3, 7, 11, 15});
    const int32_t three[] = {1, 3};
    CHECK_IS(plan.build(&loop.desc, three, 2, 19, true), MG_PLAN_ORDER, 2, -1, 0, "a parent behind its child");
}

static void check_aligning() {
    ints32 quats(2, -5);
    //                  0   1  2  3   4   5   6
    const skeleton sk({-1, 0, 1, 1, 3, 0, 5}, {3, -1, 7, 11, 15, 19, 23});
    // joint 1 is not animated; node 4's own quaternion counts
    CHECK_IS(mg_aligning_quaternions(&sk.desc, 4, 19, quats), MG_PLAN_OK, -1, -1, 0, "aligning through 4, D = 19");
    CHECK(quats == ints32({3, 11, 15}), "aligning through 4: %zu quaternions", quats.size());
    CHECK_IS(mg_aligning_quaternions(&sk.desc, 4, 18, quats), MG_PLAN_CHANNEL_OUTSIDE, 4, 15, 0, "aligning through 4, D = 18");
    CHECK_IS(mg_aligning_quaternions(&sk.desc, 0, 7, quats), MG_PLAN_OK, -1, -1, 0, "aligning through the root");
    CHECK(quats == ints32({3}), "aligning through the root: %zu quaternions", quats.size());
    CHECK_IS(mg_aligning_quaternions(&sk.desc, 1, 7, quats), MG_PLAN_OK, -1, -1, 0, "aligning through a node that is not animated");
    CHECK(quats == ints32({3}), "aligning through 1: %zu quaternions", quats.size());
    CHECK_IS(mg_aligning_quaternions(&sk.desc, 7, 27, quats), MG_PLAN_NO_JOINT, 7, -1, 0, "aligning through joint 7 of 7");
    CHECK(quats.empty(), "a failed aligning chain leaves no quaternions");
    const skeleton loop({-1, 0, 3, 2}, {3, 7, 11, 15});
    CHECK_IS(mg_aligning_quaternions(&loop.desc, 3, 19, quats), MG_PLAN_ORDER, 2, -1, 0, "aligning through a loop");
    // the offsets are not read
    mg_skeleton_desc bare = sk.desc;
    bare.offsets = nullptr;
    CHECK_IS(mg_aligning_quaternions(&bare, 6, 27, quats), MG_PLAN_OK, -1, -1, 0, "aligning without offsets");
    CHECK(quats == ints32({3, 19, 23}), "aligning through 6: %zu quaternions", quats.size());

    // the limit is on quaternions, not joints: every second joint of a straight chain animated
    const int M = MG_MAX_CHAIN;
    ints32 channel((size_t)2 * M + 1), all;
    for (int j = 0; j <= 2 * M; j++) channel[(size_t)j] = j % 2 == 0 ? 3 + 4 * (j / 2) : -1;
    for (int q = 0; q < M; q++) all.push_back(3 + 4 * q);
    const skeleton longer(straight(2 * M + 1), channel);
    CHECK_IS(mg_aligning_quaternions(&longer.desc, 2 * M - 1, 3 + 4 * M, quats), MG_PLAN_OK, -1, -1, 0, "MG_MAX_CHAIN quaternions along 2 MG_MAX_CHAIN joints");
    CHECK(quats == all, "MG_MAX_CHAIN quaternions: %zu", quats.size());
    CHECK_IS(mg_aligning_quaternions(&longer.desc, 2 * M, 7 + 4 * M, quats), MG_PLAN_TOO_LONG, 2 * M, 3 + 4 * M, M + 1, "one more animated joint");
    // (both at once: the entry points have one text for the two, "... does not fit")
    CHECK_IS(mg_aligning_quaternions(&longer.desc, 2 * M, 3 + 4 * M, quats), MG_PLAN_CHANNEL_OUTSIDE, 2 * M, 3 + 4 * M, 0, "one more animated joint, outside D as well");
}

// Which of two failures is reported.  mg_joint_positions and mg_track_plan_create refuse joint by joint -- a joint's chain, its length,
// its channels, then the next joint -- which is build(); mg_feature_points, mg_feature_points_warped and mg_point_cloud_features hold
// every joint against the skeleton first (their argument errors) and the chains against the limits afterwards: check(), then measure().
static void check_precedence() {
    const int M = MG_MAX_CHAIN;
    ints32 channel((size_t)M + 2, -1);
    channel[1] = 40;
    const skeleton sk(straight(M + 2), channel);
    mg_joint_plan plan;
    const int32_t long_then_none[] = {M + 1, M + 2}, none_then_long[] = {M + 2, M + 1}, outside_then_none[] = {2, -1}, short_long_none[] = {1, M + 1, M + 2};
    CHECK_IS(plan.build(&sk.desc, long_then_none, 2, 44, true), MG_PLAN_TOO_LONG, M + 1, -1, M + 1, "joint by joint: too long, then out of range");
    CHECK_IS(plan.build(&sk.desc, none_then_long, 2, 44, true), MG_PLAN_NO_JOINT, M + 2, -1, 0, "joint by joint: out of range, then too long");
    CHECK_IS(plan.build(&sk.desc, outside_then_none, 2, 43, true), MG_PLAN_CHANNEL_OUTSIDE, 1, 40, 0, "joint by joint: a channel outside, then out of range");
    CHECK_IS(plan.build(&sk.desc, outside_then_none, 2, 44, true), MG_PLAN_NO_JOINT, -1, -1, 0, "joint by joint: out of range behind a sound joint");
    CHECK_IS(plan.build(&sk.desc, long_then_none, 1, 43, true), MG_PLAN_TOO_LONG, M + 1, -1, M + 1, "one joint: its length before its channels");

    CHECK_IS(plan.check(&sk.desc, short_long_none, 3), MG_PLAN_NO_JOINT, M + 2, -1, 0, "the joints first: out of range behind a chain that is too long");
    CHECK(plan.chains.size() == 2 && plan.chains[0] == ints({0, 1}) && (int)plan.chains[1].size() == M + 2, "the chains ahead of the failing joint are kept");
    CHECK_IS(plan.check(&sk.desc, short_long_none, 2), MG_PLAN_OK, -1, -1, 0, "the joints first: the list without that joint");
    CHECK_IS(plan.measure(44, true), MG_PLAN_TOO_LONG, M + 1, -1, M + 1, "the limits afterwards: too long");
    CHECK_IS(plan.measure(43, true), MG_PLAN_TOO_LONG, M + 1, -1, M + 1, "the limits afterwards: chain by chain, joint 1's chain reads channel 3 only");
    const int32_t outside_then_long[] = {2, M + 1};
    CHECK_IS(plan.check(&sk.desc, outside_then_long, 2), MG_PLAN_OK, -1, -1, 0, "the joints first: two joints of the skeleton");
    CHECK_IS(plan.measure(43, true), MG_PLAN_CHANNEL_OUTSIDE, 1, 40, 0, "the limits afterwards: the first chain's channel before the second's length");
}

int main() {
    check_chains();
    check_branching();
    check_boundaries();
    check_aligning();
    check_precedence();
    if (failures) std::printf("joint_plan_check: %d checks failed\n", failures);
    return failures ? 1 : 0;
}
