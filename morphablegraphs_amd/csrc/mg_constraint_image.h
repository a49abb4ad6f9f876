// The device image of a constraint set, built as plain host code (standard headers, the C ABI and mg_pack.h only, no HIP call:
// tests/native/constraint_image_check.cpp compiles this file alone and decodes what it writes).  The layout is the one
// mg_constraint_set (mg_internal.h) documents and mg_score_device.h reads; mg_host.hip uploads the vectors as they stand.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "mg_hostdefs.h"
#include "mg_pack.h"

struct mg_constraint_image {
    std::vector<double> W, bias, par, choff, pose_tab, align, wpack, bpad;   // empty: the set has no such table
    std::vector<int32_t> woff, chain_len;
    int32_t nch = 0, rows = 0, RT = 0, align_joint = -1;
    bool has_pose = false;
};

// What a constraint type asks of the skeleton and which rows it owns.  With m = the chain's links and q = max(m, 1):
//   rows = [root xyz] + 4 q quaternion rows [+ 4 q2 of the second chain];   chain_len = m | m2 << 16
// A chain root .. joint of `len` joints has len - 1 links (the end joint's own rotation does not move it); own_quat adds the joint's
// own quaternion as one more, and so does a relative point (a non-zero ref_dir: it hangs below the joint like one more joint, its
// offset the point itself).  The chain's offsets (choff) go with the root rows: only positions need them.
enum { MG_RULE_ROOT,        // no joint: the first nch pose channels
       MG_RULE_JOINT,       // joint 0, or a skeleton that has the joint
       MG_RULE_SKELETON,    // a skeleton, and the joint(s) in it
       MG_RULE_POSE };      // a skeleton and a pose record: one block of root xyz + every animated joint's quaternion per frame
enum { MG_VEC_NONE, MG_VEC_REF, MG_VEC_REF_FINITE_TARGET, MG_VEC_TARGET_REF };   // the vectors that must be non-zero and finite
struct mg_constraint_rule { int kind, min_D; bool own_quat, relative, second, root_rows; int vectors; };
inline const mg_constraint_rule &mg_constraint_rule_of(int type) {
    static const mg_constraint_rule rules[MG_CONSTRAINT_VALUE_HEADING + 1] = {
        //                     kind              D  own    rel.   second root   vectors
        /* POSITION          */ {MG_RULE_ROOT,     3, false, false, false, false, MG_VEC_NONE},
        /* DIRECTION_2D      */ {MG_RULE_ROOT,     7, false, false, false, false, MG_VEC_NONE},
        /* JOINT_POSITION    */ {MG_RULE_SKELETON, 7, false, true,  false, true,  MG_VEC_NONE},
        /* JOINT_MIDPOINT    */ {MG_RULE_SKELETON, 7, false, false, true,  true,  MG_VEC_NONE},
        /* JOINT_ORIENTATION */ {MG_RULE_JOINT,    7, true,  false, false, false, MG_VEC_TARGET_REF},
        /* LOOK_AT           */ {MG_RULE_JOINT,    7, true,  false, false, true,  MG_VEC_REF_FINITE_TARGET},
        /* POSE              */ {MG_RULE_POSE,     7, false, false, false, false, MG_VEC_NONE},
        /* VALUE_POSITION    */ {MG_RULE_ROOT,     7, false, false, false, false, MG_VEC_NONE},
        /* VALUE_HEADING     */ {MG_RULE_JOINT,    7, true,  false, false, false, MG_VEC_REF},
    };
    return rules[type];
}

inline double mg_norm3(const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
inline bool mg_nonzero3(const double *v) { const double n = mg_norm3(v); return std::isfinite(n) && n > 0.0; }

// A constraint's row of the scorers' parameter table: {type, weight, target[3], ref_dir[3]}.  For the direction constraint the row
// carries what its residual derives from the target alone -- the unit target (tx, tz) and sqrt(tx^2 + tz^2) -- computed here once per
// set instead of by every lane for every candidate: the residual's own statements (mg_score_device.h), correctly rounded IEEE
// square roots and divisions on both sides, no contraction: the same bits.
inline void mg_constraint_par_row(const mg_keyframe_constraint &c, double *q) {
    q[0] = (double)c.type; q[1] = c.weight_factor;
    for (int i = 0; i < 3; i++) { q[2 + i] = c.target[i]; q[5 + i] = c.ref_dir[i]; }
    if (c.type == MG_CONSTRAINT_DIRECTION_2D) {
        const double tn = std::sqrt(c.target[0] * c.target[0] + c.target[1] * c.target[1]);
        const double tx = c.target[0] / tn, tz = c.target[1] / tn;
        q[2] = tx; q[3] = tz; q[4] = std::sqrt(tx * tx + tz * tz);
    }
}

// The alignment record [8]: chain length, unit previous heading (x, z), previous root (x, z), ref_dir; in start-pose mode the height
// in place of ref_dir (heights += position[1]).  Create uploads all eight; an update rewrites entries 1 to 7, the chain is structure.
inline int mg_alignment_record(const char *who, const mg_alignment_desc *al, int chain, double *rec) {
    const double hn = std::sqrt(al->heading[0] * al->heading[0] + al->heading[1] * al->heading[1]);
    MG_REQUIRE(std::isfinite(hn) && hn > 0.0 && std::isfinite(al->position[0]) && std::isfinite(al->position[2]),
               "%s: previous heading / position not finite or zero", who);
    rec[0] = (double)chain; rec[1] = al->heading[0] / hn; rec[2] = al->heading[1] / hn; rec[3] = al->position[0]; rec[4] = al->position[2];
    for (int e = 0; e < 3; e++) rec[5 + e] = al->ref_dir[e];
    if (al->joint == MG_ALIGN_START_POSE) { rec[5] = al->position[1]; rec[6] = rec[7] = 0.0; }
    return MG_OK;
}

// The image of (sk, cons[n], poses[n_poses], al) on a primitive of L components and D pose channels with the knot vector `knots`,
// mean' `means` (R) and E' `Es` (R, L); KK > 0: the MFMA operand image of W as well.  MG_OK, or the refusal with its text set.
inline int mg_constraint_image_build(int L, int D, int KK, const std::vector<double> &knots, const std::vector<double> &means, const std::vector<double> &Es,
                                     const mg_skeleton_desc *sk, const mg_keyframe_constraint *cons, int32_t n, const mg_pose_constraint *poses,
                                     int32_t n_poses, const mg_alignment_desc *al, mg_constraint_image &im) {
    im = mg_constraint_image();
    im.nch = std::min(7, D);
    im.align_joint = al ? al->joint : -1;
    // animated joints of the skeleton in skeleton order: a pose block is root xyz + one quaternion per slot
    std::vector<int> slot;
    int n_slots = 0;
    if (sk) {
        MG_REQUIRE(sk->n_joints > 0 && sk->parents && sk->offsets && sk->quat_channel, "mg_constraint_set_create_fk: incomplete skeleton");
        MG_REQUIRE(sk->parents[0] < 0, "mg_constraint_set_create_fk: joint 0 must be the root");
        for (int j = 0; j < sk->n_joints; j++) {
            MG_REQUIRE(sk->parents[j] < j, "mg_constraint_set_create_fk: joint %d: parents must precede their children", j);
            MG_REQUIRE(sk->quat_channel[j] < 0 || sk->quat_channel[j] + 4 <= D,
                       "mg_constraint_set_create_fk: joint %d: quaternion channel %d outside n_dim = %d", j, sk->quat_channel[j], D);
            slot.push_back(sk->quat_channel[j] >= 0 ? n_slots++ : -1);
        }
    }
    // (every joint is range-checked before its chain is asked for, and the skeleton's order was checked above: this cannot fail)
    auto chain_of = [&](int joint, std::vector<int> &ch) { (void)mg_joint_chain(sk ? sk->parents : nullptr, sk ? sk->n_joints : 1, joint, ch); };
    auto has_joint = [&](int joint) { return sk && joint >= 0 && joint < sk->n_joints; };
    std::vector<int> chain, chain2, al_chain;   // al_chain: root .. aligning node, every one of their quaternions turns the heading
    if (al) {
        MG_REQUIRE(D >= 7, "mg_constraint_set_create_aligned: alignment needs the root quaternion, n_dim = %d", D);
        MG_REQUIRE(al->joint == MG_ALIGN_START_POSE || al->joint == 0 || has_joint(al->joint),
                   "mg_constraint_set_create_aligned: aligning joint %d needs a skeleton that has it", al->joint);
        if (al->joint != MG_ALIGN_START_POSE) chain_of(al->joint, al_chain);   // (the start pose's rotation is given, not derived from a heading)
        im.align.resize(8);
        const int rc = mg_alignment_record("mg_constraint_set_create_aligned", al, (int)al_chain.size(), im.align.data());
        if (rc != MG_OK) return rc;
        MG_REQUIRE((int)al_chain.size() <= MG_MAX_CHAIN, "mg_constraint_set_create_aligned: chain of %d joints exceeds %d", (int)al_chain.size(), MG_MAX_CHAIN);
    }
    im.woff.assign((size_t)n + 2, 0);
    im.chain_len.assign((size_t)std::max(n, 1), 0);
    im.par.assign((size_t)std::max(n, 1) * 8, 0.0);
    im.choff.assign((size_t)std::max(n, 1) * 2 * MG_MAX_CHAIN * 3, 0.0);
    auto add_rows = [&](int c, int rows) {   // constraint c (n: the alignment) owns `rows` rows from woff[c] on; zero until they are filled
        im.woff[(size_t)c + 1] = im.woff[(size_t)c] + rows;
        im.W.resize((size_t)im.woff[(size_t)c + 1] * L, 0.0);
        im.bias.resize((size_t)im.woff[(size_t)c + 1], 0.0);
        return (size_t)im.woff[(size_t)c];
    };
    int32_t i0 = 0;
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    auto spline_row = [&](size_t row, int d) {   // pose channel d at the keyframe whose basis row is (i0, w), as a (1 x L) matrix + bias
        double b = 0.0;
        for (int j = 0; j < 4; j++) b = b + w[j] * means[(size_t)(i0 + j) * D + d];
        im.bias[row] = b;
        for (int k = 0; k < L; k++) {
            double acc = 0.0;
            for (int j = 0; j < 4; j++) acc = acc + w[j] * Es[((size_t)(i0 + j) * D + d) * L + k];
            im.W[row * L + k] = acc;
        }
    };
    // ... of the candidate's first control point (new_frames[0] of align_quaternion_frames_automatically): plain rows of E', mean'
    auto cp0_row = [&](size_t row, int d) {
        im.bias[row] = means[(size_t)d];
        for (int k = 0; k < L; k++) im.W[row * L + k] = Es[(size_t)d * L + k];
    };
    auto fill_quats = [&](size_t row, const std::vector<int> &ch, int count, auto channel_row) {   // (w,x,y,z) of ch[0 .. count-1]
        for (int i = 0; i < count; i++) {
            const int qc = sk ? sk->quat_channel[ch[(size_t)i]] : 3;
            for (int e = 0; e < 4; e++) {
                if (qc >= 0) channel_row(row + 4 * i + e, qc + e);
                else im.bias[row + 4 * i + e] = (e == 0) ? 1.0 : 0.0;   // not animated: identity, zero matrix row
            }
        }
    };
    auto fill_offsets = [&](int c, int which, const std::vector<int> &ch) {   // the links' offsets: those of ch[1 ..]
        for (size_t i = 0; i + 1 < ch.size(); i++)
            for (int e = 0; e < 3; e++) im.choff[(((size_t)c * 2 + which) * MG_MAX_CHAIN + i) * 3 + e] = sk->offsets[(size_t)ch[i + 1] * 3 + e];
    };
    for (int c = 0; c < n; c++) {
        const mg_keyframe_constraint &k = cons[c];
        const int type = k.type;
        MG_REQUIRE(type >= MG_CONSTRAINT_POSITION && type <= MG_CONSTRAINT_VALUE_HEADING,
                   "mg_constraint_set_create: constraint %d has unknown type %d", c, type);
        MG_REQUIRE(std::isfinite(k.canonical_keyframe), "mg_constraint_set_create: constraint %d keyframe not finite", c);
        MG_REQUIRE((type == MG_CONSTRAINT_VALUE_POSITION || type == MG_CONSTRAINT_VALUE_HEADING) ? (k.target[0] == 0.0 || k.target[0] == 2.0 ||
                   (type == MG_CONSTRAINT_VALUE_POSITION && k.target[0] == 1.0)) : true, "mg_constraint_set_create: constraint %d: value constraints select a component with target[0] = 0, (1,) 2", c);
        const mg_constraint_rule &r = mg_constraint_rule_of(type);
        MG_REQUIRE(D >= r.min_D, "mg_constraint_set_create: constraint %d needs more pose channels than n_dim = %d", c, D);
        mg_basis_row(knots.data(), (int)knots.size(), k.canonical_keyframe, &i0, w);
        mg_constraint_par_row(k, &im.par[(size_t)c * 8]);
        if (r.kind == MG_RULE_ROOT) {
            const size_t r0 = add_rows(c, im.nch);
            for (int d = 0; d < im.nch; d++) spline_row(r0 + d, d);
        } else if (r.kind == MG_RULE_POSE) {
            MG_REQUIRE(sk != nullptr, "mg_constraint_set_create: constraint %d (pose) needs a skeleton", c);
            MG_REQUIRE(k.joint >= 0 && k.joint < n_poses, "mg_constraint_set_create: constraint %d refers to pose %d of %d", c, k.joint, n_poses);
            const mg_pose_constraint &pc = poses[k.joint];
            MG_REQUIRE(pc.n_points > 0 && pc.n_points <= MG_MAX_POSE_POINTS && pc.joints && pc.points && pc.weights,
                       "mg_constraint_set_create: pose %d: 1..%d points with joints, points and weights", k.joint, MG_MAX_POSE_POINTS);
            double sw = 0.0;
            for (int i = 0; i < pc.n_points; i++) {
                MG_REQUIRE(has_joint(pc.joints[i]), "mg_constraint_set_create: pose %d: joint %d out of range", k.joint, pc.joints[i]);
                MG_REQUIRE(std::isfinite(pc.weights[i]) && std::isfinite(pc.points[3 * i]) && std::isfinite(pc.points[3 * i + 1]) && std::isfinite(pc.points[3 * i + 2]),
                           "mg_constraint_set_create: pose %d: point %d not finite", k.joint, i);
                sw += pc.weights[i];
            }
            MG_REQUIRE(sw != 0.0, "mg_constraint_set_create: pose %d: weights sum to zero", k.joint);
            const int block = 3 + 4 * n_slots, blocks = pc.has_velocity ? 2 : 1;
            const size_t off = im.pose_tab.size();
            im.par[(size_t)c * 8 + 2] = (double)off;
            im.pose_tab.resize(off + MG_POSE_HDR + (size_t)pc.n_points * MG_POSE_REC, 0.0);
            double *tb = &im.pose_tab[off];
            tb[0] = pc.n_points; tb[1] = pc.has_velocity ? 1.0 : 0.0; tb[2] = pc.velocity[0]; tb[3] = pc.velocity[1]; tb[4] = pc.velocity[2];
            tb[5] = block;
            for (int i = 0; i < pc.n_points; i++) {
                double *rec = tb + MG_POSE_HDR + (size_t)i * MG_POSE_REC;
                rec[0] = pc.points[3 * i]; rec[1] = pc.points[3 * i + 1]; rec[2] = pc.points[3 * i + 2]; rec[3] = pc.weights[i];
                chain_of(pc.joints[i], chain);
                const int m = (int)chain.size() - 1;
                MG_REQUIRE(m <= MG_MAX_CHAIN, "mg_constraint_set_create: pose %d: chain of %d joints exceeds %d", k.joint, m, MG_MAX_CHAIN);
                rec[4] = m;
                mg_chain_links(chain, sk->offsets, [&](int j) { return slot[(size_t)j] >= 0 ? 3 + 4 * slot[(size_t)j] : -1; }, rec + 5);   // channels of the pose block
            }
            const size_t r0 = add_rows(c, block * blocks);
            for (int blk = 0; blk < blocks; blk++) {
                if (blk == 1) mg_basis_row(knots.data(), (int)knots.size(), k.canonical_keyframe + 1.0, &i0, w);   // frame2 = evaluate(t + 1)
                const size_t rb = r0 + (size_t)blk * block;
                for (int d = 0; d < 3; d++) spline_row(rb + d, d);
                for (int j = 0; j < sk->n_joints; j++)
                    if (slot[(size_t)j] >= 0)
                        for (int e = 0; e < 4; e++) spline_row(rb + 3 + 4 * slot[(size_t)j] + e, sk->quat_channel[j] + e);
            }
        } else {
            if (r.kind == MG_RULE_SKELETON) {
                MG_REQUIRE(sk != nullptr, "mg_constraint_set_create: constraint %d needs a skeleton (mg_constraint_set_create_fk)", c);
                if (r.second)
                    MG_REQUIRE(has_joint(k.joint) && has_joint(k.joint2), "mg_constraint_set_create_fk: constraint %d: joints %d, %d out of range", c, k.joint, k.joint2);
                else
                    MG_REQUIRE(has_joint(k.joint), "mg_constraint_set_create_fk: constraint %d: joint %d out of range", c, k.joint);
            } else {
                MG_REQUIRE(k.joint == 0 || has_joint(k.joint), "mg_constraint_set_create_fk: constraint %d: joint %d needs a skeleton that has it", c, k.joint);
            }
            chain_of(k.joint, chain);
            if (r.second) chain_of(k.joint2, chain2);
            const bool relative = r.relative && (k.ref_dir[0] != 0.0 || k.ref_dir[1] != 0.0 || k.ref_dir[2] != 0.0);
            const int m = (int)chain.size() - 1 + ((r.own_quat || relative) ? 1 : 0), m2 = r.second ? (int)chain2.size() - 1 : 0;
            if (r.second)
                MG_REQUIRE(m <= MG_MAX_CHAIN && m2 <= MG_MAX_CHAIN, "mg_constraint_set_create_fk: constraint %d: chain exceeds %d joints", c, MG_MAX_CHAIN);
            else
                MG_REQUIRE(m <= MG_MAX_CHAIN, "mg_constraint_set_create_fk: constraint %d: chain of %d joints exceeds %d", c, m, MG_MAX_CHAIN);
            if (r.vectors == MG_VEC_TARGET_REF)
                MG_REQUIRE(mg_nonzero3(k.target) && mg_nonzero3(k.ref_dir), "mg_constraint_set_create: constraint %d: zero target or reference vector", c);
            else if (r.vectors != MG_VEC_NONE)
                MG_REQUIRE(mg_nonzero3(k.ref_dir), "mg_constraint_set_create: constraint %d: zero reference vector", c);
            if (r.vectors == MG_VEC_REF_FINITE_TARGET)
                MG_REQUIRE(std::isfinite(k.target[0]) && std::isfinite(k.target[1]) && std::isfinite(k.target[2]),
                           "mg_constraint_set_create: constraint %d: look-at target not finite", c);
            im.chain_len[(size_t)c] = m | (m2 << 16);
            const int q = std::max(m, 1), q2 = r.second ? std::max(m2, 1) : 0, root = r.root_rows ? 3 : 0;
            const size_t r0 = add_rows(c, root + 4 * q + 4 * q2);
            for (int d = 0; d < root; d++) spline_row(r0 + d, d);
            fill_quats(r0 + root, chain, q, spline_row);
            if (r.second) fill_quats(r0 + root + 4 * q, chain2, q2, spline_row);
            if (r.root_rows) {
                fill_offsets(c, 0, chain);
                if (r.second) fill_offsets(c, 1, chain2);
            }
            if (relative)   // the point itself as the last link
                for (int e = 0; e < 3; e++) im.choff[(((size_t)c * 2) * MG_MAX_CHAIN + (m - 1)) * 3 + e] = k.ref_dir[e];
        }
    }
    const size_t ra = add_rows(n, al ? 3 + 4 * (int)al_chain.size() : 0), rows_total = (size_t)im.woff[(size_t)n + 1];
    if (al) {
        for (int d = 0; d < 3; d++) cp0_row(ra + d, d);
        fill_quats(ra + 3, al_chain, (int)al_chain.size(), cp0_row);
    }
    im.W.resize(std::max<size_t>(rows_total, 1) * L, 0.0);
    im.bias.resize(std::max<size_t>(rows_total, 1), 0.0);
    im.has_pose = !im.pose_tab.empty();
    if (KK > 0 && rows_total > 0) {
        // the set's rows W for channels = X . W^T (mg_pack.h)
        im.RT = (int32_t)((rows_total + 15) / 16);
        im.rows = (int32_t)rows_total;
        im.wpack.resize((size_t)im.RT * KK * 64);
        im.bpad.assign((size_t)im.RT * 16, 0.0);
        std::copy(im.bias.begin(), im.bias.begin() + rows_total, im.bpad.begin());
        mg_pack_fragments(im.wpack.data(), im.RT, KK, [&](int row, int k) { return k < L && (size_t)row < rows_total ? im.W[(size_t)row * L + k] : 0.0; });
    }
    return MG_OK;
}
