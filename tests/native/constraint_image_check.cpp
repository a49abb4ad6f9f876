// What the constraint-set image of csrc/mg_constraint_image.h must contain, checked by DECODING it against a restatement of the layout
// written from the comments at mg_constraint_set / MG_POSE_* (mg_internal.h, mg_hostdefs.h) and the scorers' reads (mg_score_device.h),
// one plain case per constraint type, not from the builder's rule table; then the limits and every refusal with its full text, code
// and precedence.  Plain host code with its own main (test infrastructure, never linked into the library); exit status 0 = every
// check held.
#include "../../morphablegraphs_amd/csrc/mg_constraint_image.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 30) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static char g_err[1024] = "";
void mg_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

// ---- the primitive, by formula: L = 5, D = 3 + 4 * 4, 7 basis functions (clamped cubic knots 0 .. 4), KK = 2 ------------------------
struct Model {
    int L = 5, D = 19, NB = 7, KK = 2;
    std::vector<double> knots = {0, 0, 0, 0, 1, 2, 3, 4, 4, 4, 4}, means, Es;
    Model() {
        for (int r = 0; r < NB * D; r++) {
            means.push_back(r == 3 ? -0.0 : 0.25 * r - 7.0 + 1.0 / (r + 3.0));                     // no two alike; a negative zero in the first control point
            for (int k = 0; k < L; k++) Es.push_back((r % 7 == 3 && k == 2) ? -0.0 : 1.0 / (1.0 + r + 0.37 * k) - 0.01 * k * r);   // a few negative zeros
        }
    }
};
// ---- the skeleton: 6 joints, a branch at the root, joint 2 not animated.  19 channels hold four quaternions, so the two leaves read
// the same one; their chains differ in length and in every other joint ---------------------------------------------------------------
struct Skel {
    std::vector<int32_t> parents, qc;
    std::vector<double> offsets;
    mg_skeleton_desc desc;
    Skel(std::vector<int32_t> p, std::vector<int32_t> q) : parents(p), qc(q) {
        for (size_t j = 0; j < p.size(); j++) for (int e = 0; e < 3; e++) offsets.push_back(10.0 * j + e + 1.0 + 0.125 * e * j);
        desc = {(int32_t)p.size(), 0, parents.data(), offsets.data(), qc.data()};
    }
};
static Skel tree() { return Skel({-1, 0, 1, 2, 0, 4}, {3, 7, -1, 11, 15, 11}); }
static Skel line(int J) {   // a line of J joints, only the root animated: chains of any length on 19 channels
    std::vector<int32_t> p, q;
    for (int j = 0; j < J; j++) { p.push_back(j - 1); q.push_back(j == 0 ? 3 : -1); }
    return Skel(p, q);
}

static mg_keyframe_constraint con(int type, double t, int joint = 0, int joint2 = 0) {
    mg_keyframe_constraint k;
    std::memset(&k, 0, sizeof(k));
    k.type = type; k.joint = joint; k.joint2 = joint2; k.canonical_keyframe = t; k.weight_factor = 0.5 + type;
    k.target[0] = 1.5; k.target[1] = -2.5; k.target[2] = 3.5;
    if (type == MG_CONSTRAINT_VALUE_POSITION || type == MG_CONSTRAINT_VALUE_HEADING) k.target[0] = 2.0;
    if (type != MG_CONSTRAINT_JOINT_POSITION) { k.ref_dir[0] = 0.0; k.ref_dir[1] = 0.6; k.ref_dir[2] = 0.8; }
    return k;
}
static mg_keyframe_constraint relative(mg_keyframe_constraint k, double x, double y, double z) { k.ref_dir[0] = x; k.ref_dir[1] = y; k.ref_dir[2] = z; return k; }

struct Pose {
    std::vector<int32_t> joints;
    std::vector<double> points, weights;
    mg_pose_constraint desc;
    Pose(std::vector<int32_t> j, bool velocity) : joints(j) {
        for (size_t i = 0; i < j.size(); i++) { weights.push_back(0.5 + i); for (int e = 0; e < 3; e++) points.push_back(100.0 + 3 * i + e); }
        desc = {(int32_t)j.size(), velocity ? 1 : 0, joints.data(), points.data(), weights.data(), {0.25, -0.5, 0.75}};
    }
};

static int build(const Model &m, const mg_skeleton_desc *sk, const std::vector<mg_keyframe_constraint> &cons, const std::vector<mg_pose_constraint> &poses,
                 const mg_alignment_desc *al, mg_constraint_image &im, int D = 0, int KK = -1) {
    g_err[0] = 0;
    return mg_constraint_image_build(m.L, D ? D : m.D, KK >= 0 ? KK : m.KK, m.knots, m.means, m.Es, sk, cons.empty() ? nullptr : cons.data(), (int32_t)cons.size(),
                                     poses.empty() ? nullptr : poses.data(), (int32_t)poses.size(), al, im);
}

// ---- the restatement -------------------------------------------------------------------------------------------------------------
enum { IDENTITY_W = -1, IDENTITY_XYZ = -2 };
struct Row { int d; double t; };   // pose channel d at keyframe t (t < 0: of the first control point), or a row of the identity quaternion
static std::vector<int> path(const mg_skeleton_desc *sk, int joint) {   // root .. joint
    std::vector<int> up;
    for (int j = joint; j >= 0; j = sk ? sk->parents[j] : -1) up.insert(up.begin(), j);
    return up;
}
static void quats(std::vector<Row> &rows, const mg_skeleton_desc *sk, const std::vector<int> &p, size_t count, double t) {
    for (size_t i = 0; i < count; i++) {
        const int ch = sk ? sk->quat_channel[p[i]] : 3;
        for (int e = 0; e < 4; e++) rows.push_back({ch >= 0 ? ch + e : (e == 0 ? IDENTITY_W : IDENTITY_XYZ), t});
    }
}
static void root_xyz(std::vector<Row> &rows, double t) { for (int d = 0; d < 3; d++) rows.push_back({d, t}); }
struct Want {
    std::vector<Row> rows;
    int m = 0, m2 = 0;
    std::vector<double> off[2];   // the links' offsets of the two chains, xyz each
};
static void link_offsets(std::vector<double> &off, const mg_skeleton_desc *sk, const std::vector<int> &p) {
    for (size_t i = 1; i < p.size(); i++) for (int e = 0; e < 3; e++) off.push_back(sk->offsets[3 * p[i] + e]);
}
static Want want_of(const Model &m, const mg_skeleton_desc *sk, const mg_keyframe_constraint &k, const mg_pose_constraint *poses, int D) {
    Want w;
    const double t = k.canonical_keyframe;
    const std::vector<int> p = k.type >= MG_CONSTRAINT_JOINT_POSITION && k.type != MG_CONSTRAINT_POSE && k.type != MG_CONSTRAINT_VALUE_POSITION ? path(sk, k.joint) : std::vector<int>();
    const int len = (int)p.size();
    switch (k.type) {
        case MG_CONSTRAINT_POSITION: case MG_CONSTRAINT_DIRECTION_2D: case MG_CONSTRAINT_VALUE_POSITION:   // [nch] rows: the first min(7, D) pose channels
            for (int d = 0; d < std::min(7, D); d++) w.rows.push_back({d, t});
            break;
        case MG_CONSTRAINT_JOINT_POSITION: {   // root xyz, the quaternions that place the joint (one at least); a relative point is one more link
            const bool rel = k.ref_dir[0] != 0.0 || k.ref_dir[1] != 0.0 || k.ref_dir[2] != 0.0;
            w.m = len - 1 + (rel ? 1 : 0);
            root_xyz(w.rows, t);
            quats(w.rows, sk, p, (size_t)std::max(w.m, 1), t);
            link_offsets(w.off[0], sk, p);
            if (rel) for (int e = 0; e < 3; e++) w.off[0].push_back(k.ref_dir[e]);
            break;
        }
        case MG_CONSTRAINT_JOINT_MIDPOINT: {   // root xyz, then both chains' quaternions; chain_len = m | m2 << 16
            const std::vector<int> p2 = path(sk, k.joint2);
            w.m = len - 1; w.m2 = (int)p2.size() - 1;
            root_xyz(w.rows, t);
            quats(w.rows, sk, p, (size_t)std::max(w.m, 1), t);
            quats(w.rows, sk, p2, (size_t)std::max(w.m2, 1), t);
            link_offsets(w.off[0], sk, p);
            link_offsets(w.off[1], sk, p2);
            break;
        }
        case MG_CONSTRAINT_JOINT_ORIENTATION: case MG_CONSTRAINT_VALUE_HEADING:   // every quaternion root .. joint, nothing else
            w.m = len;
            quats(w.rows, sk, p, (size_t)len, t);
            break;
        case MG_CONSTRAINT_LOOK_AT:   // root xyz, every quaternion root .. joint; the first m - 1 links place the joint
            w.m = len;
            root_xyz(w.rows, t);
            quats(w.rows, sk, p, (size_t)len, t);
            link_offsets(w.off[0], sk, p);
            break;
        case MG_CONSTRAINT_POSE:   // a pose block per frame: root xyz + every animated joint's quaternion in skeleton order; t + 1 with a velocity
            for (int blk = 0; blk < (poses[k.joint].has_velocity ? 2 : 1); blk++) {
                root_xyz(w.rows, t + blk);
                for (int j = 0; j < sk->n_joints; j++) if (sk->quat_channel[j] >= 0) for (int e = 0; e < 4; e++) w.rows.push_back({sk->quat_channel[j] + e, t + blk});
            }
            break;
    }
    (void)m;
    return w;
}

static void check_row(const char *what, const Model &m, int D, const mg_constraint_image &im, size_t row, const Row &r) {
    for (int k = -1; k < m.L; k++) {   // k = -1: the bias
        auto src = [&](int i) { return k < 0 ? m.means[(size_t)i * D + r.d] : m.Es[((size_t)i * D + r.d) * m.L + k]; };
        double want = 0.0;
        if (r.d == IDENTITY_W || r.d == IDENTITY_XYZ) want = (k < 0 && r.d == IDENTITY_W) ? 1.0 : 0.0;
        else if (r.t < 0.0) want = src(0);
        else {
            int32_t i0;
            double w[4];
            mg_basis_row(m.knots.data(), (int)m.knots.size(), r.t, &i0, w);
            for (int j = 0; j < 4; j++) want = want + w[j] * src(i0 + j);
        }
        const double got = k < 0 ? im.bias[row] : im.W[row * m.L + k];
        CHECK(std::memcmp(&got, &want, 8) == 0, "%s: row %zu (channel %d at %g), column %d holds %.17g, expected %.17g", what, row, r.d, r.t, k, got, want);
    }
}

// the whole image of an accepted set against the restatement
static void check_image(const char *what, const Model &m, const mg_skeleton_desc *sk, const std::vector<mg_keyframe_constraint> &cons,
                        const std::vector<mg_pose_constraint> &poses, const mg_alignment_desc *al, int D = 0, int KK = -1) {
    mg_constraint_image im;
    const int rc = build(m, sk, cons, poses, al, im, D, KK);
    CHECK(rc == MG_OK, "%s: refused with %d: %s", what, rc, g_err);
    if (rc != MG_OK) return;
    D = D ? D : m.D;
    KK = KK >= 0 ? KK : m.KK;
    const size_t n = cons.size(), n1 = std::max<size_t>(n, 1);
    CHECK(im.nch == std::min(7, D) && im.align_joint == (al ? al->joint : -1), "%s: nch %d, align_joint %d", what, im.nch, im.align_joint);
    CHECK(im.woff.size() == n + 2 && im.woff[0] == 0 && im.chain_len.size() == n1 && im.par.size() == n1 * 8 && im.choff.size() == n1 * 2 * MG_MAX_CHAIN * 3,
          "%s: table sizes", what);
    if (im.woff.size() != n + 2 || im.chain_len.size() != n1 || im.par.size() != n1 * 8 || im.choff.size() != n1 * 2 * MG_MAX_CHAIN * 3) return;
    size_t row = 0, pose_at = 0;
    std::vector<double> choff(im.choff.size(), 0.0), par(im.par.size(), 0.0);
    std::vector<Want> wants;
    for (size_t c = 0; c < n; c++) {
        wants.push_back(want_of(m, sk, cons[c], poses.data(), D));
        const Want &w = wants.back();
        CHECK((size_t)im.woff[c] == row && (size_t)im.woff[c + 1] == row + w.rows.size(), "%s: constraint %zu owns rows [%d, %d), expected [%zu, %zu)", what, c,
              im.woff[c], im.woff[c + 1], row, row + w.rows.size());
        row += w.rows.size();
        CHECK(im.chain_len[c] == (w.m | (w.m2 << 16)), "%s: constraint %zu: chain_len %d, expected %d | %d << 16", what, c, im.chain_len[c], w.m, w.m2);
        for (int which = 0; which < 2; which++)
            for (size_t q = 0; q < w.off[which].size(); q++) choff[((c * 2 + which) * MG_MAX_CHAIN) * 3 + q] = w.off[which][q];
        // par: type, weight, target[3], ref_dir[3]; direction: the unit target and its norm; pose: [2] = where its table starts
        double *q = &par[c * 8];
        q[0] = cons[c].type; q[1] = cons[c].weight_factor;
        for (int e = 0; e < 3; e++) { q[2 + e] = cons[c].target[e]; q[5 + e] = cons[c].ref_dir[e]; }
        if (cons[c].type == MG_CONSTRAINT_DIRECTION_2D) {
            const double tn = std::sqrt(cons[c].target[0] * cons[c].target[0] + cons[c].target[1] * cons[c].target[1]);
            q[2] = cons[c].target[0] / tn; q[3] = cons[c].target[1] / tn; q[4] = std::sqrt(q[2] * q[2] + q[3] * q[3]);
        }
        if (cons[c].type == MG_CONSTRAINT_POSE) {
            q[2] = (double)pose_at;
            // header [0] n_points, [1] has_velocity, [2..4] velocity, [5] rows of one block; records: target xyz, weight, m, m x (block row or -1, offset)
            const mg_pose_constraint &pc = poses[cons[c].joint];
            const size_t size = MG_POSE_HDR + (size_t)pc.n_points * MG_POSE_REC;
            CHECK(im.pose_tab.size() >= pose_at + size, "%s: pose table of constraint %zu does not fit", what, c);
            if (im.pose_tab.size() < pose_at + size) return;
            std::vector<double> tab(size, 0.0), block_row((size_t)sk->n_joints, -1.0);
            int slots = 0;
            for (int j = 0; j < sk->n_joints; j++) if (sk->quat_channel[j] >= 0) block_row[j] = 3 + 4 * slots++;
            tab[0] = pc.n_points; tab[1] = pc.has_velocity ? 1 : 0; tab[2] = pc.velocity[0]; tab[3] = pc.velocity[1]; tab[4] = pc.velocity[2]; tab[5] = 3 + 4 * slots;
            for (int i = 0; i < pc.n_points; i++) {
                double *rec = &tab[MG_POSE_HDR + (size_t)i * MG_POSE_REC];
                const std::vector<int> p = path(sk, pc.joints[i]);
                for (int e = 0; e < 3; e++) rec[e] = pc.points[3 * i + e];
                rec[3] = pc.weights[i]; rec[4] = (double)p.size() - 1;
                for (size_t l = 0; l + 1 < p.size(); l++) { rec[5 + 4 * l] = block_row[p[l]]; for (int e = 0; e < 3; e++) rec[6 + 4 * l + e] = sk->offsets[3 * p[l + 1] + e]; }
            }
            CHECK(std::memcmp(tab.data(), &im.pose_tab[pose_at], size * 8) == 0, "%s: pose table of constraint %zu differs", what, c);
            pose_at += size;
        }
    }
    CHECK(im.pose_tab.size() == pose_at && im.has_pose == (pose_at > 0), "%s: pose tables hold %zu doubles, expected %zu", what, im.pose_tab.size(), pose_at);
    // choff: exact copies of the skeleton's offsets, the relative point as the last link, zero everywhere else
    CHECK(std::memcmp(choff.data(), im.choff.data(), choff.size() * 8) == 0, "%s: choff differs", what);
    CHECK(std::memcmp(par.data(), im.par.data(), par.size() * 8) == 0, "%s: par differs", what);
    // the alignment: rows of the first control point at woff[n] (root xyz, the chain's quaternions) and the record
    Want wa;
    if (al) {
        const std::vector<int> p = al->joint == MG_ALIGN_START_POSE ? std::vector<int>() : path(sk, al->joint);
        root_xyz(wa.rows, -1.0);
        quats(wa.rows, sk, p, p.size(), -1.0);
        const double hn = std::sqrt(al->heading[0] * al->heading[0] + al->heading[1] * al->heading[1]);
        const bool start = al->joint == MG_ALIGN_START_POSE;
        const double rec[8] = {(double)p.size(), al->heading[0] / hn, al->heading[1] / hn, al->position[0], al->position[2],
                               start ? al->position[1] : al->ref_dir[0], start ? 0.0 : al->ref_dir[1], start ? 0.0 : al->ref_dir[2]};
        CHECK(im.align.size() == 8 && std::memcmp(rec, im.align.data(), 64) == 0, "%s: alignment record differs", what);
        double upd[8];
        CHECK(mg_alignment_record("mg_constraint_set_update", al, 0, upd) == MG_OK && std::memcmp(upd + 1, rec + 1, 56) == 0, "%s: the update's seven values differ", what);
        wants.push_back(wa);
    } else CHECK(im.align.empty(), "%s: an alignment record without an alignment", what);
    CHECK((size_t)im.woff[n] == row && (size_t)im.woff[n + 1] == row + wa.rows.size(), "%s: alignment rows [%d, %d), expected [%zu, %zu)", what, im.woff[n], im.woff[n + 1],
          row, row + wa.rows.size());
    row += wa.rows.size();
    CHECK(im.W.size() == std::max<size_t>(row, 1) * m.L && im.bias.size() == std::max<size_t>(row, 1), "%s: W holds %zu values for %zu rows", what, im.W.size(), row);
    if ((size_t)im.woff[n + 1] != row || im.W.size() != std::max<size_t>(row, 1) * m.L || im.bias.size() != std::max<size_t>(row, 1)) return;
    size_t at = 0;
    for (const Want &w : wants) for (const Row &r : w.rows) check_row(what, m, D, im, at++, r);
    if (row == 0) CHECK(im.bias[0] == 0.0 && !std::signbit(im.bias[0]), "%s: the one row of an empty set is not zero", what);
    // Wpack: [RT][KK][64], lane l of k-step kk holds W[16 tile + (l & 15)][4 kk + (l >> 4)], zero outside; bpad: bias, zero beyond rows
    if (KK > 0 && row > 0) {
        const size_t RT = (row + 15) / 16;
        CHECK((size_t)im.RT == RT && (size_t)im.rows == row && im.wpack.size() == RT * KK * 64 && im.bpad.size() == RT * 16, "%s: RT %d, rows %d", what, im.RT, im.rows);
        if (im.wpack.size() != RT * KK * 64 || im.bpad.size() != RT * 16) return;
        for (size_t e = 0; e < im.wpack.size(); e++) {
            const size_t lane = e % 64, kk = e / 64 % KK, tile = e / 64 / KK, i = 16 * tile + (lane & 15), k = 4 * kk + (lane >> 4);
            const double want = i < row && k < (size_t)m.L ? im.W[i * m.L + k] : 0.0;
            CHECK(std::memcmp(&im.wpack[e], &want, 8) == 0, "%s: Wpack element %zu (row %zu, column %zu) holds %g", what, e, i, k, im.wpack[e]);
        }
        for (size_t r = 0; r < RT * 16; r++) { const double want = r < row ? im.bias[r] : 0.0; CHECK(std::memcmp(&im.bpad[r], &want, 8) == 0, "%s: bpad[%zu] = %g", what, r, im.bpad[r]); }
    } else CHECK(im.RT == 0 && im.rows == 0 && im.wpack.empty() && im.bpad.empty(), "%s: an MFMA image without rows or k-steps", what);
}

static void check_refused(const char *what, const Model &m, const mg_skeleton_desc *sk, const std::vector<mg_keyframe_constraint> &cons,
                          const std::vector<mg_pose_constraint> &poses, const mg_alignment_desc *al, const char *text, int D = 0) {
    mg_constraint_image im;
    const int rc = build(m, sk, cons, poses, al, im, D);
    CHECK(rc == MG_ERR_INVALID_ARGUMENT && std::string(g_err) == text, "%s: status %d \"%s\", expected %d \"%s\"", what, rc, g_err, MG_ERR_INVALID_ARGUMENT, text);
}

static mg_alignment_desc alignment(int joint) { return {joint, 0, {4.0, 5.5, -6.0}, {3.0, -4.0}, {0.6, 0.0, 0.8}}; }

static void check_layout(const Model &m) {
    const Skel sk = tree();
    const Pose still({0, 3, 5, 2}, false), moving({5, 1}, true);
    const std::vector<mg_pose_constraint> poses = {still.desc, moving.desc};
    const mg_alignment_desc root = alignment(0), leaf = alignment(3), start = alignment(MG_ALIGN_START_POSE);
    const std::vector<mg_keyframe_constraint> every = {
        con(MG_CONSTRAINT_POSITION, 0.0), con(MG_CONSTRAINT_DIRECTION_2D, 4.0),
        con(MG_CONSTRAINT_JOINT_POSITION, 1.5, 0),                                      // the root: m = 0, one quaternion row block all the same
        con(MG_CONSTRAINT_JOINT_POSITION, 2.25, 3),                                     // zero relative point, through the unanimated joint
        relative(con(MG_CONSTRAINT_JOINT_POSITION, 2.25, 3), 0.0, -3.0, 12.0),
        relative(con(MG_CONSTRAINT_JOINT_POSITION, 3.0, 0), 1.0, 0.0, 0.0),             // a relative point at the root
        con(MG_CONSTRAINT_JOINT_MIDPOINT, 0.5, 3, 5), con(MG_CONSTRAINT_JOINT_MIDPOINT, 0.5, 0, 4), con(MG_CONSTRAINT_JOINT_MIDPOINT, 3.75, 5, 0),
        con(MG_CONSTRAINT_JOINT_ORIENTATION, 1.0, 3), con(MG_CONSTRAINT_LOOK_AT, 2.0, 5), con(MG_CONSTRAINT_VALUE_HEADING, 3.5, 3),
        con(MG_CONSTRAINT_VALUE_POSITION, 4.0), con(MG_CONSTRAINT_POSE, 1.25, 0), con(MG_CONSTRAINT_POSE, 2.0, 1), con(MG_CONSTRAINT_POSE, 3.5, 1)};
    for (const mg_alignment_desc *al : {(const mg_alignment_desc *)nullptr, &root, &leaf, &start}) {
        check_image("every type", m, &sk.desc, every, poses, al);
        check_image("every type, no MFMA image", m, &sk.desc, every, poses, al, 0, 0);
        check_image("the empty set", m, &sk.desc, {}, {}, al);
        for (size_t c = 0; c < every.size(); c++) check_image("one constraint", m, &sk.desc, {every[c]}, poses, al);
    }
    // without a skeleton: joint 0 is the root's quaternion at channel 3
    const std::vector<mg_keyframe_constraint> bare = {con(MG_CONSTRAINT_LOOK_AT, 0.75, 0), con(MG_CONSTRAINT_JOINT_ORIENTATION, 4.0, 0), con(MG_CONSTRAINT_VALUE_HEADING, 0.0, 0),
                                                      con(MG_CONSTRAINT_POSITION, 2.5)};
    check_image("no skeleton", m, nullptr, bare, {}, nullptr);
    check_image("no skeleton, aligned", m, nullptr, bare, {}, &root);
    check_image("no skeleton, start pose", m, nullptr, {}, {}, &start);
    // fewer than 7 channels: position constraints only, on min(7, D) rows
    for (int D : {3, 5}) check_image("a position on few channels", m, nullptr, {con(MG_CONSTRAINT_POSITION, 1.0), con(MG_CONSTRAINT_POSITION, 3.25)}, {}, nullptr, D);
}

static void check_limits(const Model &m) {
    const int M = MG_MAX_CHAIN;
    const Skel sk = line(M + 2);   // joint j hangs on a chain of j + 1 joints
    const mg_alignment_desc fits = alignment(M - 1), over = alignment(M);
    const mg_keyframe_constraint jp = con(MG_CONSTRAINT_JOINT_POSITION, 1.0, M), rel = relative(con(MG_CONSTRAINT_JOINT_POSITION, 1.0, M - 1), 0.0, 2.0, 0.0);
    check_image("joint position, 32 links", m, &sk.desc, {jp}, {}, nullptr);
    check_image("relative point, 32 links", m, &sk.desc, {rel}, {}, nullptr);
    check_image("midpoint, 32 and 0 links", m, &sk.desc, {con(MG_CONSTRAINT_JOINT_MIDPOINT, 1.0, M, 0)}, {}, nullptr);
    check_image("midpoint, 0 and 32 links", m, &sk.desc, {con(MG_CONSTRAINT_JOINT_MIDPOINT, 1.0, 0, M)}, {}, nullptr);
    check_image("aligned to a chain of 32", m, &sk.desc, {}, {}, &fits);
    check_refused("joint position, 33 links", m, &sk.desc, {con(MG_CONSTRAINT_JOINT_POSITION, 1.0, M + 1)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: chain of 33 joints exceeds 32");
    check_refused("relative point, 33 links", m, &sk.desc, {con(MG_CONSTRAINT_POSITION, 1.0), relative(jp, 0.0, 2.0, 0.0)}, {}, nullptr,
                  "mg_constraint_set_create_fk: constraint 1: chain of 33 joints exceeds 32");
    check_refused("midpoint, 33 links", m, &sk.desc, {con(MG_CONSTRAINT_JOINT_MIDPOINT, 1.0, M + 1, 0)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: chain exceeds 32 joints");
    check_refused("midpoint, 33 links on the second chain", m, &sk.desc, {con(MG_CONSTRAINT_JOINT_MIDPOINT, 1.0, 0, M + 1)}, {}, nullptr,
                  "mg_constraint_set_create_fk: constraint 0: chain exceeds 32 joints");
    for (int type : {MG_CONSTRAINT_JOINT_ORIENTATION, MG_CONSTRAINT_LOOK_AT, MG_CONSTRAINT_VALUE_HEADING}) {   // the joint's own quaternion counts
        check_image("32 quaternions", m, &sk.desc, {con(type, 1.0, M - 1)}, {}, nullptr);
        check_refused("33 quaternions", m, &sk.desc, {con(type, 1.0, M)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: chain of 33 joints exceeds 32");
    }
    check_refused("aligned to a chain of 33", m, &sk.desc, {}, {}, &over, "mg_constraint_set_create_aligned: chain of 33 joints exceeds 32");
    const Pose deep({0, M}, false), deeper({0, M + 1}, false);
    check_image("pose point on 32 links", m, &sk.desc, {con(MG_CONSTRAINT_POSE, 1.0, 0)}, {deep.desc}, nullptr);
    check_refused("pose point on 33 links", m, &sk.desc, {con(MG_CONSTRAINT_POSE, 1.0, 0)}, {deeper.desc}, nullptr, "mg_constraint_set_create: pose 0: chain of 33 joints exceeds 32");
    const Skel small = tree();
    std::vector<int32_t> many;
    for (int i = 0; i < MG_MAX_POSE_POINTS + 1; i++) many.push_back(i % 6);
    const Pose most(std::vector<int32_t>(many.begin(), many.end() - 1), true), too_many(many, true);
    check_image("64 pose points", m, &small.desc, {con(MG_CONSTRAINT_POSE, 1.0, 0)}, {most.desc}, nullptr);
    check_refused("65 pose points", m, &small.desc, {con(MG_CONSTRAINT_POSE, 1.0, 0)}, {too_many.desc}, nullptr,
                  "mg_constraint_set_create: pose 0: 1..64 points with joints, points and weights");
}

// every refusal with its full text; where two checks could both fire, the first of the historical order wins
static void check_refusals(const Model &m) {
    const Skel sk = tree();
    const mg_skeleton_desc *s = &sk.desc;
    const mg_alignment_desc root = alignment(0);
    auto with = [](mg_keyframe_constraint k, auto change) { change(k); return k; };
    const mg_keyframe_constraint ok = con(MG_CONSTRAINT_POSITION, 1.0);
    // the skeleton, ahead of the alignment and of every constraint
    Skel bad = tree();
    bad.desc.offsets = nullptr;
    check_refused("skeleton without offsets", m, &bad.desc, {con(99, NaN)}, {}, nullptr, "mg_constraint_set_create_fk: incomplete skeleton");
    bad = tree(); bad.desc.n_joints = 0;
    check_refused("skeleton without joints", m, &bad.desc, {}, {}, nullptr, "mg_constraint_set_create_fk: incomplete skeleton");
    bad = tree(); bad.parents[0] = 0; bad.parents[2] = 4;
    check_refused("joint 0 has a parent", m, &bad.desc, {}, {}, nullptr, "mg_constraint_set_create_fk: joint 0 must be the root");
    bad = tree(); bad.parents[2] = 4; bad.qc[1] = 16;
    check_refused("channel outside n_dim, ahead of a later joint's order", m, &bad.desc, {}, {}, nullptr, "mg_constraint_set_create_fk: joint 1: quaternion channel 16 outside n_dim = 19");
    bad = tree(); bad.parents[2] = 4; bad.qc[2] = 16;
    check_refused("parents out of order, ahead of the same joint's channel", m, &bad.desc, {}, {}, &root, "mg_constraint_set_create_fk: joint 2: parents must precede their children");
    bad = tree(); bad.parents[3] = 3;
    check_refused("a joint that is its own parent", m, &bad.desc, {}, {}, nullptr, "mg_constraint_set_create_fk: joint 3: parents must precede their children");
    // the alignment, ahead of every constraint
    mg_alignment_desc al = alignment(7);
    check_refused("alignment on few channels, ahead of its joint", m, nullptr, {con(MG_CONSTRAINT_POSITION, 1.0)}, {}, &al, "mg_constraint_set_create_aligned: alignment needs the root quaternion, n_dim = 5", 5);
    check_refused("aligning joint out of range", m, s, {con(99, 1.0)}, {}, &al, "mg_constraint_set_create_aligned: aligning joint 7 needs a skeleton that has it");
    al = alignment(3);
    check_refused("aligning joint without a skeleton", m, nullptr, {}, {}, &al, "mg_constraint_set_create_aligned: aligning joint 3 needs a skeleton that has it");
    al = alignment(-2);
    check_refused("aligning joint -2", m, s, {}, {}, &al, "mg_constraint_set_create_aligned: aligning joint -2 needs a skeleton that has it");
    const Skel deep = line(MG_MAX_CHAIN + 1);
    for (int what = 0; what < 5; what++) {   // heading zero or not finite, position not finite: ahead of the chain's length
        al = alignment(MG_MAX_CHAIN);
        if (what == 0) al.heading[0] = al.heading[1] = 0.0;
        if (what == 1) al.heading[1] = NaN;
        if (what == 2) al.heading[0] = Inf;
        if (what == 3) al.position[0] = NaN;
        if (what == 4) al.position[2] = -Inf;
        check_refused("heading / position", m, &deep.desc, {con(99, 1.0)}, {}, &al, "mg_constraint_set_create_aligned: previous heading / position not finite or zero");
        double rec[8];
        g_err[0] = 0;
        CHECK(mg_alignment_record("mg_constraint_set_update", &al, 0, rec) == MG_ERR_INVALID_ARGUMENT &&
              std::string(g_err) == "mg_constraint_set_update: previous heading / position not finite or zero", "the update's refusal %d: \"%s\"", what, g_err);
    }
    al = alignment(0); al.position[1] = NaN;   // the height is not looked at outside start-pose mode
    check_image("aligned, height not finite", m, s, {ok}, {}, &al);
    // a constraint's own checks, in their order; the first bad constraint wins
    check_refused("unknown type, ahead of its keyframe", m, s, {ok, con(9, NaN), con(-1, 1.0)}, {}, nullptr, "mg_constraint_set_create: constraint 1 has unknown type 9");
    check_refused("unknown type -1", m, s, {con(-1, 1.0)}, {}, nullptr, "mg_constraint_set_create: constraint 0 has unknown type -1");
    check_refused("keyframe not finite, ahead of the component", m, s, {with(con(MG_CONSTRAINT_VALUE_HEADING, Inf), [](auto &k) { k.target[0] = 1.0; })}, {}, nullptr,
                  "mg_constraint_set_create: constraint 0 keyframe not finite");
    check_refused("keyframe NaN", m, s, {ok, ok, con(MG_CONSTRAINT_DIRECTION_2D, NaN)}, {}, nullptr, "mg_constraint_set_create: constraint 2 keyframe not finite");
    const char *component = "mg_constraint_set_create: constraint 0: value constraints select a component with target[0] = 0, (1,) 2";
    check_refused("heading component 1, ahead of D", m, nullptr, {with(con(MG_CONSTRAINT_VALUE_HEADING, 1.0), [](auto &k) { k.target[0] = 1.0; })}, {}, nullptr, component, 5);
    check_refused("position component 3", m, s, {with(con(MG_CONSTRAINT_VALUE_POSITION, 1.0), [](auto &k) { k.target[0] = 3.0; })}, {}, nullptr, component);
    check_refused("position component 0.5", m, s, {with(con(MG_CONSTRAINT_VALUE_POSITION, 1.0), [](auto &k) { k.target[0] = 0.5; })}, {}, nullptr, component);
    check_image("position component 1", m, s, {with(con(MG_CONSTRAINT_VALUE_POSITION, 1.0), [](auto &k) { k.target[0] = 1.0; })}, {}, nullptr);
    check_refused("a position on 2 channels", m, nullptr, {con(MG_CONSTRAINT_POSITION, 1.0)}, {}, nullptr, "mg_constraint_set_create: constraint 0 needs more pose channels than n_dim = 2", 2);
    for (int type = MG_CONSTRAINT_DIRECTION_2D; type <= MG_CONSTRAINT_VALUE_HEADING; type++)   // D too small, ahead of the missing skeleton and the joint
        check_refused("6 channels", m, nullptr, {ok, con(type, 1.0, 9, 9)}, {}, nullptr, "mg_constraint_set_create: constraint 1 needs more pose channels than n_dim = 6", 6);
    for (int type : {MG_CONSTRAINT_JOINT_POSITION, MG_CONSTRAINT_JOINT_MIDPOINT})   // skeleton missing, ahead of the joint
        check_refused("no skeleton", m, nullptr, {con(type, 1.0, 9, 9)}, {}, nullptr, "mg_constraint_set_create: constraint 0 needs a skeleton (mg_constraint_set_create_fk)");
    check_refused("pose without a skeleton, ahead of its index", m, nullptr, {con(MG_CONSTRAINT_POSE, 1.0, 4)}, {}, nullptr, "mg_constraint_set_create: constraint 0 (pose) needs a skeleton");
    check_refused("joint 6 of 6", m, s, {con(MG_CONSTRAINT_JOINT_POSITION, 1.0, 6)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: joint 6 out of range");
    check_refused("joint -1", m, s, {ok, con(MG_CONSTRAINT_JOINT_POSITION, 1.0, -1)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 1: joint -1 out of range");
    check_refused("midpoint, first joint", m, s, {con(MG_CONSTRAINT_JOINT_MIDPOINT, 1.0, 6, 2)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: joints 6, 2 out of range");
    check_refused("midpoint, second joint", m, s, {con(MG_CONSTRAINT_JOINT_MIDPOINT, 1.0, 2, -3)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: joints 2, -3 out of range");
    for (int type : {MG_CONSTRAINT_JOINT_ORIENTATION, MG_CONSTRAINT_LOOK_AT, MG_CONSTRAINT_VALUE_HEADING}) {
        const auto zero_ref = [](auto &k) { k.ref_dir[0] = k.ref_dir[1] = k.ref_dir[2] = 0.0; };
        // the joint, ahead of the vectors
        check_refused("joint without a skeleton", m, nullptr, {with(con(type, 1.0, 3), zero_ref)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: joint 3 needs a skeleton that has it");
        check_refused("joint 6 of 6", m, s, {with(con(type, 1.0, 6), zero_ref)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: joint 6 needs a skeleton that has it");
        check_refused("joint -1", m, s, {con(type, 1.0, -1)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: joint -1 needs a skeleton that has it");
        // the chain's length, ahead of the vectors
        check_refused("33 quaternions, ahead of the vectors", m, &deep.desc, {with(con(type, 1.0, MG_MAX_CHAIN), zero_ref)}, {}, nullptr, "mg_constraint_set_create_fk: constraint 0: chain of 33 joints exceeds 32");
        const char *text = type == MG_CONSTRAINT_JOINT_ORIENTATION ? "mg_constraint_set_create: constraint 0: zero target or reference vector" : "mg_constraint_set_create: constraint 0: zero reference vector";
        // a zero reference vector, ahead of the look-at's target
        check_refused("zero reference vector", m, s, {with(con(type, 1.0, 3), [](auto &k) { k.ref_dir[0] = k.ref_dir[1] = k.ref_dir[2] = 0.0; k.target[1] = NaN; })}, {}, nullptr, text);
        check_refused("reference vector not finite", m, s, {with(con(type, 1.0, 3), [](auto &k) { k.ref_dir[1] = Inf; })}, {}, nullptr, text);
        check_refused("reference vector NaN", m, nullptr, {with(con(type, 1.0, 0), [](auto &k) { k.ref_dir[2] = NaN; })}, {}, nullptr, text);
    }
    check_refused("zero target", m, s, {with(con(MG_CONSTRAINT_JOINT_ORIENTATION, 1.0, 3), [](auto &k) { k.target[0] = k.target[1] = k.target[2] = 0.0; })}, {}, nullptr,
                  "mg_constraint_set_create: constraint 0: zero target or reference vector");
    check_refused("target not finite", m, s, {with(con(MG_CONSTRAINT_JOINT_ORIENTATION, 1.0, 3), [](auto &k) { k.target[2] = NaN; })}, {}, nullptr,
                  "mg_constraint_set_create: constraint 0: zero target or reference vector");
    check_refused("look-at target not finite", m, s, {with(con(MG_CONSTRAINT_LOOK_AT, 1.0, 3), [](auto &k) { k.target[1] = Inf; })}, {}, nullptr,
                  "mg_constraint_set_create: constraint 0: look-at target not finite");
    check_image("look-at at the joint's own place", m, s, {with(con(MG_CONSTRAINT_LOOK_AT, 1.0, 3), [](auto &k) { k.target[0] = k.target[1] = k.target[2] = 0.0; })}, {}, nullptr);
    // poses
    const mg_keyframe_constraint pose1 = con(MG_CONSTRAINT_POSE, 1.0, 1);
    Pose good({0, 3}, false), p({1, 6, 2}, true);
    check_refused("pose index out of range", m, s, {pose1}, {good.desc}, nullptr, "mg_constraint_set_create: constraint 0 refers to pose 1 of 1");
    check_refused("pose index -1", m, s, {ok, con(MG_CONSTRAINT_POSE, 1.0, -1)}, {good.desc}, nullptr, "mg_constraint_set_create: constraint 1 refers to pose -1 of 1");
    check_refused("no poses", m, s, {con(MG_CONSTRAINT_POSE, 1.0, 0)}, {}, nullptr, "mg_constraint_set_create: constraint 0 refers to pose 0 of 0");
    const char *shape = "mg_constraint_set_create: pose 1: 1..64 points with joints, points and weights";
    p.desc.n_points = 0;
    check_refused("pose without points", m, s, {pose1}, {good.desc, p.desc}, nullptr, shape);
    p = Pose({1, 6, 2}, true); p.desc.weights = nullptr;
    check_refused("pose without weights, ahead of its joints", m, s, {pose1}, {good.desc, p.desc}, nullptr, shape);
    p = Pose({1, 6, 2}, true); p.points[1] = NaN; p.weights = {1.0, -1.0, 0.0};
    check_refused("point 0 not finite, ahead of point 1's joint", m, s, {pose1}, {good.desc, p.desc}, nullptr, "mg_constraint_set_create: pose 1: point 0 not finite");
    p = Pose({1, 6, 2}, true); p.points[3] = NaN; p.weights = {1.0, -1.0, 0.0};
    check_refused("pose joint out of range, ahead of its point and the weights", m, s, {pose1}, {good.desc, p.desc}, nullptr, "mg_constraint_set_create: pose 1: joint 6 out of range");
    p = Pose({1, 5, 2}, true); p.weights[2] = Inf;
    check_refused("weight not finite", m, s, {pose1}, {good.desc, p.desc}, nullptr, "mg_constraint_set_create: pose 1: point 2 not finite");
    p = Pose({1, 5, 2}, true); p.weights = {1.5, -2.0, 0.5};
    check_refused("weights summing to zero", m, s, {pose1}, {good.desc, p.desc}, nullptr, "mg_constraint_set_create: pose 1: weights sum to zero");
    const Pose far({0, MG_MAX_CHAIN + 1}, false);
    const Skel deeper = line(MG_MAX_CHAIN + 2);
    std::vector<double> zero(2, 0.0);
    mg_pose_constraint far_zero = far.desc;
    far_zero.weights = zero.data();
    check_refused("weights summing to zero, ahead of the chain's length", m, &deeper.desc, {con(MG_CONSTRAINT_POSE, 1.0, 0)}, {far_zero}, nullptr, "mg_constraint_set_create: pose 0: weights sum to zero");
}

int main() {
    const Model m;
    check_layout(m);
    check_limits(m);
    check_refusals(m);
    if (failures) std::printf("constraint_image_check: %d checks failed\n", failures);
    return failures ? 1 : 0;
}
