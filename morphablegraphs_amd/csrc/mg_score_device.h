// Device-side pieces of the fused constraint scorer (gfx950): the weighted residual of one constraint for one candidate
// (its argument block, mg_score_args, is in mg_internal.h), shared by the stand-alone scoring kernels (mg_score.hip) and the one-launch planner
// step (mg_options.hip) so that both produce the same bits.
// And the float64 pose statements, stated once: every kernel that walks a chain, forms a heading or aligns a pose calls these, so
// that a fused kernel gives the bits of the chain of calls it replaces.  What this header guarantees:
//   mg_quat_normalise, mg_quat_accumulate   a chain quaternion made unit, and multiplied into the accumulated orientation
//   mg_rotate, mg_fk_link                   a vector turned by a unit quaternion; one link of forward kinematics
//   mg_heading_xz                           an orientation applied to ref_dir, the xz part, made unit
//   mg_align2d_onto, mg_align2d_from        the 2-D aligning transform (c, s, tx, tz, ty)
//   mg_align_half_angle                     (cos(phi / 2), sin(phi / 2)) of its rotation
//   mg_align_position, mg_align_direction, mg_align_root_quat   the transform applied to a position, a direction, the root's quaternion
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mg_internal.h"

// q / |q|, like transformations.quaternion_matrix normalises
__device__ __forceinline__ void mg_quat_normalise(double &qw, double &qx, double &qy, double &qz) {
    const double inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= inv; qx *= inv; qy *= inv; qz *= inv;
}
// a <- a x (q / |q|): one more quaternion of a chain multiplied into the accumulated orientation (Hamilton product)
__device__ __forceinline__ void mg_quat_accumulate(double (&a)[4], double qw, double qx, double qy, double qz) {
    mg_quat_normalise(qw, qx, qy, qz);
    const double nw = a[0] * qw - a[1] * qx - a[2] * qy - a[3] * qz, nx = a[0] * qx + a[1] * qw + a[2] * qz - a[3] * qy;
    const double ny = a[0] * qy - a[1] * qz + a[2] * qw + a[3] * qx, nz = a[0] * qz + a[1] * qy - a[2] * qx + a[3] * qw;
    a[0] = nw; a[1] = nx; a[2] = ny; a[3] = nz;
}
// Product of the chain's m quaternions (rows r_q ..), each normalised.  Here and below `channel(row)` yields the candidate's pose
// channel of that row of the fused keyframe matrices (rows of constraint c start at woff[c]): a dot product per channel in the VALU
// kernel, a read from LDS in the MFMA kernel, so both produce the same value.
template <typename ChannelFn>
__device__ __forceinline__ void mg_chain_orientation(ChannelFn channel, int r_q, int m, double (&q)[4]) {
    q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
    for (int i = 0; i < m; i++) mg_quat_accumulate(q, channel(r_q + 4 * i), channel(r_q + 1 + 4 * i), channel(r_q + 2 + 4 * i), channel(r_q + 3 + 4 * i));
}
// v' = v + 2 w (u x v) + 2 u x (u x v) for a unit quaternion (w, u)
__device__ __forceinline__ void mg_rotate(const double (&q)[4], double vx, double vy, double vz, double (&out)[3]) {
    const double cx = q[2] * vz - q[3] * vy, cy = q[3] * vx - q[1] * vz, cz = q[1] * vy - q[2] * vx;
    const double dx = q[2] * cz - q[3] * cy, dy = q[3] * cx - q[1] * cz, dz = q[1] * cy - q[2] * cx;
    out[0] = vx + 2.0 * (q[0] * cx + dx);
    out[1] = vy + 2.0 * (q[0] * cy + dy);
    out[2] = vz + 2.0 * (q[0] * cz + dz);
}
// One link of forward kinematics: p += R(a) offset, a the accumulated orientation of the link's joint
__device__ __forceinline__ void mg_fk_link(const double (&a)[4], double ox, double oy, double oz, double (&p)[3]) {
    double v[3];
    mg_rotate(a, ox, oy, oz, v);
    p[0] += v[0]; p[1] += v[1]; p[2] += v[2];
}
// Forward kinematics: p = root translation (rows r_p ..) + sum_i R(q_0 .. q_i) offset_i over the chain's m links
// (quaternion rows r_q .., offsets off[m][3]).
template <typename ChannelFn>
__device__ __forceinline__ void mg_fk_position(ChannelFn channel, int r_p, int r_q, int m, const double *off, double (&p)[3]) {
    p[0] = channel(r_p); p[1] = channel(r_p + 1); p[2] = channel(r_p + 2);
    double a[4] = {1.0, 0.0, 0.0, 0.0};   // accumulated global rotation of the parent
    for (int i = 0; i < m; i++) {
        mg_quat_accumulate(a, channel(r_q + 4 * i), channel(r_q + 1 + 4 * i), channel(r_q + 2 + 4 * i), channel(r_q + 3 + 4 * i));
        mg_fk_link(a, off[3 * i], off[3 * i + 1], off[3 * i + 2], p);
    }
}

// Forward kinematics through a pose table record: link k rotates by the quaternion at row r0 + rec[5 + 4k] (identity if
// negative) and moves by the offset rec[6 + 4k ..]; rows of the pose block start at r0 (root xyz first).
template <typename ChannelFn>
__device__ __forceinline__ void mg_fk_position_table(ChannelFn channel, int r0, const double *rec, double (&p)[3]) {
    p[0] = channel(r0); p[1] = channel(r0 + 1); p[2] = channel(r0 + 2);
    double a[4] = {1.0, 0.0, 0.0, 0.0};
    const int m = (int)rec[4];
    for (int k = 0; k < m; k++) {
        const int qr = (int)rec[5 + 4 * k];
        if (qr >= 0) mg_quat_accumulate(a, channel(r0 + qr), channel(r0 + qr + 1), channel(r0 + qr + 2), channel(r0 + qr + 3));
        mg_fk_link(a, rec[6 + 4 * k], rec[7 + 4 * k], rec[8 + 4 * k], p);
    }
}

// Heading of a node: its global orientation q applied to ref_dir r, the xz part, made unit
__device__ __forceinline__ void mg_heading_xz(const double (&q)[4], double rx, double ry, double rz, double &bx, double &bz) {
    double v[3];
    mg_rotate(q, rx, ry, rz, v);
    const double inv = 1.0 / sqrt(v[0] * v[0] + v[2] * v[2]);
    bx = v[0] * inv; bz = v[2] * inv;
}

// A candidate's 2-D aligning transform: rotation about y by (cos, sin) = (c, s), then a translation in xz; ty: the start-pose mode
// raises every position by the start height
struct mg_align2d { double c, s, tx, tz, ty; };
// ... the one with the given rotation that puts the candidate's first root position (p0x, p0z) on (px, pz)
__device__ __forceinline__ mg_align2d mg_align2d_onto(double c, double s, double px, double pz, double p0x, double p0z, double ty) {
    mg_align2d t;
    t.c = c; t.s = s;
    t.tx = px - (c * p0x + s * p0z);
    t.tz = pz - (c * p0z - s * p0x);
    t.ty = ty;
    return t;
}
// ... onto a previous motion: the rotation is the angle between the previous heading h and the candidate's own heading b in its
// first control point, (cos, sin) = (h . b, h x b)
__device__ __forceinline__ mg_align2d mg_align2d_from(double hx, double hz, double bx, double bz, double px, double pz, double p0x, double p0z) {
    return mg_align2d_onto(hx * bx + hz * bz, hx * bz - hz * bx, px, pz, p0x, p0z, 0.0);
}
// (cos(phi / 2), sin(phi / 2)) of the transform's rotation: the quaternion (qaw, 0, qay, 0) the root's orientation turns by
__device__ __forceinline__ void mg_align_half_angle(double c, double s, double &qaw, double &qay) {
    const double phi = atan2(s, c);
    qaw = cos(0.5 * phi); qay = sin(0.5 * phi);
}
__device__ __forceinline__ void mg_align_position(const mg_align2d &t, double &x, double &y, double &z) {
    const double x0 = x, z0 = z;
    x = t.c * x0 + t.s * z0 + t.tx;
    y += t.ty;
    z = t.c * z0 - t.s * x0 + t.tz;
}
__device__ __forceinline__ void mg_align_direction(const mg_align2d &t, double &x, double &z) {
    const double x0 = x, z0 = z;
    x = t.c * x0 + t.s * z0;
    z = t.c * z0 - t.s * x0;
}
// (qaw, 0, qay, 0) x q
__device__ __forceinline__ void mg_align_root_quat(double qaw, double qay, double &qw, double &qx, double &qy, double &qz) {
    const double w0 = qw, x0 = qx, y0 = qy, z0 = qz;
    qw = qaw * w0 - qay * y0;
    qx = qaw * x0 + qay * z0;
    qy = qaw * y0 + qay * w0;
    qz = qaw * z0 - qay * x0;
}

// The candidate's transform in the fused scorer (mg_alignment_desc), from its own first control point (rows woff[n] ..)
template <typename ChannelFn>
__device__ __forceinline__ mg_align2d mg_candidate_alignment(const mg_score_args &a, ChannelFn channel, int64_t cand) {
    const double *al = a.align;
    const int r0 = a.woff[a.n], m = (int)al[0];
    // start-pose mode (reference objective_functions.py:38-47): the SAME rotation about y for every candidate,
    // (cos, sin) = al[1..2], the candidate's first root position moved to (al[3], ., al[4]), heights raised by al[5]
    if (m == 0) return mg_align2d_onto(al[1], al[2], al[3], al[4], channel(r0), channel(r0 + 2), al[5]);
    double q[4], bx, bz;   // global orientation of the aligning node, its heading
    mg_chain_orientation(channel, r0 + 3, m, q);
    mg_heading_xz(q, al[5], al[6], al[7], bx, bz);
    const double *pc = a.align_cand ? a.align_cand + cand * 4 - 1 : al;   // [1..4]: previous heading (x, z), previous root (x, z)
    return mg_align2d_from(pc[1], pc[2], bx, bz, pc[3], pc[4], channel(r0), channel(r0 + 2));
}

// The candidate's transform in the trajectory scorers, the root as aligning node: rotation about y and an xz translation, from the
// first control point's rows -- root(r) yields row r of the candidate's root coefficient rows (NB x 3 positions, then the first control
// point's quaternion).  mode 0: none, 1: previous frame, 2: start pose; al: the record as mg_traj_align_record normalises it.  The
// root's chain is its one quaternion: normalised and used as it is (multiplying it into the identity, the general chain's first step,
// can flip the sign of a zero component).  prev: NULL, or the candidate's OWN previous unit heading (x, z) and root position (x, z) in
// place of al[0..3] (mode 1 only; the reference vector stays the record's).
template <typename RootFn>
__device__ __forceinline__ mg_align2d mg_traj_alignment_of(int mode, const double *al, int NB, const double *prev, RootFn root) {
    if (mode == 0) return {1.0, 0.0, 0.0, 0.0, 0.0};
    const double p0x = root(0), p0z = root(2);   // (formed once: root() may be a whole fma chain)
    if (mode == 2) return mg_align2d_onto(al[0], al[1], al[2], al[3], p0x, p0z, al[4]);
    double q[4] = {root(NB * 3 + 0), root(NB * 3 + 1), root(NB * 3 + 2), root(NB * 3 + 3)}, bx, bz;
    mg_quat_normalise(q[0], q[1], q[2], q[3]);
    mg_heading_xz(q, al[4], al[5], al[6], bx, bz);
    double hx = al[0], hz = al[1], px = al[2], pz = al[3];
    if (prev) { hx = prev[0]; hz = prev[1]; px = prev[2]; pz = prev[3]; }
    return mg_align2d_from(hx, hz, bx, bz, px, pz, p0x, p0z);
}

// ROOT_ONLY: the set holds root position / 2-D direction constraints only (the caller has checked): the other kinds' code -- and
// the registers their forward-kinematics chains want -- stay out of a kernel that has none to spare (the optimiser's objective
// inside the LDS-resident mixture kernel, four waves per SIMD).  The two kinds compiled in are the same statements: the same bits.
template <bool ROOT_ONLY = false, typename ChannelFn>
__device__ __forceinline__ double mg_constraint_residual(const mg_score_args &a, int c, ChannelFn channel, int64_t cand = 0) {
    const double *par = a.par + (size_t)c * 8;
    const int type = (int)par[0];
    const int r0 = a.woff[c];
    mg_align2d al = {1.0, 0.0, 0.0, 0.0, 0.0};
    if (a.align) al = mg_candidate_alignment(a, channel, cand);
    if constexpr (!ROOT_ONLY) {
    if (type == MG_CONSTRAINT_VALUE_POSITION) {   // not an error: the (aligned) root position's component par[2] at the keyframe
        double pj[3] = {channel(r0), channel(r0 + 1), channel(r0 + 2)};
        if (a.align) mg_align_position(al, pj[0], pj[1], pj[2]);
        return par[1] * pj[(int)par[2]];
    }
    if (type == MG_CONSTRAINT_VALUE_HEADING) {   // the (aligned) unit heading's x (par[2] = 0) or z component: xz of the joint's global orientation applied to ref_dir
        double q[4], v[3];
        mg_chain_orientation(channel, r0, a.chain[c], q);
        mg_rotate(q, par[5], par[6], par[7], v);
        double hx = v[0], hz = v[2];
        if (a.align) mg_align_direction(al, hx, hz);
        const double inv = 1.0 / sqrt(hx * hx + hz * hz);
        return par[1] * ((int)par[2] == 0 ? hx : hz) * inv;
    }
    if (type == MG_CONSTRAINT_JOINT_POSITION || type == MG_CONSTRAINT_JOINT_MIDPOINT) {
        // forward kinematics along the chain: p = t_root + sum_i R(q_0 .. q_(i-1)) offset_i, unit quaternions (w,x,y,z)
        const int m = a.chain[c] & 0xffff;
        double pj[3];
        mg_fk_position(channel, r0, r0 + 3, m, a.choff + (size_t)c * 2 * MG_MAX_CHAIN * 3, pj);
        if (type == MG_CONSTRAINT_JOINT_MIDPOINT) {   // two_hand_constraint.py:71: centre of the two joints
            double pk[3];
            mg_fk_position(channel, r0, r0 + 3 + 4 * (m > 1 ? m : 1), a.chain[c] >> 16, a.choff + ((size_t)c * 2 + 1) * MG_MAX_CHAIN * 3, pk);
#pragma unroll
            for (int i = 0; i < 3; i++) pj[i] = pj[i] + 0.5 * (pk[i] - pj[i]);
        }
        if (a.align) mg_align_position(al, pj[0], pj[1], pj[2]);
        double ds = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double t = par[2 + i];
            if (t == t) ds += (t - pj[i]) * (t - pj[i]);
        }
        return par[1] * sqrt(ds);
    }
    if (type == MG_CONSTRAINT_POSE) {
        // pose_constraint.py:48-67: cloud of joint positions, optimal weighted 2-D fit onto the wanted cloud (Kovar et
        // al.), mean distance after the fit, + the velocity term of the first joint
        const double *tb = a.pose + (size_t)par[2];
        const int N = (int)tb[0], block = (int)tb[5];
        double sw = 0.0, sax = 0.0, saz = 0.0, sbx = 0.0, sbz = 0.0, num = 0.0, den = 0.0;
        for (int i = 0; i < N; i++) {
            const double *rec = tb + MG_POSE_HDR + (size_t)i * MG_POSE_REC;
            double b[3];
            mg_fk_position_table(channel, r0, rec, b);
            if (a.align) mg_align_position(al, b[0], b[1], b[2]);
            const double w = rec[3];
            num += w * (rec[0] * b[2] - b[0] * rec[2]);
            den += w * (rec[0] * b[0] + rec[2] * b[2]);
            sw += w; sax += w * rec[0]; saz += w * rec[2]; sbx += w * b[0]; sbz += w * b[2];
        }
        num -= (sax * sbz - sbx * saz) / sw;
        den -= (sax * sbx + saz * sbz) / sw;
        const double theta = atan2(num, den), ct = cos(theta), st = sin(theta);
        const double x0 = (sax - sbx * ct - sbz * st) / sw, z0 = (saz + sbx * st - sbz * ct) / sw;
        double dist = 0.0, first[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < N; i++) {
            const double *rec = tb + MG_POSE_HDR + (size_t)i * MG_POSE_REC;
            double b[3];
            mg_fk_position_table(channel, r0, rec, b);
            if (a.align) mg_align_position(al, b[0], b[1], b[2]);
            if (i == 0) { first[0] = b[0]; first[1] = b[1]; first[2] = b[2]; }
            const double bx = b[0] * ct + b[2] * st + x0, bz = b[2] * ct - b[0] * st + z0;
            const double ex = rec[0] - bx, ey = rec[1] - b[1], ez = rec[2] - bz;
            dist += sqrt(ex * ex + ey * ey + ez * ez);
        }
        double err = dist / (double)N;
        if (tb[1] != 0.0) {
            double nx[3];
            mg_fk_position_table(channel, r0 + block, tb + MG_POSE_HDR, nx);   // the first joint one frame later
            if (a.align) mg_align_position(al, nx[0], nx[1], nx[2]);
            const double vx = tb[2] - (nx[0] - first[0]), vy = tb[3] - (nx[1] - first[1]), vz = tb[4] - (nx[2] - first[2]);
            err += sqrt(vx * vx + vy * vy + vz * vz);
        }
        return par[1] * err;
    }
    if (type == MG_CONSTRAINT_LOOK_AT) {
        // look_at_constraint.py:55-66: angle between where the joint looks and where the target is
        const int m = a.chain[c];
        double pj[3], q[4], v[3];
        mg_fk_position(channel, r0, r0 + 3, m - 1, a.choff + (size_t)c * 2 * MG_MAX_CHAIN * 3, pj);
        mg_chain_orientation(channel, r0 + 3, m, q);
        mg_rotate(q, par[5], par[6], par[7], v);
        if (a.align) {
            mg_align_position(al, pj[0], pj[1], pj[2]);
            mg_align_direction(al, v[0], v[2]);
        }
        const double tx = par[2] - pj[0], ty = par[3] - pj[1], tz = par[4] - pj[2];
        const double dot = (v[0] * tx + v[1] * ty + v[2] * tz) / (sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) * sqrt(tx * tx + ty * ty + tz * tz));
        return par[1] * acos(fmin(1.0, fmax(dot, -1.0)));
    }
    if (type == MG_CONSTRAINT_JOINT_ORIENTATION) {
        // global_transform_constraint.py:109-121: angle between the joint's global orientation applied to ref_dir and the target vector
        double q[4];
        mg_chain_orientation(channel, r0, a.chain[c], q);
        double v[3];
        mg_rotate(q, par[5], par[6], par[7], v);
        if (a.align) mg_align_direction(al, v[0], v[2]);
        const double dot = (v[0] * par[2] + v[1] * par[3] + v[2] * par[4]) /
                           (sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) * sqrt(par[2] * par[2] + par[3] * par[3] + par[4] * par[4]));
        return par[1] * acos(fmin(1.0, fmax(dot, -1.0)));
    }
    }   // !ROOT_ONLY
    if (type == MG_CONSTRAINT_POSITION) {
        // _point_distance: axes whose target is NaN (the reference's None) are ignored
        double ds = 0.0;
        if (a.align) {
            double pj[3] = {channel(r0), channel(r0 + 1), channel(r0 + 2)};
            mg_align_position(al, pj[0], pj[1], pj[2]);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                double t = par[2 + i];
                if (t == t) ds += (t - pj[i]) * (t - pj[i]);
            }
            return par[1] * sqrt(ds);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double t = par[2 + i];
            if (t == t) {
                const double v = channel(r0 + i);
                ds += (t - v) * (t - v);
            }
        }
        return par[1] * sqrt(ds);
    }
    // heading = xz of (rotation of the root quaternion (w,x,y,z)) applied to ref_dir
    const double qw = channel(r0 + 3), qx = channel(r0 + 4), qy = channel(r0 + 5), qz = channel(r0 + 6);
    const double nq = qw * qw + qx * qx + qy * qy + qz * qz, s2 = 2.0 / nq;
    const double rx = par[5], ry = par[6], rz = par[7];
    const double lx = (1.0 - s2 * (qy * qy + qz * qz)) * rx + s2 * (qx * qy - qz * qw) * ry + s2 * (qx * qz + qy * qw) * rz;
    const double lz = s2 * (qx * qz - qy * qw) * rx + s2 * (qy * qz + qx * qw) * ry + (1.0 - s2 * (qx * qx + qy * qy)) * rz;
    double px = lx, pz = lz;
    if (a.align) mg_align_direction(al, px, pz);
    // par[2..4]: the unit target (tx, tz) = target / |target| and sqrt(tx^2 + tz^2), made on the host by these very statements
    // (mg_constraint_par_row): tn = sqrt(t0^2 + t1^2), tx = t0 / tn, tz = t1 / tn
    const double tx = par[2], tz = par[3];
    const double mn = sqrt(px * px + pz * pz);
    const double mx = px / mn, mz = pz / mn;
    double cosang = (tx * mx + tz * mz) / (par[4] * sqrt(mx * mx + mz * mz));
    cosang = fmin(1.0, fmax(cosang, -1.0));
    return par[1] * fabs(acos(cosang) * (180.0 / M_PI));
}

// (value, index) pairs of the first-minimum rule: the smaller value wins, ties go to the smaller index -- a total order, so
// partial results can be combined in any order
__device__ __forceinline__ void mg_min_combine(double &v, int64_t &i, double ov, int64_t oi) {
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}

