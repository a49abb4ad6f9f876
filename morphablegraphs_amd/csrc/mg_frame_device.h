// The per-frame constraints' statements and the joint tracks' statements that more than one translation unit runs, in the style of
// mg_traj_device.h: mg_frame_constraints.hip (one lane per candidate of a batch, a workgroup per four candidates' tracks) and
// mg_cluster_tree.hip (the same chain scorers and tracks inside the one-launch tree search, a lane per child of a chunk).  One
// statement of each, so the two sides cannot drift: a value has the same bits wherever it is formed.
// Also the argument blocks both sides fill (mg_fc_args, mg_track_args), the track plan, and the host routines that make them.
#pragma once
#include "mg_internal.h"
#include "mg_score_device.h"
#include "mg_spline_device.h"
#include "mg_traj_device.h"

// ---------------------------------------------------------------------------------------------------------------------
// the chain scorers (mg_score_frame_constraint[s], mg_options_frame_lists, mg_cluster_tree_search_frames)
// ---------------------------------------------------------------------------------------------------------------------
struct mg_fc_traj { const double *poly, *arc; double full; int32_t n_seg, G; int32_t poly_off, arc_off; };   // *_off: the table's place in LDS (doubles), TABLES_LDS kernels
// Where a trajectory's tables are read from: the copies the workgroup made in LDS (TABLES_LDS: every look-up of the walks below is a
// dependent read -- the closest-point search makes about 17 per frame, the arc-length search 10 -- so LDS latency instead of L2's is
// most of the kernel's time), or global memory when the list's tables do not fit.
template <bool TABLES_LDS> __device__ __forceinline__ const double *mg_fc_poly(const mg_fc_traj &t, const double *lds) {
    if constexpr (TABLES_LDS) return lds + t.poly_off; else return t.poly;
}
template <bool TABLES_LDS> __device__ __forceinline__ const double *mg_fc_arc(const mg_fc_traj &t, const double *lds) {
    if constexpr (TABLES_LDS) return lds + t.arc_off; else return t.arc;
}
struct mg_fc_args {
    const double *tracks;        // (B, T, J, 3), or (B, T, D) frames for MG_FRAME_JOINT_ROTATION
    double *out, *res;
    const double *points;
    int64_t B;
    int32_t T, J, type, nf, n_points, accumulate, quat_channel;
    int32_t search;              // MG_FRAME_JOINT_TRAJECTORY: 0 the reference's search, 1 the monotone walk (MG_OPT_TRAJECTORY_SEARCH)
    double weight, start_arc;
    double target[3];
    int32_t axis_on[3];
    double quat[4];
    mg_fc_traj traj[MG_FRAME_MAX_JOINTS];
    double arc0[MG_FRAME_MAX_JOINTS], range_start[MG_FRAME_MAX_JOINTS], range_end[MG_FRAME_MAX_JOINTS];
    int32_t has_range[MG_FRAME_MAX_JOINTS];
};

__device__ __forceinline__ void mg_fc_point(const mg_fc_traj &t, const double *poly, double u, double *p) {
    const double scaled = t.n_seg * u;
    int index = (int)floor(scaled);
    if (index >= t.n_seg) {
        const double *q = poly + (size_t)t.n_seg * 12;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
        return;
    }
    const double tt = scaled - index;
    const double *A = poly + (size_t)index * 12;
#pragma unroll
    for (int d = 0; d < 3; d++) p[d] = ((A[d] * tt + A[3 + d]) * tt + A[6 + d]) * tt + A[9 + d];
}

// ParameterizedSpline.query_point_by_absolute_arc_length on a list's trajectory: the one statement of it, mg_traj_point_by_arc
// (mg_traj_device.h), which the arc-length queries (mg_trajectory_arc.hip) run as well
__device__ __forceinline__ void mg_fc_point_by_arc(const mg_fc_traj &t, const double *poly, const double *arcs, double arc, double *p) {
    mg_traj_point_by_arc(poly, arcs, t.n_seg, t.G, t.full, arc, p);
}

__device__ __forceinline__ void mg_fc_rotmat(const double *q, double *m) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    m[0] = 1.0 - 2.0 * (y * y + z * z); m[1] = 2.0 * (x * y - z * w); m[2] = 2.0 * (x * z + y * w);
    m[3] = 2.0 * (x * y + z * w); m[4] = 1.0 - 2.0 * (x * x + z * z); m[5] = 2.0 * (y * z - x * w);
    m[6] = 2.0 * (x * z - y * w); m[7] = 2.0 * (y * z + x * w); m[8] = 1.0 - 2.0 * (x * x + y * y);
}

// one constraint for candidate b: its weighted error (and, if a.res is set, its residual vector)
template <bool TABLES_LDS>
__device__ __forceinline__ double mg_fc_evaluate(const mg_fc_args &a, const int64_t b, const double *lds) {
    const int T = a.T, J = a.J;
    const double *tr = a.tracks + b * (int64_t)T * J * 3;
    double err = 0.0;
    if (a.type == MG_FRAME_JOINT_TRAJECTORY) {
        // TrajectoryConstraint on the joint whose track this is (trajectory_constraint.py:79-121): per frame the distance to the closest
        // point of the spline at or after the previous frame's parameter; the error is the average (mg_score_trajectory_points'
        // arithmetic: mg_traj_device.h)
        const mg_fc_traj &t = a.traj[0];
        const double invG = 1.0 / (double)t.G;
        const double *poly = mg_fc_poly<TABLES_LDS>(t, lds);
        double min_u = a.start_arc, sum = 0.0;       // (start_arc carries the constraint's min_u)
        if (a.search == 0) {                         // the reference's search: this lane's frames at its own pace (mg_traj_chain)
            mg_traj_chain(poly, t.n_seg, T, min_u,
                          [&](int f, double *q) { const double *pp = tr + (int64_t)f * 3; q[0] = pp[0]; q[1] = pp[1]; q[2] = pp[2]; },
                          [&](int f, double dist, double, int) { sum += dist; if (a.res) a.res[b * T + f] = a.weight * dist; });
        } else {
            for (int f = 0; f < T; f++) {
                const double *pp = tr + (int64_t)f * 3;
                const double q[3] = {pp[0], pp[1], pp[2]};
                const double dist = mg_traj_closest_dist(poly, t.n_seg, t.G, invG, &min_u, q);
                sum += dist;
                if (a.res) a.res[b * T + f] = a.weight * dist;
            }
        }
        err = a.weight * (T > 0 ? sum / (double)T : 0.0);
    } else if (a.type == MG_FRAME_CA_POSITION) {
        // errors[i] = _point_distance(position, joint position in frame i); error = min (global_transform_ca_constraint.py:33-39)
        // (the minimum of the distances is the root of the minimum of their squares, exactly: sqrt is monotone and correctly rounded --
        // one root per candidate instead of one per frame, the same bits)
        double best2 = INFINITY;
        auto frame = [&](const double x, const double y, const double z) {
            const double p[3] = {x, y, z};
            double d2 = 0.0;
#pragma unroll
            for (int d = 0; d < 3; d++)
                if (a.axis_on[d]) { const double v = a.target[d] - p[d]; d2 += v * v; }
            best2 = d2 < best2 ? d2 : best2;
        };
        int f = 0;
        if ((((size_t)tr) & 15) == 0) {
            // two frames = six doubles = three 16-byte loads (a lane reads its own candidate's 3.7 KB: wider requests, half as many)
            const double2 *t2 = (const double2 *)tr;
#pragma unroll 2
            for (; f + 2 <= a.nf; f += 2) {
                const double2 u0 = t2[(f >> 1) * 3], u1 = t2[(f >> 1) * 3 + 1], u2 = t2[(f >> 1) * 3 + 2];
                frame(u0.x, u0.y, u1.x);
                frame(u1.y, u2.x, u2.y);
            }
        }
        for (; f < a.nf; f++) frame(tr[(int64_t)f * 3], tr[(int64_t)f * 3 + 1], tr[(int64_t)f * 3 + 2]);
        err = a.weight * sqrt(best2);
        if (a.res) a.res[b] = err;
    } else if (a.type == MG_FRAME_DISCRETE_TRAJECTORY) {
        // per frame the distance to the list's point of the same index, unconstrained axes zeroed, frames beyond the list 0;
        // error = the average over ALL frames (discrete_trajectory_constraint.py:66-90)
        double sum = 0.0;
        for (int f = 0; f < T; f++) {
            double r = 0.0;
            if (f < a.n_points) {
                double d2 = 0.0;
#pragma unroll
                for (int d = 0; d < 3; d++)
                    if (a.axis_on[d]) { const double v = tr[(int64_t)f * 3 + d] - a.points[(int64_t)f * 3 + d]; d2 += v * v; }
                r = sqrt(d2);
            }
            sum += r;
            if (a.res) a.res[b * T + f] = a.weight * r;
        }
        err = a.weight * (sum / T);
    } else if (a.type == MG_FRAME_LOCAL_TRAJECTORY) {
        // the arc length walked so far picks the target on the spline; squared xz distance, summed (local_trajectory_constraint.py:61-78)
        double arc = a.start_arc, sum = 0.0, last[3] = {0.0, 0.0, 0.0};
        const double *poly = mg_fc_poly<TABLES_LDS>(a.traj[0], lds), *arcs = mg_fc_arc<TABLES_LDS>(a.traj[0], lds);
        for (int f = 0; f < a.nf; f++) {
            const double *p = tr + (int64_t)f * 3;
            if (f > 0) arc += sqrt((last[0] - p[0]) * (last[0] - p[0]) + (last[1] - p[1]) * (last[1] - p[1]) + (last[2] - p[2]) * (last[2] - p[2]));
            double tg[3];
            mg_fc_point_by_arc(a.traj[0], poly, arcs, arc, tg);
            const double dx = tg[0] - p[0], dz = tg[2] - p[2];
            const double r = dx * dx + dz * dz;
            sum += r;
            if (a.res) a.res[b * a.nf + f] = a.weight * r;
            last[0] = p[0]; last[1] = p[1]; last[2] = p[2];
        }
        err = a.weight * sum;
    } else if (a.type == MG_FRAME_TRAJECTORY_SET) {
        // trajectory_set_constraint.py:82-104: per frame, if any trajectory is active at its joint's arc length, the distance between
        // the mean of ALL components of the joints' positions and the mean of all components of their targets (np.average over a list
        // of points is one number); a frame's step is added to the arc lengths AFTER the frame has been looked up, from the second on
        double arcs[MG_FRAME_MAX_JOINTS], last[MG_FRAME_MAX_JOINTS][3];
        for (int j = 0; j < J; j++) arcs[j] = a.arc0[j];
        double sum = 0.0;
        for (int f = 0; f < a.nf; f++) {
            const double *p = tr + (int64_t)f * J * 3;
            bool active = false;
            for (int j = 0; j < J; j++) active = active || (a.has_range[j] && a.range_start[j] <= arcs[j] && arcs[j] <= a.range_end[j]);
            double r = 0.0;
            if (active) {
                double actual = 0.0, target = 0.0;
                for (int j = 0; j < J; j++) {
                    double tg[3];
                    mg_fc_point_by_arc(a.traj[j], mg_fc_poly<TABLES_LDS>(a.traj[j], lds), mg_fc_arc<TABLES_LDS>(a.traj[j], lds), arcs[j], tg);
                    actual += p[j * 3] + p[j * 3 + 1] + p[j * 3 + 2];
                    target += tg[0] + tg[1] + tg[2];
                }
                r = fabs(actual / (3.0 * J) - target / (3.0 * J));
            }
            if (f > 0)
                for (int j = 0; j < J; j++) {
                    const double dx = p[j * 3] - last[j][0], dy = p[j * 3 + 1] - last[j][1], dz = p[j * 3 + 2] - last[j][2];
                    arcs[j] += sqrt(dx * dx + dy * dy + dz * dz);
                }
            for (int j = 0; j < J; j++) { last[j][0] = p[j * 3]; last[j][1] = p[j * 3 + 1]; last[j][2] = p[j * 3 + 2]; }
            sum += r;
            if (a.res) a.res[b * a.nf + f] = a.weight * r;
        }
        err = a.weight * (sum / a.nf);
    } else {   // MG_FRAME_JOINT_ROTATION: tracks = frames (B, T, J = n_dim), the first one read
        // the Frobenius norm of the difference of the wanted and the joint's LOCAL rotation matrix (joint_rotation_constraint.py:55-72)
        const double *q = a.tracks + b * (int64_t)T * J + a.quat_channel;
        const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double qn[4] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n};
        double m0[9], m1[9], s2 = 0.0;
        mg_fc_rotmat(a.quat, m0);
        mg_fc_rotmat(qn, m1);
#pragma unroll
        for (int e = 0; e < 9; e++) s2 += (m0[e] - m1[e]) * (m0[e] - m1[e]);
        err = a.weight * sqrt(s2);
        if (a.res) a.res[b] = err;
    }
    return err;
}

// the workgroup's copies of a constraint's tables (a table two trajectories share is written twice with the same values), made by
// its `threads` threads of which this one is `tid`
__device__ __forceinline__ void mg_fc_stage_tables(const mg_fc_args &a, double *lds, int tid, int threads) {
    for (int j = 0; j < MG_FRAME_MAX_JOINTS; j++) {
        const mg_fc_traj &t = a.traj[j];
        if (!t.poly) continue;
        if (t.poly_off >= 0) for (int e = tid; e < t.n_seg * 12 + 3; e += threads) lds[t.poly_off + e] = t.poly[e];
        if (t.arc_off >= 0) for (int e = tid; e <= t.G; e += threads) lds[t.arc_off + e] = t.arc[e];
    }
}

// The host routines of mg_frame_constraints.hip that the tree search calls as well:
// desc -> kernel arguments (validated); the output pointers are the caller's business
int mg_fc_args_from_desc(const char *who, mg_primitive *p, const mg_frame_constraint_desc *c, const double *tracks_dev, int64_t B, int32_t T, int32_t J,
                         double *residuals_dev, mg_fc_args *out);
// mg_fc_place_tables' places in LDS (doubles from the tables' base) for a list's tables, and the bytes they take; 0 with every
// offset -1 when there is nothing to stage or the scorers' own bound (MG_FC_LDS_MAX) refuses them.  *has_tables: the list holds a table.
size_t mg_fc_place_list_tables(mg_fc_args *c, int n, bool *has_tables);
// ... and taken back: every table is read from memory
void mg_fc_unplace_tables(mg_fc_args *c, int n);

// ---------------------------------------------------------------------------------------------------------------------
// the joint tracks (mg_joint_tracks, mg_options_frame_lists, mg_cluster_tree_search_frames)
// ---------------------------------------------------------------------------------------------------------------------
#define MG_TRACK_REC (1 + 4 * MG_MAX_CHAIN)       // chain length m, then per link (quaternion channel or -1, offset xyz): mg_joint_positions' record
struct mg_track_plan {
    mg_primitive *prim = nullptr;
    int32_t n_requests = 0, n_chan = 0, align_m = -1;        // align_m: links of the aligning node's chain (-1: plans without alignment support)
    int32_t align_joint = -1;                                // the node that chain belongs to
    int32_t req_joint0[MG_TRACK_MAX_REQUESTS + 1] = {0};     // request q owns records req_joint0[q] .. req_joint0[q + 1]
    double *d_records = nullptr;    // [n_joints_total][MG_TRACK_REC]
    double *d_align_rec = nullptr;  // [MG_TRACK_REC]: the aligning node's chain (quaternion channels only are read)
    int32_t *d_chan = nullptr;      // [n_chan] pose channels kept in LDS
    int32_t *d_slot = nullptr;      // [D] channel -> slot or -1
};

struct mg_track_args {
    const double *Et64, *mean;
    const void *lat;
    int64_t B, ld;
    int32_t L, R, D, NB, lat_f64, n_requests, n_chan, align_mode;   // align_mode 0 none, 1 previous frame, 2 start pose
    const double *records, *align_rec;
    const int32_t *chan, *slot;
    int32_t req_joint0[MG_TRACK_MAX_REQUESTS + 1], T[MG_TRACK_MAX_REQUESTS];
    const int32_t *i0[MG_TRACK_MAX_REQUESTS];
    const double *w[MG_TRACK_MAX_REQUESTS];
    double *out[MG_TRACK_MAX_REQUESTS];
    double h0, h1, px, py, pz, ref[3];
    int32_t align_m;
};
// the arguments of one option's / search's tracks (validated); lds_out: mg_joint_tracks_kernel's dynamic LDS
int mg_track_fill_args(const char *who, mg_track_plan *pl, const void *lat, int dt, int64_t B, int64_t ld, const mg_alignment_desc *al,
                       const mg_time_grid *const *grids, double *const *tracks_dev, mg_track_args *out, size_t *lds_out);

// The control-point staging of a workgroup of BLOCK threads that owns CANDS candidates (mg_joint_tracks_body, mg_point_clouds_kernel):
// from their latents s_all [CANDS][L] in LDS (staged by the caller, a barrier behind them) the control points of the kept channels
// chan[0 .. nc) into cp_all [CANDS][NB][nc]; the caller's barrier follows.
// (mg_control_point's statement for CANDS candidates side by side: one read of an eigenvector element feeds all of them, which the
// helper's one-chain form cannot express)
template <int CANDS, int BLOCK>
__device__ __forceinline__ void mg_track_control_points(const double *Et64, const double *mean, int L, int R, int D, int NB, int nc, const int32_t *chan,
                                                        const double *s_all, double *cp_all) {
    const int tid = threadIdx.x, ncp = NB * nc;
    for (int e = tid; e < ncp; e += BLOCK) {
        const int i = e / nc, q = e - i * nc;
        const int r = i * D + chan[q];
        double acc[CANDS];
#pragma unroll
        for (int c = 0; c < CANDS; c++) acc[c] = mean[r];
        for (int k = 0; k < L; k++) {
            const double ev = Et64[(size_t)k * R + r];
#pragma unroll
            for (int c = 0; c < CANDS; c++) acc[c] = fma(ev, s_all[c * L + k], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < CANDS; c++) cp_all[(size_t)c * ncp + e] = acc[c];
    }
}

// A candidate's aligning transform from its FIRST control point (a clamped spline's value at t = 0), into al[8]: c, s, tx, tz, ty, then
// the half angle (aw, ay) its root quaternion turns by.  cp: its control points of the kept channels [NB][n_chan]; slot: channel -> slot.
template <typename SlotFn>
__device__ __forceinline__ void mg_track_alignment(const mg_track_args &a, const double *cp, SlotFn slot, double *al) {
    auto ch0 = [&](int ch) { return cp[slot(ch)]; };
    const double p0x = ch0(0), p0z = ch0(2);
    mg_align2d t;
    if (a.align_mode == 2) {
        t = mg_align2d_onto(a.h0, a.h1, a.px, a.pz, p0x, p0z, a.py);
    } else {
        // the aligning node's heading at t = 0 (what a MG_CONSTRAINT_VALUE_HEADING constraint of weight 1 probes: the weight's
        // multiplication is exact)
        double q[4] = {1.0, 0.0, 0.0, 0.0}, bx, bz;
        const double *rec = a.align_rec;
        for (int i = 0; i < a.align_m; i++) {
            const int qc = (int)rec[1 + 4 * i];
            mg_quat_accumulate(q, ch0(qc), ch0(qc + 1), ch0(qc + 2), ch0(qc + 3));
        }
        mg_heading_xz(q, a.ref[0], a.ref[1], a.ref[2], bx, bz);
        t = mg_align2d_from(a.h0, a.h1, bx, bz, a.px, a.pz, p0x, p0z);
    }
    al[0] = t.c; al[1] = t.s; al[2] = t.tx; al[3] = t.tz; al[4] = t.ty;
    mg_align_half_angle(t.c, t.s, al[5], al[6]);
}

// Joint record `rec`'s global position in the frame whose basis rows are (i0, wf): the frame's channels by four taps of the
// candidate's control points cp [NB][nc], the root turned and moved by al (aligned), then the chain (mg_joint_positions_kernel's
// loop, the root's quaternion turned with the candidate first).
template <typename SlotFn>
__device__ __forceinline__ void mg_track_point(const double *cp, int nc, SlotFn slot, int i0, const double *wf, const double *rec, bool aligned, const double *al,
                                               int D, double (&p)[3]) {
    const double *cf = cp + (size_t)i0 * nc;
    auto chan = [&](int ch) {       // the frame's channel: four taps of its control points
        const double *cq = cf + slot(ch);
        return mg_taps4(wf, cq, nc);
    };
    p[0] = chan(0); p[1] = chan(1); p[2] = chan(2);
    if (aligned) {
        const mg_align2d t = {al[0], al[1], al[2], al[3], al[4]};
        mg_align_position(t, p[0], p[1], p[2]);
    }
    const int m = (int)rec[0];
    double q[4] = {1.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < m; k++) {
        const int ch = (int)rec[1 + 4 * k];
        if (ch >= 0) {
            double qw = chan(ch), qx = chan(ch + 1), qy = chan(ch + 2), qz = chan(ch + 3);
            if (aligned && ch == 3 && D >= 7) mg_align_root_quat(al[5], al[6], qw, qx, qy, qz);
            mg_quat_accumulate(q, qw, qx, qy, qz);
        }
        mg_fk_link(q, rec[2 + 4 * k], rec[3 + 4 * k], rec[4 + 4 * k], p);
    }
}
