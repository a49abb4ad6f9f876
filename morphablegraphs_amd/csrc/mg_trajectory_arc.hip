// Arc-length queries on a trajectory (gfx950): what a planner asks of the reference's ParameterizedSpline between the scoring launches
// (constraints/spatial_constraints/splines/parameterized_spline.py), for a batch:
//   mg_trajectory_points_by_arc_length   :131-155 query_point_by_absolute_arc_length, :186-207 get_tangent_at_arc_length, the angle of
//                                        :217-240 get_angle_at_arc_length_2d -- one lane per query
//   mg_trajectory_arc_length_of_points   :242-273 get_absolute_arc_length_of_point -- one wave per point
//   mg_trajectory_points_at_parameters   the curve's points at given parameters -- one lane each
// on the tables every trajectory carries whatever its spline type (mg_trajectory.hip): the cubic pieces, the relative arc lengths at
// k / granularity, and the parameters the reference's scan visits (u += 1.0 / granularity while u <= 1.0, built on the host: the
// kernels never form a parameter).  Each statement below has a twin in morphablegraphs_amd/spline_types.py, in the same order of
// operations; the library is compiled without contraction, so device and host agree bit for bit (tests/test_gpu_trajectory_arc.py).
// Nothing here has been timed: the scan is 1001 cubic evaluations and table look-ups per point, spread over the 64 lanes of a wave.
#include <climits>
#include <cmath>
#include <cstring>

#include "mg_construct.h"
#include "mg_traj_device.h"

struct mg_arc_tables { const double *poly, *arc, *uk; double full; int32_t n_seg, G, n_uk; };

// RelativeArcLengthMap.get_absolute_arc_length (arc_length_map.py:73-90), statement for statement: step_size = 1.0 / granularity,
// table_index = int(t / step_size) -- a quotient that rounds, truncated --; below the table's last entry the linear interpolation
// between the entries' parameters index / granularity (the table's first column), times the full length; at the last entry its
// value times the full length.  The index is clamped to the table (the reference would raise past it; t never leaves [0, 1] here).
MG_HD __forceinline__ double mg_arc_absolute(const double *arcs, int G, double full, double t) {
    const double step_size = 1.0 / (double)G;
    int table_index = (int)(t / step_size);
    table_index = table_index < 0 ? 0 : (table_index > G ? G : table_index);
    if (table_index < G) {
        const double t_i = table_index / (double)G, t_i_1 = (table_index + 1) / (double)G;
        const double a_i = arcs[table_index], a_i_1 = arcs[table_index + 1];
        const double arc_length = a_i + ((t - t_i) / (t_i_1 - t_i)) * (a_i_1 - a_i);
        return arc_length * full;
    }
    return arcs[table_index] * full;
}

// the distance of the scan and the norm of the tangent: products and sums each rounded, in x, y, z order
MG_HD __forceinline__ double mg_arc_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// acos as fdlibm states it (e_acos.c, Sun Microsystems 1993: a rational approximation R(z) of (asin(x) - x) / x^3 on |x| < 0.5, the
// half-angle identities with a split square root above), in plain IEEE operations and a correctly rounded sqrt: below one ulp, and --
// unlike a library call -- the same bits from any compiler that does not contract.  |x| > 1 and NaN give NaN.
MG_HD __forceinline__ double mg_arc_acos(double x) {
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
    const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const double ax = fabs(x);
    if (!(ax < 1.0)) {
        if (x == 1.0) return 0.0;
        if (x == -1.0) return pi + 2.0 * pio2_lo;
        return nan("");
    }
    const double z = ax < 0.5 ? x * x : (x < 0.0 ? (1.0 + x) * 0.5 : (1.0 - x) * 0.5);
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    if (ax < 0.5) return pio2_hi - (x - (pio2_lo - r * x));
    const double s = sqrt(z);
    if (x < 0.0) {
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    unsigned long long bits;
    memcpy(&bits, &s, 8);
    bits &= 0xffffffff00000000ull;           // df: s with the low word cleared, so that df * df is exact
    double df;
    memcpy(&df, &bits, 8);
    const double c = (z - df * df) / (s + df);
    const double w = r * s + c;
    return 2.0 * (df + w);
}

// ---- one lane per query ------------------------------------------------------------------------------------------------------------
struct mg_arc_query_args {
    mg_arc_tables t;
    const double *arc;
    int64_t n;
    double eval_range;
    double *points, *tangents, *angles;
    double ref[2];
    int32_t *exhausted;      // set to 1 by a row whose widening ran out of rounds
};

#define MG_ARC_QUERY_BLOCK 256
__global__ __launch_bounds__(MG_ARC_QUERY_BLOCK) void mg_arc_query_kernel(mg_arc_query_args a) {
    const int64_t i = (int64_t)blockIdx.x * MG_ARC_QUERY_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const mg_arc_tables &t = a.t;
    const double arc = a.arc[i];
    const double none = nan("");
    double start[3] = {none, none, none}, dir[3] = {none, none, none}, angle = none;
    if (isfinite(arc)) {
        mg_traj_point_by_arc(t.poly, t.arc, t.n_seg, t.G, t.full, arc, start);
        if (a.tangents || a.angles) {
            // get_tangent_at_arc_length: the chord over [arc - r, arc + r], r widened by 0.1 while its ends coincide ("cases where the
            // granularity of the spline is too low"; also both ends past the end of the path, which give the last control point)
            double eval_range = a.eval_range, magnitude = 0.0;
            for (int round = 0; round <= MG_ARC_MAX_WIDENINGS && magnitude == 0.0; round++) {
                double p1[3], p2[3];
                mg_traj_point_by_arc(t.poly, t.arc, t.n_seg, t.G, t.full, arc - eval_range, p1);
                mg_traj_point_by_arc(t.poly, t.arc, t.n_seg, t.G, t.full, arc + eval_range, p2);
                dir[0] = p2[0] - p1[0]; dir[1] = p2[1] - p1[1]; dir[2] = p2[2] - p1[2];
                magnitude = mg_arc_norm3(dir[0], dir[1], dir[2]);
                eval_range += 0.1;
            }
            if (magnitude == 0.0) {
                *a.exhausted = 1;            // (every writer stores the same value)
                dir[0] = dir[1] = dir[2] = none;
            } else {
                dir[0] /= magnitude; dir[1] /= magnitude; dir[2] /= magnitude;
                if (a.angles) {
                    // get_angle_at_arc_length_2d: a = reference / |reference|, b = (tangent x, tangent z) / |.|, degrees(acos(a . b))
                    const double na = sqrt(a.ref[0] * a.ref[0] + a.ref[1] * a.ref[1]);
                    const double a0 = a.ref[0] / na, a1 = a.ref[1] / na;
                    const double nb = sqrt(dir[0] * dir[0] + dir[2] * dir[2]);
                    const double b0 = dir[0] / nb, b1 = dir[2] / nb;
                    angle = mg_arc_acos(a0 * b0 + a1 * b1) * (180.0 / 3.141592653589793);
                }
            }
        }
    }
    if (a.points) { a.points[3 * i] = start[0]; a.points[3 * i + 1] = start[1]; a.points[3 * i + 2] = start[2]; }
    if (a.tangents) { a.tangents[3 * i] = dir[0]; a.tangents[3 * i + 1] = dir[1]; a.tangents[3 * i + 2] = dir[2]; }
    if (a.angles) a.angles[i] = angle;
}

struct mg_arc_param_args { mg_arc_tables t; const double *u, *u_max; int64_t n; double *points; };
__global__ __launch_bounds__(MG_ARC_QUERY_BLOCK) void mg_arc_points_at_kernel(mg_arc_param_args a) {
    const int64_t i = (int64_t)blockIdx.x * MG_ARC_QUERY_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    double u = a.u[i];
    if (a.u_max) u = fmin(u, a.u_max[i]);
    double p[3] = {nan(""), nan(""), nan("")};
    if (isfinite(u)) mg_traj_point(a.t.poly, a.t.n_seg, fmin(1.0, fmax(0.0, u)), p);     // (the curve is defined on [0, 1])
    a.points[3 * i] = p[0]; a.points[3 * i + 1] = p[1]; a.points[3 * i + 2] = p[2];
}

// ---- one wave per point ------------------------------------------------------------------------------------------------------------
struct mg_arc_scan_args {
    mg_arc_tables t;
    const double *points, *min_arc;
    int64_t n;
    double *arc_out, *min_point;
    int32_t *min_index;
};

// A workgroup of four waves serves MG_ARC_SCAN_POINTS points, two per wave one after the other, so that a copy of the tables in
// LDS is shared by eight scans.  TABLES_LDS: [12 n_seg + 3] the pieces, [G + 1] the arc lengths, [n_uk] the parameters, copied by the
// whole workgroup; otherwise every look-up goes to global memory (L2: the tables are the same for every point).
// A lane visits the parameters lane, lane + 64, ... in ascending order and keeps its first strict minimum; the wave then reduces on
// (distance, index) with the smaller index winning among equal distances -- a total order, so the butterfly's pairing does not show.
#define MG_ARC_SCAN_BLOCK 256
#define MG_ARC_SCAN_POINTS 8
#define MG_ARC_LDS_MAX (64 * 1024)
template <bool TABLES_LDS>
__global__ __launch_bounds__(MG_ARC_SCAN_BLOCK) void mg_arc_scan_kernel(mg_arc_scan_args a) {
    extern __shared__ double lds[];
    const mg_arc_tables &t = a.t;
    const double *poly = t.poly, *arcs = t.arc, *uk = t.uk;
    if constexpr (TABLES_LDS) {
        const int n_poly = t.n_seg * 12 + 3, n_arc = t.G + 1;
        for (int e = threadIdx.x; e < n_poly; e += MG_ARC_SCAN_BLOCK) lds[e] = t.poly[e];
        for (int e = threadIdx.x; e < n_arc; e += MG_ARC_SCAN_BLOCK) lds[n_poly + e] = t.arc[e];
        for (int e = threadIdx.x; e < t.n_uk; e += MG_ARC_SCAN_BLOCK) lds[n_poly + n_arc + e] = t.uk[e];
        poly = lds; arcs = lds + n_poly; uk = lds + n_poly + n_arc;
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < MG_ARC_SCAN_POINTS; j += MG_ARC_SCAN_BLOCK / 64) {
        const int64_t i = (int64_t)blockIdx.x * MG_ARC_SCAN_POINTS + j;
        if (i >= a.n) break;                                      // (the same in every lane of the wave; no barrier follows)
        const double qx = a.points[3 * i], qy = a.points[3 * i + 1], qz = a.points[3 * i + 2];
        const double min_arc_length = a.min_arc ? a.min_arc[i] : 0.0;
        double min_distance = INFINITY;
        int min_k = INT_MAX;
        for (int k = lane; k < t.n_uk; k += 64) {
            const double u = uk[k];
            if (mg_arc_absolute(arcs, t.G, t.full, u) > min_arc_length) {
                double p[3];
                mg_traj_point(poly, t.n_seg, u, p);
                const double distance = mg_arc_norm3(p[0] - qx, p[1] - qy, p[2] - qz);
                if (distance < min_distance) { min_distance = distance; min_k = k; }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(min_distance, off);
            const int ok = __shfl_xor(min_k, off);
            if (od < min_distance || (od == min_distance && ok < min_k)) { min_distance = od; min_k = ok; }
        }
        if (lane == 0) {
            if (min_k == INT_MAX) {                               // no parameter qualified: -1, the point's row stays as it was
                a.arc_out[i] = -1.0;
                if (a.min_index) a.min_index[i] = -1;
            } else {
                const double u = uk[min_k];
                a.arc_out[i] = mg_arc_absolute(arcs, t.G, t.full, u);
                if (a.min_index) a.min_index[i] = min_k;
                if (a.min_point) {
                    double p[3];
                    mg_traj_point(poly, t.n_seg, u, p);
                    a.min_point[3 * i] = p[0]; a.min_point[3 * i + 1] = p[1]; a.min_point[3 * i + 2] = p[2];
                }
            }
        }
    }
}

// ---- the entry points --------------------------------------------------------------------------------------------------------------
// what the three share: the primitive and its trajectory, n, the tables and the launch's grid at per_workgroup queries a workgroup
static int mg_arc_check(const char *who, mg_primitive *p, const mg_trajectory *t, int64_t n, int per_workgroup, mg_arc_tables *tables, unsigned *grid) {
    MG_REQUIRE(p && t && t->prim == p, "%s: NULL primitive or trajectory, or a trajectory of another primitive", who);
    MG_REQUIRE(n >= 0, "%s: %lld queries", who, (long long)n);
    MG_REQUIRE_AS((n + per_workgroup - 1) / per_workgroup <= 0x7fffffff, MG_ERR_UNSUPPORTED, "%s: too many queries for one launch", who);
    *tables = {t->d_poly, t->d_arc, t->d_uk, t->full_arc, t->n_seg, t->granularity, t->n_uk};
    *grid = (unsigned)((n + per_workgroup - 1) / per_workgroup);
    return MG_OK;
}

extern "C" int mg_trajectory_sample_parameters(const mg_trajectory *t, double *u_host, int32_t *n_samples) {
    MG_REQUIRE(t, "mg_trajectory_sample_parameters: NULL trajectory");
    if (n_samples) *n_samples = t->n_uk;
    if (u_host) {
        MG_HIP_CHECK(hipSetDevice(t->prim->ctx->device));
        MG_HIP_CHECK(hipMemcpy(u_host, t->d_uk, (size_t)t->n_uk * sizeof(double), hipMemcpyDeviceToHost));
    }
    return MG_OK;
}

extern "C" int mg_trajectory_points_by_arc_length(mg_primitive *p, const mg_trajectory *t, const double *arc_dev, int64_t n, double eval_range,
                                                  double *points_dev, double *tangents_dev, double *angles_dev, const double *reference_dir) {
    const char *who = "mg_trajectory_points_by_arc_length";
    mg_arc_query_args a;
    unsigned grid;
    { const int rc = mg_arc_check(who, p, t, n, MG_ARC_QUERY_BLOCK, &a.t, &grid); if (rc != MG_OK) return rc; }
    MG_REQUIRE(std::isfinite(eval_range) && eval_range >= 0.0, "%s: eval_range %g", who, eval_range);
    if (n == 0) return MG_OK;
    MG_REQUIRE(arc_dev && (points_dev || tangents_dev || angles_dev), "%s: NULL pointer", who);
    MG_REQUIRE(!angles_dev || reference_dir, "%s: angles need a reference direction", who);
    mg_context *ctx = p->ctx;
    a.arc = arc_dev; a.n = n; a.eval_range = eval_range; a.points = points_dev; a.tangents = tangents_dev; a.angles = angles_dev;
    a.ref[0] = reference_dir ? reference_dir[0] : 0.0; a.ref[1] = reference_dir ? reference_dir[1] : 0.0;
    a.exhausted = nullptr;
    // a call with tangents reads back whether a row's widening ran out: the flag lives in the call's own block
    int32_t exhausted = 0;
    mg_workspace ws(ctx, who);
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    if (tangents_dev || angles_dev) {
        const mg_staged flag = ws.inout(&exhausted, sizeof(exhausted));
        const int rc = ws.upload();
        if (rc != MG_OK) return rc;
        a.exhausted = flag.dev<int32_t>();
    }
    mg_prof_begin(ctx, MG_PROF_TRAJECTORY);
    hipLaunchKernelGGL(mg_arc_query_kernel, dim3(grid), dim3(MG_ARC_QUERY_BLOCK), 0, ctx->stream, a);
    mg_prof_end(ctx, MG_PROF_TRAJECTORY);
    MG_HIP_CHECK(hipGetLastError());
    { const int rc = ws.download(); if (rc != MG_OK) return rc; }
    MG_REQUIRE_AS(!exhausted, MG_ERR_UNSUPPORTED, "%s: a tangent's two points still coincide after %d widenings of eval_range (their rows are NaN)", who,
                  MG_ARC_MAX_WIDENINGS);
    return MG_OK;
}

extern "C" int mg_trajectory_points_at_parameters(mg_primitive *p, const mg_trajectory *t, const double *u_dev, const double *u_max_dev, int64_t n,
                                                  double *points_dev) {
    const char *who = "mg_trajectory_points_at_parameters";
    mg_arc_param_args a;
    unsigned grid;
    { const int rc = mg_arc_check(who, p, t, n, MG_ARC_QUERY_BLOCK, &a.t, &grid); if (rc != MG_OK) return rc; }
    if (n == 0) return MG_OK;
    MG_REQUIRE(u_dev && points_dev, "%s: NULL pointer", who);
    mg_context *ctx = p->ctx;
    a.u = u_dev; a.u_max = u_max_dev; a.n = n; a.points = points_dev;
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    mg_prof_begin(ctx, MG_PROF_TRAJECTORY);
    hipLaunchKernelGGL(mg_arc_points_at_kernel, dim3(grid), dim3(MG_ARC_QUERY_BLOCK), 0, ctx->stream, a);
    mg_prof_end(ctx, MG_PROF_TRAJECTORY);
    MG_HIP_CHECK(hipGetLastError());
    return MG_OK;
}

extern "C" int mg_trajectory_arc_length_of_points(mg_primitive *p, const mg_trajectory *t, const double *points_dev, const double *min_arc_dev, int64_t n,
                                                  double *arc_out_dev, double *min_point_dev, int32_t *min_index_dev) {
    const char *who = "mg_trajectory_arc_length_of_points";
    mg_arc_scan_args a;
    unsigned grid;
    { const int rc = mg_arc_check(who, p, t, n, MG_ARC_SCAN_POINTS, &a.t, &grid); if (rc != MG_OK) return rc; }
    if (n == 0) return MG_OK;
    MG_REQUIRE(points_dev && arc_out_dev, "%s: NULL pointer", who);
    mg_context *ctx = p->ctx;
    a.points = points_dev; a.min_arc = min_arc_dev; a.n = n; a.arc_out = arc_out_dev; a.min_point = min_point_dev; a.min_index = min_index_dev;
    const size_t table_bytes = ((size_t)t->n_seg * 12 + 3 + (size_t)t->granularity + 1 + (size_t)t->n_uk) * sizeof(double);
    MG_HIP_CHECK(hipSetDevice(ctx->device));
    return mg_dispatch_flags(table_bytes <= MG_ARC_LDS_MAX, [&](auto TABLES_LDS) {
        mg_prof_begin(ctx, MG_PROF_TRAJECTORY);
        hipLaunchKernelGGL(mg_arc_scan_kernel<decltype(TABLES_LDS)::value>, dim3(grid), dim3(MG_ARC_SCAN_BLOCK),
                           decltype(TABLES_LDS)::value ? table_bytes : 0, ctx->stream, a);
        mg_prof_end(ctx, MG_PROF_TRAJECTORY);
        MG_HIP_CHECK(hipGetLastError());
        return (int)MG_OK;
    });
}
