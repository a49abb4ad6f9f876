// Spatial alignment of motions and the per-frame preparation in front of the fPCA (reference construction/
// motion_model_constructor.py: _align_frames_spatially, :244-263, and the first two statements of
// run_spatial_dimension_reduction, :359-360; construction/utils.py: rotate_frames, normalize_root_translation,
// align_quaternion_frames), float64.
//
//   mg_align_motions_spatially   every motion is turned about y so that frame `frame_idx` faces `ref_orientation`, and moved so
//                                that this frame's root position is the origin.  A frame is (x, y, z, then J quaternions
//                                (w, x, y, z)), the root's first.  The contract of one motion, r = ref_orientation / |r| (one
//                                square root and two divisions on the host), f = frame `frame_idx`, every expression one product
//                                and one addition at a time in the written order (no fma):
//                                  heading   n = 1 / sqrt(((fw fw + fx fx) + fy fy) + fz fz), a = (fw n, fx n, fy n, fz n),
//                                            v = (0, 0, 1), c = a.xyz x v, d = a.xyz x c, b = (vx + 2 (aw cx + dx), vz + 2 (aw cz
//                                            + dz)), l = bx bx + bz bz; the motion is refused unless l is finite and > 0;
//                                            m = 1 / sqrt(l), h = (bx m, bz m): the statements of mg_candidate_alignment
//                                            (mg_score_device.h) for a chain of one joint;
//                                  rotation  cos = hx rx + hz rz, sin = hx rz - hz rx (h . r, h x r), taken from the two unit
//                                            vectors, never through an angle: (x, z) -> (cos x - sin z, sin x + cos z) takes h
//                                            onto r.  As a quaternion about y: cos >= 0: ch = sqrt((1 + cos) / 2), sh = sin /
//                                            (2 ch); cos < 0: sh = copysign(sqrt((1 - cos) / 2), sin), ch = sin / (2 sh);
//                                            q_y = (ch, 0, -sh, 0).  No branch of it divides by 0: 180 degrees is not special;
//                                  root position   p' = (cos x - sin z, y, sin x + cos z), out = p' - delta, delta = p' of frame
//                                            `frame_idx`, height included (delta = copy(ma[0, :3]) after rotate_frames);
//                                  root quaternion q / |q| as in the heading (n, four products), then the Hamilton product
//                                            q_y (x) q: (ch w + sh y, ch x - sh z, ch y - sh w, ch z + sh x), all four negated
//                                            when the first is < 0 (the sign quaternion_from_matrix returns);
//                                  every other channel is copied.
//                                A workgroup of 256 lanes per (motion, block of SA_FRAMES frames).  Lane 0 forms the motion's
//                                transform from frame `frame_idx` itself (no second launch; every workgroup of a motion runs the
//                                same statements on the same frame), the first lanes turn a frame's root each into LDS, then
//                                all lanes stream the block's frames as one run of consecutive doubles: lane i reads and writes
//                                element i, i + 256, ..., so a wave's accesses are 512 consecutive bytes whatever D is.
//   mg_prepare_aligned_frames    (N, F, D) frames: scale_vec = the largest |x|, |y|, |z| of the root positions (a maximum is exact
//                                in any order: per-workgroup maxima by an LDS tree, then one workgroup over those), the root
//                                positions divided by it -- unless one of the three is 0: then nothing is scaled and the scale is
//                                reported as ones -- and every quaternion of the first n_joints whose dot product with the
//                                same joint's quaternion in frame 0 of motion 0, ((r0 q0 + r1 q1) + r2 q2) + r3 q3, is < 0 is
//                                negated.  The same frame blocks and the same streaming as above.
//
// Neither kernel has an atomic, and no result depends on the grid: a motion gives the same bits alone or in any batch.  Non-
// finite input, a zero root quaternion and a heading without an x-z part are found by check kernels and answered before the
// kernel proper is launched: nothing is written then.
#include "mg_dtw_device.h"

#include <algorithm>

#define SA_BLOCK 256
#define SA_FRAMES 32
#define SA_MAX_JOINTS 64
#define SA_MAX_PARTIALS 1024

struct sa_transform {
    double c, s, dx, dy, dz;
    int ok;
};

// the transform of one motion from its frame `frame_idx` (f: that frame), r = (rx, rz) of length 1
__device__ __forceinline__ sa_transform sa_motion_transform(const double *__restrict__ f, double rx, double rz) {
    double aw = f[3], ax = f[4], ay = f[5], az = f[6];
    const double n = 1.0 / sqrt(((aw * aw + ax * ax) + ay * ay) + az * az);
    aw = aw * n, ax = ax * n, ay = ay * n, az = az * n;
    const double vx = 0.0, vy = 0.0, vz = 1.0;
    const double cx = ay * vz - az * vy, cy = az * vx - ax * vz, cz = ax * vy - ay * vx;
    const double dx = ay * cz - az * cy, dz = ax * cy - ay * cx;
    const double bx = vx + 2.0 * (aw * cx + dx), bz = vz + 2.0 * (aw * cz + dz);
    const double l = bx * bx + bz * bz;
    sa_transform t;
    t.ok = isfinite(l) && l > 0.0;
    const double m = 1.0 / sqrt(l);
    const double hx = bx * m, hz = bz * m;
    t.c = hx * rx + hz * rz;
    t.s = hx * rz - hz * rx;
    t.dx = t.c * f[0] - t.s * f[2];
    t.dy = f[1];
    t.dz = t.s * f[0] + t.c * f[2];
    return t;
}

// flag[0]: a value that is not finite; flag[1]: a root quaternion whose squared norm is 0 or not finite
static __global__ __launch_bounds__(SA_BLOCK) void sa_check_kernel(const double *__restrict__ x, int64_t n, int32_t D, int32_t *__restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (e >= n) return;
    if (!isfinite(x[e])) flag[0] = 1;
    if (e % D == 3) {
        const double n2 = ((x[e] * x[e] + x[e + 1] * x[e + 1]) + x[e + 2] * x[e + 2]) + x[e + 3] * x[e + 3];
        if (!(isfinite(n2) && n2 > 0.0)) flag[1] = 1;
    }
}

// one workgroup: first[0] = the first motion whose heading has no x-z part (n_motions: none)
static __global__ __launch_bounds__(SA_BLOCK) void sa_heading_check_kernel(const double *__restrict__ in, const int64_t *__restrict__ off, int64_t n_motions,
                                                                           int32_t D, int64_t frame_idx, double rx, double rz, int64_t *__restrict__ first) {
    __shared__ int64_t red[SA_BLOCK];
    int64_t mine = n_motions;
    for (int64_t n = threadIdx.x; n < n_motions; n += SA_BLOCK) {
        const sa_transform t = sa_motion_transform(in + (off[n] + frame_idx) * D, rx, rz);
        if (!t.ok && n < mine) mine = n;
    }
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int s = SA_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && red[threadIdx.x + s] < red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) first[0] = red[0];
}

__global__ __launch_bounds__(SA_BLOCK) void sa_align_kernel(const double *__restrict__ in, const int64_t *__restrict__ off, int32_t D, int64_t frame_idx,
                                                            double rx, double rz, double *__restrict__ out, double *__restrict__ transforms, int64_t n0) {
    __shared__ double s_t[8];
    __shared__ double s_root[SA_FRAMES][7];
    const int tid = threadIdx.x;
    const int64_t n = n0 + blockIdx.y, b0 = off[n], F = off[n + 1] - b0;
    const int64_t f0 = (int64_t)blockIdx.x * SA_FRAMES;
    if (f0 >= F) return;   // whole workgroup: this motion is shorter than the longest
    const int nf = (int)(F - f0 < SA_FRAMES ? F - f0 : SA_FRAMES);
    if (tid == 0) {
        const sa_transform t = sa_motion_transform(in + (b0 + frame_idx) * D, rx, rz);
        double ch, sh;
        if (t.c >= 0.0) {
            ch = sqrt((1.0 + t.c) / 2.0);
            sh = t.s / (2.0 * ch);
        } else {
            sh = copysign(sqrt((1.0 - t.c) / 2.0), t.s);
            ch = t.s / (2.0 * sh);
        }
        s_t[0] = t.c, s_t[1] = t.s, s_t[2] = t.dx, s_t[3] = t.dy, s_t[4] = t.dz, s_t[5] = ch, s_t[6] = sh, s_t[7] = t.ok ? 1.0 : 0.0;
        if (t.ok && transforms && blockIdx.x == 0) {
            double *tr = transforms + 5 * n;
            tr[0] = t.c, tr[1] = t.s, tr[2] = t.dx, tr[3] = t.dy, tr[4] = t.dz;
        }
    }
    __syncthreads();
    if (s_t[7] == 0.0) return;   // the check kernel has refused such a motion before this launch: never a NaN in `out`
    const double *src = in + (b0 + f0) * D;
    double *dst = out + (b0 + f0) * D;
    if (tid < nf) {
        const double *f = src + (int64_t)tid * D;
        const double c = s_t[0], s = s_t[1], ch = s_t[5], sh = s_t[6];
        double *r = s_root[tid];
        r[0] = (c * f[0] - s * f[2]) - s_t[2];
        r[1] = f[1] - s_t[3];
        r[2] = (s * f[0] + c * f[2]) - s_t[4];
        double w = f[3], x = f[4], y = f[5], z = f[6];
        const double nq = 1.0 / sqrt(((w * w + x * x) + y * y) + z * z);
        w = w * nq, x = x * nq, y = y * nq, z = z * nq;
        double pw = ch * w + sh * y, px = ch * x - sh * z, py = ch * y - sh * w, pz = ch * z + sh * x;
        if (pw < 0.0) pw = -pw, px = -px, py = -py, pz = -pz;
        r[3] = pw, r[4] = px, r[5] = py, r[6] = pz;
    }
    __syncthreads();
    const int total = nf * D;   // at most 32 * 259
    for (int e = tid; e < total; e += SA_BLOCK) {
        const int f = e / D, c = e - f * D;
        dst[e] = c < 7 ? s_root[f][c] : src[e];
    }
}

// partial[3 b + c] = the largest |channel c| over the rows workgroup b visits
static __global__ __launch_bounds__(SA_BLOCK) void pa_max_partial_kernel(const double *__restrict__ x, int64_t n_rows, int32_t D, double *__restrict__ partial) {
    __shared__ double red[3][SA_BLOCK];
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * SA_BLOCK + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * SA_BLOCK) {
        const double *p = x + r * D;
        m0 = fmax(m0, fabs(p[0])), m1 = fmax(m1, fabs(p[1])), m2 = fmax(m2, fabs(p[2]));
    }
    red[0][threadIdx.x] = m0, red[1][threadIdx.x] = m1, red[2][threadIdx.x] = m2;
    __syncthreads();
    for (int s = SA_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < 3; c++) red[c][threadIdx.x] = fmax(red[c][threadIdx.x], red[c][threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[3 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

// scale[c] = the largest of partial[3 b + c], b < n_partials (one workgroup)
static __global__ __launch_bounds__(SA_BLOCK) void pa_max_final_kernel(const double *__restrict__ partial, int32_t n_partials, double *__restrict__ scale) {
    __shared__ double red[3][SA_BLOCK];
    double m[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < n_partials; b += SA_BLOCK)
        for (int c = 0; c < 3; c++) m[c] = fmax(m[c], partial[3 * b + c]);
    for (int c = 0; c < 3; c++) red[c][threadIdx.x] = m[c];
    __syncthreads();
    for (int s = SA_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < 3; c++) red[c][threadIdx.x] = fmax(red[c][threadIdx.x], red[c][threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x < 3) scale[threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(SA_BLOCK) void pa_prepare_kernel(const double *__restrict__ in, int64_t n_rows, int32_t D, int32_t n_quat_channels, double s0,
                                                              double s1, double s2, int32_t do_scale, double *__restrict__ out) {
    const int64_t f0 = (int64_t)blockIdx.x * SA_FRAMES;
    const int nf = (int)(n_rows - f0 < SA_FRAMES ? n_rows - f0 : SA_FRAMES);
    const double *src = in + f0 * D;
    double *dst = out + f0 * D;
    const int total = nf * D;
    for (int e = threadIdx.x; e < total; e += SA_BLOCK) {
        const int f = e / D, c = e - f * D;
        double v = src[e];
        if (c < 3) {
            if (do_scale) v = v / (c == 0 ? s0 : c == 1 ? s1 : s2);
        } else if (c < 3 + n_quat_channels) {
            const int j0 = 3 + ((c - 3) & ~3);
            const double *q = src + f * D + j0, *r = in + j0;   // r: the joint's quaternion in frame 0 of motion 0
            const double dot = ((r[0] * q[0] + r[1] * q[1]) + r[2] * q[2]) + r[3] * q[3];
            if (dot < 0.0) v = -v;
        }
        dst[e] = v;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
#define SA_MAX_ELEMENTS ((int64_t)1 << 39)

extern "C" int mg_align_motions_spatially(mg_context *ctx, const double *frames_dev, const int64_t *offsets, int64_t n_motions, int32_t n_dim,
                                          int64_t frame_idx, const double *ref_orientation, double *out_dev, double *transforms_dev) {
    const char *who = "mg_align_motions_spatially";
    MG_REQUIRE_AS(ctx && offsets && ref_orientation, MG_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    MG_REQUIRE_AS(n_motions >= 0, MG_ERR_INVALID_ARGUMENT, "%s: n_motions = %lld", who, (long long)n_motions);
    MG_REQUIRE_AS(n_dim >= 7 && (n_dim - 3) % 4 == 0 && (n_dim - 3) / 4 <= SA_MAX_JOINTS, MG_ERR_UNSUPPORTED,
                  "%s: %d channels (3 + 4 J with 1 <= J <= %d)", who, n_dim, SA_MAX_JOINTS);
    int64_t longest = 0;
    const int rc = mg_check_offsets(who, offsets, n_motions, ((int64_t)1 << 31) - 1, "fewer than 2^31", MG_ERR_UNSUPPORTED, &longest);
    if (rc != MG_OK || n_motions == 0) return rc;
    MG_REQUIRE_AS(frames_dev && out_dev, MG_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    MG_REQUIRE_AS(frames_dev != out_dev, MG_ERR_INVALID_ARGUMENT, "%s: out_dev is frames_dev (every workgroup of a motion reads frame %lld)", who,
                  (long long)frame_idx);
    const int64_t total = offsets[n_motions] * n_dim;
    MG_REQUIRE_AS(total < SA_MAX_ELEMENTS, MG_ERR_UNSUPPORTED, "%s: %lld values (fewer than 2^39)", who, (long long)total);
    for (int64_t n = 0; n < n_motions; n++)
        MG_REQUIRE_AS(frame_idx >= 0 && frame_idx < offsets[n + 1] - offsets[n], MG_ERR_INVALID_ARGUMENT, "%s: frame_idx = %lld, motion %lld has %lld frames",
                      who, (long long)frame_idx, (long long)n, (long long)(offsets[n + 1] - offsets[n]));
    const double r0 = ref_orientation[0], r1 = ref_orientation[1];
    const double rn = std::sqrt(r0 * r0 + r1 * r1);
    MG_REQUIRE_AS(std::isfinite(rn) && rn > 0.0, MG_ERR_INVALID_ARGUMENT, "%s: ref_orientation = (%g, %g)", who, r0, r1);
    const double rx = r0 / rn, rz = r1 / rn;
    dtw_block blk(ctx, who);
    const int rb = dtw_block_create(&blk, offsets, n_motions, nullptr, 0, 0);
    if (rb != MG_OK) return rb;
    int64_t *first_dev = (int64_t *)(blk.flag + 4);
    hipLaunchKernelGGL(sa_check_kernel, dim3((unsigned)((total + SA_BLOCK - 1) / SA_BLOCK)), dim3(SA_BLOCK), 0, ctx->stream, frames_dev, total, n_dim, blk.flag);
    hipLaunchKernelGGL(sa_heading_check_kernel, dim3(1), dim3(SA_BLOCK), 0, ctx->stream, frames_dev, (const int64_t *)blk.off, n_motions, n_dim, frame_idx, rx,
                       rz, first_dev);
    MG_HIP_CHECK(hipGetLastError());
    int64_t flags[3] = {0, 0, 0};   // two int32 flags, 8 bytes unused, the first refused motion
    MG_HIP_CHECK(hipMemcpyAsync(flags, blk.flag, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int32_t *f32 = (const int32_t *)flags;
    MG_REQUIRE_AS(!f32[0], MG_ERR_INVALID_ARGUMENT, "%s: the frames hold non-finite values", who);
    MG_REQUIRE_AS(!f32[1], MG_ERR_INVALID_ARGUMENT, "%s: a root quaternion is zero (or its norm overflows)", who);
    MG_REQUIRE_AS(flags[2] >= n_motions, MG_ERR_INVALID_ARGUMENT, "%s: motion %lld: the root of frame %lld turns z onto the y axis (no heading)", who,
                  (long long)flags[2], (long long)frame_idx);
    const unsigned blocks_x = (unsigned)((longest + SA_FRAMES - 1) / SA_FRAMES);
    for (int64_t n0 = 0; n0 < n_motions; n0 += 65535) {   // grid.y limit
        const int64_t nb = std::min<int64_t>(65535, n_motions - n0);
        hipLaunchKernelGGL(sa_align_kernel, dim3(blocks_x, (unsigned)nb), dim3(SA_BLOCK), 0, ctx->stream, frames_dev, (const int64_t *)blk.off, n_dim, frame_idx,
                           rx, rz, out_dev, transforms_dev, n0);
    }
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

extern "C" int mg_prepare_aligned_frames(mg_context *ctx, const double *frames_dev, int64_t n_motions, int32_t n_frames, int32_t n_dim, int32_t n_joints,
                                         double *out_dev, double *scale_vec) {
    const char *who = "mg_prepare_aligned_frames";
    MG_REQUIRE_AS(ctx && scale_vec, MG_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    MG_REQUIRE_AS(n_motions >= 0 && n_frames >= 1 && n_dim >= 3 && n_joints >= 0 && 3 + 4 * (int64_t)n_joints <= n_dim, MG_ERR_INVALID_ARGUMENT,
                  "%s: n_motions = %lld, n_frames = %d, n_dim = %d, n_joints = %d", who, (long long)n_motions, n_frames, n_dim, n_joints);
    MG_REQUIRE_AS(n_dim <= (1 << 20), MG_ERR_UNSUPPORTED, "%s: %d channels (at most 2^20)", who, n_dim);
    scale_vec[0] = scale_vec[1] = scale_vec[2] = 1.0;
    if (n_motions == 0) return MG_OK;
    MG_REQUIRE_AS(frames_dev && out_dev, MG_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    MG_REQUIRE_AS(frames_dev != out_dev, MG_ERR_INVALID_ARGUMENT, "%s: out_dev is frames_dev (every workgroup reads frame 0 of motion 0)", who);
    MG_REQUIRE_AS(n_motions < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED, "%s: %lld motions (fewer than 2^31)", who, (long long)n_motions);
    const int64_t n_rows = n_motions * n_frames, total = n_rows * n_dim;
    MG_REQUIRE_AS(total < SA_MAX_ELEMENTS && n_rows / SA_FRAMES < ((int64_t)1 << 31) - 1, MG_ERR_UNSUPPORTED,
                  "%s: %lld frames of %d values (fewer than 2^39 values and 2^36 frames)", who, (long long)n_rows, n_dim);
    const int n_partials = (int)std::min<int64_t>(SA_MAX_PARTIALS, (n_rows + SA_BLOCK - 1) / SA_BLOCK);
    mg_workspace ws(ctx, who);
    const size_t o_flag = ws.carve(256), o_scale = ws.carve(256), o_partial = ws.carve((size_t)n_partials * 3 * 8);
    const int ra = ws.alloc();
    if (ra != MG_OK) return ra;
    int32_t *flag = ws.at<int32_t>(o_flag);
    double *scale_dev = ws.at<double>(o_scale), *partial = ws.at<double>(o_partial);
    MG_HIP_CHECK(hipMemsetAsync(flag, 0, 256, ctx->stream));
    dtw_launch_nonfinite(ctx, frames_dev, total, flag);
    hipLaunchKernelGGL(pa_max_partial_kernel, dim3((unsigned)n_partials), dim3(SA_BLOCK), 0, ctx->stream, frames_dev, n_rows, n_dim, partial);
    hipLaunchKernelGGL(pa_max_final_kernel, dim3(1), dim3(SA_BLOCK), 0, ctx->stream, (const double *)partial, n_partials, scale_dev);
    MG_HIP_CHECK(hipGetLastError());
    int32_t bad = 0;
    double scale[3] = {1.0, 1.0, 1.0};
    MG_HIP_CHECK(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipMemcpyAsync(scale, scale_dev, sizeof(scale), hipMemcpyDeviceToHost, ctx->stream));
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MG_REQUIRE_AS(!bad, MG_ERR_INVALID_ARGUMENT, "%s: the frames hold non-finite values", who);
    const int do_scale = scale[0] != 0.0 && scale[1] != 0.0 && scale[2] != 0.0;
    hipLaunchKernelGGL(pa_prepare_kernel, dim3((unsigned)((n_rows + SA_FRAMES - 1) / SA_FRAMES)), dim3(SA_BLOCK), 0, ctx->stream, frames_dev, n_rows, n_dim,
                       4 * n_joints, scale[0], scale[1], scale[2], do_scale, out_dev);
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (do_scale) scale_vec[0] = scale[0], scale_vec[1] = scale[1], scale_vec[2] = scale[2];
    return MG_OK;
}
