// Cutting motion clips out of captures at keyframe poses (reference construction/keyframe_detection.py: KeyframeDetector.
// find_instance, find_instances, calculate_distances, argmin, argmin_multi; construction/segmentation.py: Segmentation.
// extract_single_segments, extract_segments), float64.
//
//   mg_keyframe_distances   dist[k][f] = the cell of mg_dtw.hip's header comment with A = frame f of the concatenated captures and
//                           B = keyframe k (the reference calls distance_measure(f, keyframe): the keyframe is fitted onto the
//                           frame, the mean divides by the keyframe's J).  The statements are those of mg_dtw_device.h, the ones
//                           dtw_distance_grids_kernel compiles: dist[k][f] has the bits of that kernel's cell (f, 0) for
//                           (reference motion = the capture, one motion = the one-frame keyframe).  A workgroup is one wave, a lane
//                           per frame; its 64 frames (contiguous in the table whatever motion they belong to) are loaded once,
//                           coalesced, into LDS rows an odd number of doubles apart (the 32 lanes of a half wave read 32 different
//                           bank pairs), next to the K keyframes, their one-cloud sums (formed once per workgroup) and the weights,
//                           which every lane reads at one address.  A lane forms its frame's two sums once and runs the K cells.
//                           Plain VALU, for the reason given in mg_dtw.hip.  (64 + K) (3 J | 1) doubles of LDS: 32 KB at J = 19,
//                           K = 2; 112 KB at J = 64, K = 8, a workgroup per CU.
//   mg_segment_search       one workgroup of 256 lanes per motion, all motions in one launch.  Every arg-min is the FIRST index
//                           of the least value (argmin's strict `<`): lanes walk their frames in rising order and keep the first,
//                           waves and the workgroup reduce (value, index) pairs lexicographically.
//                           MG_SEGMENT_SINGLE: (argmin of the start distances, argmin of the end distances), always one pair.
//                           MG_SEGMENT_MULTI (segmentation.py:61-80): m = min of the start distances; instances = the frames with
//                           v <= m + threshold (that one addition), listed in frame order by a ballot / prefix-sum compaction, 256
//                           frames a step; instance i's window ends at instance i + 1, the last one's at F - 1; a wave takes 64
//                           instances, drops the windows with end - start < min_segment_size and runs the others one after the
//                           other, e = start + argmin(end distances[start : window end)), kept if e - start > min_segment_size;
//                           a second ordered compaction writes the kept (start, e) pairs.  Windows are disjoint: O(F) per motion.
//
// No atomics, no grid barriers; nothing depends on the batch or the schedule.  Limits and non-finite inputs (a check kernel) are
// answered before either kernel is launched.  The reference's `v < min_v` silently skips a NaN; here it is refused.
#include "mg_dtw_device.h"

#include <algorithm>
#include <climits>

#define SEG_MAX_KEYFRAMES 8
#define SEG_FRAMES 64      // frames, and lanes, of a keyframe-distance workgroup
#define SEG_BLOCK 256
#define SEG_WAVES (SEG_BLOCK / 64)

__global__ __launch_bounds__(SEG_FRAMES) void keyframe_distances_kernel(const double *__restrict__ clouds, int64_t total, int32_t J,
                                                                        const double *__restrict__ keyframes, int32_t K, const double *__restrict__ w,
                                                                        double *__restrict__ dist) {
    extern __shared__ double seg_lds[];
    const int tid = threadIdx.x;
    const int row_len = 3 * J, stride = row_len | 1;
    double *sF = seg_lds, *sK = sF + SEG_FRAMES * stride, *sW = sK + K * stride, *sums = sW + DTW_MAX_JOINTS;   // sums: [K][2], then sw
    const int64_t f0 = (int64_t)blockIdx.x * SEG_FRAMES;
    const int rows = (int)(total - f0 < SEG_FRAMES ? total - f0 : SEG_FRAMES);
    const double *src = clouds + f0 * row_len;
    for (int e = tid; e < SEG_FRAMES * row_len; e += SEG_FRAMES) {
        const int r = e / row_len, c = e % row_len;
        sF[r * stride + c] = r < rows ? src[e] : 0.0;
    }
    for (int e = tid; e < K * row_len; e += SEG_FRAMES) sK[(e / row_len) * stride + e % row_len] = keyframes[e];
    if (tid < J) sW[tid] = w[tid];
    __syncthreads();
    if (tid < K) {
        dtw_cloud_sums(sK + tid * stride, sW, J, &sums[2 * tid], &sums[2 * tid + 1]);
    } else if (tid == K) {
        sums[2 * SEG_MAX_KEYFRAMES] = dtw_weight_sum(sW, J);
    }
    __syncthreads();
    const double *a = sF + tid * stride;
    double sax, saz;
    dtw_cloud_sums(a, sW, J, &sax, &saz);
    const double sw = sums[2 * SEG_MAX_KEYFRAMES];
    for (int k = 0; k < K; k++) {
        const double cell = dtw_cell(a, sK + k * stride, sW, J, sax, saz, sums[2 * k], sums[2 * k + 1], sw);
        if (tid < rows) dist[(int64_t)k * total + f0 + tid] = cell;
    }
}

// ---- (value, index) pairs in lexicographic order: the first index of the least value ------------------------------------------
__device__ __forceinline__ void seg_take(double &v, int32_t &i, double ov, int32_t oi) {
    if (ov < v || (ov == v && oi < i)) v = ov, i = oi;
}

__device__ __forceinline__ void seg_wave_argmin(double &v, int32_t &i) {   // every lane ends with the wave's pair
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int32_t oi = __shfl_xor(i, o);
        seg_take(v, i, ov, oi);
    }
}

// the pair of d[0 .. F) in every lane of the workgroup (INT32_MAX for no frame at all)
__device__ __forceinline__ void seg_block_argmin(const double *__restrict__ d, int32_t F, double *s_v, int32_t *s_i, double &v, int32_t &i) {
    v = INFINITY, i = INT32_MAX;
    for (int64_t f = threadIdx.x; f < F; f += SEG_BLOCK) {
        const double x = d[f];
        if (x < v) v = x, i = (int32_t)f;
    }
    seg_wave_argmin(v, i);
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v, s_i[threadIdx.x >> 6] = i;
    __syncthreads();
    v = s_v[0], i = s_i[0];
    for (int wv = 1; wv < SEG_WAVES; wv++) seg_take(v, i, s_v[wv], s_i[wv]);
    __syncthreads();   // s_v, s_i are free again
}

// where a lane's flagged element goes in an ordered list that already has `base` entries; returns the workgroup's count
__device__ __forceinline__ int32_t seg_compact_step(bool flag, int32_t base, int32_t *s_cnt, int32_t *pos) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int32_t before = 0, all = 0;
    for (int wv = 0; wv < SEG_WAVES; wv++) {
        const int32_t c = s_cnt[wv];
        before += wv < wave ? c : 0;
        all += c;
    }
    *pos = base + before + __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();   // s_cnt is free again
    return all;
}

// work: 2 * total int32 (the instances of every motion where its frames lie, then their ends); MG_SEGMENT_MULTI only
__global__ __launch_bounds__(SEG_BLOCK) void segment_search_kernel(const double *__restrict__ start_dist, const double *__restrict__ end_dist,
                                                                   const int64_t *__restrict__ off, const int64_t *__restrict__ seg_off, int32_t mode,
                                                                   double threshold, int32_t min_size, int32_t *work, int64_t total,
                                                                   int32_t *__restrict__ segments, int32_t *__restrict__ counts) {
    __shared__ double s_v[SEG_WAVES];
    __shared__ int32_t s_i[SEG_WAVES], s_cnt[SEG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = blockIdx.x, b0 = off[n];
    const int32_t F = (int32_t)(off[n + 1] - b0);
    const int64_t cap = seg_off[n + 1] - seg_off[n];
    const double *sd = start_dist + b0, *ed = end_dist + b0;
    int32_t *pairs = segments + 2 * seg_off[n];
    double m;
    int32_t m_at;
    seg_block_argmin(sd, F, s_v, s_i, m, m_at);
    if (mode == MG_SEGMENT_SINGLE) {
        double ev;
        int32_t e_at;
        seg_block_argmin(ed, F, s_v, s_i, ev, e_at);
        if (tid == 0) pairs[0] = m_at, pairs[1] = e_at, counts[n] = 1;
        return;
    }
    const double limit = m + threshold;
    int32_t *inst = work + b0, *ends = work + total + b0;
    int32_t n_inst = 0;
    for (int64_t c0 = 0; c0 < F; c0 += SEG_BLOCK) {
        const int64_t f = c0 + tid;
        const bool flag = f < F && sd[f] <= limit;
        int32_t pos;
        const int32_t all = seg_compact_step(flag, n_inst, s_cnt, &pos);
        if (flag) inst[pos] = (int32_t)f;
        n_inst += all;
    }
    __threadfence_block();
    __syncthreads();
    for (int64_t c0 = (int64_t)wave * 64; c0 < n_inst; c0 += SEG_BLOCK) {   // the same for a wave's lanes
        const int64_t i = c0 + lane;
        int32_t st = 0, we = 0, my_end = -1;
        bool live = false;
        if (i < n_inst) {
            st = inst[i];
            we = i + 1 < n_inst ? inst[i + 1] : F - 1;
            live = we - st >= min_size;
        }
        unsigned long long todo = __ballot(live);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1;
            const int32_t s = __shfl(st, src), w_end = __shfl(we, src);
            double v = INFINITY;
            int32_t at = INT32_MAX;
            for (int64_t f = (int64_t)s + lane; f < w_end; f += 64) {
                const double x = ed[f];
                if (x < v) v = x, at = (int32_t)f;
            }
            seg_wave_argmin(v, at);
            const int32_t e = at == INT32_MAX ? s : at;   // a window without frames: argmin's index 0
            if (lane == src && e - s > min_size) my_end = e;
        }
        if (i < n_inst) ends[i] = my_end;
    }
    __threadfence_block();
    __syncthreads();
    int32_t kept = 0;
    for (int64_t c0 = 0; c0 < n_inst; c0 += SEG_BLOCK) {
        const int64_t i = c0 + tid;
        const int32_t e = i < n_inst ? ends[i] : -1;
        int32_t pos;
        const int32_t all = seg_compact_step(e >= 0, kept, s_cnt, &pos);
        if (e >= 0 && pos < cap) pairs[2 * pos] = inst[i], pairs[2 * pos + 1] = e;
        kept += all;
    }
    if (tid == 0) counts[n] = kept;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static int seg_check_offsets(const char *who, const int64_t *offsets, int64_t n_motions, int code_too_long) {
    int64_t longest = 0;
    return mg_check_offsets(who, offsets, n_motions, INT32_MAX, "fewer than 2^31", code_too_long, &longest);
}

extern "C" int mg_keyframe_distances(mg_context *ctx, const double *clouds_dev, const int64_t *offsets, int64_t n_motions, int32_t n_joints,
                                     const double *keyframes_dev, int32_t n_keyframes, const double *weights, double *dist_dev) {
    MG_REQUIRE_AS(ctx && offsets, MG_ERR_INVALID_ARGUMENT, "mg_keyframe_distances: NULL argument");
    MG_REQUIRE_AS(n_motions >= 0, MG_ERR_INVALID_ARGUMENT, "mg_keyframe_distances: n_motions = %lld", (long long)n_motions);
    MG_REQUIRE_AS(n_joints >= 1 && n_joints <= DTW_MAX_JOINTS, MG_ERR_INVALID_ARGUMENT, "mg_keyframe_distances: %d joints (1 to %d)", n_joints,
                  DTW_MAX_JOINTS);
    MG_REQUIRE_AS(n_keyframes >= 1 && n_keyframes <= SEG_MAX_KEYFRAMES, MG_ERR_INVALID_ARGUMENT, "mg_keyframe_distances: %d keyframes (1 to %d)",
                  n_keyframes, SEG_MAX_KEYFRAMES);
    const int rc = seg_check_offsets("mg_keyframe_distances", offsets, n_motions, MG_ERR_INVALID_ARGUMENT);
    if (rc != MG_OK || n_motions == 0) return rc;
    MG_REQUIRE_AS(clouds_dev && keyframes_dev && dist_dev, MG_ERR_INVALID_ARGUMENT, "mg_keyframe_distances: NULL argument");
    const int64_t total = offsets[n_motions];
    MG_REQUIRE_AS((total + SEG_FRAMES - 1) / SEG_FRAMES <= INT32_MAX, MG_ERR_INVALID_ARGUMENT, "mg_keyframe_distances: %lld frames", (long long)total);
    double ones[DTW_MAX_JOINTS];
    const int rw = dtw_weights("mg_keyframe_distances", weights, n_joints, ones);
    if (rw != MG_OK) return rw;
    dtw_block blk(ctx, "mg_keyframe_distances");
    const int rb = dtw_block_create(&blk, offsets, 0, ones, n_joints, 0);   // the kernel needs no offsets
    if (rb != MG_OK) return rb;
    const int64_t row_len = 3 * (int64_t)n_joints;
    dtw_launch_nonfinite(ctx, clouds_dev, total * row_len, blk.flag);
    dtw_launch_nonfinite(ctx, keyframes_dev, n_keyframes * row_len, blk.flag);
    int32_t flag = 0;
    const int rf = dtw_flag_after(ctx, blk, &flag);
    if (rf != MG_OK) return rf;
    MG_REQUIRE_AS(!flag, MG_ERR_INVALID_ARGUMENT, "mg_keyframe_distances: the point clouds or the keyframes hold non-finite values");
    const size_t lds = ((size_t)(SEG_FRAMES + n_keyframes) * ((3 * n_joints) | 1) + DTW_MAX_JOINTS + 2 * SEG_MAX_KEYFRAMES + 1) * 8;   // at most 111 816 bytes
    if (lds > 64 * 1024)
        MG_HIP_CHECK(mg_lds_opt_in((int)lds, keyframe_distances_kernel));
    hipLaunchKernelGGL(keyframe_distances_kernel, dim3((unsigned)((total + SEG_FRAMES - 1) / SEG_FRAMES)), dim3(SEG_FRAMES), lds, ctx->stream, clouds_dev,
                       total, n_joints, keyframes_dev, n_keyframes, (const double *)blk.w, dist_dev);
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

extern "C" int mg_segment_search(mg_context *ctx, const double *start_dist_dev, const double *end_dist_dev, const int64_t *offsets, int64_t n_motions,
                                 int32_t mode, double threshold, int32_t min_segment_size, const int64_t *segment_offsets, int32_t *segments_dev,
                                 int32_t *counts_dev) {
    MG_REQUIRE_AS(ctx && offsets && segment_offsets, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: NULL argument");
    MG_REQUIRE_AS(n_motions >= 0, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: n_motions = %lld", (long long)n_motions);
    MG_REQUIRE_AS(n_motions < ((int64_t)1 << 31), MG_ERR_UNSUPPORTED, "mg_segment_search: %lld motions (fewer than 2^31)", (long long)n_motions);
    MG_REQUIRE_AS(mode == MG_SEGMENT_SINGLE || mode == MG_SEGMENT_MULTI, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: mode %d", mode);
    if (mode == MG_SEGMENT_MULTI) {
        MG_REQUIRE_AS(!std::isnan(threshold), MG_ERR_INVALID_ARGUMENT, "mg_segment_search: the threshold is not a number");
        MG_REQUIRE_AS(min_segment_size >= 0, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: min_segment_size = %d", min_segment_size);
    }
    const int rc = seg_check_offsets("mg_segment_search", offsets, n_motions, MG_ERR_UNSUPPORTED);
    if (rc != MG_OK) return rc;
    MG_REQUIRE_AS(segment_offsets[0] >= 0, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: segment_offsets[0] = %lld", (long long)segment_offsets[0]);
    for (int64_t n = 0; n < n_motions; n++) {
        const int64_t f = offsets[n + 1] - offsets[n], room = segment_offsets[n + 1] - segment_offsets[n];
        const int64_t need = mode == MG_SEGMENT_SINGLE ? 1 : f / ((int64_t)min_segment_size + 1) + 1;
        MG_REQUIRE_AS(room >= need, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: motion %lld of %lld frames has room for %lld pairs (%lld needed)", (long long)n,
                      (long long)f, (long long)room, (long long)need);
    }
    if (n_motions == 0) return MG_OK;
    MG_REQUIRE_AS(start_dist_dev && end_dist_dev && segments_dev && counts_dev, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: NULL argument");
    const int64_t total = offsets[n_motions];
    const size_t seg_off_bytes = mg_workspace::align(((size_t)n_motions + 1) * 8);
    dtw_block blk(ctx, "mg_segment_search");
    const int rb = dtw_block_create(&blk, offsets, n_motions, nullptr, 0, seg_off_bytes + (mode == MG_SEGMENT_MULTI ? (size_t)total * 8 : 0));
    if (rb != MG_OK) return rb;
    MG_HIP_CHECK(hipMemcpyAsync(blk.extra, segment_offsets, ((size_t)n_motions + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    dtw_launch_nonfinite(ctx, start_dist_dev, total, blk.flag);
    dtw_launch_nonfinite(ctx, end_dist_dev, total, blk.flag);
    int32_t flag = 0;
    const int rf = dtw_flag_after(ctx, blk, &flag);
    if (rf != MG_OK) return rf;
    MG_REQUIRE_AS(!flag, MG_ERR_INVALID_ARGUMENT, "mg_segment_search: the distances hold non-finite values");
    hipLaunchKernelGGL(segment_search_kernel, dim3((unsigned)n_motions), dim3(SEG_BLOCK), 0, ctx->stream, start_dist_dev, end_dist_dev,
                       (const int64_t *)blk.off, (const int64_t *)blk.extra, mode, threshold, min_segment_size, (int32_t *)(blk.extra + seg_off_bytes), total,
                       segments_dev, counts_dev);
    MG_HIP_CHECK(hipGetLastError());
    MG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MG_OK;
}
