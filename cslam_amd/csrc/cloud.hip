// cloud.hip -- the voxel filters (gfx950): coloured keyframe clouds from RGB-D frames, the merged swarm map, and the
// down-sampling of lidar keyframes.  One chain, bounds to segments, written once (cloud_filter_run) for three grid rules.
//
// Lidar: replaces `downsample` of cslam/lidar_pr/icp_utils.py:93-100 (drop the non-finite rows, then open3d's
// voxel_down_sample) for a batch of clouds.  Per cloud: origin = min over the finite rows - voxel / 2, voxel index per
// axis = floor((p - origin) / voxel) with a true division, one output row per occupied voxel = the sum of its points in
// CLOUD ORDER, accumulated one after another from the first, divided once by the count.  Rows come out in ascending
// lexicographic voxel index, x most significant.  All arithmetic is float64 (GridOpen3d of cloud.h).
//
// Clouds and map: replaces, for a batch of keyframes, `create_colored_pointcloud` (src/front_end/visualization_utils.cpp:8-137, unit
// rules of depth_traits.h:50-64), `RGBDHandler::visualization_pointcloud_voxel_subsampling` (rgbd_handler.cpp:640-663:
// pcl::VoxelGrid, then pcl::PassThrough on z), and what the reference's visualiser does with the result: every keyframe
// cloud placed at its optimised pose, here merged into one voxel grid.  The rules are in cloud.h, written once for the
// kernels and the host tests; include/cslam_hip.h states them and tests/cloud_reference.py restates them in numpy.
//
//   cloud_project_kernel : the organised cloud of every frame (float32 xyz, packed rgb; NaN rows for invalid depths), and
//                          in the same pass the min / max per axis over its finite rows and the number of other rows:
//                          wave shuffles, then LDS, one partial per workgroup, no float atomics.
//   cloud_bounds_kernel  : the same reduction over rows that already exist (an explicit cloud, the transformed map rows,
//                          a lidar cloud).  A minimum does not depend on the order it is taken in.
//   cloud_meta_kernel    : templated on the rule; folds the partials per cloud: the rule's base (the cell of the minimum, or
//                          open3d's origin), the bits each axis needs from the index of the maximum (every step of a rule
//                          is monotone, so that is the largest index), status 1 for an index of 2^21 or more.
//   cloud_key_kernel     : templated on the rule; the indices packed with the cloud's OWN widths by cloud_shift (cloud.h):
//                          iz << (bx + by) | iy << bx | ix for the PCL and map rules, so ascending key is PCL's linear
//                          order (x fastest); ix << (by + bz) | iy << bz | iz for open3d's.  A row that does not exist
//                          (non-finite, or of a cloud beyond the range) gets the engine's "row does not exist" bit.
//   voxel engine         : voxel.hip's stable radix sort, segment heads, scan and offsets (voxel_engine.h).
//   cloud_segment_kernel : one wave per voxel, templated on the scalar (float32 keyframes, float64 map and lidar): 64 points
//                          are gathered side by side, then every lane adds them in sorted order, one at a time, from
//                          broadcast lanes.  Equal keys are in cloud order because the sort is stable, so this is
//                          `np.add.at`'s and open3d's AccumulatedPoint's order whatever the segment's length.  Colours are
//                          integer sums in 64 bits, so they are reduced across the wave; truncating division by the count.
//   clip                 : cloud_clip_flag_kernel marks the filter's rows with 0 <= z <= max_range, the engine's scan and
//                          rank kernels number them, cloud_gather_kernel moves them.  No host wait of its own.
//   cloud_transform_kernel: pw = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3] in float64 for the map.
//
// The chained keyframe call STORES the organised cloud (16 bytes per pixel, in the call's scratch) instead of recomputing a
// point from its 2-byte depth in the key and segment kernels.  The segment kernel gathers in sorted order, so a recomputed
// point would need its frame's camera and size per gathered row; the stored form gives the bounds, key and segment kernels
// one source for all three entry points, and its traffic (16 B written, 12 + 16 B read per pixel) is small beside the
// radix passes (24 B per pixel and pass).  tools/perf_keyframe_clouds.py prints the split.
//
// Each call waits on the host once, after cloud_meta_kernel: the widest key of the batch and whether any row is missing
// (8 bytes: they select the sort passes), and for a lidar call without host offsets the offsets themselves.
// No float atomics and no sum whose order depends on scheduling: a cloud's bytes are the same alone or in any batch.
#define CLOUD_HD __host__ __device__
#include "common.h"
#include "cloud.h"
#include "voxel_engine.h"

#pragma clang fp contract(off)

template <typename S> __device__ __forceinline__ S cloud_inf();
template <> __device__ __forceinline__ float cloud_inf<float>() { return INFINITY; }
template <> __device__ __forceinline__ double cloud_inf<double>() { return (double)INFINITY; }
__device__ __forceinline__ float cloud_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double cloud_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float cloud_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double cloud_max(double a, double b) { return fmax(a, b); }

template <typename S> __device__ __forceinline__ void cloud_take(S v[CLOUD_NPART], unsigned &miss, S x, S y, S z) {
    if (cloud_finite(x) && cloud_finite(y) && cloud_finite(z)) {
        v[0] = cloud_min(v[0], x); v[1] = cloud_min(v[1], y); v[2] = cloud_min(v[2], z);
        v[3] = cloud_max(v[3], x); v[4] = cloud_max(v[4], y); v[5] = cloud_max(v[5], z);
    } else {
        ++miss;
    }
}

// the workgroup's partial: wave shuffles, then LDS (a minimum does not depend on the order it is taken in)
template <typename S> __device__ __forceinline__ void cloud_reduce_store(S v[CLOUD_NPART], unsigned miss, S *__restrict__ part,
                                                                          uint32_t *__restrict__ part_missing) {
    __shared__ S s_w[CLOUD_BOUNDS_BLOCK / 64][CLOUD_NPART];
    __shared__ unsigned s_m[CLOUD_BOUNDS_BLOCK / 64];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < CLOUD_NPART; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const S u = __shfl_xor(v[k], o, 64);
            v[k] = k < 3 ? cloud_min(v[k], u) : cloud_max(v[k], u);
        }
        if ((t & 63) == 0) s_w[t >> 6][k] = v[k];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) miss += __shfl_xor(miss, o, 64);
    if ((t & 63) == 0) s_m[t >> 6] = miss;
    __syncthreads();
    const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (t < CLOUD_NPART) {
        S a = s_w[0][t];
        for (int w = 1; w < CLOUD_BOUNDS_BLOCK / 64; ++w) a = t < 3 ? cloud_min(a, s_w[w][t]) : cloud_max(a, s_w[w][t]);
        part[slot * CLOUD_NPART + t] = a;
    }
    if (t == CLOUD_NPART) {
        unsigned m = 0;
        for (int w = 0; w < CLOUD_BOUNDS_BLOCK / 64; ++w) m += s_m[w];
        part_missing[slot] = m;
    }
}

template <typename T> struct CloudDepthType;
template <> struct CloudDepthType<uint16_t> { static constexpr int value = CLOUD_DEPTH_U16; };
template <> struct CloudDepthType<float> { static constexpr int value = CLOUD_DEPTH_F32; };

// frame c owns the pixels off[c] .. off[c + 1] - 1 of image (channels bytes each) and depth, hw[c] = (H, W)
template <typename T>
__global__ __launch_bounds__(CLOUD_BOUNDS_BLOCK) void cloud_project_kernel(const uint8_t *__restrict__ image, int channels,
                                                                           const T *__restrict__ depth, const int64_t *__restrict__ off,
                                                                           const int32_t *__restrict__ hw, const double *__restrict__ cam,
                                                                           float *__restrict__ pts, uint32_t *__restrict__ rgb,
                                                                           float *__restrict__ part, uint32_t *__restrict__ part_missing) {
    const int c = blockIdx.y;
    const int64_t i0 = off[c], i1 = off[c + 1];
    const uint32_t W = (uint32_t)hw[2 * c + 1];           // a frame holds fewer than 2^31 pixels: 32-bit division
    const double cam4[4] = {cam[4 * c], cam[4 * c + 1], cam[4 * c + 2], cam[4 * c + 3]};
    float k[4];
    cloud_constants(cam4, CloudDepthType<T>::value, k);
    float v[CLOUD_NPART] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned miss = 0;
    for (int64_t i = i0 + (int64_t)blockIdx.x * CLOUD_BOUNDS_BLOCK + threadIdx.x; i < i1; i += (int64_t)gridDim.x * CLOUD_BOUNDS_BLOCK) {
        const uint32_t p = (uint32_t)(i - i0), row = p / W;
        float q[3];
        cloud_project((int)(p - row * W), (int)row, depth[i], k, q);
        pts[3 * i] = q[0]; pts[3 * i + 1] = q[1]; pts[3 * i + 2] = q[2];
        if (channels == 3) {
            rgb[i] = cloud_pack_rgb(image[3 * i + 2], image[3 * i + 1], image[3 * i]);
        } else {
            const uint32_t g = image[i];
            rgb[i] = cloud_pack_rgb(g, g, g);
        }
        cloud_take(v, miss, q[0], q[1], q[2]);
    }
    cloud_reduce_store(v, miss, part, part_missing);
}

template <typename S>
__global__ __launch_bounds__(CLOUD_BOUNDS_BLOCK) void cloud_bounds_kernel(const S *__restrict__ pts, const int64_t *__restrict__ off,
                                                                          S *__restrict__ part, uint32_t *__restrict__ part_missing) {
    const int c = blockIdx.y;
    // the lidar call may run this before the host has checked the offsets: a negative start reads no row at all
    const int64_t i0 = off[c], i1 = i0 >= 0 ? off[c + 1] : i0;
    S v[CLOUD_NPART] = {cloud_inf<S>(), cloud_inf<S>(), cloud_inf<S>(), -cloud_inf<S>(), -cloud_inf<S>(), -cloud_inf<S>()};
    unsigned miss = 0;
    for (int64_t i = i0 + (int64_t)blockIdx.x * CLOUD_BOUNDS_BLOCK + threadIdx.x; i < i1; i += (int64_t)gridDim.x * CLOUD_BOUNDS_BLOCK)
        cloud_take(v, miss, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    cloud_reduce_store(v, miss, part, part_missing);
}

// per cloud: base[3] and meta = {shift of the rule's most significant axis, shift of iy, key bits, dead};
// head = {widest key, any row missing}
template <typename Rule, typename S = typename Rule::S>
__global__ __launch_bounds__(64) void cloud_meta_kernel(const S *__restrict__ part, const uint32_t *__restrict__ part_missing, int nb,
                                                        int n_clouds, typename Rule::P param, S *__restrict__ base, int *__restrict__ meta,
                                                        int *__restrict__ head, int32_t *__restrict__ status) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_clouds) return;
    S lo[3] = {cloud_inf<S>(), cloud_inf<S>(), cloud_inf<S>()}, hi[3] = {-cloud_inf<S>(), -cloud_inf<S>(), -cloud_inf<S>()};
    uint32_t missing = 0;
    for (int b = 0; b < nb; ++b) {
        const S *p = part + ((int64_t)c * nb + b) * CLOUD_NPART;
        for (int a = 0; a < 3; ++a) { lo[a] = cloud_min(lo[a], p[a]); hi[a] = cloud_max(hi[a], p[3 + a]); }
        missing |= part_missing[(int64_t)c * nb + b];      // no branch: the loads of a thread's whole fold can be in flight together
    }
    int bits[3] = {0, 0, 0}, over = 0;
    S o[3] = {(S)0, (S)0, (S)0};
    if (lo[0] <= hi[0]) over = Rule::range(lo, hi, param, o, bits);           // the cloud has a finite row
    for (int a = 0; a < 3; ++a) base[3 * c + a] = o[a];
    const int kb = over ? 0 : bits[0] + bits[1] + bits[2];
    meta[4 * c] = bits[1] + bits[2 - Rule::MAJOR];
    meta[4 * c + 1] = bits[2 - Rule::MAJOR];
    meta[4 * c + 2] = kb;
    meta[4 * c + 3] = over;
    status[c] = over;
    atomicMax(&head[0], kb);
    if (over || missing) atomicOr(&head[1], 1);
}

template <typename Rule, typename S = typename Rule::S>
__global__ __launch_bounds__(256) void cloud_key_kernel(const S *__restrict__ pts, const int64_t *__restrict__ off, int n_clouds, int64_t n,
                                                        typename Rule::P param, const S *__restrict__ base, const int *__restrict__ meta,
                                                        int invalid_shift,
                                                        uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                        uint16_t *__restrict__ cloud_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_clouds;                             // the last c with off[c] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const int c = lo;
    const S x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    uint64_t key;
    if (cloud_finite(x) && cloud_finite(y) && cloud_finite(z) && !meta[4 * c + 3]) {
        key = Rule::key(Rule::index(x, param, base[3 * c]), Rule::index(y, param, base[3 * c + 1]), Rule::index(z, param, base[3 * c + 2]),
                        meta[4 * c], meta[4 * c + 1]);
    } else {
        key = cloud_shift(1u, invalid_shift & 63);         // the host saw head[1] != 0, so invalid_shift is 0 .. 63 here
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
    cloud_of[i] = (uint16_t)c;
}

// RGB: the cloud has colours (rgb and out_rgb are null without)
template <typename S, bool RGB>
__global__ __launch_bounds__(VOXEL_SEG_BLOCK) void cloud_segment_kernel(const S *__restrict__ pts, const uint32_t *__restrict__ rgb,
                                                                        const uint32_t *__restrict__ idx,
                                                                        const uint32_t *__restrict__ seg_start,
                                                                        const uint32_t *__restrict__ seg_end,
                                                                        const uint32_t *__restrict__ rows, S *__restrict__ out,
                                                                        uint32_t *__restrict__ out_rgb, int32_t *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (VOXEL_SEG_BLOCK / 64);
    const int64_t n_rows = *rows;
    for (int64_t r = (int64_t)blockIdx.x * (VOXEL_SEG_BLOCK / 64) + (threadIdx.x >> 6); r < n_rows; r += nw) {
        const int64_t s = seg_start[r], e = seg_end[r];
        S ax = (S)0, ay = (S)0, az = (S)0;
        unsigned long long cr = 0, cg = 0, cb = 0;         // this lane's share of the integer sums
        for (int64_t c0 = s; c0 < e; c0 += 64) {
            const int m = (int)(e - c0 < 64 ? e - c0 : 64);
            S x = (S)0, y = (S)0, z = (S)0;
            if (lane < m) {
                const int64_t i = idx[c0 + lane];
                x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
                if (RGB) {
                    const uint32_t w = rgb[i];
                    cr += w & 255u; cg += (w >> 8) & 255u; cb += (w >> 16) & 255u;
                }
            }
            for (int q = 0; q < m; ++q) {                  // every lane adds the same points in the same order
                ax = ax + __shfl(x, q, 64);
                ay = ay + __shfl(y, q, 64);
                az = az + __shfl(z, q, 64);
            }
        }
        if (RGB) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                cr += __shfl_xor(cr, o, 64); cg += __shfl_xor(cg, o, 64); cb += __shfl_xor(cb, o, 64);
            }
        }
        if (lane == 0) {
            const S cnt = (S)(e - s);
            out[3 * r] = ax / cnt;
            out[3 * r + 1] = ay / cnt;
            out[3 * r + 2] = az / cnt;
            const unsigned long long k = (unsigned long long)(e - s);
            if (RGB) out_rgb[r] = cloud_pack_rgb((uint32_t)(cr / k), (uint32_t)(cg / k), (uint32_t)(cb / k));
            if (counts) counts[r] = (int32_t)(e - s);
        }
    }
}

// flags[j] of the filter's row j: 1 = kept, 2 = dropped or no row (j >= *rows); kept rows per workgroup
__global__ __launch_bounds__(VOXEL_FLAG_BLOCK) void cloud_clip_flag_kernel(const float *__restrict__ mid, const uint32_t *__restrict__ rows,
                                                                           int64_t n, float max_range, uint8_t *__restrict__ flags,
                                                                           uint32_t *__restrict__ tile_count) {
    __shared__ unsigned s_n;
    const int t = threadIdx.x;
    if (t == 0) s_n = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * VOXEL_FLAG_BLOCK + t;
    bool keep = false;
    if (j < n) {
        keep = j < (int64_t)*rows && cloud_clip_keep(mid[3 * j + 2], max_range);
        flags[j] = keep ? 1 : 2;
    }
    const unsigned long long m = __ballot(keep);
    if ((t & 63) == 0 && m) atomicAdd(&s_n, (unsigned)__popcll(m));
    __syncthreads();
    if (t == 0) tile_count[blockIdx.x] = s_n;
}

__global__ __launch_bounds__(256) void cloud_gather_kernel(const uint32_t *__restrict__ src, const uint32_t *__restrict__ kept,
                                                           const float *__restrict__ mid, const uint32_t *__restrict__ mid_rgb,
                                                           const int32_t *__restrict__ mid_counts, float *__restrict__ out,
                                                           uint32_t *__restrict__ out_rgb, int32_t *__restrict__ out_counts) {
    const int64_t m = *kept;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < m; r += (int64_t)gridDim.x * 256) {
        const int64_t j = src[r];
        out[3 * r] = mid[3 * j]; out[3 * r + 1] = mid[3 * j + 1]; out[3 * r + 2] = mid[3 * j + 2];
        if (out_rgb) out_rgb[r] = mid_rgb[j];
        if (out_counts) out_counts[r] = mid_counts[j];
    }
}

// row i of keyframe c (off[c] <= i < off[c + 1]) under pose c (row-major 4 x 4); a non-finite row becomes three NaNs
template <typename T>
__global__ __launch_bounds__(256) void cloud_transform_kernel(const T *__restrict__ pts, const int64_t *__restrict__ off, int n_kf, int64_t n,
                                                              const double *__restrict__ poses, double *__restrict__ pw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_kf;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const double *Tm = poses + 16 * (int64_t)lo;
    const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
    const bool ok = cloud_finite(x) && cloud_finite(y) && cloud_finite(z);
    for (int r = 0; r < 3; ++r)
        pw[3 * i + r] = ok ? ((Tm[4 * r] * x + Tm[4 * r + 1] * y) + Tm[4 * r + 2] * z) + Tm[4 * r + 3] : (double)NAN;
}

__global__ void cloud_pair_kernel(int64_t *__restrict__ one_off, int64_t n) {
    one_off[0] = 0;
    one_off[1] = n;
}

// ---- host side ---------------------------------------------------------------------------------
// one pair for every entry point: launches on one stream are ordered, and a scratch is per (device, stream)
static StreamScratch g_cloud_head_scratch, g_cloud_scratch;

// Stage times of the last call of one family of entry points: the lidar calls for tools/perf_voxel.py
// (cslam_voxel_profile), the cloud and map calls for tools/perf_keyframe_clouds.py (cslam_cloud_profile).
struct FilterProfile {
    enum { EV = 8 };                                       // begin, project / bounds + meta | wait | keys | sort | heads | segments | clip
    const char *const how;                                 // what read() says when no profiled call was made
    std::mutex mu;
    bool on = false, have = false, made = false;
    hipEvent_t ev[EV] = {};
    int info[4] = {0, 0, 0, 0};
    explicit FilterProfile(const char *how_) : how(how_) {}

    int enable(int enable) {
        std::lock_guard<std::mutex> lock(mu);
        on = enable != 0;
        have = false;
        return CSLAM_OK;
    }
    int begin(bool *prof) {                                // a call starts: is it profiled?
        std::lock_guard<std::mutex> lock(mu);
        *prof = on;
        if (on && !made) {
            for (int k = 0; k < EV; ++k) HIP_TRY(hipEventCreate(&ev[k]));
            made = true;
        }
        have = false;
        return CSLAM_OK;
    }
    void mark(bool prof, int k, hipStream_t st) {
        if (prof) (void)hipEventRecord(ev[k], st);
    }
    void end(const VoxelPlan &pl) {
        std::lock_guard<std::mutex> lock(mu);
        info[0] = pl.key_passes;
        info[1] = pl.cloud_passes;
        info[2] = pl.key_bits;
        info[3] = (int)pl.tiles;
        have = true;
    }
    int read(double *ms, int count, int32_t *info_out) {   // the first `count` intervals
        ARG_CHECK(ms && info_out, "NULL argument");
        std::lock_guard<std::mutex> lock(mu);
        ARG_CHECK(have, how);
        HIP_TRY(hipEventSynchronize(ev[count]));
        for (int k = 0; k < count; ++k) {
            float f = 0.f;
            HIP_TRY(hipEventElapsedTime(&f, ev[k], ev[k + 1]));
            ms[k] = f;
        }
        for (int k = 0; k < 4; ++k) info_out[k] = info[k];
        return CSLAM_OK;
    }
};
static FilterProfile g_vox_prof("no profiled call: cslam_voxel_profile(1), then cslam_voxel_downsample_dev");
static FilterProfile g_cloud_prof("no profiled call: cslam_cloud_profile(1), then a cloud or map call");

// the shared offsets rule and the one limit of the sort
static int cloud_shape(const int64_t *off, int n_clouds, RaggedShape *s) {
    int rc = offsets_check(off, n_clouds, s);
    if (rc) return rc;
    ARG_CHECK(s->total <= VOXEL_MAX_POINTS, "more points than an int32 index addresses");
    return CSLAM_OK;
}

// frame c holds hw[c] = (H, W) pixels, both at least 1, and its offsets say the same
static int cloud_frames_shape(const int64_t *off, const int32_t *hw, int n, RaggedShape *s) {
    int rc = cloud_shape(off, n, s);
    if (rc) return rc;
    for (int c = 0; c < n; ++c) {
        ARG_CHECK(hw[2 * c] >= 1 && hw[2 * c + 1] >= 1, "a frame is at least 1 x 1");
        ARG_CHECK((int64_t)hw[2 * c] * hw[2 * c + 1] == off[c + 1] - off[c], "the pixel offsets do not match the frame sizes");
    }
    return CSLAM_OK;
}

// What a filter call is made of besides its rule: whose profile it is, the name its errors carry, its clouds, the clip of
// the keyframe filter, the caller's colours and the outputs.  `n` = the rows of all clouds, from host offsets the entry
// point has checked; where it has none (the lidar call allows that), `d_unread_off` = the device offsets, which the run
// reads back before its one wait and checks after it, and n is not used.  `n_store` = the rows the head block keeps.
template <typename S> struct FilterCall {
    FilterProfile *prof;
    const char *name;
    int n_clouds;
    int64_t n, n_store;
    const int64_t *d_unread_off;
    bool clip;
    float max_range;
    const uint32_t *d_rgb_in;
    bool rgb_stored;                                       // the colours are the head block's (the chain), not the caller's
    S *d_out;
    uint32_t *d_out_rgb;
    int32_t *d_counts;
    int64_t *d_out_offsets;
    int32_t *d_status;
};

// The filter behind every entry point: bounds to segments, written once.  `produce(h, nb, &pts, &eng_off)` launches what
// fills h.part / h.part_missing for the clouds and says which rows and offsets the engine reads.  With `clip` the filter's
// rows go to h.mid* and the kept ones to the outputs; without, straight to the outputs.
template <typename Rule, typename Produce>
static int cloud_filter_run(const FilterCall<typename Rule::S> &f, typename Rule::P param, hipStream_t st, Produce produce) {
    typedef typename Rule::S S;
    const int n_clouds = f.n_clouds;
    const bool clip = f.clip;
    FilterProfile &pf = *f.prof;
    int rc;
    bool prof;
    if ((rc = pf.begin(&prof))) return rc;
    // before the wait: everything whose launch shape depends on n_clouds alone (and on n where the host knows it)
    const int nb = cloud_bounds_blocks(n_clouds);
    CloudHead<S> h;
    auto head_layout = [&](Carver &cv) { cloud_head_layout<S>(cv, n_clouds, nb, f.n_store, clip ? f.n : 0, &h); };
    SCRATCH_CARVE(g_cloud_head_scratch, st, (size_t)1 << 16, head_layout);
    pf.mark(prof, 0, st);
    HIP_TRY(hipMemsetAsync(h.head, 0, 8, st));
    const S *pts = nullptr;
    const int64_t *eng_off = nullptr;
    if ((rc = produce(h, nb, &pts, &eng_off))) return rc;
    const uint32_t *rgb = f.rgb_stored ? h.rgb : f.d_rgb_in;
    hipLaunchKernelGGL(cloud_meta_kernel<Rule>, dim3((unsigned)ceil_div64(n_clouds, 64)), dim3(64), 0, st, h.part, h.part_missing, nb, n_clouds,
                       param, h.base, h.meta, h.head, f.d_status);
    pf.mark(prof, 1, st);
    int h_head[2] = {0, 0};
    std::vector<int64_t> read_off;
    HIP_TRY(hipMemcpyAsync(h_head, h.head, 8, hipMemcpyDeviceToHost, st));
    if (f.d_unread_off && (rc = read_back_async(read_off, f.d_unread_off, (size_t)n_clouds + 1, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));                     // the one host wait
    RaggedShape sh = {};
    if (f.d_unread_off && (rc = cloud_shape(read_off.data(), n_clouds, &sh))) return rc;
    const int64_t n = f.d_unread_off ? sh.total : f.n;
    VoxelPlan pl;
    if (voxel_make_plan(n, n_clouds, h_head[0], h_head[1], nullptr, &pl)) {
        cslam_set_error("%s: sizes outside the plan's limits", f.name);
        return CSLAM_E_INVALID;
    }
    pf.mark(prof, 2, st);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(f.d_out_offsets, 0, ((size_t)n_clouds + 1) * 8, st));
        for (int k = 3; k < FilterProfile::EV; ++k) pf.mark(prof, k, st);
    } else {
        SCRATCH_HERE(base, g_cloud_scratch, st, pl.bytes, (size_t)1 << 20);
        voxel_make_plan(n, n_clouds, h_head[0], h_head[1], base, &pl);     // the same plan, placed
        hipLaunchKernelGGL(cloud_key_kernel<Rule>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, pts, eng_off, n_clouds, n, param, h.base,
                           h.meta, pl.invalid_shift, pl.keys[0], pl.idx[0], pl.cloud_of);
        pf.mark(prof, 3, st);
        int cur = 0;
        if ((rc = voxel_engine_sort_heads(&pl, eng_off, n_clouds, clip ? h.mid_off : f.d_out_offsets, prof ? pf.ev[4] : nullptr, st, &cur)))
            return rc;
        pf.mark(prof, 5, st);
        const int64_t want = ceil_div64(n, VOXEL_SEG_BLOCK / 64);
        const int64_t cap = (int64_t)(cslam_cu_count() > 0 ? cslam_cu_count() : 256) * 8;
        const auto segment_kernel = rgb ? cloud_segment_kernel<S, true> : cloud_segment_kernel<S, false>;
        hipLaunchKernelGGL(segment_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(VOXEL_SEG_BLOCK), 0, st, pts, rgb, pl.idx[cur],
                           pl.seg_start, pl.seg_end, pl.rows, clip ? h.mid : f.d_out, clip ? h.mid_rgb : f.d_out_rgb,
                           clip ? h.mid_counts : f.d_counts);
        pf.mark(prof, 6, st);
        if (clip) {                                        // the segment kernel is done with flags, rank and the segment ends
            hipLaunchKernelGGL(cloud_clip_flag_kernel, dim3((unsigned)pl.flag_tiles), dim3(VOXEL_FLAG_BLOCK), 0, st, (const float *)h.mid,
                               pl.rows, n, f.max_range, pl.flags, pl.tile_count);
            if ((rc = voxel_engine_compact(pl.flags, n, pl.tile_count, h.kept, pl.rank, pl.seg_start, pl.seg_end, h.mid_off, n_clouds,
                                           f.d_out_offsets, st)))
                return rc;
            const int64_t blocks = ceil_div64(n, 256);
            hipLaunchKernelGGL(cloud_gather_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, st, pl.seg_start, h.kept,
                               (const float *)h.mid, rgb ? h.mid_rgb : nullptr, h.mid_counts, (float *)f.d_out, rgb ? f.d_out_rgb : nullptr,
                               f.d_counts);
        }
        pf.mark(prof, 7, st);
    }
    HIP_TRY(hipGetLastError());
    if (prof) pf.end(pl);
    return CSLAM_OK;
}

// `produce` for clouds that are the caller's own rows: their bounds, and the engine reads them where they are
template <typename S> static auto cloud_own_rows(const S *d_points, const int64_t *d_offsets, int n_clouds, hipStream_t st) {
    return [=](CloudHead<S> &h, int nb, const S **pts, const int64_t **eng_off) {
        hipLaunchKernelGGL(cloud_bounds_kernel<S>, dim3((unsigned)nb, (unsigned)n_clouds), dim3(CLOUD_BOUNDS_BLOCK), 0, st, d_points, d_offsets,
                           h.part, h.part_missing);
        *pts = d_points;
        *eng_off = d_offsets;
        return CSLAM_OK;
    };
}

template <typename... A>
static void cloud_launch_project(int depth_type, dim3 grid, hipStream_t st, const uint8_t *image, int channels, const void *depth, A... rest) {
    if (depth_type == CLOUD_DEPTH_U16)
        hipLaunchKernelGGL(cloud_project_kernel<uint16_t>, grid, dim3(CLOUD_BOUNDS_BLOCK), 0, st, image, channels, (const uint16_t *)depth, rest...);
    else
        hipLaunchKernelGGL(cloud_project_kernel<float>, grid, dim3(CLOUD_BOUNDS_BLOCK), 0, st, image, channels, (const float *)depth, rest...);
}

#define CLOUD_FRAME_CHECKS()                                                                                     \
    BATCH_COUNT_CHECK(n_frames);                                                                                 \
    ARG_CHECK(depth_type == CLOUD_DEPTH_U16 || depth_type == CLOUD_DEPTH_F32, "depth_type must be 0 (uint16) or 1 (float32)"); \
    ARG_CHECK(channels == 1 || channels == 3, "channels must be 1 or 3");                                        \
    ARG_CHECK(d_image && d_depth && d_offsets && d_hw && d_cam && h_offsets && h_hw, "NULL argument");           \
    RaggedShape sh = {};                                                                                         \
    if (int rc_ = cloud_frames_shape(h_offsets, h_hw, n_frames, &sh)) return rc_

CSLAM_API int cslam_cloud_from_depth_dev(const uint8_t *d_image, int channels, const void *d_depth, int depth_type,
                                         const int64_t *d_offsets, const int32_t *d_hw, const double *d_cam, int n_frames,
                                         float *d_points, uint32_t *d_rgb, const int64_t *h_offsets, const int32_t *h_hw, void *stream) {
    CLOUD_FRAME_CHECKS();
    ARG_CHECK(d_points && d_rgb, "NULL argument");
    PTR_DEVICE(d_offsets);
    hipStream_t st = (hipStream_t)stream;
    const int nb = cloud_bounds_blocks(n_frames);
    CloudHead<float> h;
    auto head_layout = [&](Carver &cv) { cloud_head_layout<float>(cv, n_frames, nb, 0, 0, &h); };
    SCRATCH_CARVE(g_cloud_head_scratch, st, (size_t)1 << 16, head_layout);
    cloud_launch_project(depth_type, dim3((unsigned)nb, (unsigned)n_frames), st, d_image, channels, d_depth, d_offsets, d_hw, d_cam, d_points,
                         d_rgb, h.part, h.part_missing);                   // the partials are not read here
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

#define CLOUD_LEAF_CHECKS()                                                                                      \
    ARG_CHECK(leaf > 0.0 && leaf < INFINITY, "voxel must be positive and finite");                               \
    ARG_CHECK(max_range >= 0.0, "max_range must not be negative or NaN")

CSLAM_API int cslam_cloud_voxel_dev(const float *d_points, const uint32_t *d_rgb, const int64_t *d_offsets, int n_clouds, double leaf,
                                    double max_range, float *d_out, uint32_t *d_out_rgb, int32_t *d_counts, int64_t *d_out_offsets,
                                    int32_t *d_status, const int64_t *h_offsets, void *stream) {
    CLOUD_LEAF_CHECKS();
    BATCH_COUNT_CHECK(n_clouds);
    ARG_CHECK(d_offsets && d_out_offsets && d_status && h_offsets, "NULL argument");
    RaggedShape sh = {};
    if (int rc = cloud_shape(h_offsets, n_clouds, &sh)) return rc;
    ARG_CHECK((d_points && d_out && (!d_rgb || d_out_rgb)) || sh.total == 0, "NULL argument");
    PTR_DEVICE(d_offsets);
    hipStream_t st = (hipStream_t)stream;
    const FilterCall<float> f = {&g_cloud_prof, "cloud filter", n_clouds, sh.total, 0, nullptr, true, (float)max_range, d_rgb, false,
                                 d_out, d_out_rgb, d_counts, d_out_offsets, d_status};
    return cloud_filter_run<GridPcl>(f, 1.0f / (float)leaf, st, cloud_own_rows(d_points, d_offsets, n_clouds, st));
}

// Lidar keyframes: open3d's rule in float64 on the caller's own rows, no clip and no colours.  The one entry point that may
// come without host offsets: the bounds pass then runs on offsets nobody has checked (cloud_bounds_kernel's guard), and
// the run reads them back before its one wait and checks them after it.
CSLAM_API int cslam_voxel_downsample_dev(const double *d_points, const int64_t *d_offsets, int n_clouds, double voxel,
                                         double *d_out, int64_t *d_out_offsets, int32_t *d_counts, int32_t *d_status,
                                         const int64_t *h_offsets, void *stream) {
    ARG_CHECK(voxel > 0.0 && voxel < INFINITY, "voxel must be positive and finite");
    BATCH_COUNT_CHECK(n_clouds);
    ARG_CHECK(d_offsets && d_out_offsets && d_status, "NULL argument");
    RaggedShape sh = {};
    if (h_offsets)
        if (int rc = cloud_shape(h_offsets, n_clouds, &sh)) return rc;
    ARG_CHECK((d_points && d_out) || (h_offsets && sh.total == 0), "NULL argument");
    PTR_DEVICE(d_offsets);
    hipStream_t st = (hipStream_t)stream;
    const FilterCall<double> f = {&g_vox_prof, "voxel down-sampling", n_clouds, sh.total, 0, h_offsets ? nullptr : d_offsets, false, 0.0f,
                                  nullptr, false, d_out, nullptr, d_counts, d_out_offsets, d_status};
    return cloud_filter_run<GridOpen3d>(f, GridOpen3dParam{voxel, voxel / 2.0}, st, cloud_own_rows(d_points, d_offsets, n_clouds, st));
}

CSLAM_API int cslam_cloud_keyframes_dev(const uint8_t *d_image, int channels, const void *d_depth, int depth_type,
                                        const int64_t *d_offsets, const int32_t *d_hw, const double *d_cam, int n_frames, double leaf,
                                        double max_range, float *d_out, uint32_t *d_out_rgb, int32_t *d_counts, int64_t *d_out_offsets,
                                        int32_t *d_status, const int64_t *h_offsets, const int32_t *h_hw, void *stream) {
    CLOUD_LEAF_CHECKS();
    CLOUD_FRAME_CHECKS();
    ARG_CHECK(d_out && d_out_rgb && d_out_offsets && d_status, "NULL argument");
    PTR_DEVICE(d_offsets);
    hipStream_t st = (hipStream_t)stream;
    auto produce = [&](CloudHead<float> &h, int nb, const float **pts, const int64_t **eng_off) {
        cloud_launch_project(depth_type, dim3((unsigned)nb, (unsigned)n_frames), st, d_image, channels, d_depth, d_offsets, d_hw, d_cam, h.pts,
                             h.rgb, h.part, h.part_missing);
        *pts = h.pts;
        *eng_off = d_offsets;
        return CSLAM_OK;
    };
    const FilterCall<float> f = {&g_cloud_prof, "cloud filter", n_frames, sh.total, sh.total, nullptr, true, (float)max_range, nullptr, true,
                                 d_out, d_out_rgb, d_counts, d_out_offsets, d_status};
    return cloud_filter_run<GridPcl>(f, 1.0f / (float)leaf, st, produce);
}

CSLAM_API int cslam_map_assemble_dev(const void *d_points, int dtype, const uint32_t *d_rgb, const int64_t *d_offsets, const double *d_poses,
                                     int n_keyframes, double voxel, double *d_out, uint32_t *d_out_rgb, int32_t *d_counts,
                                     int64_t *d_out_offsets, int32_t *d_status, const int64_t *h_offsets, void *stream) {
    ARG_CHECK(voxel > 0.0 && voxel < INFINITY, "voxel must be positive and finite");
    ARG_CHECK(dtype == CSLAM_F32 || dtype == CSLAM_F64, "dtype must be CSLAM_F32 or CSLAM_F64");
    BATCH_COUNT_CHECK(n_keyframes);
    ARG_CHECK(d_offsets && d_poses && d_out_offsets && d_status && h_offsets, "NULL argument");
    RaggedShape sh = {};
    if (int rc = cloud_shape(h_offsets, n_keyframes, &sh)) return rc;
    ARG_CHECK((d_points && d_out && (!d_rgb || d_out_rgb)) || sh.total == 0, "NULL argument");
    PTR_DEVICE(d_offsets);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = sh.total;
    auto produce = [&](CloudHead<double> &h, int nb, const double **pts, const int64_t **eng_off) {
        hipLaunchKernelGGL(cloud_pair_kernel, dim3(1), dim3(1), 0, st, h.one_off, n);
        if (n > 0) {
            const dim3 grid((unsigned)ceil_div64(n, 256));
            if (dtype == CSLAM_F32)
                hipLaunchKernelGGL(cloud_transform_kernel<float>, grid, dim3(256), 0, st, (const float *)d_points, d_offsets, n_keyframes, n,
                                   d_poses, h.pts);
            else
                hipLaunchKernelGGL(cloud_transform_kernel<double>, grid, dim3(256), 0, st, (const double *)d_points, d_offsets, n_keyframes, n,
                                   d_poses, h.pts);
        }
        hipLaunchKernelGGL(cloud_bounds_kernel<double>, dim3((unsigned)nb, 1u), dim3(CLOUD_BOUNDS_BLOCK), 0, st, (const double *)h.pts, h.one_off,
                           h.part, h.part_missing);
        *pts = h.pts;
        *eng_off = h.one_off;
        return CSLAM_OK;
    };
    // the whole map is one cloud of the engine: its rows are the keyframes' rows in keyframe order
    const FilterCall<double> f = {&g_cloud_prof, "cloud filter", 1, n, n, nullptr, false, 0.0f, d_rgb, false,
                                  d_out, d_out_rgb, d_counts, d_out_offsets, d_status};
    return cloud_filter_run<GridMap>(f, voxel, st, produce);
}

// the lidar read reports the first six intervals: that call has no clip
CSLAM_API int cslam_voxel_profile(int enable) { return g_vox_prof.enable(enable); }
CSLAM_API int cslam_voxel_profile_read(double ms[6], int32_t info[4]) { return g_vox_prof.read(ms, 6, info); }
CSLAM_API int cslam_cloud_profile(int enable) { return g_cloud_prof.enable(enable); }
CSLAM_API int cslam_cloud_profile_read(double ms[7], int32_t info[4]) { return g_cloud_prof.read(ms, 7, info); }
