// The arithmetic rules of cloud.hip, once: the back-projection of a depth pixel, the three grid rules of the voxel filters
// (PCL's for keyframe clouds, the map's, open3d's for lidar clouds) with the one key packing they share, the colour
// packing, and how the call's first scratch block is carved.  Plain C++ without HIP (the kernels
// include it with CLOUD_HD = __host__ __device__), so that the host tests compile the very same functions and a
// stand-alone program runs them under host sanitizers.  Every float operation is written once and nothing is contracted.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include "ragged.h"
#include "voxel_plan.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifndef CLOUD_HD
#define CLOUD_HD
#endif

#define CLOUD_DEPTH_U16 0        // uint16 millimetres
#define CLOUD_DEPTH_F32 1        // float32 metres
#define CLOUD_BOUNDS_BLOCK 256   // threads per workgroup of the projection and bounds kernels
#define CLOUD_NPART 6            // min[3], max[3] of a workgroup's rows; the missing rows are counted beside them
#define CLOUD_CELL_LIMIT 2147483648.0   // a cell number of this magnitude or more does not fit PCL's int

// (cx_f, cy_f, kx, ky) of a camera (fx, fy, cx, cy): depth_image_to_pointcloud's center_x / constant_x, where the unit of a
// uint16 depth is folded into the constant (double(float(1) * float(0.001)) / fx, rounded to float once)
CLOUD_HD static inline void cloud_constants(const double cam[4], int depth_type, float k[4]) {
    const double unit = depth_type == CLOUD_DEPTH_U16 ? (double)(1.0f * 0.001f) : 1.0;
    k[0] = (float)cam[2];
    k[1] = (float)cam[3];
    k[2] = (float)(unit / cam[0]);
    k[3] = (float)(unit / cam[1]);
}

CLOUD_HD static inline bool cloud_depth_valid(uint16_t d) { return d != 0; }
CLOUD_HD static inline bool cloud_depth_valid(float d) { return fabsf(d) <= 3.4028234663852886e38f; }   // isfinite: 0 and below are valid
CLOUD_HD static inline float cloud_depth_metres(uint16_t d) { return (float)d * 0.001f; }
CLOUD_HD static inline float cloud_depth_metres(float d) { return d; }

// the point of pixel (u, v) with depth d; three NaNs for an invalid depth
template <typename T> CLOUD_HD static inline void cloud_project(int u, int v, T d, const float k[4], float p[3]) {
    if (!cloud_depth_valid(d)) {
        p[0] = p[1] = p[2] = NAN;
        return;
    }
    const float df = (float)d;
    p[0] = (((float)u - k[0]) * df) * k[2];
    p[1] = (((float)v - k[1]) * df) * k[3];
    p[2] = cloud_depth_metres(d);
}

// colours travel as one uint32 per point: r | g << 8 | b << 16
CLOUD_HD static inline uint32_t cloud_pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

CLOUD_HD static inline bool cloud_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }
CLOUD_HD static inline bool cloud_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// The cell of a coordinate.  Keyframe filter (float): floor(p * inv) with inv = 1.0f / leaf, PCL VoxelGrid's rule.  Map
// (double): floor(p / voxel) with a true division, a grid anchored at the world origin.  `scale` is inv or voxel.
CLOUD_HD static inline float cloud_cell(float p, float scale) { return floorf(p * scale); }
CLOUD_HD static inline double cloud_cell(double p, double scale) { return floor(p / scale); }

// What the bounds of a cloud give: base[a] = the cell of the minimum (PCL's min_b as a float, exact below 2^31), bits[a] =
// the bits the largest index needs.  Returns 1 (the cloud's status) for a non-finite cell, a cell of magnitude 2^31 or
// more, or an index of 2^21 or more.  The index of the maximum is the largest index: every step is monotone.
template <typename S> CLOUD_HD static inline int cloud_axis_range(const S lo[3], const S hi[3], S scale, S base[3], int bits[3]) {
    int over = 0;
    for (int a = 0; a < 3; ++a) {
        base[a] = (S)0;
        bits[a] = 0;
    }
    for (int a = 0; a < 3; ++a) {
        const S c0 = cloud_cell(lo[a], scale), c1 = cloud_cell(hi[a], scale);
        if (!(cloud_finite(c0) && cloud_finite(c1) && (double)c0 > -CLOUD_CELL_LIMIT && (double)c0 < CLOUD_CELL_LIMIT)) {
            over = 1;
            continue;
        }
        base[a] = c0;
        const S q = c1 - c0;
        if (!(q >= (S)0 && q < (S)(1 << VOXEL_AXIS_BITS))) {
            over = 1;
            continue;
        }
        int b = 0;
        for (uint32_t w = (uint32_t)q; w; w >>= 1) ++b;
        bits[a] = b;
    }
    return over;
}

// index of a coordinate inside its cloud: below 2^21 for every finite row of a cloud with status 0
// (through int32, as PCL's static_cast<int> does: exact, and one hardware conversion)
template <typename S> CLOUD_HD static inline uint32_t cloud_index(S p, S scale, S base) {
    return (uint32_t)(int32_t)(cloud_cell(p, scale) - base);
}

// x << s for 0 <= s < 64, from 32-bit shifts only: v_lshlrev_b32 and v_lshrrev_b32, wherever the allocator puts the amount.
// Written as a 64-bit shift by a per-lane amount, a key kernel of 16 VGPRs compiled to `v_lshlrev_b64 v[6:7], v15, v[10:11]`.
// For gfx90a the same compiler wraps exactly that instruction in `v_swap_b32 v0, v15` (its guard for a 64-bit shift whose
// amount sits in the last register of an 8-register block); for gfx950 it emits it bare, and on an MI355X some waves then
// packed iy with a shift of 0 (tools/probe_shift64.hip shows the instruction alone).  Which register holds the amount is
// the allocator's choice, so EVERY key of every rule is packed by this function: no key kernel shifts 64 bits by a
// per-lane amount.
CLOUD_HD static inline uint64_t cloud_shift(uint32_t x, int s) {
    const uint32_t lo = s < 32 ? x << s : 0u;
    const uint32_t hi = s == 0 ? 0u : (s < 32 ? x >> (32 - s) : x << (s - 32));
    return ((uint64_t)hi << 32) | lo;
}

// iz most significant: ascending key = ascending (iz, iy, ix), the order of PCL's linear index
CLOUD_HD static inline uint64_t cloud_key(uint32_t ix, uint32_t iy, uint32_t iz, int shift_y, int shift_z) {
    return cloud_shift(iz, shift_z) | cloud_shift(iy, shift_y) | ix;
}

// ---- the three grid rules, as the kernels take them ---------------------------------------------------------------
// A rule names its scalar S and its parameter P, the most significant axis of its key (MAJOR: the shift of that axis is
// meta[0] = bits[1] + bits[2 - MAJOR], the shift of y is meta[1] = bits[2 - MAJOR]), and
//   range(lo, hi, param, base, bits): what the bounds of a cloud give, returning the cloud's status
//   index(p, param, base)           : the index of a coordinate, below 2^21 for every finite row of a cloud with status 0
//   key(ix, iy, iz, shift_major, shift_y)
template <typename T> struct GridCells {                   // cloud_cell above in either precision: base = the cell of the minimum
    typedef T S;
    typedef T P;
    static constexpr int MAJOR = 2;
    CLOUD_HD static inline int range(const T lo[3], const T hi[3], T scale, T base[3], int bits[3]) {
        return cloud_axis_range(lo, hi, scale, base, bits);
    }
    CLOUD_HD static inline uint32_t index(T p, T scale, T base) { return cloud_index(p, scale, base); }
    CLOUD_HD static inline uint64_t key(uint32_t ix, uint32_t iy, uint32_t iz, int shift_major, int shift_y) {
        return cloud_key(ix, iy, iz, shift_y, shift_major);
    }
};
typedef GridCells<float> GridPcl;                          // keyframe filter: floorf(p * inv), param = inv = 1.0f / leaf
typedef GridCells<double> GridMap;                         // swarm map: floor(p / voxel), param = voxel

// Lidar down-sampling, open3d's voxel_down_sample: base = origin = min - voxel / 2 (the half is computed on the host),
// index = floor((p - origin) / voxel) with a true division, x most significant.  The index of the maximum is the largest
// index (every step is monotone); status 1 when it is not in [0, 2^21), which includes a NaN or infinite quotient.
struct GridOpen3dParam { double voxel, half; };
struct GridOpen3d {
    typedef double S;
    typedef GridOpen3dParam P;
    static constexpr int MAJOR = 0;
    CLOUD_HD static inline double cell(double p, double voxel, double origin) { return floor((p - origin) / voxel); }
    CLOUD_HD static inline int range(const double lo[3], const double hi[3], P g, double base[3], int bits[3]) {
        int over = 0;
        for (int a = 0; a < 3; ++a) {
            base[a] = lo[a] - g.half;
            bits[a] = 0;
            const double q = cell(hi[a], g.voxel, base[a]);
            if (!(q >= 0.0 && q < (double)(1 << VOXEL_AXIS_BITS))) {
                over = 1;
                continue;
            }
            for (uint32_t w = (uint32_t)q; w; w >>= 1) ++bits[a];
        }
        return over;
    }
    CLOUD_HD static inline uint32_t index(double p, P g, double base) { return (uint32_t)(int32_t)cell(p, g.voxel, base); }
    CLOUD_HD static inline uint64_t key(uint32_t ix, uint32_t iy, uint32_t iz, int shift_major, int shift_y) {
        return cloud_key(iz, iy, ix, shift_y, shift_major);      // the same packing with x and z exchanged
    }
};

// clip of the keyframe filter's rows: PassThrough on z with limits [0, max_range], both ends kept
CLOUD_HD static inline bool cloud_clip_keep(float z, float max_range) { return 0.0f <= z && z <= max_range; }

// workgroups per cloud of the projection and bounds kernels: about 2048 in all, 64 at the most.  One frame or the whole map
// therefore runs this stage on 64 workgroups; with 512 the kernel is shorter but cloud_meta_kernel, which folds a cloud's
// partials in one thread, takes longer than that saves (one 480 x 640 frame: 39 us with 64, 91 us with 512, measured).
#define CLOUD_BOUNDS_MAX_BLOCKS 64
static inline int cloud_bounds_blocks(int n_clouds) {
    const int nb = 2048 / (n_clouds < 1 ? 1 : n_clouds);
    return nb < 1 ? 1 : (nb > CLOUD_BOUNDS_MAX_BLOCKS ? CLOUD_BOUNDS_MAX_BLOCKS : nb);
}

// The first scratch block of a call, carved before the host wait.  S = float for keyframes, double for the map.
// n_pts = the rows the block keeps (the organised cloud of the chain, the transformed rows of the map; 0 when the caller's
// own rows are read), n_mid = the rows of the unclipped filter output (0 for the map, which has no clip).
template <typename S> struct CloudHead {
    S *pts, *part, *base, *mid;
    uint32_t *rgb, *part_missing, *mid_rgb, *kept;
    int32_t *mid_counts;
    int64_t *one_off, *mid_off;
    int *meta, *head;
    size_t bytes;
};

template <typename S> static inline void cloud_head_layout(Carver &cv, int n_clouds, int nb, int64_t n_pts, int64_t n_mid, CloudHead<S> *h) {
    h->pts = cv.take<S>((size_t)n_pts * 3);
    h->rgb = cv.take<uint32_t>((size_t)n_pts);
    h->part = cv.take<S>((size_t)n_clouds * nb * CLOUD_NPART);
    h->part_missing = cv.take<uint32_t>((size_t)n_clouds * nb);
    h->base = cv.take<S>((size_t)n_clouds * 3);
    h->meta = cv.take<int>((size_t)n_clouds * 4);
    h->head = cv.take<int>(2);
    h->kept = cv.take<uint32_t>(1);
    h->one_off = cv.take<int64_t>(2);
    h->mid = cv.take<S>((size_t)n_mid * 3);
    h->mid_rgb = cv.take<uint32_t>((size_t)n_mid);
    h->mid_counts = cv.take<int32_t>((size_t)n_mid);
    h->mid_off = cv.take<int64_t>((size_t)n_clouds + 1);
    h->bytes = cv.at;
}
