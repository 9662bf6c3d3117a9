// voxel.hip -- batched voxel down-sampling of lidar keyframes (gfx950).
//
// Replaces `downsample` of cslam/lidar_pr/icp_utils.py:93-100 (drop the non-finite rows, then open3d's
// voxel_down_sample) for a batch of clouds.  Per cloud: origin = min over the finite rows - voxel / 2, voxel index per
// axis = floor((p - origin) / voxel) with a true division, one output row per occupied voxel = the sum of its points in
// CLOUD ORDER, accumulated one after another from the first, divided once by the count.  Rows come out in ascending
// lexicographic voxel index, x most significant.  All arithmetic is float64 and nothing is contracted.
//
//   vox_bounds_kernel  : min and max per axis over the finite rows, and the number of non-finite rows (a minimum does
//                        not depend on the order it is taken in); vox_meta_kernel folds the partials per cloud.
//   vox_meta_kernel    : origin; the index of the maximum is the largest index (every step of the rule is monotone), so
//                        it gives the bits bx, by, bz an axis needs; an index of 2^21 or more sets the cloud's status.
//   vox_key_kernel     : key = ix << (by + bz) | iy << bz | iz per point, packed with the cloud's own widths: ascending
//                        key = ascending (ix, iy, iz).  A row that does not exist (non-finite, or of a cloud beyond the
//                        range) gets the one bit above the widest key of the batch, which sorts it behind its cloud.
//   radix passes       : a STABLE least-significant-digit sort of (key, point index), 8 bits per pass: histogram per
//                        tile, a scan of the [digit][tile] counts (one workgroup per digit), scatter.  Inside a tile a key's place among equal
//                        digits comes from wave ballots (the lanes with the same digit) and mbcnt (how many of them are
//                        below this lane) on per-wave LDS counters, so equal digits keep their order.  Only the passes
//                        whose bits are occupied run: the key's, then those of the cloud number, which is the digit
//                        above the key (read through the point index, so a batch is one sort whatever the key width).
//                        A cloud therefore stays in its own rows [offsets[c], offsets[c+1]) of the sorted order.
//   vox_flag / vox_rank: a sorted position is a segment head when its key or its cloud differs from the position
//                        before; the scan of the heads numbers the output rows and gives d_out_offsets.
//   vox_segment_kernel : one wave per voxel segment: 64 points are gathered side by side, then every lane adds them in
//                        sorted order, one at a time.  Equal keys are in cloud order because the sort is stable, so
//                        this is `np.add.at`'s and open3d's AccumulatedPoint's order whatever the segment's length.
// No float atomics and no sum whose order depends on scheduling: a cloud's output is the same bits alone or in any batch.
//
// The call waits on the host once, between vox_meta_kernel and the rest: it reads the widest key of the batch and whether
// any row does not exist (8 bytes: they select the sort passes), and the offsets when no host copy was given.
#include "common.h"
#include "voxel_plan.h"
#include "voxel_engine.h"

#pragma clang fp contract(off)

#define VOX_BOUNDS_BLOCK 256
#define VOX_NPART 7                                        // min[3], max[3], non-finite rows

__device__ __forceinline__ bool vox_finite(double x, double y, double z) {
    return fabs(x) <= 1.7976931348623157e308 && fabs(y) <= 1.7976931348623157e308 && fabs(z) <= 1.7976931348623157e308;
}

// floor((p - origin) / voxel): the one place the rule is written
__device__ __forceinline__ double vox_index(double p, double origin, double voxel) {
    return floor(__ddiv_rn(__dsub_rn(p, origin), voxel));
}

__global__ __launch_bounds__(VOX_BOUNDS_BLOCK) void vox_bounds_kernel(const double *__restrict__ pts,
                                                                      const int64_t *__restrict__ off,
                                                                      double *__restrict__ part) {
    __shared__ double s_w[VOX_BOUNDS_BLOCK / 64][VOX_NPART];
    const int c = blockIdx.y, t = threadIdx.x;
    const int64_t i0 = off[c], i1 = i0 >= 0 ? off[c + 1] : 0;      // offsets not yet checked by the host read nothing below row 0
    double v[VOX_NPART] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
    for (int64_t i = i0 + (int64_t)blockIdx.x * VOX_BOUNDS_BLOCK + t; i < i1; i += (int64_t)gridDim.x * VOX_BOUNDS_BLOCK) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (vox_finite(x, y, z)) {
            v[0] = fmin(v[0], x); v[1] = fmin(v[1], y); v[2] = fmin(v[2], z);
            v[3] = fmax(v[3], x); v[4] = fmax(v[4], y); v[5] = fmax(v[5], z);
        } else {
            v[6] += 1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < VOX_NPART; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double u = __shfl_xor(v[k], o, 64);
            v[k] = k < 3 ? fmin(v[k], u) : (k < 6 ? fmax(v[k], u) : v[k] + u);      // counts are small integers: exact
        }
        if ((t & 63) == 0) s_w[t >> 6][k] = v[k];
    }
    __syncthreads();
    if (t < VOX_NPART) {
        double a = s_w[0][t];
        for (int w = 1; w < VOX_BOUNDS_BLOCK / 64; ++w) a = t < 3 ? fmin(a, s_w[w][t]) : (t < 6 ? fmax(a, s_w[w][t]) : a + s_w[w][t]);
        part[((int64_t)c * gridDim.x + blockIdx.x) * VOX_NPART + t] = a;
    }
}

// per cloud: origin[3] and meta = {shift of ix, shift of iy, key bits, dead}; head = {widest key, any row missing}
__global__ __launch_bounds__(64) void vox_meta_kernel(const double *__restrict__ part, int nb, int n_clouds, double voxel, double half,
                                                      double *__restrict__ origin, int *__restrict__ meta, int *__restrict__ head,
                                                      int32_t *__restrict__ status) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_clouds) return;
    double v[VOX_NPART] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
    for (int b = 0; b < nb; ++b) {
        const double *p = part + ((int64_t)c * nb + b) * VOX_NPART;
        for (int k = 0; k < 3; ++k) { v[k] = fmin(v[k], p[k]); v[3 + k] = fmax(v[3 + k], p[3 + k]); }
        v[6] += p[6];
    }
    int bits[3] = {0, 0, 0}, over = 0;
    double o[3] = {0.0, 0.0, 0.0};
    if (v[0] <= v[3]) {                                    // the cloud has a finite row
        for (int a = 0; a < 3; ++a) {
            o[a] = __dsub_rn(v[a], half);
            const double q = vox_index(v[3 + a], o[a], voxel);
            if (!(q >= 0.0 && q < (double)(1 << VOXEL_AXIS_BITS))) over = 1;      // also an infinite or NaN quotient
            else bits[a] = q == 0.0 ? 0 : 64 - __clzll((long long)q);
        }
    }
    for (int a = 0; a < 3; ++a) origin[3 * c + a] = o[a];
    const int kb = over ? 0 : bits[0] + bits[1] + bits[2];
    meta[4 * c] = bits[1] + bits[2];
    meta[4 * c + 1] = bits[2];
    meta[4 * c + 2] = kb;
    meta[4 * c + 3] = over;
    status[c] = over;
    atomicMax(&head[0], kb);
    if (over || v[6] > 0.0) atomicOr(&head[1], 1);
}

__global__ __launch_bounds__(256) void vox_key_kernel(const double *__restrict__ pts, const int64_t *__restrict__ off, int n_clouds,
                                                      int64_t n, double voxel, const double *__restrict__ origin,
                                                      const int *__restrict__ meta, int invalid_shift,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                      uint16_t *__restrict__ cloud_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_clouds;                             // the cloud with off[c] <= i < off[c + 1]: the last c with off[c] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const int c = lo;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    uint64_t key;
    if (vox_finite(x, y, z) && !meta[4 * c + 3]) {
        const uint64_t ix = (uint64_t)vox_index(x, origin[3 * c], voxel);
        const uint64_t iy = (uint64_t)vox_index(y, origin[3 * c + 1], voxel);
        const uint64_t iz = (uint64_t)vox_index(z, origin[3 * c + 2], voxel);
        key = (ix << meta[4 * c]) | (iy << meta[4 * c + 1]) | iz;
    } else {
        key = 1ull << (invalid_shift & 63);                     // the host saw head[1] != 0, so invalid_shift is 0 .. 63 here
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
    cloud_of[i] = (uint16_t)c;
}

__device__ __forceinline__ unsigned vox_digit(uint64_t key, uint32_t idx, const uint16_t *__restrict__ cloud_of, int shift,
                                              int from_cloud) {
    return from_cloud ? ((unsigned)cloud_of[idx] >> shift) & 255u : (unsigned)(key >> shift) & 255u;
}

// hist[digit][tile]
__global__ __launch_bounds__(VOXEL_SORT_BLOCK) void vox_hist_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                                    const uint16_t *__restrict__ cloud_of, int64_t n, int shift,
                                                                    int from_cloud, uint32_t *__restrict__ hist) {
    __shared__ unsigned s_h[256];
    const int t = threadIdx.x;
    s_h[t] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * VOXEL_TILE;
    for (int r = 0; r < VOXEL_TILE / VOXEL_SORT_BLOCK; ++r) {
        const int64_t j = base + r * VOXEL_SORT_BLOCK + t;
        if (j < n) atomicAdd(&s_h[vox_digit(keys[j], idx[j], cloud_of, shift, from_cloud)], 1u);
    }
    __syncthreads();
    hist[(size_t)t * gridDim.x + blockIdx.x] = s_h[t];
}

// inclusive scan over the 64 lanes
__device__ __forceinline__ unsigned vox_wave_scan(unsigned v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// One workgroup per digit: hist[digit][tile] becomes the digit's keys in earlier tiles, totals[digit] its keys in all.
__global__ __launch_bounds__(VOXEL_SORT_BLOCK) void vox_digit_scan_kernel(uint32_t *__restrict__ hist, int64_t tiles,
                                                                          uint32_t *__restrict__ totals) {
    __shared__ unsigned s_w[VOXEL_SORT_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t *row = hist + (size_t)blockIdx.x * tiles;
    unsigned carry = 0;
    for (int64_t c0 = 0; c0 < tiles; c0 += VOXEL_SORT_BLOCK) {
        const int64_t i = c0 + t;
        const unsigned v = i < tiles ? row[i] : 0u;
        const unsigned incl = vox_wave_scan(v, lane);
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        unsigned before = carry, chunk = 0;
        for (int k = 0; k < VOXEL_SORT_BLOCK / 64; ++k) {
            if (k < w) before += s_w[k];
            chunk += s_w[k];
        }
        if (i < tiles) row[i] = before + incl - v;
        carry += chunk;
        __syncthreads();                                   // s_w is written again in the next chunk
    }
    if (t == 0) totals[blockIdx.x] = carry;
}

// in-place exclusive scan of a[0 .. m) by one workgroup; *total = the sum
__global__ __launch_bounds__(VOXEL_SCAN_BLOCK) void vox_scan_kernel(uint32_t *__restrict__ a, int64_t m, uint32_t *__restrict__ total) {
    __shared__ unsigned s_w[VOXEL_SCAN_BLOCK / 64 + 1];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t chunk = (m + VOXEL_SCAN_BLOCK - 1) / VOXEL_SCAN_BLOCK;
    const int64_t lo = t * chunk < m ? t * chunk : m, hi = lo + chunk < m ? lo + chunk : m;
    unsigned sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += a[i];
    const unsigned incl = vox_wave_scan(sum, lane);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    if (t == 0) {
        unsigned run = 0;
        for (int k = 0; k < VOXEL_SCAN_BLOCK / 64; ++k) { const unsigned u = s_w[k]; s_w[k] = run; run += u; }
        s_w[VOXEL_SCAN_BLOCK / 64] = run;
    }
    __syncthreads();
    unsigned run = s_w[w] + incl - sum;
    for (int64_t i = lo; i < hi; ++i) { const unsigned u = a[i]; a[i] = run; run += u; }
    if (t == 0 && total) *total = s_w[VOXEL_SCAN_BLOCK / 64];
}

// A wave owns VOXEL_TILE / 4 consecutive keys of the tile and takes them 64 at a time.  In one such round the lanes with
// this lane's digit are found by one ballot per digit bit; the lane's place among them is mbcnt of that mask; the digit's
// count from the wave's earlier rounds is in s_cnt[wave][digit], which the lowest lane of the group then raises.
__global__ __launch_bounds__(VOXEL_SORT_BLOCK) void vox_scatter_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                                       const uint16_t *__restrict__ cloud_of, int64_t n, int shift,
                                                                       int from_cloud, const uint32_t *__restrict__ scanned,
                                                                       const uint32_t *__restrict__ totals,
                                                                       uint64_t *__restrict__ keys_out, uint32_t *__restrict__ idx_out) {
    constexpr int WAVES = VOXEL_SORT_BLOCK / 64, ROUNDS = VOXEL_TILE / VOXEL_SORT_BLOCK;
    __shared__ unsigned s_cnt[WAVES][256];
    __shared__ unsigned s_dig[WAVES];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int e = t; e < WAVES * 256; e += VOXEL_SORT_BLOCK) (&s_cnt[0][0])[e] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * VOXEL_TILE + (int64_t)w * (ROUNDS * 64);
    uint64_t k[ROUNDS];
    uint32_t ix[ROUNDS];
    unsigned place[ROUNDS];                                // digit in the top 8 bits, place inside the wave's keys below
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t j = base + r * 64 + lane;
        const bool live = j < n;
        k[r] = live ? keys[j] : 0;
        ix[r] = live ? idx[j] : 0;
        const unsigned d = live ? vox_digit(k[r], ix[r], cloud_of, shift, from_cloud) : 0u;
        unsigned long long same = __ballot(live);
#pragma unroll
        for (int b = 0; b < VOXEL_RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long has = __ballot(live && bit);
            same &= bit ? has : ~has;
        }
        const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));
        const unsigned before = live ? s_cnt[w][d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (live && below == 0) s_cnt[w][d] = before + (unsigned)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        place[r] = (d << 24) | (before + below);           // before + below < VOXEL_TILE
    }
    const unsigned dig_total = totals[t];                  // thread t = digit t from here: the keys of the smaller digits ...
    const unsigned dig_incl = vox_wave_scan(dig_total, lane);
    if (lane == 63) s_dig[w] = dig_incl;
    __syncthreads();
    {                                                      // ... of this digit in earlier tiles, then where each wave's start
        unsigned run = dig_incl - dig_total + scanned[(size_t)t * gridDim.x + blockIdx.x];
        for (int v = 0; v < w; ++v) run += s_dig[v];
        for (int v = 0; v < WAVES; ++v) { const unsigned c = s_cnt[v][t]; s_cnt[v][t] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t j = base + r * 64 + lane;
        if (j < n) {
            const unsigned dst = s_cnt[w][place[r] >> 24] + (place[r] & 0xffffffu);
            keys_out[dst] = k[r];
            idx_out[dst] = ix[r];
        }
    }
}

// flags[j]: 2 = the row does not exist, 1 = first point of a voxel, 0 = a further point of it; heads per workgroup
__global__ __launch_bounds__(VOXEL_FLAG_BLOCK) void vox_flag_kernel(const uint64_t *__restrict__ keys, const uint16_t *__restrict__ cloud_of,
                                                                    int64_t n, int invalid_shift, uint8_t *__restrict__ flags,
                                                                    uint32_t *__restrict__ tile_count) {
    __shared__ unsigned s_n;
    const int t = threadIdx.x;
    if (t == 0) s_n = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * VOXEL_FLAG_BLOCK + t;
    bool head = false;
    if (j < n) {
        const uint64_t key = keys[j];
        const bool missing = invalid_shift >= 0 && ((key >> invalid_shift) & 1ull);
        // sorted position j belongs to cloud_of[j]: the sort keeps every cloud inside its own rows
        head = !missing && (j == 0 || cloud_of[j] != cloud_of[j - 1] || key != keys[j - 1]);
        flags[j] = missing ? 2 : (head ? 1 : 0);
    }
    const unsigned long long m = __ballot(head);
    if ((t & 63) == 0 && m) atomicAdd(&s_n, (unsigned)__popcll(m));
    __syncthreads();
    if (t == 0) tile_count[blockIdx.x] = s_n;
}

// rank[j] = heads before j; the head of row r notes where r starts, the last point of r where it ends
__global__ __launch_bounds__(VOXEL_FLAG_BLOCK) void vox_rank_kernel(const uint8_t *__restrict__ flags, int64_t n,
                                                                    const uint32_t *__restrict__ tile_excl, uint32_t *__restrict__ rank,
                                                                    uint32_t *__restrict__ seg_start, uint32_t *__restrict__ seg_end) {
    __shared__ unsigned s_w[VOXEL_FLAG_BLOCK / 64];
    const int t = threadIdx.x, w = t >> 6;
    const int64_t j = (int64_t)blockIdx.x * VOXEL_FLAG_BLOCK + t;
    const int f = j < n ? flags[j] : 2;
    const unsigned long long m = __ballot(f == 1);
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if ((t & 63) == 0) s_w[w] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned r = tile_excl[blockIdx.x] + below;
    for (int v = 0; v < w; ++v) r += s_w[v];
    if (j >= n) return;
    rank[j] = r;
    if (f == 1) seg_start[r] = (uint32_t)j;
    if (f != 2 && (j + 1 == n || flags[j + 1] != 0)) seg_end[r + (f == 1) - 1] = (uint32_t)(j + 1);
}

__global__ void vox_out_offsets_kernel(const int64_t *__restrict__ off, int n_clouds, int64_t n, const uint32_t *__restrict__ rank,
                                       const uint32_t *__restrict__ rows, int64_t *__restrict__ out_off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_clouds) return;
    const int64_t o = off[c];
    out_off[c] = o < n ? (int64_t)rank[o] : (int64_t)*rows;
}

__global__ __launch_bounds__(VOXEL_SEG_BLOCK) void vox_segment_kernel(const double *__restrict__ pts, const uint32_t *__restrict__ idx,
                                                                      const uint32_t *__restrict__ seg_start,
                                                                      const uint32_t *__restrict__ seg_end,
                                                                      const uint32_t *__restrict__ rows, double *__restrict__ out,
                                                                      int32_t *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (VOXEL_SEG_BLOCK / 64);
    const int64_t n_rows = *rows;
    for (int64_t r = (int64_t)blockIdx.x * (VOXEL_SEG_BLOCK / 64) + (threadIdx.x >> 6); r < n_rows; r += nw) {
        const int64_t s = seg_start[r], e = seg_end[r];
        double ax = 0.0, ay = 0.0, az = 0.0;               // np.add.at starts from zeros as well
        for (int64_t c0 = s; c0 < e; c0 += 64) {
            const int m = (int)(e - c0 < 64 ? e - c0 : 64);
            double x = 0.0, y = 0.0, z = 0.0;
            if (lane < m) {
                const int64_t i = idx[c0 + lane];
                x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
            }
            for (int q = 0; q < m; ++q) {                  // every lane adds the same points in the same order
                ax = __dadd_rn(ax, __shfl(x, q, 64));
                ay = __dadd_rn(ay, __shfl(y, q, 64));
                az = __dadd_rn(az, __shfl(z, q, 64));
            }
        }
        if (lane == 0) {
            const double cnt = (double)(e - s);
            out[3 * r] = __ddiv_rn(ax, cnt);
            out[3 * r + 1] = __ddiv_rn(ay, cnt);
            out[3 * r + 2] = __ddiv_rn(az, cnt);
            if (counts) counts[r] = (int32_t)(e - s);
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------
// the engine cloud.hip shares (voxel_engine.h)
int voxel_engine_compact(const uint8_t *flags, int64_t n, uint32_t *tile_count, uint32_t *total, uint32_t *rank, uint32_t *src,
                         uint32_t *seg_end, const int64_t *d_offsets, int n_clouds, int64_t *d_out_offsets, hipStream_t st) {
    const int64_t flag_tiles = ceil_div64(n, VOXEL_FLAG_BLOCK);
    hipLaunchKernelGGL(vox_scan_kernel, dim3(1), dim3(VOXEL_SCAN_BLOCK), 0, st, tile_count, flag_tiles, total);
    hipLaunchKernelGGL(vox_rank_kernel, dim3((unsigned)flag_tiles), dim3(VOXEL_FLAG_BLOCK), 0, st, flags, n, tile_count, rank, src, seg_end);
    hipLaunchKernelGGL(vox_out_offsets_kernel, dim3((unsigned)ceil_div64((int64_t)n_clouds + 1, 256)), dim3(256), 0, st, d_offsets,
                       n_clouds, n, rank, total, d_out_offsets);
    return CSLAM_OK;
}

int voxel_engine_sort_heads(const VoxelPlan *pl, const int64_t *d_offsets, int n_clouds, int64_t *d_out_offsets,
                            hipEvent_t after_sort, hipStream_t st, int *cur_out) {
    const int64_t n = pl->n;
    int cur = 0;
    for (int pass = 0; pass < pl->key_passes + pl->cloud_passes; ++pass) {
        int shift, from_cloud;
        voxel_pass_digit(pl, pass, &shift, &from_cloud);
        hipLaunchKernelGGL(vox_hist_kernel, dim3((unsigned)pl->tiles), dim3(VOXEL_SORT_BLOCK), 0, st, pl->keys[cur], pl->idx[cur], pl->cloud_of, n,
                           shift, from_cloud, pl->hist);
        hipLaunchKernelGGL(vox_digit_scan_kernel, dim3(256), dim3(VOXEL_SORT_BLOCK), 0, st, pl->hist, pl->tiles, pl->totals);
        hipLaunchKernelGGL(vox_scatter_kernel, dim3((unsigned)pl->tiles), dim3(VOXEL_SORT_BLOCK), 0, st, pl->keys[cur], pl->idx[cur], pl->cloud_of, n,
                           shift, from_cloud, pl->hist, pl->totals, pl->keys[cur ^ 1], pl->idx[cur ^ 1]);
        cur ^= 1;
    }
    if (after_sort) (void)hipEventRecord(after_sort, st);
    hipLaunchKernelGGL(vox_flag_kernel, dim3((unsigned)pl->flag_tiles), dim3(VOXEL_FLAG_BLOCK), 0, st, pl->keys[cur], pl->cloud_of, n,
                       pl->invalid_shift, pl->flags, pl->tile_count);
    *cur_out = cur;
    return voxel_engine_compact(pl->flags, n, pl->tile_count, pl->rows, pl->rank, pl->seg_start, pl->seg_end, d_offsets, n_clouds,
                                d_out_offsets, st);
}

static StreamScratch g_voxel_head_scratch, g_voxel_scratch;

// stage times of the last call, for tools/perf_voxel.py (cslam_voxel_profile)
enum { VOX_EV = 7 };                                       // begin, bounds + meta | wait | keys | sort | heads | segments
static struct {
    std::mutex mu;
    bool on = false, have = false;
    hipEvent_t ev[VOX_EV] = {};
    bool made = false;
    int info[4] = {0, 0, 0, 0};
} g_vox_prof;

static void vox_mark(bool on, int k, hipStream_t st) {
    if (on) (void)hipEventRecord(g_vox_prof.ev[k], st);
}

// the shared offsets rule and the one limit of the sort
static int vox_shape(const int64_t *off, int n_clouds, RaggedShape *s) {
    int rc = offsets_check(off, n_clouds, s);
    if (rc) return rc;
    ARG_CHECK(s->total <= VOXEL_MAX_POINTS, "more points than an int32 index addresses");
    return CSLAM_OK;
}

CSLAM_API int cslam_voxel_downsample_dev(const double *d_points, const int64_t *d_offsets, int n_clouds, double voxel,
                                         double *d_out, int64_t *d_out_offsets, int32_t *d_counts, int32_t *d_status,
                                         const int64_t *h_offsets, void *stream) {
    ARG_CHECK(voxel > 0.0 && voxel < INFINITY, "voxel must be positive and finite");
    BATCH_COUNT_CHECK(n_clouds);
    ARG_CHECK(d_offsets && d_out_offsets && d_status, "NULL argument");
    int rc;
    RaggedShape sh = {};
    if (h_offsets && (rc = vox_shape(h_offsets, n_clouds, &sh))) return rc;
    ARG_CHECK((d_points && d_out) || (h_offsets && sh.total == 0), "NULL argument");
    PTR_DEVICE(d_offsets);
    hipStream_t st = (hipStream_t)stream;
    bool prof;
    {
        std::lock_guard<std::mutex> lock(g_vox_prof.mu);
        prof = g_vox_prof.on;
        if (prof && !g_vox_prof.made) {
            for (int k = 0; k < VOX_EV; ++k) HIP_TRY(hipEventCreate(&g_vox_prof.ev[k]));
            g_vox_prof.made = true;
        }
        g_vox_prof.have = false;
    }
    // before the wait: bounds and meta, whose launch shape depends on n_clouds alone
    int nb = 2048 / n_clouds;
    nb = nb < 1 ? 1 : (nb > 64 ? 64 : nb);
    double *part, *origin;
    int *meta, *head;
    auto head_layout = [&](Carver &cv) {
        part = cv.take<double>((size_t)n_clouds * nb * VOX_NPART);
        origin = cv.take<double>((size_t)n_clouds * 3);
        meta = cv.take<int>((size_t)n_clouds * 4);
        head = cv.take<int>(2);                            // 8 bytes in a piece of 256
    };
    SCRATCH_CARVE(g_voxel_head_scratch, st, (size_t)1 << 16, head_layout);
    vox_mark(prof, 0, st);
    HIP_TRY(hipMemsetAsync(head, 0, 8, st));
    hipLaunchKernelGGL(vox_bounds_kernel, dim3((unsigned)nb, (unsigned)n_clouds), dim3(VOX_BOUNDS_BLOCK), 0, st, d_points, d_offsets, part);
    hipLaunchKernelGGL(vox_meta_kernel, dim3((unsigned)ceil_div64(n_clouds, 64)), dim3(64), 0, st, part, nb, n_clouds, voxel, voxel / 2.0,
                       origin, meta, head, d_status);
    vox_mark(prof, 1, st);
    int h_head[2] = {0, 0};
    std::vector<int64_t> read_off;
    HIP_TRY(hipMemcpyAsync(h_head, head, 8, hipMemcpyDeviceToHost, st));
    if (!h_offsets && (rc = read_back_async(read_off, d_offsets, (size_t)n_clouds + 1, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));                     // the one host wait
    if (!h_offsets && (rc = vox_shape(read_off.data(), n_clouds, &sh))) return rc;
    const int64_t n = sh.total;
    VoxelPlan pl;
    if (voxel_make_plan(n, n_clouds, h_head[0], h_head[1], nullptr, &pl)) {
        cslam_set_error("voxel down-sampling: sizes outside the plan's limits");
        return CSLAM_E_INVALID;
    }
    vox_mark(prof, 2, st);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_out_offsets, 0, ((size_t)n_clouds + 1) * 8, st));
        for (int k = 3; k < VOX_EV; ++k) vox_mark(prof, k, st);
    } else {
        SCRATCH_HERE(base, g_voxel_scratch, st, pl.bytes, (size_t)1 << 20);
        voxel_make_plan(n, n_clouds, h_head[0], h_head[1], base, &pl);     // the same plan, placed
        hipLaunchKernelGGL(vox_key_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, d_points, d_offsets, n_clouds, n, voxel,
                           origin, meta, pl.invalid_shift, pl.keys[0], pl.idx[0], pl.cloud_of);
        vox_mark(prof, 3, st);
        int cur = 0;
        if ((rc = voxel_engine_sort_heads(&pl, d_offsets, n_clouds, d_out_offsets, prof ? g_vox_prof.ev[4] : nullptr, st, &cur))) return rc;
        vox_mark(prof, 5, st);
        const int64_t want = ceil_div64(n, VOXEL_SEG_BLOCK / 64);
        const int64_t cap = (int64_t)(cslam_cu_count() > 0 ? cslam_cu_count() : 256) * 8;
        hipLaunchKernelGGL(vox_segment_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(VOXEL_SEG_BLOCK), 0, st, d_points, pl.idx[cur],
                           pl.seg_start, pl.seg_end, pl.rows, d_out, d_counts);
        vox_mark(prof, 6, st);
    }
    HIP_TRY(hipGetLastError());
    if (prof) {
        std::lock_guard<std::mutex> lock(g_vox_prof.mu);
        g_vox_prof.info[0] = pl.key_passes;
        g_vox_prof.info[1] = pl.cloud_passes;
        g_vox_prof.info[2] = pl.key_bits;
        g_vox_prof.info[3] = (int)pl.tiles;
        g_vox_prof.have = true;
    }
    return CSLAM_OK;
}

CSLAM_API int cslam_voxel_profile(int enable) {
    std::lock_guard<std::mutex> lock(g_vox_prof.mu);
    g_vox_prof.on = enable != 0;
    g_vox_prof.have = false;
    return CSLAM_OK;
}

CSLAM_API int cslam_voxel_profile_read(double ms[6], int32_t info[4]) {
    ARG_CHECK(ms && info, "NULL argument");
    std::lock_guard<std::mutex> lock(g_vox_prof.mu);
    ARG_CHECK(g_vox_prof.have, "no profiled call: cslam_voxel_profile(1), then cslam_voxel_downsample_dev");
    HIP_TRY(hipEventSynchronize(g_vox_prof.ev[VOX_EV - 1]));
    for (int k = 0; k + 1 < VOX_EV; ++k) {
        float f = 0.f;
        HIP_TRY(hipEventElapsedTime(&f, g_vox_prof.ev[k], g_vox_prof.ev[k + 1]));
        ms[k] = f;
    }
    for (int k = 0; k < 4; ++k) info[k] = g_vox_prof.info[k];
    return CSLAM_OK;
}
