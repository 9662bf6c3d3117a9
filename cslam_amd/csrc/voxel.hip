// voxel.hip -- the voxel engine (gfx950): the part of every voxel filter that does not depend on how a key was made.
//
// The three filters of the library -- lidar down-sampling (open3d's rule), the keyframe cloud filter (PCL's rule) and the
// swarm map -- are one chain with three grid rules.  The rules are in cloud.h; the chain (bounds, meta, keys, this engine,
// segment sums) and every entry point, `cslam_voxel_downsample_dev` included, are in cloud.hip.  This file holds what runs
// between the key kernel and the segment kernel, on a placed VoxelPlan (voxel_plan.h), behind voxel_engine.h:
//
//   radix passes       : a STABLE least-significant-digit sort of (key, point index), 8 bits per pass: histogram per
//                        tile, a scan of the [digit][tile] counts (one workgroup per digit), scatter.  Inside a tile a
//                        key's place among equal digits comes from wave ballots (the lanes with the same digit) and mbcnt
//                        (how many of them are below this lane) on per-wave LDS counters, so equal digits keep their
//                        order.  Only the passes whose bits are occupied run: the key's, then those of the cloud number,
//                        which is the digit above the key (read through the point index, so a batch is one sort whatever
//                        the key width).  A cloud therefore stays in its own rows [offsets[c], offsets[c+1]) of the
//                        sorted order, and equal keys stay in cloud order, which is what fixes the order of every sum.
//   vox_flag / vox_rank: a sorted position is a segment head when its key or its cloud differs from the position
//                        before; the scan of the heads numbers the output rows and gives d_out_offsets.  A row that does
//                        not exist carries the one bit above the widest key of the batch and sorts behind its cloud.
//   compaction         : the same scan and rank kernels over any flags (the clip of the keyframe filter).
// Integer arithmetic only; no atomics decide a position.  Enqueues only: the chain's one host wait is before the key kernel.
#include "common.h"
#include "voxel_plan.h"
#include "voxel_engine.h"

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

// ---- host side ---------------------------------------------------------------------------------
// what cloud.hip's chain calls (voxel_engine.h)
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
