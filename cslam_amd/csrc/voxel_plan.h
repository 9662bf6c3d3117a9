// Host-side planning of cslam_voxel_downsample_dev (voxel.hip): which radix passes run and how the scratch is carved.
// Plain C++ without HIP, so that it can also be compiled into a stand-alone program and run under host sanitizers.
#pragma once
#include <stdint.h>
#include <stddef.h>

#define VOXEL_TILE 2048          // keys per workgroup per radix pass (256 threads x 8 keys, a wave owns 512 in a row)
#define VOXEL_SORT_BLOCK 256     // threads per workgroup of the histogram and scatter kernels
#define VOXEL_SEG_BLOCK 256      // threads per workgroup of the segment kernel: 4 waves, one voxel segment per wave at a time
#define VOXEL_RADIX_BITS 8
#define VOXEL_AXIS_BITS 21       // a voxel index on any axis is below 2^21: three axes make 63 key bits
#define VOXEL_SCAN_BLOCK 1024    // the one workgroup that scans the segment heads per tile
#define VOXEL_FLAG_BLOCK 256     // positions per workgroup of the segment-head kernels
#define VOXEL_MAX_POINTS (0x7fffffffll - VOXEL_TILE)

struct VoxelPlan {
    int key_bits;                // occupied bits of the widest cloud key, plus the "row does not exist" bit when one is needed
    int key_passes, cloud_passes;
    int invalid_shift;           // position of that bit, -1 when every row of the batch exists
    int64_t n, tiles, flag_tiles;
    // byte offsets into the scratch, each a multiple of 256
    size_t o_keys[2], o_idx[2], o_cloud, o_flags, o_rank, o_start, o_end, o_hist, o_totals, o_tile_count, o_rows, bytes;
};

static inline int voxel_bits_of(uint64_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

static inline size_t voxel_carve(size_t *at, size_t bytes) {
    const size_t here = *at;
    *at = here + (bytes + 255) / 256 * 256;
    return here;
}

// n points in n_clouds clouds; max_key_bits = the largest bx + by + bz over the clouds (0 .. 63); any_invalid = some
// row is non-finite or belongs to a cloud beyond the index range.  Returns 0, or -1 on sizes outside the limits.
static inline int voxel_make_plan(int64_t n, int n_clouds, int max_key_bits, int any_invalid, VoxelPlan *p) {
    if (n < 0 || n > VOXEL_MAX_POINTS || n_clouds < 1 || n_clouds > 65535) return -1;
    if (max_key_bits < 0 || max_key_bits > 3 * VOXEL_AXIS_BITS) return -1;
    p->n = n;
    p->invalid_shift = any_invalid ? max_key_bits : -1;
    p->key_bits = max_key_bits + (any_invalid ? 1 : 0);
    p->key_passes = (p->key_bits + VOXEL_RADIX_BITS - 1) / VOXEL_RADIX_BITS;
    p->cloud_passes = (voxel_bits_of((uint64_t)(n_clouds - 1)) + VOXEL_RADIX_BITS - 1) / VOXEL_RADIX_BITS;
    p->tiles = (n + VOXEL_TILE - 1) / VOXEL_TILE;
    p->flag_tiles = (n + VOXEL_FLAG_BLOCK - 1) / VOXEL_FLAG_BLOCK;
    size_t at = 0;
    const size_t un = (size_t)n;
    for (int k = 0; k < 2; ++k) {
        p->o_keys[k] = voxel_carve(&at, un * 8);
        p->o_idx[k] = voxel_carve(&at, un * 4);
    }
    p->o_cloud = voxel_carve(&at, un * 2);
    p->o_flags = voxel_carve(&at, un);
    p->o_rank = voxel_carve(&at, un * 4);
    p->o_start = voxel_carve(&at, un * 4);
    p->o_end = voxel_carve(&at, un * 4);
    p->o_hist = voxel_carve(&at, (size_t)p->tiles * (1u << VOXEL_RADIX_BITS) * 4);
    p->o_totals = voxel_carve(&at, (1u << VOXEL_RADIX_BITS) * 4);
    p->o_tile_count = voxel_carve(&at, (size_t)p->flag_tiles * 4);
    p->o_rows = voxel_carve(&at, 4);
    p->bytes = at;
    return 0;
}

// digit of radix pass `pass`: the key's bits first, the cloud number above them
static inline void voxel_pass_digit(const VoxelPlan *p, int pass, int *shift, int *from_cloud) {
    *from_cloud = pass >= p->key_passes;
    *shift = VOXEL_RADIX_BITS * (*from_cloud ? pass - p->key_passes : pass);
}
