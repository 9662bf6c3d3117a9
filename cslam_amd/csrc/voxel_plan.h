// Host-side planning of a voxel filter call (the chain of cloud.hip on the engine of voxel.hip): which radix passes run
// and how the scratch is carved.
// Plain C++ without HIP, so that it can also be compiled into a stand-alone program and run under host sanitizers.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "ragged.h"

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
    // the pieces of the scratch, each on a multiple of 256 bytes: null from a plan that was made without the block
    uint64_t *keys[2];
    uint32_t *idx[2], *rank, *seg_start, *seg_end, *hist, *totals, *tile_count, *rows;
    uint16_t *cloud_of;
    uint8_t *flags;
    size_t bytes;
};

static inline int voxel_bits_of(uint64_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// n points in n_clouds clouds; max_key_bits = the largest bx + by + bz over the clouds (0 .. 63); any_invalid = some
// row is non-finite or belongs to a cloud beyond the index range; base = the scratch block of p->bytes, or null to learn
// p->bytes.  Returns 0, or -1 on sizes outside the limits.
static inline int voxel_make_plan(int64_t n, int n_clouds, int max_key_bits, int any_invalid, void *base, VoxelPlan *p) {
    if (n < 0 || n > VOXEL_MAX_POINTS || n_clouds < 1 || n_clouds > 65535) return -1;
    if (max_key_bits < 0 || max_key_bits > 3 * VOXEL_AXIS_BITS) return -1;
    p->n = n;
    p->invalid_shift = any_invalid ? max_key_bits : -1;
    p->key_bits = max_key_bits + (any_invalid ? 1 : 0);
    p->key_passes = (p->key_bits + VOXEL_RADIX_BITS - 1) / VOXEL_RADIX_BITS;
    p->cloud_passes = (voxel_bits_of((uint64_t)(n_clouds - 1)) + VOXEL_RADIX_BITS - 1) / VOXEL_RADIX_BITS;
    p->tiles = (n + VOXEL_TILE - 1) / VOXEL_TILE;
    p->flag_tiles = (n + VOXEL_FLAG_BLOCK - 1) / VOXEL_FLAG_BLOCK;
    Carver cv(base);
    const size_t un = (size_t)n;
    for (int k = 0; k < 2; ++k) {
        p->keys[k] = cv.take<uint64_t>(un);
        p->idx[k] = cv.take<uint32_t>(un);
    }
    p->cloud_of = cv.take<uint16_t>(un);
    p->flags = cv.take<uint8_t>(un);
    p->rank = cv.take<uint32_t>(un);
    p->seg_start = cv.take<uint32_t>(un);
    p->seg_end = cv.take<uint32_t>(un);
    p->hist = cv.take<uint32_t>((size_t)p->tiles << VOXEL_RADIX_BITS);
    p->totals = cv.take<uint32_t>((size_t)1 << VOXEL_RADIX_BITS);
    p->tile_count = cv.take<uint32_t>((size_t)p->flag_tiles);
    p->rows = cv.take<uint32_t>(1);
    p->bytes = cv.at;
    return 0;
}

// digit of radix pass `pass`: the key's bits first, the cloud number above them
static inline void voxel_pass_digit(const VoxelPlan *p, int pass, int *shift, int *from_cloud) {
    *from_cloud = pass >= p->key_passes;
    *shift = VOXEL_RADIX_BITS * (*from_cloud ? pass - p->key_passes : pass);
}
