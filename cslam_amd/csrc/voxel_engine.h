// The voxel engine (voxel.hip), which does not depend on how a key was made: the stable radix sort of (key, point index),
// the segment heads, their scan and the output offsets.  The one filter chain of cloud.hip calls it, for all three grid
// rules, on a placed VoxelPlan whose keys[0], idx[0] and cloud_of the key kernel has filled.  Hidden visibility: not part
// of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "voxel_plan.h"

// The radix passes the plan selects, then flags, rank, seg_start, seg_end and *rows of the sorted order, and
// d_out_offsets[c] = the first output row of cloud c (n_clouds + 1 entries).  *cur = which of keys[] / idx[] holds the
// sorted order.  `after_sort`: an event to record between the sort and the heads, or null.  Enqueues only.
int voxel_engine_sort_heads(const VoxelPlan *pl, const int64_t *d_offsets, int n_clouds, int64_t *d_out_offsets,
                            hipEvent_t after_sort, hipStream_t st, int *cur);

// Compaction by flags (1 = kept, 2 = dropped) over n positions, with the same scan and rank kernels: tile_count holds the
// kept positions per VOXEL_FLAG_BLOCK positions; on return *total = the kept positions, rank[j] = the kept ones before j,
// src[r] = the position of kept row r, and d_out_offsets[c] = rank[d_offsets[c]] (*total from position n on).
int voxel_engine_compact(const uint8_t *flags, int64_t n, uint32_t *tile_count, uint32_t *total, uint32_t *rank, uint32_t *src,
                         uint32_t *seg_end, const int64_t *d_offsets, int n_clouds, int64_t *d_out_offsets, hipStream_t st);
