// direct_dev.h -- what the register-resident direct convolutions share (conv_stem_direct_h.hip, conv_direct_r.hip, conv_direct_p.hip;
// conv_direct_h.hip takes the block partition and the max |y| tail): each piece defined once, `__device__ __forceinline__`, constexpr or,
// where a function changed a kernel, a macro.  hipcc's register allocation in these kernels is fragile: a kernel adopts a piece only
// where its block loop compiles to the same instructions as its own text did (profiles/direct_family_isa_diff.log), and says so in one
// line where it keeps its own.
#pragma once
#include <hip/hip_fp16.h>
#include "common.h"
#include "pairs.h"

typedef unsigned dd_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned dd_u32x4 __attribute__((ext_vector_type(4)));
typedef float dd_f32x2 __attribute__((ext_vector_type(2)));

// ---- blocks to workgroups, XCD-aware ----------------------------------------------------------------------------------------------
// Workgroup w runs on XCD w % 8 (round-robin dispatch), and every XCD has an L2 of its own.  Each XCD takes one CONTIGUOUS eighth of the
// blocks, its workgroups walk it side by side -- the blocks whose input patches overlap (left / right neighbours, and the row below a
// block row later) are then read through ONE L2 at about the same time.  (Block b -> workgroup b % grid: every halo line was fetched by
// two or three XCDs, 723 MB of L2 misses for the stem's 154 MB image input.)  Workgroup `wg_j` of the `wg_per` that share an XCD's range
// [blk_beg, blk_beg + blk_cnt) runs its blocks wg_j, wg_j + wg_per, ...: `n_mine` of them (blk_cnt may be <= 0 for the last XCDs of a
// tiny launch).  PAIRS: the workgroups 2 j, 2 j + 1 of an XCD walk the SAME blocks (`half` tells them apart); the launch has an even
// number of workgroups per XCD.
struct DirectPart { int wg_j, wg_per, blk_beg, blk_cnt, n_mine, half; };
template <bool PAIRS = false>
__device__ __forceinline__ DirectPart direct_partition(int nblk) {
    DirectPart q;
    const bool by_xcd = (gridDim.x & (PAIRS ? 15 : 7)) == 0;
    const int wg_xcd = by_xcd ? (int)blockIdx.x & 7 : 0, wg_raw = by_xcd ? (int)blockIdx.x >> 3 : (int)blockIdx.x;
    q.half = PAIRS ? wg_raw & 1 : 0;
    q.wg_j = PAIRS ? wg_raw >> 1 : wg_raw;
    q.wg_per = (by_xcd ? (int)gridDim.x >> 3 : (int)gridDim.x) >> (PAIRS ? 1 : 0);
    const int per_xcd = by_xcd ? (nblk + 7) >> 3 : nblk;
    q.blk_beg = wg_xcd * per_xcd;
    q.blk_cnt = min(per_xcd, nblk - q.blk_beg);
    q.n_mine = q.blk_cnt > q.wg_j ? (q.blk_cnt - q.wg_j + q.wg_per - 1) / q.wg_per : 0;
    return q;
}

// the workgroup's block number bi as (image, block row, block column) of a gyb x gxb grid of blocks per image; behind its last block:
// the last block of the XCD's range once more (what is staged for it is never used)
struct DirectBlk { int img, by, bx; };
__device__ __forceinline__ DirectBlk direct_decode_blk(const DirectPart &q, int bi, int gxb, int gyb) {
    int blk = q.wg_j + bi * q.wg_per;
    blk = q.blk_beg + (blk < q.blk_cnt ? blk : q.blk_cnt - 1);
    const int per_img = gxb * gyb;
    DirectBlk b;
    b.img = blk / per_img;
    const int rem = blk - b.img * per_img;
    b.by = rem / gxb; b.bx = rem - b.by * gxb;
    return b;
}

// ---- max |y| of the launch: the lanes' maxima -> wave (shuffles) -> workgroup (LDS atomic) -> the slot (one global atomic per workgroup,
// and only where it would raise the slot).  `lds_slot`: four bytes of LDS nobody uses any more; every thread of the workgroup calls it,
// with ITS OWN my_amax (left holding the wave's maximum), tid = threadIdx.x and lane = tid & 63: with a copy of the maximum, or the ids
// recomputed here, hipcc numbers the caller's registers differently all through its block loop.
__device__ __forceinline__ void amax_publish(float &my_amax, unsigned *amax_out, void *lds_slot, int tid, int lane) {
    unsigned *s_amax = (unsigned *)lds_slot;
    if (tid == 0) *s_amax = 0u;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) my_amax = fmaxf(my_amax, __shfl_xor(my_amax, o, 64));
    if (lane == 0) atomicMax(s_amax, __float_as_uint(my_amax));
    __syncthreads();
    if (tid == 0 && *s_amax > *(volatile unsigned *)amax_out) atomicMax(amax_out, *s_amax);
}

// ---- the 64-channel pair patch: 10 x 18 pixels of an 8 x 16 block with its halo, as exact fp16 pairs in LDS ---------------------------
// 320 bytes per pixel: [hi 64 halfs | lo 64 halfs | 64 pad] = 20 sixteen-byte slots, and the 16-byte chunk c (8 channels) of a half sits
// at chunk c ^ DPATCH_SWZ(pixel column).  Found by search over pitch and swizzle (profiles/r04_v55_*): every ds_read_b128 lane group of a
// fragment read (8 pixels of K group g, the other 8 of K group g + 1) falls on 16 distinct slots for every column shift, K step and
// half, and the stem's first-layer ds_write_b64 (16 consecutive pixels, one 8-byte quarter-chunk each) collide 2.5-way on average --
// 288 bytes without swizzle: the same reads, 3.75-way writes, 1.1k cycles per block.
constexpr int DPATCH_PP = 320;                 // bytes per patch pixel
constexpr int DPATCH_RP = 18 * DPATCH_PP;      // 5 760 per patch row
constexpr int DPATCH_BYTES = 10 * DPATCH_RP;   // 57 600 per buffer
constexpr int DPATCH_NPIX = 180;
constexpr int DPATCH_LO = 128;                 // the lo halves of a chunk: this many bytes behind its hi halves
// (macros: written as functions, hipcc orders the staging tables of conv3x3_direct_r2_kernel differently and numbers its registers
// differently all through the block loop)
#define DPATCH_SWZ(pc) (((pc) >> 1) & 3)
// byte offset of (patch row, patch column, 16-byte chunk of the hi halves, its 8-byte half `q`) in a patch buffer
#define DPATCH_OFF(pr, pc, chunk, q) ((pr) * DPATCH_RP + (pc) * DPATCH_PP + (((chunk) ^ DPATCH_SWZ(pc)) << 4) + (q) * 8)

// ---- staging of float32 activations: four consecutive channels (one 16-byte load) times s, split into fp16 hi + lo, to dst() and
// DPATCH_LO behind it (vector instructions are what this staging costs: the scale is two packed multiplies).  The destination is a
// callable, evaluated where the stores are: computed as an argument, in front of the split, a select between patch and sink is
// scheduled differently in conv3x3_direct_r_kernel's block loop.
template <class Dst>
__device__ __forceinline__ void dpatch_split_store(dd_u32x4 v, float s, Dst dst) {
    dd_f32x2 w01 = dd_f32x2{__uint_as_float(v.x), __uint_as_float(v.y)} * dd_f32x2{s, s};
    dd_f32x2 w23 = dd_f32x2{__uint_as_float(v.z), __uint_as_float(v.w)} * dd_f32x2{s, s};
    asm("" : "+v"(w01), "+v"(w23));                            // (used AS pairs: hipcc keeps the two v_pk_mul_f32)
    const __half2 h01 = __floats2half2_rn(w01[0], w01[1]), h23 = __floats2half2_rn(w23[0], w23[1]);
    const float d0 = sub_half<0>(w01[0], h01), d1 = sub_half<1>(w01[1], h01), d2 = sub_half<0>(w23[0], h23), d3 = sub_half<1>(w23[1], h23);
    const __half2 l01 = __floats2half2_rn(d0, d1), l23 = __floats2half2_rn(d2, d3);
    char *d = dst();
    *(uint2 *)d = make_uint2(*(const unsigned *)&h01, *(const unsigned *)&h23);
    *(uint2 *)(d + DPATCH_LO) = make_uint2(*(const unsigned *)&l01, *(const unsigned *)&l23);
}

// ---- output in the PAIR FORMAT of conv_igemm.hip ([pixel][32-channel block][hi 32 | lo 32] fp16 of s y): four consecutive channels of
// a pixel, `off` = the byte offset of their hi halves in the buffer (out of its range for a lane that does not store), the lo run 64
// bytes on.  neg1 = a RUN-TIME -1: with the literal hipcc folds fma(h, -1, u) into a conversion and a subtraction.  STORE = false
// (measurement build): the arithmetic without the stores.  (conv3x3_direct_r_kernel writes the same lines out: see there.)
template <bool STORE = true>
__device__ __forceinline__ void pair_store4(float v0, float v1, float v2, float v3, float s_out, float neg1, __amdgpu_buffer_rsrc_t rs, int off) {
    const float u0 = v0 * s_out, u1 = v1 * s_out, u2 = v2 * s_out, u3 = v3 * s_out;
    const unsigned h01 = pack_half2(u0, u1), h23 = pack_half2(u2, u3);
    const unsigned l01 = pack_half2(fma_half<0>(h01, neg1, u0), fma_half<1>(h01, neg1, u1));
    const unsigned l23 = pack_half2(fma_half<0>(h23, neg1, u2), fma_half<1>(h23, neg1, u3));
    if (STORE) {
        __builtin_amdgcn_raw_buffer_store_b64((dd_u32x2){h01, h23}, rs, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b64((dd_u32x2){l01, l23}, rs, off, 64, 0);
    } else asm volatile("" :: "v"(h01), "v"(h23), "v"(l01), "v"(l23), "v"(off));
}
