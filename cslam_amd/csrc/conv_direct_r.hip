// conv_direct_r.hip -- 3x3 / stride 1 / pad 1 convolution 64 -> 128 channels (VGG-16 conv2_1 on 112 x 112 maps: cslam/vpr/netvlad.py:
// 163-171,227) as ONE direct kernel whose weights never leave the register files (gfx950), fp32-grade on the fp16 matrix pipe.
//
// conv_stem_direct_h.hip's second layer with the activation read from HBM instead of computed from the image (what the two share is
// written once, in direct_dev.h): 64 x 128 x 9 weights as exact fp16 pairs are 295 KB -- 288 registers per lane for each of the four
// one-per-SIMD waves of a workgroup.  Wave w owns OUTPUT channels 32 w .. 32 w + 31 (two 16-row A tiles of v_mfma_f32_16x16x32_f16) for
// all 128 pixels of an 8 x 16 block:
//   * weights [9 taps][2 K steps of 32 channels][2 channel tiles][hi | lo] loaded once per kernel: no weight stream through L2 / LDS, no
//     weight ring, no stage barriers (conv_direct_h.hip streams 16 KB per (tap, slab) stage and synchronises after each);
//   * the 10 x 18-pixel x 64-channel patch of the input in LDS as exact fp16 pairs (direct_dev.h's pair patch: 320-byte pixels,
//     swizzled 16-byte chunks), shared by the four waves, double buffered: block i + 1's patch is loaded (float32, HBM / L2 -> registers)
//     during block i's first columns and split into the idle buffer during its later ones, a few vector instructions behind every MFMA;
//   * a B fragment = one patch row (16 pixels) x 32 channels at a column shift dx serves the three taps dy = 0, 1, 2 and both channel
//     tiles: 2 fragment reads per up to 18 MFMAs (conv_direct_h.hip: 8 per 12);
//   * no partial sums, ONE barrier per block.
// Arithmetic as conv_direct_h.hip: x scaled by the power of two s_x from the producer's max |x| slot and split into hi + lo when the patch
// is staged; w split offline (`direct_r_pair_weights`); acc = wh xh + wh xl + wl xh; y = [pool](relu(acc / (s_x s_w) + bias)).
//
// 128 -> 128 channels (VGG-16 conv2_2, + MaxPool2d) runs on the SAME body (conv3x3_direct_r2_kernel, round 6).  128 x 128 x 9 weights as
// fp16 pairs are 590 KB: more than a compute unit's 512 KB of registers, which is why conv_direct_h.hip streams them through an LDS ring
// -- 16 KB per (tap, 32-channel slab) and 256 pixels, 14.8 GB of L2 -> LDS traffic per 256 frames, and with it that kernel sits 15-25 %
// above what its flop and its HBM bytes cost at the board's power cap.  HALF the output channels are 295 KB and
// fit: the two workgroups 2 j, 2 j + 1 of an XCD walk the SAME blocks, one per output-channel half, so the input leaves HBM once (the
// partner's reads hit the XCD's L2) and no weight ever moves again.  Wave w owns output channels 64 half + 16 w .. + 15 (ONE 16-row A
// tile) for all 128 pixels of an 8 x 16 block and all 128 input channels: a block is two passes over the 64-channel patch (slab 0,
// slab 1; the accumulators stay), each pass stages the next one's patch -- (same block, slab 1), then (next block, slab 0) -- inside its
// MFMA stream; 2 fragment reads per up to 9 MFMAs; the epilogue rides in slab 1's last column.  What differs between the two is `DRForm`.
#include <stdlib.h>
#include <type_traits>
#include <hip/hip_fp16.h>
#include "common.h"
#include "pairs.h"
#include "direct_dev.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define DR_NEL 12                      // float4 elements per thread and patch: 180 pixels x 16 = 2880 <= 12 x 256
// a staged element's stores (dpatch_split_store): 8 bytes of hi halves at its destination, 8 of lo halves 128 bytes further; an element
// that does not exist (the last staging round's) goes to a sink, 16 (lane & 63) into it -- no branch around a store
#define DR_SINK_END (63 * 16 + DPATCH_LO + 8)

// ---- what conv2_1 (R2 = false) and conv2_2 (R2 = true) do differently: everything else below is one text
template <bool R2> struct DRForm {
    // 16-channel A tiles per wave: conv2_1's four waves share 128 output channels, conv2_2's share the 64 of their workgroup's half
    static constexpr int MT = R2 ? 1 : 2;
    // 64-channel slabs of the input = passes over the patch per block (the accumulators stay; a wave's 288 weight registers are
    // [9 taps][2 K steps][MT tiles x NSLAB slabs = 2][hi | lo] either way)
    static constexpr int NSLAB = R2 ? 2 : 1;
    // workgroups 2 j, 2 j + 1 of an XCD walk the same blocks, one per output-channel half (direct_partition<true>)
    static constexpr bool WG_PAIRS = R2;
    // weight taps pinned in the accumulation half of the register file, next to the accumulators: 6 x 32 + 64 = 7 x 32 + 32 = the 256 AGPRs
    static constexpr int AGPR_TAPS = R2 ? 7 : 6;
    // the per-element source offsets of the staging loads.  conv2_2 has registers to spare and a vector instruction budget that is short
    // -- three slots per MFMA and wave, and half the MFMAs per patch: the offsets live in registers (an add and a select per request
    // instead of ten instructions).  conv2_1 recomputes them from the thread id at every load: twelve more registers spilled
    static constexpr bool SRC_IN_REGS = R2;
    // the sink.  conv2_2: one behind EACH patch buffer at the same offset (one add per destination, no select), DR_SINK_END = 1144 bytes
    // rounded up to keep the second buffer at the first one's alignment mod 256 -- the bank pattern of the fragment reads.  conv2_1: one
    // behind both buffers, chosen by a select when the element is split
    static constexpr bool SINK_PER_BUF = R2;
    static constexpr int SINKB = R2 ? 1280 : 4096;
    static constexpr int BUF = DPATCH_BYTES + (SINK_PER_BUF ? SINKB : 0);
    static constexpr int LDS = 2 * BUF + (SINK_PER_BUF ? 0 : SINKB);
    // vector instructions the scheduler places behind every MFMA of a region (twice as many in the column that carries the epilogue):
    // conv2_2's regions have half the MFMAs for the same staging
    static constexpr int VALU_PER_MFMA = R2 ? 4 : 2;
    // the staging splits start in column 3 in both: three columns behind the loads.  conv2_2's three columns are 216 MFMAs -- with two, as
    // conv2_1's twice-as-long columns would allow, its first splits stalled on HBM latency: 2.03-2.09 ms against 1.98-2.00; splits in the
    // last two columns only: no better
    static constexpr int SPLIT_COL0 = 3;
    // the second word of packed patch columns is filled in a loop of its own in conv2_1 and inside the table loop in conv2_2, as each
    // was written: either way round, hipcc orders the other kernel's tables differently and with them its whole block loop
    static constexpr bool PC2_OWN_LOOP = !R2;
    static_assert(DR_SINK_END <= SINKB, "a sink store leaves its sink");
    static_assert(!SINK_PER_BUF || BUF % 256 == 0, "the second buffer moves in the banks");
};

struct ConvDirectRArgs {
    const float *x; const f16x8 *w2; const float *bias; float *y;
    int B, H, W, gxb, gyb, nblk;
    const unsigned *amax_in; float inv_sw; unsigned *amax_out;
    float wl1, bmax; unsigned *bound_out;          // OUTP: y leaves in pair format (conv_igemm.hip), scaled for the bound max|x| wl1 + bmax
};

#ifdef CSLAM_ABLATIONS
__device__ unsigned long long *dr_prof = nullptr;             // measurement build: [six columns (+ staging), epilogue, barrier, blocks] ticks of wave 0 / workgroup 0 (conv2_1)
extern "C" __attribute__((visibility("default"))) int cslam_debug_dr_prof_dev(void *d_buf) {
    unsigned long long *q = (unsigned long long *)d_buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(dr_prof), &q, sizeof(q)) == hipSuccess ? 0 : -2;
}
#define DR_PROF 1
#else
#define DR_PROF 0
#endif
#define DR_C(T) std::integral_constant<int, T>{}

// DBG (builds with -DCSLAM_ABLATIONS only; WRONG results, timing): 1 = no patch staging inside the loop, 4 = no stores, 8 = no requests
// inside the loop (the splits work on stale registers), 16 = requests, no splits
// OUTP (conv2_1, no pooling): y is written in the PAIR FORMAT of conv_igemm.hip -- [pixel][32-channel block][hi 32 | lo 32] fp16 of s y, s
// the power of two that brings the bound max|x| wl1 + bmax (stored to bound_out) into [2^13, 2^14) -- so that the next layer (conv2_2,
// conv_direct_h.hip) stages its patch without converting anything (0.34 of its 2.5 ms were the split's vector instructions)
template <bool R2, bool POOL, bool RELU, int DBG, bool OUTP>
__device__ __forceinline__ void conv3x3_direct_r_body(ConvDirectRArgs p) {
    typedef DRForm<R2> F;
    constexpr int MT = F::MT, NSLAB = F::NSLAB;
    static_assert(!(POOL && OUTP), "the pair-format output is written un-pooled");
    static_assert(!(R2 && OUTP), "the pair-format output is conv2_1's");
    extern __shared__ __attribute__((aligned(16))) char dr_smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gq = lane >> 4, l15 = lane & 15;

    const float amax = fminf(fmaxf(__uint_as_float(*p.amax_in), 1e-30f), 1e30f);        // (for OUTP's bound: the scale clamps on its own)
    const float sx = scale_le_32752(__uint_as_float(*p.amax_in));
    const float inv = p.inv_sw / sx;
    float s_out = 1.0f, neg1 = -1.0f;
    if (!R2) asm volatile("" : "+v"(neg1));                    // (a run-time -1 for the pair-format store: pair_store4, direct_dev.h)
    if (OUTP) {
        const float bound = (amax * p.wl1 + p.bmax) * 1.001f;  // >= max |y| whatever the rounding of the products
        s_out = scale_in_2p13_2p14(bound);
        if (blockIdx.x == 0 && threadIdx.x == 0) *p.bound_out = __float_as_uint(bound);
    }

    // blocks to workgroups (R2: to workgroup pairs) by XCD
    const DirectPart part = direct_partition<F::WG_PAIRS>(p.nblk);
    const int half = part.half, n_mine = part.n_mine;
    if (n_mine <= 0) return;

    // ---- this wave's weights: [tap][K step][channel tile (R2: slab)][hi | lo], 288 registers; 256 of them, with the accumulators, pinned
    // in the accumulation half of the register file (MFMA operands and nothing else)
    f16x8 wr[9][2][2][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                for (int hl = 0; hl < 2; ++hl) {
                    wr[tap][ks][ts][hl] = p.w2[((((((half * 4 + wave) * 9 + tap) * 2 + ks) * 2 + ts) * 2 + hl) * 64) + lane];
                    if (tap < F::AGPR_TAPS) asm volatile("" : "+a"(wr[tap][ks][ts][hl]));
                }
    float4 bv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
        bv[mt] = p.bias ? *(const float4 *)(p.bias + 64 * half + 16 * MT * wave + 16 * mt + 4 * gq) : make_float4(0.f, 0.f, 0.f, 0.f);

    typedef DirectBlk Blk;
    auto decode_blk = [&](int bi) { return direct_decode_blk(part, bi, p.gxb, p.gyb); };

    // ---- patch staging: element e = i * 256 + tid = (pixel e >> 4, float4 e & 15 of the slab's 64 channels)
    int st_dst[DR_NEL];                                        // destination in a patch buffer (no element: its sink, or -1 where patch_split selects)
    int st_src[F::SRC_IN_REGS ? DR_NEL : 1];                   // source offset from the patch's first pixel (-1: none)
    unsigned st_pc = 0, st_pc2 = 0;                            // packed patch columns (5 bits each)
#pragma unroll
    for (int i = 0; i < DR_NEL; ++i) {
        const int e = i * 256 + tid, px = e >> 4, f4 = e & 15;
        const int pr = (px * 3641) >> 16, pc = px - 18 * pr;   // px / 18 for px < 4096
        const bool valid = px < DPATCH_NPIX;
        st_dst[i] = valid ? DPATCH_OFF(pr, pc, f4 >> 1, f4 & 1) : (F::SINK_PER_BUF ? DPATCH_BYTES + (tid & 63) * 16 : -1);
        if constexpr (F::SRC_IN_REGS) st_src[i] = valid ? ((pr * p.W + pc) * (64 * NSLAB) + f4 * 4) * 4 : -1;
        if (i < 6) st_pc |= (unsigned)(valid ? pc : 0) << (5 * i);
        else if (!F::PC2_OWN_LOOP) st_pc2 |= (unsigned)(valid ? pc : 0) << (5 * (i - 6));
    }
    if (F::PC2_OWN_LOOP) {
#pragma unroll
        for (int i = 6; i < DR_NEL; ++i) {
            const int e = i * 256 + tid, px = e >> 4;
            const int pr = (px * 3641) >> 16, pc = px - 18 * pr;
            st_pc2 |= (unsigned)(px < DPATCH_NPIX ? pc : 0) << (5 * (i - 6));
        }
    }
    const int img_bytes = p.H * p.W * (256 * NSLAB);
    u32x4 stg[DR_NEL];
    // the image is the buffer: rows above and below it are out of its range and read as zero; columns left and right of it would read the
    // neighbouring row's pixels and are zeroed when the registers are split.  Every lane issues every load (no branch): counted waits.
    auto patch_load = [&](const Blk &b, int slab, int i) {
        const __amdgpu_buffer_rsrc_t rsX = buf_rsrc((const char *)p.x + (int64_t)b.img * img_bytes, img_bytes, RSRC_LIM16);
        const int blk_off = ((b.by * 8 - 1) * p.W + (b.bx * 16 - 1)) * (256 * NSLAB) + slab * 256;
        if constexpr (F::SRC_IN_REGS) {
            int off = st_src[i] + blk_off;
            asm volatile("" : "+v"(off));                      // (computed by every lane: one select, no branch)
            stg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsX, st_src[i] >= 0 ? off : 0x7fffffff, 0, 0);
        } else {
            int t = tid;
            asm volatile("" : "+v"(t));                        // opaque: the twelve offsets are loop invariants otherwise, hoisted and spilled
            const int e = i * 256 + t, px = e >> 4;
            const int pr = (px * 3641) >> 16, pc = px - 18 * pr;
            int off = ((pr * p.W + pc) * 64 + (e & 15) * 4) * 4 + blk_off;
            asm volatile("" : "+v"(off));                      // computed by every lane: written as one select hipcc turns the "expensive" arm
            stg[i] = __builtin_amdgcn_raw_buffer_load_b128(rsX, px < DPATCH_NPIX ? off : 0x7fffffff, 0, 0);     // into a branch, and a branch ends the region
        }
    };
    auto patch_split = [&](const Blk &b, int i, char *patch) {
        // (vector instructions are what this staging costs -- three slots per MFMA and wave: the column test is one bit-field extract, one
        // add and one unsigned compare, the scale two packed multiplies)
        const unsigned pc = __builtin_amdgcn_ubfe(i < 6 ? st_pc : st_pc2, 5 * (i < 6 ? i : i - 6), 5);
        const float s = (unsigned)(b.bx * 16 - 1) + pc < (unsigned)p.W ? sx : 0.0f;         // (column - 1 wraps to a large number)
        // (branch-free: a region must stay ONE basic block for its instruction order to be set; what does not exist goes to the sink)
        dpatch_split_store(stg[i], s, [&] { return F::SINK_PER_BUF || st_dst[i] >= 0 ? patch + st_dst[i] : dr_smem + 2 * F::BUF + (tid & 63) * 16; });
    };

    // ---- the products.  acc[r][mt]: output row r, lane (l15, gq) = pixel column l15, channels 64 half + 16 MT wave + 16 mt + 4 gq .. + 3
    f32x4 acc[8][MT];
    int fr_off[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) fr_off[dx] = DPATCH_OFF(0, l15 + dx, gq, 0);
    f16x8 fh[3], fl[3];
    auto frag_read = [&](auto col_tag, auto r_tag, const char *patch) {
        constexpr int COL = decltype(col_tag)::value, R = decltype(r_tag)::value;
        constexpr int DX = COL >> 1, KS = COL & 1, SLOT = (R + COL) % 3;
        fh[SLOT] = *(const f16x8 *)(patch + fr_off[DX] + R * DPATCH_RP + KS * 64);
        fl[SLOT] = *(const f16x8 *)(patch + fr_off[DX] + R * DPATCH_RP + KS * 64 + DPATCH_LO);
    };
    // ---- epilogue, a row (pair) at a time: output row r has its last contribution in the LAST column's patch row r + 2, so its bias /
    // ReLU / stores ride in that column's next region, under the MFMAs of the rows still open -- only the last row (pair) is left
    // behind the block's last MFMA.  (As one phase behind the columns: 3.5k of a block's 21k cycles, the matrix pipe idle.)  Buffer stores,
    // the image's output map = the buffer (a lane that does not store gets an offset out of its range: no branch).
    float my_amax = 0.0f;
    const int Ho = POOL ? p.H >> 1 : p.H, Wo = POOL ? p.W >> 1 : p.W;
    Blk eb = {0, 0, 0};                                        // the block being multiplied
    auto epi_rows = [&](int k) {                               // POOL: pooled row k (output rows 2 k, 2 k + 1); else output row k
        const __amdgpu_buffer_rsrc_t rsY = buf_rsrc((const char *)(p.y + (int64_t)eb.img * Ho * Wo * 128), (int64_t)Ho * Wo * 512, RSRC_LIM16);
        const int ox = eb.bx * 16 + l15;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int ch_off = (64 * half + 16 * MT * wave + 16 * mt + 4 * gq) * 4;
            float4 v;
            bool store;
            int off;
            if (POOL) {
                const int py = eb.by * 4 + k;
                v.x = max_f32_xor1(max_f32(acc[2 * k][mt][0], acc[2 * k + 1][mt][0])); v.y = max_f32_xor1(max_f32(acc[2 * k][mt][1], acc[2 * k + 1][mt][1]));
                v.z = max_f32_xor1(max_f32(acc[2 * k][mt][2], acc[2 * k + 1][mt][2])); v.w = max_f32_xor1(max_f32(acc[2 * k][mt][3], acc[2 * k + 1][mt][3]));
                store = ((l15 & 1) == 0) & ((ox >> 1) < Wo) & (py < Ho);
                off = (py * Wo + (ox >> 1)) * 512 + ch_off;
            } else {
                const int oy = eb.by * 8 + k;
                v.x = acc[k][mt][0]; v.y = acc[k][mt][1]; v.z = acc[k][mt][2]; v.w = acc[k][mt][3];
                store = (ox < p.W) & (oy < p.H);
                off = (oy * p.W + ox) * 512 + ch_off;
            }
            v.x = v.x * inv + bv[mt].x; v.y = v.y * inv + bv[mt].y; v.z = v.z * inv + bv[mt].z; v.w = v.w * inv + bv[mt].w;
            if (RELU) { v.x = fmaxf(v.x, 0.0f); v.y = fmaxf(v.y, 0.0f); v.z = fmaxf(v.z, 0.0f); v.w = fmaxf(v.w, 0.0f); }
            float m = max_f32(max_f32(fabsf(v.x), fabsf(v.y)), max_f32(fabsf(v.z), fabsf(v.w)));
            asm volatile("" : "+v"(m), "+v"(off));             // (both computed by every lane: no branch around them)
            my_amax = max_f32(my_amax, store ? m : 0.0f);
            if (OUTP) {
                // the lane's four channels 32 wave + 16 mt + 4 gq .. + 3 of the pixel: block `wave`, hi run at its halfs 16 mt + 4 gq
                // (pair_store4 of direct_dev.h written out: through the helper hipcc schedules this epilogue differently inside the block loop)
                const float u0 = v.x * s_out, u1 = v.y * s_out, u2 = v.z * s_out, u3 = v.w * s_out;
                const unsigned h01 = pack_half2(u0, u1), h23 = pack_half2(u2, u3);
                const unsigned l01 = pack_half2(fma_half<0>(h01, neg1, u0), fma_half<1>(h01, neg1, u1));
                const unsigned l23 = pack_half2(fma_half<0>(h23, neg1, u2), fma_half<1>(h23, neg1, u3));
                const int offp = store ? off - ch_off + wave * 128 + (16 * mt + 4 * gq) * 2 : 0x7fffffff;
                __builtin_amdgcn_raw_buffer_store_b64((dd_u32x2){h01, h23}, rsY, offp, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64((dd_u32x2){l01, l23}, rsY, offp, 64, 0);
            } else {
                u32x4 bits;
                bits.x = __float_as_uint(v.x); bits.y = __float_as_uint(v.y); bits.z = __float_as_uint(v.z); bits.w = __float_as_uint(v.w);
                if (!(DBG & 4)) __builtin_amdgcn_raw_buffer_store_b128(bits, rsY, store ? off : 0x7fffffff, 0, 0);
                else asm volatile("" :: "v"(bits));
            }
        }
    };

    // one scheduling region per patch row: the fragment two rows ahead, the row's 3 MT .. 9 MT MFMAs, and a slice of the next pass's staging
    // (column 0: its loads, columns 3 .. 5: the split of four elements each); SL = the slab this pass multiplies, `nslab` the one it stages
    auto rstep = [&](auto col_tag, auto r_tag, auto slab_tag, const char *patch, const Blk &nblk, int nslab, char *npatch) {
        constexpr int COL = decltype(col_tag)::value, R = decltype(r_tag)::value, SL = decltype(slab_tag)::value;
        constexpr int DX = COL >> 1, KS = COL & 1, SLOT = (R + COL) % 3;
        constexpr bool EPI = SL == NSLAB - 1 && COL == 5;       // the block's last column: finished output rows leave
        if constexpr (R + 2 < 10) frag_read(col_tag, std::integral_constant<int, (R + 2) % 10>{}, patch);
        else if constexpr (COL < 5) frag_read(std::integral_constant<int, (COL + 1) % 6>{}, std::integral_constant<int, (R + 2) % 10>{}, patch);
        if constexpr (COL == 0 && R >= 1 && R <= 6 && !(DBG & 1) && !(DBG & 8)) { patch_load(nblk, nslab, 2 * (R - 1)); patch_load(nblk, nslab, 2 * (R - 1) + 1); }
#pragma unroll
        for (int prod = 0; prod < 3; ++prod)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int r = R - dy;
                    if (r < 0 || r > 7) continue;
                    const int ts = R2 ? SL : mt;               // the weights' third index: this slab's, or this channel tile's
                    const f16x8 a = prod == 2 ? wr[3 * dy + DX][KS][ts][1] : wr[3 * dy + DX][KS][ts][0];
                    const f16x8 b = prod == 1 ? fl[SLOT] : fh[SLOT];
                    acc[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, (SL == 0 && COL == 0 && prod == 0 && dy == 0) ? (f32x4)(0.0f) : acc[r][mt], 0, 0, 0);
                }
        if constexpr (COL >= F::SPLIT_COL0 && (R == 1 || R == 3 || R == 5 || R == 7) && !(DBG & 1) && !(DBG & 16)) patch_split(nblk, 4 * (COL - F::SPLIT_COL0) + (R - 1) / 2, npatch);
        if constexpr (EPI && !POOL && R >= 3) epi_rows(R - 3);                                  // output row R - 3 was finished by the last region
        if constexpr (EPI && POOL && (R == 4 || R == 6 || R == 8)) epi_rows((R - 4) / 2);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
        constexpr int NM = 3 * MT * ((R < 2 ? R + 1 : 3) - (R > 7 ? R - 7 : 0));
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, EPI ? 2 * F::VALU_PER_MFMA : F::VALU_PER_MFMA, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto column = [&](auto col_tag, auto slab_tag, const char *patch, const Blk &nblk, int nslab, char *npatch) {
        rstep(col_tag, DR_C(0), slab_tag, patch, nblk, nslab, npatch); rstep(col_tag, DR_C(1), slab_tag, patch, nblk, nslab, npatch);
        rstep(col_tag, DR_C(2), slab_tag, patch, nblk, nslab, npatch); rstep(col_tag, DR_C(3), slab_tag, patch, nblk, nslab, npatch);
        rstep(col_tag, DR_C(4), slab_tag, patch, nblk, nslab, npatch); rstep(col_tag, DR_C(5), slab_tag, patch, nblk, nslab, npatch);
        rstep(col_tag, DR_C(6), slab_tag, patch, nblk, nslab, npatch); rstep(col_tag, DR_C(7), slab_tag, patch, nblk, nslab, npatch);
        rstep(col_tag, DR_C(8), slab_tag, patch, nblk, nslab, npatch); rstep(col_tag, DR_C(9), slab_tag, patch, nblk, nslab, npatch);
    };
    // one pass: slab SL of the block in `patch` is multiplied, (nblk, nslab) is staged into `npatch`
    auto pass = [&](auto slab_tag, const char *patch, const Blk &nblk, int nslab, char *npatch) {
        frag_read(DR_C(0), DR_C(0), patch);
        frag_read(DR_C(0), DR_C(1), patch);
        column(DR_C(0), slab_tag, patch, nblk, nslab, npatch); column(DR_C(1), slab_tag, patch, nblk, nslab, npatch);
        column(DR_C(2), slab_tag, patch, nblk, nslab, npatch); column(DR_C(3), slab_tag, patch, nblk, nslab, npatch);
        column(DR_C(4), slab_tag, patch, nblk, nslab, npatch); column(DR_C(5), slab_tag, patch, nblk, nslab, npatch);
    };

    [[maybe_unused]] unsigned long long t_main = 0, t_epi = 0, t_bar = 0, t1 = 0, t2 = 0, t3 = 0;
    // ---- prologue: (block 0, slab 0) into buffer 0
    Blk cb = decode_blk(0);
#pragma unroll
    for (int i = 0; i < DR_NEL; ++i) patch_load(cb, 0, i);
#pragma unroll
    for (int i = 0; i < DR_NEL; ++i) patch_split(cb, i, dr_smem);
    __syncthreads();
    char *const buf0 = dr_smem, *const buf1 = dr_smem + F::BUF;
    for (int bi = 0; bi < n_mine; ++bi) {
        const int cur = bi & 1;                                // (one slab: the block's patch and the idle buffer swap roles)
        const char *const patch = dr_smem + cur * F::BUF;
        char *const npatch = dr_smem + (cur ^ 1) * F::BUF;
        const Blk nb = decode_blk(bi + 1);
        eb = cb;
        if constexpr (NSLAB == 2) {
            pass(DR_C(0), buf0, cb, 1, buf1);                  // slab 0 of the block; its slab 1 is staged into the other buffer
            __syncthreads();
            pass(DR_C(1), buf1, nb, 0, buf0);                  // slab 1; the next block's slab 0 is staged
            epi_rows(POOL ? 3 : 7);
        } else {
            if (DR_PROF) t1 = __builtin_amdgcn_s_memtime();
            pass(DR_C(0), patch, nb, 0, npatch);                // the next block's patch is staged into the idle buffer
            if (DR_PROF) { t2 = __builtin_amdgcn_s_memtime(); t_main += t2 - t1; }
            epi_rows(POOL ? 3 : 7);                            // the last row (pair): nothing left to hide it under
            if (DR_PROF) { t3 = __builtin_amdgcn_s_memtime(); t_epi += t3 - t2; }
        }
        // ONE barrier per pass: the next one's patch is whole, everybody is through this one's
        __syncthreads();
        if (DR_PROF && NSLAB == 1) t_bar += __builtin_amdgcn_s_memtime() - t3;
        cb = nb;
    }
#ifdef CSLAM_ABLATIONS
    if (NSLAB == 1 && dr_prof && blockIdx.x == 0 && tid == 0) { dr_prof[0] = t_main; dr_prof[1] = t_epi; dr_prof[2] = t_bar; dr_prof[3] = (unsigned long long)n_mine; }
#endif

    if (p.amax_out) amax_publish(my_amax, p.amax_out, dr_smem, tid, lane);
}

// the two kernels: conv2_1 (64 -> 128 channels) and conv2_2 (128 -> 128, one output-channel half per workgroup)
template <bool POOL, bool RELU, int DBG = 0, bool OUTP = false>
__global__ __launch_bounds__(256, 1) void conv3x3_direct_r_kernel(ConvDirectRArgs p) { conv3x3_direct_r_body<false, POOL, RELU, DBG, OUTP>(p); }
template <bool POOL, bool RELU, int DBG = 0>
__global__ __launch_bounds__(256, 1) void conv3x3_direct_r2_kernel(ConvDirectRArgs p) { conv3x3_direct_r_body<true, POOL, RELU, DBG, false>(p); }

/* y = [pool](relu(conv3x3(x, w) + bias)), Cout = 128; x, y NHWC float32; d_amax = 4-byte slot holding (a bound of) max |x|; d_amax_out (or
 * NULL): zeroed slot that receives max |y|.  r2 = 0: Cin = 64, d_w2r = `direct_r_pair_weights` (vpr/winograd.py): [4 output-channel
 * quarters][9 taps][2 K steps][2 channel tiles][hi | lo][64 lanes][8] halfs of s_w w, inv_sw = 1 / s_w.  r2 = 1: Cin = 128, d_w2r =
 * `direct_r2_pair_weights`: [2 output-channel halves][4 quarters of a half][9 taps][2 K steps][2 input-channel slabs][hi | lo][64 lanes][8]. */
static int conv_direct_r_launch(int r2, const float *d_x, const void *d_w2r, const float *d_bias, int B, int H, int W, int Cin,
                                int Cout, int relu, int pool, const unsigned *d_amax, float inv_sw,
                                unsigned *d_amax_out, float *d_y, void *stream, int out_pairs, float wl1, float bmax, unsigned *d_bound_out) {
    PTR_DEVICE(d_x);
    ARG_CHECK(!out_pairs || (!pool && relu && d_bound_out && wl1 >= 0.0f && bmax >= 0.0f), "pair-format output: ReLU, no pooling, wl1, bmax and the bound slot");
    ARG_CHECK(d_x && d_w2r && d_y && d_amax, "NULL argument");
    ARG_CHECK(B >= 1 && H >= 1 && W >= 1, "empty map");
    if (r2) ARG_CHECK(Cin == 128 && Cout == 128, "Cin and Cout must be 128");
    else ARG_CHECK(Cin == 64 && Cout == 128, "Cin must be 64 and Cout 128");
    ARG_CHECK(!pool || ((H % 2) == 0 && (W % 2) == 0), "pooling needs even H and W");
    ARG_CHECK(inv_sw > 0.0f, "inv_sw must be positive");
    ARG_CHECK((int64_t)H * W * 512 < 0x7ffffff0ll, "one image's maps must stay below 2 GiB (32-bit buffer offsets)");
    ConvDirectRArgs a;
    a.x = d_x; a.w2 = (const f16x8 *)d_w2r; a.bias = d_bias; a.y = d_y;
    a.B = B; a.H = H; a.W = W;
    a.gxb = (int)ceil_div64(W, 16); a.gyb = (int)ceil_div64(H, 8);
    const int64_t nblk = (int64_t)B * a.gxb * a.gyb;
    ARG_CHECK(nblk < (1ll << 30), "too many blocks for one launch");
    a.nblk = (int)nblk;
    a.amax_in = d_amax; a.inv_sw = inv_sw; a.amax_out = d_amax_out;
    a.wl1 = wl1; a.bmax = bmax; a.bound_out = d_bound_out;
    const int n_cu = cslam_cu_count();
    ARG_CHECK(n_cu >= 1 + r2, "no HIP device");
    // one workgroup per block stream; r2: workgroup pairs (block stream, output-channel half) -- whole pairs only, XCD-aligned when the
    // device allows it
    const int wpb = 1 + r2;
    int grid = !r2 || n_cu % 16 == 0 ? n_cu : (n_cu & ~1);
    if (wpb * nblk < grid) grid = (int)(wpb * nblk);
    const dim3 g(grid), b(256);
    hipStream_t st = (hipStream_t)stream;
    constexpr int lds = DRForm<false>::LDS, lds2 = DRForm<true>::LDS;
#ifdef CSLAM_ABLATIONS
    if (const char *e = getenv("CSLAM_DR_DBG")) {              // timing-only ablations (wrong results): 1 = no staging inside the loop, 4 = no stores, r2: 8 = no requests, 16 = no splits
        const int d = atoi(e);
        if (r2) {
            if (d == 1) return launch_lds<conv3x3_direct_r2_kernel<true, true, 1>>(g, b, lds2, st, a);
            if (d == 4) return launch_lds<conv3x3_direct_r2_kernel<true, true, 4>>(g, b, lds2, st, a);
            if (d == 5) return launch_lds<conv3x3_direct_r2_kernel<true, true, 5>>(g, b, lds2, st, a);
            if (d == 8) return launch_lds<conv3x3_direct_r2_kernel<true, true, 8>>(g, b, lds2, st, a);
            if (d == 16) return launch_lds<conv3x3_direct_r2_kernel<true, true, 16>>(g, b, lds2, st, a);
        } else if (!out_pairs) {
            if (d == 1) return launch_lds<conv3x3_direct_r_kernel<false, true, 1>>(g, b, lds, st, a);
            if (d == 4) return launch_lds<conv3x3_direct_r_kernel<false, true, 4>>(g, b, lds, st, a);
            if (d == 5) return launch_lds<conv3x3_direct_r_kernel<false, true, 5>>(g, b, lds, st, a);
        }
    }
#endif
    if (out_pairs) return launch_lds<conv3x3_direct_r_kernel<false, true, 0, true>>(g, b, lds, st, a);
    if (r2) {
        if (pool) return relu ? launch_lds<conv3x3_direct_r2_kernel<true, true>>(g, b, lds2, st, a) : launch_lds<conv3x3_direct_r2_kernel<true, false>>(g, b, lds2, st, a);
        return relu ? launch_lds<conv3x3_direct_r2_kernel<false, true>>(g, b, lds2, st, a) : launch_lds<conv3x3_direct_r2_kernel<false, false>>(g, b, lds2, st, a);
    }
    if (pool) return relu ? launch_lds<conv3x3_direct_r_kernel<true, true>>(g, b, lds, st, a) : launch_lds<conv3x3_direct_r_kernel<true, false>>(g, b, lds, st, a);
    return relu ? launch_lds<conv3x3_direct_r_kernel<false, true>>(g, b, lds, st, a) : launch_lds<conv3x3_direct_r_kernel<false, false>>(g, b, lds, st, a);
}
/* VGG-16 conv2_1 (64 -> 128 channels): cslam/vpr/netvlad.py:163-171,227. */
CSLAM_API int cslam_conv3x3_direct_r_dev(const float *d_x, const void *d_w2r, const float *d_bias, int B, int H, int W, int Cin,
                                         int Cout, int relu, int pool, const unsigned *d_amax, float inv_sw,
                                         unsigned *d_amax_out, float *d_y, void *stream) {
    return conv_direct_r_launch(0, d_x, d_w2r, d_bias, B, H, W, Cin, Cout, relu, pool, d_amax, inv_sw, d_amax_out, d_y, stream, 0, 0.0f, 0.0f, nullptr);
}
/* VGG-16 conv2_2 (128 -> 128 channels, + MaxPool2d): cslam/vpr/netvlad.py:163-171,227. */
CSLAM_API int cslam_conv3x3_direct_r2_dev(const float *d_x, const void *d_w2r2, const float *d_bias, int B, int H, int W, int Cin,
                                          int Cout, int relu, int pool, const unsigned *d_amax, float inv_sw,
                                          unsigned *d_amax_out, float *d_y, void *stream) {
    return conv_direct_r_launch(1, d_x, d_w2r2, d_bias, B, H, W, Cin, Cout, relu, pool, d_amax, inv_sw, d_amax_out, d_y, stream, 0, 0.0f, 0.0f, nullptr);
}
/* conv2_1 (64 -> 128 channels, + bias + ReLU, no pooling) with y written in the PAIR FORMAT of cslam_conv_igemm_h2p_dev:
 * [B,H,W,4 blocks][hi 32 | lo 32] fp16 of s y, s the power of two of the bound *d_amax wl1 + bmax, which goes to d_bound_out (wl1 = max_co
 * sum |w[co]|, bmax = max |bias|); d_amax_out (optional, zeroed) receives the measured max |y|.  VGG-16 conv2_1 in front of a conv2_2
 * that stages its patch from pairs (cslam_conv3x3_direct_hp_dev): cslam/vpr/netvlad.py:163-171,227. */
CSLAM_API int cslam_conv3x3_direct_r_pairs_dev(const float *d_x, const void *d_w2r, const float *d_bias, int B, int H, int W, int Cin,
                                               int Cout, const unsigned *d_amax, float inv_sw, float wl1, float bmax,
                                               unsigned *d_amax_out, unsigned *d_bound_out, void *d_y, void *stream) {
    return conv_direct_r_launch(0, d_x, d_w2r, d_bias, B, H, W, Cin, Cout, 1, 0, d_amax, inv_sw, d_amax_out, (float *)d_y, stream, 1, wl1, bmax, d_bound_out);
}
