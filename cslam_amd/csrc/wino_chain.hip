// wino_chain.hip -- F(4x4, 3x3) output transform of layer L chained into the input transform of layer L + 1 (gfx950).
// Between two Winograd layers on the same map the activation y_L is written by wino4_output_kernel (winograd.hip) and read
// straight back by wino4_input_h2_kernel (wino_gemm.hip): 64 + 64 bytes per tile and channel next to the 144 of M in and the
// 144 of V out.  Both transforms are per-channel spatial operations, so a workgroup that owns one frame x one group of CG
// channels and walks the map's full-width tile rows top to bottom needs no halo of recomputed tiles: it keeps the last pixel
// rows of y_L in an LDS ring and y_L never reaches HBM.
//   step r:  M (tile row r, loaded during step r - 1) -> A^T M A, descale, bias, ReLU -> 4 pixel rows into the ring
//            barrier;  the loads of M (tile row r + 1) are issued;
//            pixel rows 4 r - 5 .. 4 r of the ring -> B^T d B of tile row r - 1 -> fp16 pairs -> V2;  barrier
// One thread = one tile x 4 consecutive channels in both halves (the operation order of the two kernels it replaces: y and V2
// are bit-equal to theirs for the same scales).  The scale of V_{L+1} cannot come from the measured max |y_L| -- that is known
// when the kernel ends -- so it comes from the a-priori bound  max |x_L| wl1 + bmax  (wl1 = largest L1 norm of an output channel's
// 3x3 weights, bmax = max |bias|); the measured maximum still goes to a slot: it is the next layer's max |x|.
#include "common.h"
#include "pairs.h"
#include <hip/hip_fp16.h>

typedef float cf4 __attribute__((ext_vector_type(4)));
typedef unsigned cu2 __attribute__((ext_vector_type(2)));
typedef unsigned cu4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wc_at4(const cf4 m0, const cf4 m1, const cf4 m2, const cf4 m3, const cf4 m4, const cf4 m5,
                                       cf4 &s0, cf4 &s1, cf4 &s2, cf4 &s3) {   // winograd.hip::wino4_at on 4 channels
    const cf4 a = m1 + m2, bq = m1 - m2, c = m3 + m4, e = m3 - m4;
    s0 = m0 + a + c;
    s1 = bq + 2.0f * e;
    s2 = a + 4.0f * c;
    s3 = bq + 8.0f * e + m5;
}
__device__ __forceinline__ void wc_bt4(cf4 &d0, cf4 &d1, cf4 &d2, cf4 &d3, cf4 &d4, cf4 &d5) {   // = wino_gemm.hip::wg_bt4
    const cf4 r0 = 4.0f * d0 - 5.0f * d2 + d4;
    const cf4 r1 = -4.0f * (d1 + d2) + d3 + d4;
    const cf4 r2 = 4.0f * (d1 - d2) - d3 + d4;
    const cf4 r3 = 2.0f * (d3 - d1) - d2 + d4;
    const cf4 r4 = 2.0f * (d1 - d3) - d2 + d4;
    const cf4 r5 = 4.0f * d1 - 5.0f * d3 + d5;
    d0 = r0; d1 = r1; d2 = r2; d3 = r3; d4 = r4; d5 = r5;
}

#define WC_THREADS 128
#define WC_RING 9              // pixel rows of y in LDS: exactly the live ones, 4 r - 5 .. 4 r + 3 at step r (two barriers per step; 12 rows would
                               // need one, but 9 let TWO workgroups share a compute unit's LDS, and the two waves of one fill only two of its SIMDs)

struct WcArgs {
    const float *mb;           // the workgroup's M: tile row 0, tile column 0, first channel of the group, frequency 0 (wave-uniform: the
    __half *vb;                //   address arithmetic of the 72 loads and stores of a step stays on the scalar unit); its V2 likewise
    unsigned moff, voff;       // this thread's element inside a tile row of M (floats) / of V2 (halfs; the odd lane's lo block included)
    float *rp;                 // ring + its channel offset
    int64_t mplane, vplane, mrow, vrow;     // floats / halfs per frequency, per tile row
    int H, TH, Wr, tj;
    float inv, sc;
    cf4 bv;
    cf4 clim;                  // +inf where column 4 tj + j lies in the map, 0 where the tile hangs over it
    bool odd;
};

// One step of the walk (see the head of the file); OUT / LOAD / IN say which of its three parts tile row r has: the first and the last
// two steps lack some, and with the parts compiled in or out the loads of M are unconditional (no copies of the 36 loaded registers,
// which would wait for them in the middle of the transform they are to overlap).
template <int CG, bool OUT, bool LOAD, bool IN>
__device__ __forceinline__ void wc_step(const WcArgs &a, const int r, cf4 (&m)[36], float &vmax) {
    if (OUT) {
        // ---- output transform of tile row r, exactly wino4_output_kernel<true, false>'s arithmetic
        cf4 s[4][6];
#pragma unroll
        for (int j = 0; j < 6; ++j)
            wc_at4(m[j], m[6 + j], m[12 + j], m[18 + j], m[24 + j], m[30 + j], s[0][j], s[1][j], s[2][j], s[3][j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cf4 o[4];
            wc_at4(s[i][0], s[i][1], s[i][2], s[i][3], s[i][4], s[i][5], o[0], o[1], o[2], o[3]);
            const int h = 4 * r + i;
            float *row = a.rp + ((h % WC_RING) * a.Wr + 4 * a.tj) * CG;
            // pixels of a tile that hangs over the map (14 -> 16) are zeros to the next layer and no part of max |y|: min(v, 0) = 0 for
            // the ReLU's v >= 0, min(v, +inf) = v
            const cf4 lim = h < a.H ? a.clim : (cf4)(0.0f);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cf4 v = __builtin_elementwise_max(o[j] * a.inv + a.bv, (cf4)(0.0f));
                v = __builtin_elementwise_min(v, (cf4)(lim[j]));
                vmax = fmaxf(fmaxf(vmax, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
                *(cf4 *)(row + j * CG) = v;
            }
        }
    }
    __syncthreads();
    if (LOAD) {
        const float *p = a.mb + (r + 1) * a.mrow;
#pragma unroll
        for (int q = 0; q < 36; ++q) m[q] = __builtin_nontemporal_load((const cf4 *)(p + q * a.mplane + a.moff));
    }
    if (IN) {
        // ---- input transform of tile row r - 1 out of the ring, exactly wino4_input_h2_kernel<true>'s arithmetic
        // The ring holds zeros where a tile hangs over the map; the row above and below the tiles and the column left and right of
        // them are not in it: those reads go to a slot that holds something else and are replaced by zeros, with the predicate and the
        // select of wino4_input_h2_kernel -- the compiler then contracts B^T d B into the same fused multiply-adds as there, which V2's
        // last bit depends on.  Every read is made unconditional (the empty asm): a predicated LDS read becomes a branch and a wait apiece.
        const int h0 = 4 * (r - 1) - 1, w0 = 4 * a.tj - 1;
        const int Hr = 4 * a.TH;
        cf4 d[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int hh = h0 + i;
            const float *row = a.rp + ((hh + WC_RING) % WC_RING) * a.Wr * CG;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int ww = w0 + j;
                const bool in = (hh >= 0) & (hh < Hr) & (ww >= 0) & (ww < a.Wr);
                cf4 v = *(const cf4 *)(row + (j == 0 ? max(ww, 0) : j == 5 ? min(ww, a.Wr - 1) : ww) * CG);
                asm("" : "+v"(v));
                d[i][j] = in ? v * a.sc : (cf4)(0.0f);
            }
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) wc_bt4(d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]);
#pragma unroll
        for (int i = 0; i < 6; ++i) wc_bt4(d[i][0], d[i][1], d[i][2], d[i][3], d[i][4], d[i][5]);
        __half *o = a.vb + (r - 1) * a.vrow;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const cf4 v = d[i][j];
                const __half2 h0v = __floats2half2_rn(v.x, v.y), h1v = __floats2half2_rn(v.z, v.w);
                const __half2 l0v = __floats2half2_rn(sub_half<0>(v.x, h0v), sub_half<1>(v.y, h0v));
                const __half2 l1v = __floats2half2_rn(sub_half<0>(v.z, h1v), sub_half<1>(v.w, h1v));
                cu2 hi, lo;
                hi.x = *(const unsigned *)&h0v; hi.y = *(const unsigned *)&h1v;
                lo.x = *(const unsigned *)&l0v; lo.y = *(const unsigned *)&l1v;
                // lanes 2k / 2k + 1 hold channels 8k .. 8k + 7 of one tile: the even lane stores the 16 bytes of hi halves, the odd lane
                // the 16 bytes of lo halves (CG / 4 is even: a lane's partner is a thread of the workgroup)
                const cu2 give = a.odd ? hi : lo;
                cu2 got;
                got.x = (unsigned)__builtin_amdgcn_mov_dpp((int)give.x, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
                got.y = (unsigned)__builtin_amdgcn_mov_dpp((int)give.y, 0xB1, 0xF, 0xF, true);
                cu4 v16;
                if (a.odd) { v16.x = got.x; v16.y = got.y; v16.z = lo.x; v16.w = lo.y; }
                else { v16.x = hi.x; v16.y = hi.y; v16.z = got.x; v16.w = got.y; }
                __builtin_nontemporal_store(v16, (cu4 *)(o + (6 * i + j) * a.vplane + a.voff));
            }
    }
    __syncthreads();           // the next step's rows overwrite the oldest ones this step has read
}

// M [36][T][C] float32 (T = B TH TW tiles) -> V2 [36][T][C/32][hi 32 | lo 32] fp16 of the NEXT layer.  Workgroup = (frame, channel
// group of CG) with TW CG / 4 threads; thread = (tile column tid / (CG/4), channels 4 (tid % (CG/4)) ..+3).
// *vscale: the slot V_L was scaled by (M carries sV sU); *amax_x: measured max |x_L|; *amax_out (zeroed): max |y_L|;
// *bound_out: the bound V2 is scaled by -- layer L + 1's output stage descales with it.
template <int CG>
__global__ __launch_bounds__(WC_THREADS) void wino4_chain_h2_kernel(const float *__restrict__ M, const float *__restrict__ bias,
                                                                     int B, int H, int W, int C,
                                                                     const unsigned *__restrict__ vscale, float inv_su,
                                                                     const unsigned *__restrict__ amax_x, float wl1, float bmax,
                                                                     unsigned *__restrict__ amax_out,
                                                                     unsigned *__restrict__ bound_out, __half *__restrict__ V2) {
    extern __shared__ __attribute__((aligned(16))) float ring[];        // [WC_RING][4 TW][CG]
    __shared__ unsigned wg_amax;
    constexpr int C4G = CG / 4;
    WcArgs a;
    a.H = H;
    a.TH = (H + 3) >> 2;
    const int TW = (W + 3) >> 2;
    a.Wr = 4 * TW;
    const int ncg = C / CG;
    const int b = blockIdx.x / ncg, cg = blockIdx.x - b * ncg;
    a.tj = threadIdx.x / C4G;
    const int c4 = threadIdx.x % C4G;
    const int c = cg * CG + 4 * c4;
    const int64_t T = (int64_t)B * a.TH * TW;
    const int64_t t0 = (int64_t)b * a.TH * TW;                          // the frame's first tile
    if (threadIdx.x == 0) wg_amax = 0u;

    a.inv = inv_su / scale_le_327_68(__uint_as_float(*vscale));
    const float bound = fmaf(__uint_as_float(*amax_x), wl1, bmax);
    a.sc = scale_le_327_68(bound);
    if (blockIdx.x == 0 && threadIdx.x == 0) *bound_out = __float_as_uint(bound);
    a.bv = bias ? *(const cf4 *)(bias + c) : (cf4)(0.0f);
#pragma unroll
    for (int j = 0; j < 4; ++j) a.clim[j] = 4 * a.tj + j < W ? __builtin_inff() : 0.0f;
    a.odd = threadIdx.x & 1;
    a.mplane = T * C;
    a.vplane = T * 2 * C;
    a.mrow = (int64_t)TW * C;
    a.vrow = (int64_t)TW * 2 * C;
    a.mb = M + t0 * C + cg * CG;
    a.vb = V2 + t0 * 2 * C + cg * 2 * CG;
    a.moff = a.tj * C + 4 * c4;
    a.voff = a.tj * 2 * C + (c4 >> 3) * 64 + (4 * c4 & 31) + (a.odd ? 32 - 4 : 0);
    a.rp = ring + 4 * c4;
    float vmax = 0.0f;

    cf4 m[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) m[q] = __builtin_nontemporal_load((const cf4 *)(a.mb + q * a.mplane + a.moff));
    const int TH = a.TH;
    if (TH == 1) {
        wc_step<CG, true, false, false>(a, 0, m, vmax);
    } else {
        wc_step<CG, true, true, false>(a, 0, m, vmax);
#pragma unroll 1
        for (int r = 1; r < TH - 1; ++r) wc_step<CG, true, true, true>(a, r, m, vmax);
        wc_step<CG, true, false, true>(a, TH - 1, m, vmax);
    }
    wc_step<CG, false, false, true>(a, TH, m, vmax);
    // max |y|: wave maximum, LDS maximum of the workgroup, one global atomic and only if it would raise the slot (atomicMax on the bits
    // of non-negative floats: the result does not depend on the order)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&wg_amax, __float_as_uint(vmax));
    __syncthreads();
    if (threadIdx.x == 0 && wg_amax > *(volatile unsigned *)amax_out) atomicMax(amax_out, wg_amax);
}

template <int CG>
static int wino4_chain_launch(const float *d_M, const float *d_bias, int B, int H, int W, int C, const unsigned *d_vscale,
                              float inv_su, const unsigned *d_amax_x, float wl1, float bmax, unsigned *d_amax_out,
                              unsigned *d_bound_out, void *d_V2, void *stream) {
    const size_t lds = (size_t)WC_RING * 4 * ((W + 3) / 4) * CG * sizeof(float);
    ARG_CHECK(lds <= 144 * 1024, "map too wide for the LDS ring");
    static DeviceOnce once;
    int dev;
    if (once.todo(&dev)) {
        HIP_TRY(hipFuncSetAttribute((const void *)wino4_chain_h2_kernel<CG>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
        once.done(dev);
    }
    hipLaunchKernelGGL(wino4_chain_h2_kernel<CG>, dim3((unsigned)((int64_t)B * (C / CG))), dim3(((W + 3) / 4) * (CG / 4)), lds, (hipStream_t)stream,
                       d_M, d_bias, B, H, W, C, d_vscale, inv_su, d_amax_x, wl1, bmax, d_amax_out, d_bound_out, (__half *)d_V2);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_wino4_chain_h2_dev(const float *d_M, const float *d_bias, int B, int H, int W, int C,
                                       const unsigned *d_vscale, float inv_su, const unsigned *d_amax_x, float wl1, float bmax,
                                       unsigned *d_amax_out, unsigned *d_bound_out, void *d_V2, void *stream) {
    PTR_DEVICE(d_M);
    ARG_CHECK(d_M && d_V2 && d_vscale && d_amax_x && d_amax_out && d_bound_out, "NULL argument");
    ARG_CHECK(B >= 1 && H >= 1 && W >= 1, "empty map");
    ARG_CHECK(C >= 32 && (C % 32) == 0, "C must be a multiple of 32");
    ARG_CHECK(inv_su > 0.0f && wl1 >= 0.0f && bmax >= 0.0f, "inv_su must be positive, wl1 and bmax non-negative");
    const int TW = (W + 3) / 4;
    ARG_CHECK(TW <= 16, "maps wider than 64 pixels stay on the separate transforms");
    ARG_CHECK((int64_t)B * (C / 32) < (1LL << 31), "too many frames for one launch");
    // the widest channel group whose tile row fits the workgroup: 128-byte runs of M per tile at 32 channels, 512 at 128
    if (TW <= 4 && (C % 128) == 0)
        return wino4_chain_launch<128>(d_M, d_bias, B, H, W, C, d_vscale, inv_su, d_amax_x, wl1, bmax, d_amax_out, d_bound_out, d_V2, stream);
    if (TW <= 8 && (C % 64) == 0)
        return wino4_chain_launch<64>(d_M, d_bias, B, H, W, C, d_vscale, inv_su, d_amax_x, wl1, bmax, d_amax_out, d_bound_out, d_V2, stream);
    return wino4_chain_launch<32>(d_M, d_bias, B, H, W, C, d_vscale, inv_su, d_amax_x, wl1, bmax, d_amax_out, d_bound_out, d_V2, stream);
}
