// pairs.h -- the primitives of the fp32-grade kernels on the fp16 matrix pipe, one definition each: buffer descriptors and 16-byte
// LDS-DMA requests, the power-of-two activation scales, the exact split of a float into an fp16 pair hi + lo and the arithmetic on
// packed pairs.  A float times a power of two splits exactly into hi = fp16(v), lo = fp16(v - hi) (11 + 11 significant bits); the
// products of fp16 halves are exact in the MFMA's fp32 accumulator, so  x w = xh wh + xl wh + xh wl  (the dropped xl wl is 2^-22 of
// the product) is an fp32-grade product.  The weights are split on the host (vpr/heads.py::pair_split).
#pragma once
#include <stdint.h>
#include <hip/hip_fp16.h>

typedef _Float16 pair_f16x2 __attribute__((ext_vector_type(2)));

// ---- memory

// Buffer descriptor of [base, base + bytes), base and size made wave-uniform: a lane's offset is one register, the stage's an SGPR,
// and offsets beyond the size read as zero (stores to them are dropped).  The size is clamped at `lim`; two clamps are in use --
// RSRC_LIM16 in conv_stem_direct_h.hip, conv_direct_r.hip and conv_direct_p.hip, RSRC_LIM everywhere else.
#define RSRC_LIM 0x7fffffff
#define RSRC_LIM16 0x7ffffff0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const char *base, int64_t bytes, int64_t lim) {
    const uint64_t a = (uint64_t)base;
    const uint64_t u = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)a);
    const int n = __builtin_amdgcn_readfirstlane((int)(bytes > lim ? lim : bytes));
    return __builtin_amdgcn_make_buffer_rsrc((void *)u, 0, n, 0x00020000);
}
// LDS-DMA in the MUBUF encoding (`buffer_load_dwordx4 ... lds`): 16 bytes per lane to lds_wave_base + 16 lane.  `global_load_lds` is
// FLAT-encoded with an LDS operand: hipcc's waitcnt pass marks it "pending flat" and from then on turns every `lgkmcnt(N)` into
// `lgkmcnt(0)` -- a K step's MFMAs then wait for ALL fragment reads issued before them.  The buffer form carries no such mark, takes
// the stage's offset in an SGPR (soff) and the lane's in ONE register (voff).  AUX: cache-policy bits (gfx940+: bit 0 = sc0, bit 1 = nt,
// bit 4 = sc1).  (A __device__ function, not the builtin inside a kernel's lambda: with the LDS-DMA builtin called from a lambda
// hipcc 7.2's HOST pass emits no launch stub for the kernel and says nothing -- the library then fails to load with an undefined symbol.)
template <int AUX = 0>
__device__ __forceinline__ void buf_lds16(__amdgpu_buffer_rsrc_t rs, int voff, int soff, char *lds_wave_base) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)lds_wave_base, 16, voff, soff, 0, AUX);
}

// ---- power-of-two activation scales s from max |x| (clamped to [1e-30, 1e30]).  Three rules, each for its own bracket of max|x| s:

// A: max|x| s <= 327.68 -- the F(4x4) input transform (B^T d B grows max |x| by up to 100) stays below 2^15
__device__ __forceinline__ float scale_le_327_68(float amax) {
    const float a = fminf(fmaxf(amax, 1e-30f), 1e30f);
    int e;
    (void)frexpf(327.68f / a, &e);                        // r = m 2^e, m in [0.5, 1): floor(log2 r) = e - 1
    return ldexpf(1.0f, e - 1);
}
// B: max|x| s <= 2^15 - 16 = 32752 (fp16 holds 65504; the products stay far inside fp32)
__device__ __forceinline__ float scale_le_32752(float amax) {
    const float a = fminf(fmaxf(amax, 1e-30f), 1e30f);
    int e;
    (void)frexpf(32752.0f / a, &e);
    return ldexpf(1.0f, e - 1);
}
// C: max|x| s in [2^13, 2^14) -- the scale of the pair-format maps: the hi halves keep 11 bits, the lo halves stay normal fp16 numbers
// for every value within 2^-10 of the maximum (smaller ones lose nothing that matters: their absolute error is 2^-25 of the scaled maximum)
__device__ __forceinline__ float scale_in_2p13_2p14(float amax) {
    const float a = fminf(fmaxf(amax, 1e-30f), 1e30f);
    int e;
    (void)frexpf(a, &e);
    return ldexpf(1.0f, 14 - e);
}

// ---- pairs

// v - (float)half HI of the packed pair h: one v_fma_mix_f32 (the fp16 operand is read straight out of the packed register; written as
// fmaf((float)half, -1, v) hipcc 7.2 converts the half back to float and subtracts: three instructions per value).  __host__ too: it is
// called from kernel lambdas that the host pass compiles as well.
template <int HI>
__host__ __device__ __forceinline__ float sub_half(float v, __half2 h) {
#if defined(__HIP_DEVICE_COMPILE__)
    float d;
    const unsigned hb = *(const unsigned *)&h;
    if (HI) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hb), "v"(v));
    else asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hb), "v"(v));
    return d;
#else
    return v - (HI ? __high2float(h) : __low2float(h));
#endif
}
// (float)half HI of hb * s + v: hipcc selects ONE v_fma_mix_f32 for this (as inline assembly the scheduler cannot place it: a
// sched_group_barrier pipeline leaves every asm statement of a region behind the region's last MFMA)
template <int HI>
__device__ __forceinline__ float fma_half(unsigned hb, float s, float v) {
    return __builtin_fmaf((float)__builtin_bit_cast(pair_f16x2, hb)[HI], s, v);
}
__device__ __forceinline__ unsigned pack_half2(float a, float b) {       // (fp16 rn(a), fp16 rn(b)) in one dword
    const __half2 h = __floats2half2_rn(a, b);
    return *(const unsigned *)&h;
}
__device__ __forceinline__ unsigned pack_pair(float v) {                 // [fp16(v) | fp16(v - fp16(v)) << 16]
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    return (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
}

// ---- maxima

__device__ __forceinline__ float max_f32(float a, float b) {   // (fmaxf first canonicalises both operands: two more instructions per maximum)
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// max(v, v of lane ^ 1): a DPP quad permutation (as `__shfl_xor` it is a ds_bpermute_b32 with an LDS round trip behind it)
__device__ __forceinline__ float max_f32_xor1(float v) {
    const float a = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(a));
    return r;
}
