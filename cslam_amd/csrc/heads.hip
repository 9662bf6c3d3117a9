// heads.hip -- descriptor heads of the two extractors + the image transform (gfx950).
//
//   l2_normalize      F.normalize(p=2)  layers.py:32-36 / netvlad.py:105-106,126-128,
//                     and sklearn.preprocessing.normalize (netvlad.py:235-236)
//   vlad_aggregate    NetVLADLayer.forward                    cslam/vpr/netvlad.py:94-130
//   gem_fc_head       L2Norm -> GeM -> Flatten -> Linear -> L2Norm
//                                          cslam/vpr/cosplace_utils/network.py:23-29, layers.py:8-36
//   preprocess        CenterCrop -> Resize(bicubic, PIL, antialias, 8-bit) -> ToTensor -> Normalize
//                                          cslam/vpr/netvlad.py:202-208, cosplace.py:73-79
//
// All of these are HBM-bandwidth bound: one workgroup per image / row,
// coalesced reads along the contiguous (pixel) axis, wave64 shuffle reductions, LDS for the
// per-image intermediates.  float32 arithmetic like the reference's torch float32 modules.
#include <stdlib.h>
#include "common.h"
#include "pairs.h"
#include <mutex>
#include <vector>

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// block-wide sum (blockDim.x multiple of 64, <= 1024); red: >= 16 floats of LDS
__device__ __forceinline__ float block_sum_f32(float v, float *red) {
    v = wave_sum_f32(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.0f;
    for (int w = 0; w < nw; ++w) t += red[w];
    return t;
}

// ------------------------------------------------------------- l2 normalise ----
__global__ __launch_bounds__(256) void l2_normalize_kernel(float *__restrict__ x, int d, int64_t ld, float eps,
                                                           int zero_norm_to_one) {
    __shared__ float red[16];
    float *row = x + (int64_t)blockIdx.x * ld;
    float s = 0.0f;
    for (int c = threadIdx.x; c < d; c += blockDim.x) { float v = row[c]; s += v * v; }
    float nrm = sqrtf(block_sum_f32(s, red));
    float den = zero_norm_to_one ? (nrm == 0.0f ? 1.0f : nrm) : fmaxf(nrm, eps);
    for (int c = threadIdx.x; c < d; c += blockDim.x) row[c] = row[c] / den;
}

CSLAM_API int cslam_l2_normalize_dev(float *d_x, int64_t n, int d, int64_t ld, float eps,
                                     int zero_norm_to_one, void *stream) {
    PTR_DEVICE(d_x);
    ARG_CHECK(d_x || n == 0, "NULL argument");
    ARG_CHECK(n >= 0 && d > 0 && ld >= d, "bad n / d / ld");
    if (n == 0) return CSLAM_OK;
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, d_x, d, ld,
                       eps, zero_norm_to_one);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

// ------------------------------------------------------------- NetVLAD head ----
// One workgroup per image.  K = 64 clusters (netvlad.py:176), C <= 512 channels.
// Pixels are processed in chunks of PCH: phase B (one thread per pixel) computes the pixel's
// inverse L2 norm and the 64 soft-assignment logits in ONE pass over the channels
// (logit = inv_norm * sum_c W[k,c] x[c,p], linear), softmax over k -> a[p][k] in LDS;
// phase C (one thread per channel) accumulates V[k,c] += a[p][k] * x[c,p]*inv_norm[p].
#define VK 64
#define VPCH 128
#define VWCH 32
__global__ __launch_bounds__(512) void vlad_generic_kernel(const float *__restrict__ feat, const float *__restrict__ W,
                                                   const float *__restrict__ bias, const float *__restrict__ cent,
                                                   int C, int P, float *__restrict__ out, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *a_lds = (float *)smem;                    // [VPCH][VK]
    float *w_lds = a_lds + VPCH * VK;                // [VWCH][VK]  (transposed weight chunk)
    float *invn = w_lds + VWCH * VK;                 // [VPCH]
    float *red = invn + VPCH;                        // [16][VK] + 16
    const int tid = threadIdx.x, nt = blockDim.x;
    const float *x = feat + (size_t)blockIdx.x * C * P;
    const int c_own = tid;                           // channel owned in phase C (tid < C)

    float acc[VK], asum[VK];
#pragma unroll
    for (int k = 0; k < VK; ++k) { acc[k] = 0.0f; asum[k] = 0.0f; }

    for (int p0 = 0; p0 < P; p0 += VPCH) {
        const int pn = P - p0 < VPCH ? P - p0 : VPCH;
        // ---- phase B: thread tid < pn owns pixel p0 + tid
        float lg[VK];
#pragma unroll
        for (int k = 0; k < VK; ++k) lg[k] = 0.0f;
        float ss = 0.0f;
        for (int c0 = 0; c0 < C; c0 += VWCH) {
            __syncthreads();
            for (int e = tid; e < VWCH * VK; e += nt) {        // w_lds[cc][k] = W[k][c0+cc]
                int k = e / VWCH, cc = e - k * VWCH;
                w_lds[cc * VK + k] = (c0 + cc < C) ? W[(size_t)k * C + c0 + cc] : 0.0f;
            }
            __syncthreads();
            if (tid < pn) {
                const int cn = C - c0 < VWCH ? C - c0 : VWCH;
                for (int cc = 0; cc < cn; ++cc) {
                    float xv = x[(size_t)(c0 + cc) * P + p0 + tid];
                    ss += xv * xv;
                    const float4 *wr = (const float4 *)(w_lds + cc * VK);
#pragma unroll
                    for (int k4 = 0; k4 < VK / 4; ++k4) {
                        float4 w4 = wr[k4];
                        lg[4 * k4 + 0] += w4.x * xv; lg[4 * k4 + 1] += w4.y * xv;
                        lg[4 * k4 + 2] += w4.z * xv; lg[4 * k4 + 3] += w4.w * xv;
                    }
                }
            }
        }
        if (tid < pn) {
            float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);           // F.normalize(dim=1), netvlad.py:105-106
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < VK; ++k) { lg[k] = lg[k] * inv + (bias ? bias[k] : 0.0f); mx = fmaxf(mx, lg[k]); }
            float se = 0.0f;
#pragma unroll
            for (int k = 0; k < VK; ++k) { lg[k] = expf(lg[k] - mx); se += lg[k]; }
            float rs = 1.0f / se;
#pragma unroll
            for (int k = 0; k < VK; ++k) a_lds[tid * VK + k] = lg[k] * rs;   // softmax over clusters, :109-110
            invn[tid] = inv;
        }
        __syncthreads();
        // ---- phase C: thread c_own < C accumulates over the chunk's pixels
        if (c_own < C) {
            for (int pp = 0; pp < pn; ++pp) {
                float xv = x[(size_t)c_own * P + p0 + pp] * invn[pp];
                const float4 *ar = (const float4 *)(a_lds + pp * VK);
#pragma unroll
                for (int k4 = 0; k4 < VK / 4; ++k4) {
                    float4 a4 = ar[k4];
                    acc[4 * k4 + 0] += a4.x * xv; acc[4 * k4 + 1] += a4.y * xv;
                    acc[4 * k4 + 2] += a4.z * xv; acc[4 * k4 + 3] += a4.w * xv;
                    asum[4 * k4 + 0] += a4.x; asum[4 * k4 + 1] += a4.y;
                    asum[4 * k4 + 2] += a4.z; asum[4 * k4 + 3] += a4.w;
                }
            }
        }
    }
    // V[k,c] = sum_p a[k,p] (x[c,p] - cent[k,c])  (netvlad.py:115-124)
#pragma unroll
    for (int k = 0; k < VK; ++k)
        acc[k] = (c_own < C) ? acc[k] - asum[k] * cent[(size_t)k * C + c_own] : 0.0f;
    // intra-normalisation over c for every k (netvlad.py:126), then global L2 (:127-128)
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < VK; ++k) {
        float s = wave_sum_f32(acc[k] * acc[k]);
        if (lane == 0) red[wave * VK + k] = s;
    }
    __syncthreads();
    float gsum = 0.0f;
#pragma unroll
    for (int k = 0; k < VK; ++k) {
        float t = 0.0f;
        for (int w = 0; w < nw; ++w) t += red[w * VK + k];
        float nk = sqrtf(t);
        float sc = 1.0f / fmaxf(nk, 1e-12f);
        acc[k] *= sc;
        float nn = nk * sc;
        gsum += nn * nn;
    }
    float gs = 1.0f / fmaxf(sqrtf(gsum), 1e-12f);
    if (c_own < C) {
        float *o = out + (size_t)blockIdx.x * ldo;
#pragma unroll
        for (int k = 0; k < VK; ++k) o[(size_t)k * C + c_own] = acc[k] * gs;
    }
}

// Fast path (P <= 256 pixels, e.g. NetVLAD's 14x14): the image's feature map is streamed twice
// through LDS in 32-channel slabs (contiguous 32*P floats in NCHW, coalesced, next slab prefetched
// into registers while the current one is consumed), so no thread ever waits on a dependent
// global load.  Sweep 1: thread = pixel, accumulates ||x_p||^2 and the 64 logits; softmax -> a[p][k]
// (pre-scaled by 1/||x_p||) in LDS.  Sweep 2: thread = (channel in slab, group of 4 clusters),
// V[k,c] = sum_p a'[p][k] x[c,p] with x read conflict-free (slab row stride P_PAD = 257) and a' as one
// broadcast ds_read_b128; the 16x4 results per thread stay in registers until the two normalisations.
#define VL_CC 32
#define VL_PMAX 256
#define VL_PPAD 257
// NHWC: the feature map is [P][C] (channels_last storage, what the Winograd trunk writes) instead of [C][P]: a slab element is
// then (pixel e / 32, channel e % 32) -- 128-byte runs per pixel -- and the layout conversion pass before the head is gone.
template <bool NHWC>
__global__ __launch_bounds__(512) void vlad_fast_kernel(const float *__restrict__ feat, const float *__restrict__ W,
                                                        const float *__restrict__ bias, const float *__restrict__ cent,
                                                        int C, int P, float *__restrict__ out, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *a_lds = (float *)smem;                     // [VL_PMAX][VK]   a'[p][k] = softmax * inv_norm
    float *xs = a_lds + VL_PMAX * VK;                 // [VL_CC][VL_PPAD]
    float *ws = xs + VL_CC * VL_PPAD;                 // [VL_CC][VK]
    float *invn = ws + VL_CC * VK;                    // [VL_PMAX]
    float *asum = invn + VL_PMAX;                     // [VK]
    float *red = asum + VK;                           // [VK] + 16
    const int tid = threadIdx.x;
    const float *x = feat + (size_t)blockIdx.x * C * P;
    const int nslab = (C + VL_CC - 1) / VL_CC;
    const int slab_elems = VL_CC * P;                 // <= 8192
    constexpr int NPF = (VL_CC * VL_PMAX + 511) / 512;   // 16 prefetch registers per thread

    float pf[NPF];
    auto prefetch = [&](int sl) {
        const int base = sl * slab_elems, limit = C * P;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            int e = i * 512 + tid;
            if (NHWC) {
                const int pp = e >> 5, cc = e & 31, c = sl * VL_CC + cc;
                pf[i] = (pp < P && c < C) ? x[(size_t)pp * C + c] : 0.0f;
            } else {
                pf[i] = (e < slab_elems && base + e < limit) ? x[base + e] : 0.0f;
            }
        }
    };
    // slab element e = i*512 + tid lives at (channel e / P, pixel e % P): walk it incrementally
    const int cc_start = tid / P, pp_start = tid - cc_start * P, dq = 512 / P, dr = 512 - dq * P;
    auto commit = [&]() {
        if (NHWC) {
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
                const int e = i * 512 + tid, pp = e >> 5, cc = e & 31;
                if (pp < P) xs[cc * VL_PPAD + pp] = pf[i];
            }
            return;
        }
        int cc = cc_start, pp = pp_start;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            if (i * 512 + tid < slab_elems) xs[cc * VL_PPAD + pp] = pf[i];
            cc += dq; pp += dr;
            if (pp >= P) { pp -= P; ++cc; }
        }
    };

    // ---------------- sweep 1: norms + logits (thread = pixel)
    // the two halves of the workgroup split each slab's channels: thread (half, pixel)
    const int half = tid >> 8, px = tid & 255;
    float lg[VK];
#pragma unroll
    for (int k = 0; k < VK; ++k) lg[k] = 0.0f;
    float ss = 0.0f;
    prefetch(0);
    for (int sl = 0; sl < nslab; ++sl) {
        __syncthreads();                               // previous slab fully consumed
        commit();
        const int c0 = sl * VL_CC;
        for (int e = tid; e < VL_CC * VK; e += 512) {  // ws[cc][k] = W[k][c0+cc]; lanes along k: conflict-free
            int cc = e >> 6, k = e & 63;
            ws[cc * VK + k] = (c0 + cc < C) ? W[(size_t)k * C + c0 + cc] : 0.0f;
        }
        if (sl + 1 < nslab) prefetch(sl + 1);
        __syncthreads();
        if (px < P) {
#pragma unroll 4
            for (int ci = 0; ci < VL_CC / 2; ++ci) {
                const int cc = half * (VL_CC / 2) + ci;
                float xv = xs[cc * VL_PPAD + px];
                ss += xv * xv;
                const float4 *wr = (const float4 *)(ws + cc * VK);
#pragma unroll
                for (int k4 = 0; k4 < VK / 4; ++k4) {
                    float4 w4 = wr[k4];
                    lg[4 * k4 + 0] += w4.x * xv; lg[4 * k4 + 1] += w4.y * xv;
                    lg[4 * k4 + 2] += w4.z * xv; lg[4 * k4 + 3] += w4.w * xv;
                }
            }
        }
    }
    // combine the two halves through a_lds, then softmax in the lower half
    if (half == 1 && px < P) {
#pragma unroll
        for (int k = 0; k < VK; ++k) a_lds[px * VK + k] = lg[k];
        invn[px] = ss;
    }
    __syncthreads();
    if (half == 0 && px < P) {
        ss += invn[px];
        float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);            // F.normalize(dim=1), netvlad.py:105-106
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < VK; ++k) {
            lg[k] = (lg[k] + a_lds[px * VK + k]) * inv + (bias ? bias[k] : 0.0f);
            mx = fmaxf(mx, lg[k]);
        }
        float se = 0.0f;
#pragma unroll
        for (int k = 0; k < VK; ++k) { lg[k] = expf(lg[k] - mx); se += lg[k]; }
        float rs = 1.0f / se;
#pragma unroll
        for (int k = 0; k < VK; ++k) a_lds[px * VK + k] = lg[k] * rs;      // softmax, netvlad.py:109-110
        invn[px] = inv;
    }
    prefetch(0);                                       // sweep 2 starts from the first slab again
    __syncthreads();
    if (tid < VK) {                                    // asum[k] = sum_p a[p][k]  (unscaled)
        float s = 0.0f;
        for (int pp = 0; pp < P; ++pp) s += a_lds[pp * VK + tid];
        asum[tid] = s;
    }
    __syncthreads();
    for (int e = tid; e < P * VK; e += 512) a_lds[e] *= invn[e / VK];       // a' = a / ||x_p||

    // ---------------- sweep 2: V[k,c] (thread = channel-in-slab x 4 clusters)
    const int cl = tid & 31, k0 = (tid >> 5) * 4;
    float vout[16][4];
#pragma unroll
    for (int sl = 0; sl < 16; ++sl)
#pragma unroll
        for (int j = 0; j < 4; ++j) vout[sl][j] = 0.0f;
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) {
        if (sl < nslab) {
            __syncthreads();
            commit();
            if (sl + 1 < nslab) prefetch(sl + 1);
            __syncthreads();
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            const float *xr = xs + cl * VL_PPAD;
#pragma unroll 4
            for (int pp = 0; pp < P; ++pp) {
                float xv = xr[pp];
                float4 a4 = *(const float4 *)(a_lds + pp * VK + k0);
                a0 += a4.x * xv; a1 += a4.y * xv; a2 += a4.z * xv; a3 += a4.w * xv;
            }
            const int c = sl * VL_CC + cl;
            if (c < C) {
                // V[k,c] = sum_p a[k,p] (x[c,p]/||x_p|| - cent[k,c])   (netvlad.py:115-124)
                vout[sl][0] = a0 - asum[k0 + 0] * cent[(size_t)(k0 + 0) * C + c];
                vout[sl][1] = a1 - asum[k0 + 1] * cent[(size_t)(k0 + 1) * C + c];
                vout[sl][2] = a2 - asum[k0 + 2] * cent[(size_t)(k0 + 2) * C + c];
                vout[sl][3] = a3 - asum[k0 + 3] * cent[(size_t)(k0 + 3) * C + c];
            }
        }
    }
    // intra-normalisation over c for every k (netvlad.py:126): the 32 lanes sharing k0 hold all c
    float sc[4], gpart = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = 0.0f;
#pragma unroll
        for (int sl = 0; sl < 16; ++sl) s += vout[sl][j] * vout[sl][j];
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        float nk = sqrtf(s);
        sc[j] = 1.0f / fmaxf(nk, 1e-12f);
        float nn = nk * sc[j];
        gpart += nn * nn;
    }
    // global L2 over all K*C (netvlad.py:127-128): sum the 16 cluster groups
    __syncthreads();
    if (cl == 0) red[tid >> 5] = gpart;
    __syncthreads();
    float gsum = 0.0f;
#pragma unroll
    for (int g = 0; g < 16; ++g) gsum += red[g];
    const float gs = 1.0f / fmaxf(sqrtf(gsum), 1e-12f);
    float *o = out + (size_t)blockIdx.x * ldo;
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) {
        const int c = sl * VL_CC + cl;
        if (sl < nslab && c < C) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[(size_t)(k0 + j) * C + c] = vout[sl][j] * sc[j] * gs;
        }
    }
}

// ---- the batch form on the f32 matrix pipe (round 3) -------------------------------------------------------------------
// vlad_fast_kernel does the two small contractions of NetVLADLayer.forward (netvlad.py:109: logits = W x; :115-124:
// V = a x^T - (sum a) cent) with one v_fma per LDS read or two: 1.2 us per frame, LDS-instruction-bound, a tenth of what the
// 0.53 MB a frame moves would cost at HBM speed.  Here both run on v_mfma_f32_32x32x2_f32 (exact f32 products and f32
// accumulation: an fmaf chain, so the result is as good as the VALU form's, in another summation order):
//   sweep 1  logits [pixel][cluster] = x [pixel][channel] W^T:  wave w = pixels 32 w .. 32 w + 31, two 32-cluster tiles,
//            K = the 128 channels of a slab;  sum x^2 per pixel on the VALU beside it
//   softmax  per pixel (thread = pixel), a' = softmax / ||x_p||, asum[k] = sum_p softmax
//   sweep 2  V [cluster][channel] = a'^T x:  wave w = cluster tile w >> 2, channel tile w & 3 of the slab, K = the pixels
//   then V - asum cent, intra-normalisation over the channels of a cluster, global L2, stores in 128-byte runs.
// x [P][C] channels-last (what the trunk writes), streamed twice in slabs of 128 channels through LDS rows of 132 floats
// (16-byte stores and reads; lanes along pixels -- sweep 1's A operand, one ds_read_b128 per four K-steps -- spread over all
// banks, lanes along channels -- sweep 2's B operand -- are consecutive); the next slab (and its 128 x 64 block of W) is
// prefetched into registers under the current slab's MFMAs.  C a multiple of 128 up to 512, 32 <= P <= 200 (14 x 14 = 196).
typedef float vf32x16 __attribute__((ext_vector_type(16)));
#define VM_CS 128
#define VM_XS 132                      // LDS row pitch of a slab of x in floats
#define VM_AP 65                       // LDS row pitch of the assignment (and of the W block) in floats
#define VM_PP 200                      // padded pixel count (even, >= P): LDS rows
#define VM_LDS_FLOATS (VM_PP * VM_XS + VM_PP * VM_AP + 256 + VK + 8 * VK + 16)
// PAIRS: the final store also writes the row as the fp16 hi / lo pairs the PCA projection multiplies (gemm_nt.hip: the layout and
// the arithmetic of pca_pairs_rows_kernel on the float32 row, so the same bits) -- A2 [S][B][K C / S / 32][hi 32 | lo 32] of s v,
// s the power of two from the bound a_given of max |v|, S = K >> kshift splits of whole clusters; `out` may then be NULL.
template <bool PAIRS>
__global__ __launch_bounds__(512) void vlad_mfma_kernel(const float *__restrict__ feat, const float *__restrict__ W,
                                                        const float *__restrict__ bias, const float *__restrict__ cent,
                                                        int C, int P, float *__restrict__ out, int64_t ldo,
                                                        unsigned short *__restrict__ A2, int kshift, float a_given) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xs = (float *)smem;                        // [VM_PP][VM_XS]
    float *a_lds = xs + VM_PP * VM_XS;                // [VM_PP][VM_AP] logits -> softmax -> a'; sweep 1: ws [VM_CS][VM_AP] lives here
    float *invn = a_lds + VM_PP * VM_AP;              // [256]
    float *asum = invn + 256;                         // [VK]
    float *red = asum + VK;                           // [8][VK] + 16
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, l31 = lane & 31;
    const float *x = feat + (size_t)blockIdx.x * C * P;
    const int nslab = C / VM_CS;
    constexpr int NPF = (VM_PP * VM_CS / 4 + 511) / 512;          // float4 prefetch registers per thread (13)
    constexpr int NWF = VM_CS * VK / 512;                          // W prefetch registers per thread (16)

    float4 pf[NPF];
    float wpf[NWF];
    // addresses as (uniform base) + (one 32-bit per-thread offset): the thirteen + sixteen loads share two offset registers
    const unsigned xoff = (unsigned)(tid >> 5) * (unsigned)C + 4u * (tid & 31);      // pixel tid >> 5 (+ 16 i), float4 tid & 31
    const unsigned woff = (unsigned)(tid >> 7) * (unsigned)C + (tid & 127);          // W row tid >> 7 (+ 4 i), channel tid & 127
    auto prefetch = [&](int sl, bool with_w) {
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const float *base = x + (size_t)(i * 16) * C + sl * VM_CS;                 // 32 float4 per pixel row of the slab
            pf[i] = i * 16 + (tid >> 5) < P ? *(const float4 *)(base + xoff) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (with_w) {
#pragma unroll
            for (int i = 0; i < NWF; ++i) wpf[i] = (W + (size_t)(i * 4) * C + sl * VM_CS)[woff];   // lanes along the channels of a row
        }
    };
    auto commit = [&](bool with_w) {                                   // rows P .. VM_PP - 1 are written as zeros
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = i * 512 + tid, pp = e >> 5, c4 = e & 31;
            if (pp < VM_PP) *(float4 *)(xs + pp * VM_XS + 4 * c4) = pf[i];
        }
        if (with_w) {
#pragma unroll
            for (int i = 0; i < NWF; ++i) {
                const int e = i * 512 + tid, k = e >> 7, cc = e & 127;
                a_lds[cc * VM_AP + k] = wpf[i];                          // ws[cc][k] = W[k][c0 + cc]
            }
        }
    };

    // ---------------- sweep 1
    const float *ws = a_lds;
    const int px = tid & 255, half = tid >> 8;                         // sum of squares: thread = (pixel, half of the slab)
    float ss = 0.0f;
    vf32x16 lg[2];                                                     // running totals; every slab sums in four chains of its own
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[n][r] = 0.0f;
    const int prow = (32 * wave + l31 < VM_PP ? 32 * wave + l31 : VM_PP - 1) * VM_XS;    // wave 6 reaches past the padded rows
    const bool mm1 = 32 * wave < P;                                    // this wave's pixel tile holds real pixels
    prefetch(0, true);
    for (int sl = 0; sl < nslab; ++sl) {
        __syncthreads();                                               // previous slab consumed (xs and ws)
        commit(true);
        if (sl + 1 < nslab) prefetch(sl + 1, true);
        __syncthreads();
        if (px < P) {
            const float4 *xr = (const float4 *)(xs + px * VM_XS + half * (VM_CS / 2));
#pragma unroll 4
            for (int c4 = 0; c4 < VM_CS / 8; ++c4) {
                const float4 v = xr[c4];
                ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
            }
        }
        if (mm1) {
            // K order: step 4 j + i takes channel 8 j + 4 h + i from the lanes of half h (both operands agree; any order of
            // the channels is a valid sum) -- one 16-byte read of x feeds four K-steps
            // (short chains: the error of a 512-term sum stays that of a blocked sum; and four independent MFMA chains).
            // The operands of group j + 1 are read from LDS while group j's eight MFMAs run.
            vf32x16 acc[2][2];
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[q][n][r] = 0.0f;
            float4 xa[2];
            float wv[2][8];
            auto fetch = [&](int j, int q) {
                xa[q] = *(const float4 *)(xs + prow + 8 * j + 4 * h);
                const float *wr = ws + (8 * j + 4 * h) * VM_AP + l31;
#pragma unroll
                for (int i = 0; i < 4; ++i) { wv[q][2 * i] = wr[i * VM_AP]; wv[q][2 * i + 1] = wr[i * VM_AP + 32]; }
            };
            auto mm = [&](int q) {
                const float av[4] = {xa[q].x, xa[q].y, xa[q].z, xa[q].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], wv[q][2 * i], acc[q][0], 0, 0, 0);
                    acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], wv[q][2 * i + 1], acc[q][1], 0, 0, 0);
                }
            };
            fetch(0, 0);
#pragma unroll 1
            for (int j = 0; j < VM_CS / 8; j += 2) {
                fetch(j + 1, 1);
                __builtin_amdgcn_sched_barrier(0);                     // keep the reads ahead of the MFMAs they hide under
                mm(0);
                __builtin_amdgcn_sched_barrier(0);
                fetch(j + 2 < VM_CS / 8 ? j + 2 : j, 0);
                __builtin_amdgcn_sched_barrier(0);
                mm(1);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) lg[n][r] += acc[0][n][r] + acc[1][n][r];
        }
    }
    if (nslab > 1) prefetch(nslab - 2, false);                         // sweep 2 walks the slabs backwards: the last one is in LDS
    __syncthreads();                                                   // ws (in a_lds) no longer needed
    if (half == 1 && px < P) invn[px] = ss;
    if (mm1) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p_ = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (p_ < VM_PP) a_lds[p_ * VM_AP + 32 * n + l31] = lg[n][r];
            }
    }
    __syncthreads();
    if (half == 0 && px < P) {
        ss += invn[px];
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);             // F.normalize(dim=1), netvlad.py:105-106
        float v[VK];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < VK; ++k) {
            v[k] = a_lds[px * VM_AP + k] * inv + (bias ? bias[k] : 0.0f);
            mx = fmaxf(mx, v[k]);
        }
        float se = 0.0f;
#pragma unroll
        for (int k = 0; k < VK; ++k) { v[k] = expf(v[k] - mx); se += v[k]; }
        const float rs = 1.0f / se;
#pragma unroll
        for (int k = 0; k < VK; ++k) a_lds[px * VM_AP + k] = v[k] * rs;  // softmax, netvlad.py:109-110
        invn[px] = inv;
    }
    __syncthreads();
    {                                                                  // asum[k] = sum_p a[p][k]  (unscaled): 8 partial sums
        const int k = tid & 63, part = tid >> 6;
        float s = 0.0f;
        for (int pp = part; pp < P; pp += 8) s += a_lds[pp * VM_AP + k];
        red[part * VK + k] = s;
    }
    __syncthreads();
    if (tid < VK) {
        float s = 0.0f;
#pragma unroll
        for (int part = 0; part < 8; ++part) s += red[part * VK + tid];
        asum[tid] = s;
    }
    for (int e = tid; e < VM_PP * VK; e += 512) {                       // a' = a / ||x_p||; padded pixels: 0
        const int pp = e >> 6, k = e & 63;
        a_lds[pp * VM_AP + k] = pp < P ? a_lds[pp * VM_AP + k] * invn[pp] : 0.0f;
    }

    // ---------------- sweep 2: wave = (cluster tile ct, channel tile nt of the slab), K = pixels
    const int ct = wave >> 2, nt = wave & 3;
    vf32x16 vo[4];
    const int kp2 = (P + 1) >> 1;                                      // pixel pairs (rows P .. VM_PP - 1 are zero on both sides)
#pragma unroll
    for (int t = 0; t < 4; ++t) {                                      // vo[t] = slab nslab - 1 - t
        const int sl = nslab - 1 - t;
#pragma unroll
        for (int r = 0; r < 16; ++r) vo[t][r] = 0.0f;
        if (sl >= 0) {
            __syncthreads();                                           // a' and asum complete (first pass) / previous slab consumed
            if (t > 0) {
                commit(false);
                if (sl > 0) prefetch(sl - 1, false);
                __syncthreads();
            }
            const float *ar = a_lds + h * VM_AP + 32 * ct + l31, *xr = xs + h * VM_XS + 32 * nt + l31;
            const int c = sl * VM_CS + 32 * nt + l31;
            float cv[16];                                              // this wave's centroid entries: in flight under the MFMAs
#pragma unroll
            for (int r = 0; r < 16; ++r) cv[r] = cent[(size_t)(32 * ct + (r & 3) + 8 * (r >> 2) + 4 * h) * C + c];
            vf32x16 v1;                                                // two chains over the pixel pairs (even / odd)
#pragma unroll
            for (int r = 0; r < 16; ++r) v1[r] = 0.0f;
            // groups of four pixel pairs (the rows up to VM_PP are zero on both sides: the last group may run past P);
            // group g + 1's operands are read from LDS while group g's MFMAs run
            const int ng = (kp2 + 3) >> 2;
            float na[4], nb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { na[i] = ar[2 * i * VM_AP]; nb[i] = xr[2 * i * VM_XS]; }
#pragma unroll 1
            for (int g = 0; g < ng; ++g) {
                float ca[4], cb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { ca[i] = na[i]; cb[i] = nb[i]; }
                const int gn = g + 1 < ng ? g + 1 : g;
#pragma unroll
                for (int i = 0; i < 4; ++i) { na[i] = ar[(8 * gn + 2 * i) * VM_AP]; nb[i] = xr[(8 * gn + 2 * i) * VM_XS]; }
                __builtin_amdgcn_sched_barrier(0);                     // reads first, then the MFMAs they hide under
                vo[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[0], cb[0], vo[t], 0, 0, 0);
                v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[1], cb[1], v1, 0, 0, 0);
                vo[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[2], cb[2], vo[t], 0, 0, 0);
                v1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[3], cb[3], v1, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) vo[t][r] += v1[r];
            // V[k,c] = sum_p a[k,p] (x[c,p]/||x_p|| - cent[k,c])   (netvlad.py:115-124)
#pragma unroll
            for (int r = 0; r < 16; ++r) vo[t][r] -= asum[32 * ct + (r & 3) + 8 * (r >> 2) + 4 * h] * cv[r];
        }
    }
    // intra-normalisation over c for every k (netvlad.py:126): a cluster's channels sit in the 32 lanes of a half-wave, the
    // slabs (registers) and the four channel-tile waves of the cluster tile
    float part[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) s = fmaf(vo[t][r], vo[t][r], s);
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        part[r] = s;
    }
    __syncthreads();
    if (l31 == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[nt * VK + 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * h] = part[r];
    }
    __syncthreads();
    float sc[16], gpart = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float s = (red[k] + red[VK + k]) + (red[2 * VK + k] + red[3 * VK + k]);
        const float nk = sqrtf(s);
        sc[r] = 1.0f / fmaxf(nk, 1e-12f);
        const float nn = nk * sc[r];
        gpart += nn * nn;                                              // the same in the four nt waves: taken from nt == 0 below
    }
    // global L2 over all K*C (netvlad.py:127-128): the 64 clusters' squared norms; lanes l31 == 0 of the nt == 0 waves hold them
    if (nt == 0 && l31 == 0) red[4 * VK + 2 * ct + h] = gpart;
    __syncthreads();
    const float gsum = (red[4 * VK] + red[4 * VK + 1]) + (red[4 * VK + 2] + red[4 * VK + 3]);
    const float gs = 1.0f / fmaxf(sqrtf(gsum), 1e-12f);
    float *o = out + (size_t)blockIdx.x * ldo;
    float psc = 1.0f;
    if (PAIRS) {                                                       // the input scale of pca_pairs_rows_kernel
        const float a = fminf(fmaxf(a_given, 1e-30f), 1e30f);
        int e;
        (void)frexpf(16384.0f / a, &e);
        psc = ldexpf(1.0f, e - 1);
    }
    const int kb = (C << kshift) >> 5;                                 // 128-byte blocks per pair row of a split
    const bool odd = l31 & 1;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int sl = nslab - 1 - t;
        if (sl >= 0) {
            const int c = sl * VM_CS + 32 * nt + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float val = vo[t][r] * sc[r] * gs;
                if (!PAIRS || out) o[(size_t)k * C + c] = val;
                if (PAIRS) {
                    // element k C + c of the row = split k >> kshift, column cc of it; the 32 lanes of a half-wave hold one block's
                    // 32 columns: neighbours exchange so that the even lane stores two hi halves and the odd lane two lo halves
                    const float sv = val * psc;
                    const unsigned mine = pack_pair(sv);
                    const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)mine, 0xB1, 0xF, 0xF, true);   // lane ^ 1
                    const unsigned word = odd ? ((other >> 16) | (mine & 0xffff0000u)) : ((mine & 0xffffu) | (other << 16));
                    const int cc = (k & ((1 << kshift) - 1)) * C + c;
                    const int64_t blk = ((int64_t)(k >> kshift) * gridDim.x + blockIdx.x) * kb + (cc >> 5);
                    *(unsigned *)(A2 + blk * 64 + (odd ? 32 + l31 - 1 : l31)) = word;
                }
            }
        }
    }
}

// ---- small batches (the online path: one keyframe per call) ----------------------------------------------
// vlad_fast_kernel keeps one image in one workgroup, which is the right shape for a batch (256 images fill the chip)
// but leaves 255 CUs idle for a single keyframe (272 us, latency of 32 dependent slab steps).  For B <= 8 the same
// arithmetic is split three ways: (1) soft-assignment per 16-pixel tile, (2) residual aggregation per 32-channel
// slab, (3) the two normalisations per cluster.  Partial sums cross kernels through a small scratch buffer and
// are always added in a fixed order (deterministic).  netvlad.py:94-130.
#define VS_PT 16
__global__ __launch_bounds__(256) void vlad_wt_kernel(const float *__restrict__ W, int C, float *__restrict__ Wt) {
    const int e = blockIdx.x * 256 + threadIdx.x;          // Wt[c][k] = W[k][c]
    if (e < C * VK) Wt[e] = W[(size_t)(e & (VK - 1)) * C + (e >> 6)];
}

__global__ __launch_bounds__(256) void vlad_assign_kernel(const float *__restrict__ feat, const float *__restrict__ Wt,
                                                          const float *__restrict__ bias, int C, int P, int ntile,
                                                          float *__restrict__ a_out, float *__restrict__ asum_part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *xs = sm;                          // [C][VS_PT]
    float *part = xs + (size_t)C * VS_PT;    // [16][VS_PT] partial sums of squares
    float *lg = part + 16 * VS_PT;           // [VS_PT][VK]
    float *invn = lg + VS_PT * VK;           // [VS_PT]
    const int b = blockIdx.y, tile = blockIdx.x, p0 = tile * VS_PT, tid = threadIdx.x;
    const float *x = feat + (size_t)b * C * P;
    for (int e = tid; e < C * VS_PT; e += 256) {
        const int c = e >> 4, pp = e & 15;
        xs[e] = (p0 + pp < P) ? x[(size_t)c * P + p0 + pp] : 0.0f;
    }
    __syncthreads();
    {
        const int pp = tid & 15, cp = tid >> 4;
        float s = 0.0f;
        for (int c = cp; c < C; c += 16) { float v = xs[c * VS_PT + pp]; s += v * v; }
        part[cp * VS_PT + pp] = s;
    }
    const int k = tid & 63, pg = tid >> 6;   // wave pg owns pixels 4pg..4pg+3: xs reads are wave broadcasts
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
        const float w = Wt[(size_t)c * VK + k];
        const float4 xv = *(const float4 *)(xs + c * VS_PT + pg * 4);
        a0 += w * xv.x; a1 += w * xv.y; a2 += w * xv.z; a3 += w * xv.w;
    }
    lg[(pg * 4 + 0) * VK + k] = a0; lg[(pg * 4 + 1) * VK + k] = a1;
    lg[(pg * 4 + 2) * VK + k] = a2; lg[(pg * 4 + 3) * VK + k] = a3;
    __syncthreads();
    if (tid < VS_PT) {
        float ss = 0.0f;
        for (int cp = 0; cp < 16; ++cp) ss += part[cp * VS_PT + tid];
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);            // F.normalize(dim=1), netvlad.py:105-106
        float mx = -INFINITY;
        for (int kk = 0; kk < VK; ++kk) {
            float v = lg[tid * VK + kk] * inv + (bias ? bias[kk] : 0.0f);
            lg[tid * VK + kk] = v;
            mx = fmaxf(mx, v);
        }
        float se = 0.0f;
        for (int kk = 0; kk < VK; ++kk) { float v = expf(lg[tid * VK + kk] - mx); lg[tid * VK + kk] = v; se += v; }
        const float rs = 1.0f / se;
        for (int kk = 0; kk < VK; ++kk) lg[tid * VK + kk] *= rs;      // softmax, netvlad.py:109-110
        invn[tid] = inv;
    }
    __syncthreads();
    if (tid < VK) {
        float s = 0.0f;
        for (int pp = 0; pp < VS_PT; ++pp)
            if (p0 + pp < P) s += lg[pp * VK + tid];
        asum_part[((size_t)b * ntile + tile) * VK + tid] = s;
    }
    for (int e = tid; e < VS_PT * VK; e += 256) {
        const int pp = e >> 6;
        if (p0 + pp < P) a_out[((size_t)b * P + p0 + pp) * VK + (e & 63)] = lg[e] * invn[pp];   // a' = a / ||x_p||
    }
}

// grid (nslab, B), 512 threads: thread = (channel in slab, group of 4 clusters), as in sweep 2 of vlad_fast_kernel
__global__ __launch_bounds__(512) void vlad_slab_kernel(const float *__restrict__ feat, const float *__restrict__ a_in,
                                                        const float *__restrict__ asum_part, int ntile,
                                                        const float *__restrict__ cent, int C, int P, int nslab,
                                                        float *__restrict__ out, int64_t ldo, float *__restrict__ ss_part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *a_lds = sm;                              // [P][VK]
    float *xs = a_lds + (size_t)VL_PMAX * VK;       // [VL_CC][VL_PPAD]
    float *asum = xs + VL_CC * VL_PPAD;             // [VK]
    const int sl = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *x = feat + ((size_t)b * C + (size_t)sl * VL_CC) * P;
    for (int e = tid; e < P * VK; e += 512) a_lds[e] = a_in[(size_t)b * P * VK + e];
    const int nch = (C - sl * VL_CC) < VL_CC ? (C - sl * VL_CC) : VL_CC;
    for (int e = tid; e < VL_CC * P; e += 512) {
        const int cc = e / P, pp = e - cc * P;
        xs[cc * VL_PPAD + pp] = cc < nch ? x[e] : 0.0f;
    }
    if (tid < VK) {
        float s = 0.0f;
        for (int t = 0; t < ntile; ++t) s += asum_part[((size_t)b * ntile + t) * VK + tid];
        asum[tid] = s;
    }
    __syncthreads();
    const int cl = tid & 31, k0 = (tid >> 5) * 4;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float *xr = xs + cl * VL_PPAD;
#pragma unroll 4
    for (int pp = 0; pp < P; ++pp) {
        const float xv = xr[pp];
        const float4 a4 = *(const float4 *)(a_lds + pp * VK + k0);
        a0 += a4.x * xv; a1 += a4.y * xv; a2 += a4.z * xv; a3 += a4.w * xv;
    }
    const int c = sl * VL_CC + cl;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c < C) {
        // V[k,c] = sum_p a[k,p] (x[c,p]/||x_p|| - cent[k,c])   (netvlad.py:115-124)
        v[0] = a0 - asum[k0 + 0] * cent[(size_t)(k0 + 0) * C + c];
        v[1] = a1 - asum[k0 + 1] * cent[(size_t)(k0 + 1) * C + c];
        v[2] = a2 - asum[k0 + 2] * cent[(size_t)(k0 + 2) * C + c];
        v[3] = a3 - asum[k0 + 3] * cent[(size_t)(k0 + 3) * C + c];
        float *o = out + (size_t)b * ldo;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[(size_t)(k0 + j) * C + c] = v[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = v[j] * v[j];
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (cl == 0) ss_part[((size_t)b * VK + k0 + j) * nslab + sl] = s;
    }
}

// grid (VK, B), 256 threads: intra-normalisation of cluster k (netvlad.py:126) and the global L2 (:127-128)
__global__ __launch_bounds__(256) void vlad_norm_kernel(float *__restrict__ out, int64_t ldo,
                                                        const float *__restrict__ ss_part, int nslab, int C) {
    __shared__ float nn2[VK];
    __shared__ float scs[VK];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (tid < VK) {
        float s = 0.0f;
        for (int sl = 0; sl < nslab; ++sl) s += ss_part[((size_t)b * VK + tid) * nslab + sl];
        const float nk = sqrtf(s);
        const float sc = 1.0f / fmaxf(nk, 1e-12f);
        const float nn = nk * sc;
        scs[tid] = sc;
        nn2[tid] = nn * nn;
    }
    __syncthreads();
    float gsum = 0.0f;
    for (int kk = 0; kk < VK; ++kk) gsum += nn2[kk];
    const float f = scs[k] * (1.0f / fmaxf(sqrtf(gsum), 1e-12f));
    float *o = out + (size_t)b * ldo + (size_t)k * C;
    for (int c = tid; c < C; c += 256) o[c] *= f;
}

// scratch of the small-batch path: per (device, stream), grow-only (common.h)
static StreamScratch g_vs_scratch;

static int vlad_aggregate(const float *d_feat, const float *d_assign_w, const float *d_assign_b,
                          const float *d_centroids, int B, int C, int P, int K,
                          float *d_out, int64_t ldo, void *stream, bool nhwc) {
    PTR_DEVICE(d_feat);
    ARG_CHECK(d_feat && d_assign_w && d_centroids && d_out, "NULL argument");
    ARG_CHECK(K == VK, "K must be 64 (reference: num_clusters=64, netvlad.py:176)");
    ARG_CHECK(C >= 1 && C <= 512 && P >= 1 && B >= 0, "need 1 <= C <= 512 (reference encoder_dim = 512, netvlad.py:162)");
    ARG_CHECK(ldo >= (int64_t)K * C, "output pitch smaller than K*C");
    if (B == 0) return CSLAM_OK;
    if (nhwc) {
        ARG_CHECK(P <= VL_PMAX && B > 8, "the channels-last form is the batch kernel's (B > 8, P <= 256)");
        // NetVLAD's own shape (512 channels, 14 x 14): the two contractions on the f32 matrix pipe; other shapes: the VALU form
        if (C % VM_CS == 0 && C <= 4 * VM_CS && P <= VM_PP && P >= 32) {
            const size_t lds_m = (size_t)VM_LDS_FLOATS * 4;
            static DeviceOnce once;
            int once_dev;
            if (once.todo(&once_dev)) {
                HIP_TRY(hipFuncSetAttribute((const void *)vlad_mfma_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_m));
                once.done(once_dev);
            }
            hipLaunchKernelGGL(vlad_mfma_kernel<false>, dim3(B), dim3(512), lds_m, (hipStream_t)stream, d_feat, d_assign_w, d_assign_b,
                               d_centroids, C, P, d_out, ldo, (unsigned short *)nullptr, 0, 0.0f);
            HIP_TRY(hipGetLastError());
            return CSLAM_OK;
        }
        size_t lds = (size_t)(VL_PMAX * VK + VL_CC * VL_PPAD + VL_CC * VK + VL_PMAX + VK + VK + 16) * 4;
        HIP_TRY(hipFuncSetAttribute((const void *)vlad_fast_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(vlad_fast_kernel<true>, dim3(B), dim3(512), lds, (hipStream_t)stream, d_feat, d_assign_w,
                           d_assign_b, d_centroids, C, P, d_out, ldo);
        HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    if (B <= 8 && P <= VL_PMAX) {
        hipStream_t st = (hipStream_t)stream;
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        const int ntile = (P + VS_PT - 1) / VS_PT, nslab = (C + VL_CC - 1) / VL_CC;
        const size_t n_wt = (size_t)C * VK, n_a = (size_t)B * P * VK, n_as = (size_t)B * ntile * VK;
        const size_t n_ss = (size_t)B * VK * nslab, need = n_wt + n_a + n_as + n_ss;
        SCRATCH_GET(g_vs, float *, g_vs_scratch, dev, stream, need * 4, (size_t)4 << 20);
        float *wt = g_vs, *a = wt + n_wt, *as = a + n_a, *ss = as + n_as;
        hipLaunchKernelGGL(vlad_wt_kernel, dim3((unsigned)((C * VK + 255) / 256)), dim3(256), 0, st, d_assign_w, C, wt);
        const size_t lds1 = ((size_t)C * VS_PT + 16 * VS_PT + VS_PT * VK + VS_PT) * 4;
        HIP_TRY(hipFuncSetAttribute((const void *)vlad_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
        hipLaunchKernelGGL(vlad_assign_kernel, dim3(ntile, B), dim3(256), lds1, st, d_feat, wt, d_assign_b, C, P, ntile, a, as);
        const size_t lds2 = ((size_t)VL_PMAX * VK + VL_CC * VL_PPAD + VK) * 4;
        HIP_TRY(hipFuncSetAttribute((const void *)vlad_slab_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
        hipLaunchKernelGGL(vlad_slab_kernel, dim3(nslab, B), dim3(512), lds2, st, d_feat, a, as, ntile, d_centroids, C, P,
                           nslab, d_out, ldo, ss);
        hipLaunchKernelGGL(vlad_norm_kernel, dim3(VK, B), dim3(256), 0, st, d_out, ldo, ss, nslab, C);
        HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    if (P <= VL_PMAX) {
        size_t lds = (size_t)(VL_PMAX * VK + VL_CC * VL_PPAD + VL_CC * VK + VL_PMAX + VK + VK + 16) * 4;
        HIP_TRY(hipFuncSetAttribute((const void *)vlad_fast_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(vlad_fast_kernel<false>, dim3(B), dim3(512), lds, (hipStream_t)stream, d_feat, d_assign_w,
                           d_assign_b, d_centroids, C, P, d_out, ldo);
    } else {
        int threads = (int)round_up64(C > VPCH ? C : VPCH, 64);
        size_t lds = (size_t)(VPCH * VK + VWCH * VK + VPCH + 16 * VK + 16) * 4;
        HIP_TRY(hipFuncSetAttribute((const void *)vlad_generic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(vlad_generic_kernel, dim3(B), dim3(threads), lds, (hipStream_t)stream, d_feat, d_assign_w,
                           d_assign_b, d_centroids, C, P, d_out, ldo);
    }
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_vlad_aggregate_dev(const float *d_feat, const float *d_assign_w, const float *d_assign_b,
                                       const float *d_centroids, int B, int C, int P, int K,
                                       float *d_out, int64_t ldo, void *stream) {
    return vlad_aggregate(d_feat, d_assign_w, d_assign_b, d_centroids, B, C, P, K, d_out, ldo, stream, false);
}

CSLAM_API int cslam_vlad_aggregate_nhwc_dev(const float *d_feat, const float *d_assign_w, const float *d_assign_b,
                                            const float *d_centroids, int B, int C, int P, int K,
                                            float *d_out, int64_t ldo, void *stream) {
    return vlad_aggregate(d_feat, d_assign_w, d_assign_b, d_centroids, B, C, P, K, d_out, ldo, stream, true);
}

// The matrix form with the pair rows of the projection written by its final store (vlad_mfma_kernel<true>): one pass over the
// VLAD vector less in each direction than cslam_vlad_aggregate_nhwc_dev + the row kernel of cslam_pca_project_pairs_dev, which it
// equals bit for bit.  d_A2 [S][B][K C / S / 32][hi 32 | lo 32] fp16; d_out [B][K C] (pitch ldo) or NULL.  Only the shapes of the
// matrix form (C a multiple of 128 up to 512, 32 <= P <= 200), any B >= 1; S a power of two up to K (whole clusters per split).
CSLAM_API int cslam_vlad_aggregate_nhwc_pairs_dev(const float *d_feat, const float *d_assign_w, const float *d_assign_b,
                                                  const float *d_centroids, int B, int C, int P, int K, float x_bound, int S,
                                                  void *d_A2, float *d_out, int64_t ldo, void *stream) {
    PTR_DEVICE(d_feat);
    ARG_CHECK(d_feat && d_assign_w && d_centroids && d_A2, "NULL argument");
    ARG_CHECK(K == VK, "K must be 64 (reference: num_clusters=64, netvlad.py:176)");
    ARG_CHECK(C >= VM_CS && C % VM_CS == 0 && C <= 4 * VM_CS && P <= VM_PP && P >= 32 && B >= 0,
              "the pair-row form is the matrix kernel's: C a multiple of 128 up to 512, 32 <= P <= 200");
    ARG_CHECK(S >= 1 && S <= VK && (S & (S - 1)) == 0, "S must be a power of two up to K");
    ARG_CHECK(x_bound > 0.0f, "a bound of max |v| must be given (1 for the L2-normalised vector)");
    ARG_CHECK((uintptr_t)d_A2 % 16 == 0, "the pair rows must be 16-byte aligned");
    ARG_CHECK(!d_out || ldo >= (int64_t)K * C, "output pitch smaller than K*C");
    if (B == 0) return CSLAM_OK;
    int kshift = 0;
    while ((S << kshift) < VK) ++kshift;
    const size_t lds_m = (size_t)VM_LDS_FLOATS * 4;
    static DeviceOnce once;
    int once_dev;
    if (once.todo(&once_dev)) {
        HIP_TRY(hipFuncSetAttribute((const void *)vlad_mfma_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_m));
        once.done(once_dev);
    }
    hipLaunchKernelGGL(vlad_mfma_kernel<true>, dim3(B), dim3(512), lds_m, (hipStream_t)stream, d_feat, d_assign_w, d_assign_b,
                       d_centroids, C, P, d_out, ldo, (unsigned short *)d_A2, kshift, x_bound);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

// ------------------------------------------------------------ CosPlace head ----
__global__ __launch_bounds__(256) void gem_fc_kernel(const float *__restrict__ feat, float pw, float eps,
                                                     const float *__restrict__ W, const float *__restrict__ bias,
                                                     int C, int P, int Dout, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *invn = (float *)smem;          // [P]
    float *g = invn + P;                  // [C]
    float *o = g + C;                     // [Dout]
    float *red = o + Dout;                // [16]
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const float *x = feat + (size_t)blockIdx.x * C * P;
    // L2Norm over channels per pixel (layers.py:32-36)
    for (int p = tid; p < P; p += nt) {
        float s = 0.0f;
        for (int c = 0; c < C; ++c) { float v = x[(size_t)c * P + p]; s += v * v; }
        invn[p] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    }
    __syncthreads();
    // GeM (layers.py:8-9): avg_pool(clamp(x, min=eps)^p)^(1/p)
    const float ip = 1.0f / pw, invP = 1.0f / (float)P;
    for (int c = tid; c < C; c += nt) {
        float s = 0.0f;
        for (int p = 0; p < P; ++p) s += powf(fmaxf(x[(size_t)c * P + p] * invn[p], eps), pw);
        g[c] = powf(s * invP, ip);
    }
    __syncthreads();
    // Linear (network.py:27): one wave per output feature
    for (int d = wave; d < Dout; d += nw) {
        const float *wr = W + (size_t)d * C;
        float s = 0.0f;
        for (int c = lane; c < C; c += 64) s += wr[c] * g[c];
        s = wave_sum_f32(s);
        if (lane == 0) o[d] = s + (bias ? bias[d] : 0.0f);
    }
    __syncthreads();
    float s = 0.0f;
    for (int d = tid; d < Dout; d += nt) s += o[d] * o[d];
    float nrm = sqrtf(block_sum_f32(s, red));
    float sc = 1.0f / fmaxf(nrm, 1e-12f);
    for (int d = tid; d < Dout; d += nt) out[(size_t)blockIdx.x * Dout + d] = o[d] * sc;
}

CSLAM_API int cslam_gem_fc_head_dev(const float *d_feat, float p, float eps, const float *d_W,
                                    const float *d_b, int B, int C, int P, int Dout,
                                    float *d_out, void *stream) {
    PTR_DEVICE(d_feat);
    ARG_CHECK(d_feat && d_W && d_out, "NULL argument");
    ARG_CHECK(B >= 0 && C >= 1 && P >= 1 && Dout >= 1, "bad sizes");
    size_t lds = (size_t)(P + C + Dout + 16) * 4;
    ARG_CHECK(lds <= 150 * 1024, "C + P + Dout too large for one workgroup's LDS");
    if (B == 0) return CSLAM_OK;
    HIP_TRY(hipFuncSetAttribute((const void *)gem_fc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(gem_fc_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, d_feat, p, eps, d_W, d_b, C,
                       P, Dout, d_out);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

// The same head on a channels_last map, feat [B][P][C] (what the trunks of vpr/winograd.py write): the pixel norms are wave
// reductions over contiguous channel runs, the GeM sums read a pixel's channels coalesced; one workgroup per frame as above.
// C a multiple of 4 (16-byte runs).
__global__ __launch_bounds__(256) void gem_fc_nhwc_kernel(const float *__restrict__ feat, float pw, float eps,
                                                          const float *__restrict__ W, const float *__restrict__ bias,
                                                          int C, int P, int Dout, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *invn = (float *)smem;          // [P]
    float *g = invn + P;                  // [C]
    float *o = g + C;                     // [Dout]
    float *red = o + Dout;                // [16]
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const float *x = feat + (size_t)blockIdx.x * C * P;
    const int C4 = C >> 2;
    for (int p0 = wave * 4; p0 < P; p0 += nw * 4) {                    // L2Norm over channels per pixel (layers.py:32-36): four pixels a step
        float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = lane; c < C4; c += 64) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (p0 + j < P) {
                    const float4 v = ((const float4 *)(x + (size_t)(p0 + j) * C))[c];
                    s4[j] += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = wave_sum_f32(s4[j]);
            if (lane == 0 && p0 + j < P) invn[p0 + j] = 1.0f / fmaxf(sqrtf(t), 1e-12f);
        }
    }
    __syncthreads();
    const float ip = 1.0f / pw, invP = 1.0f / (float)P;                // GeM (layers.py:8-9): avg_pool(clamp(x, min=eps)^p)^(1/p)
    const bool cube = pw == 3.0f;                                      // the reference's trained p starts at 3: x^3 without powf
    // (a workgroup is one frame and the launch is about one round of workgroups: what counts is the LENGTH of the dependent chains --
    // eight loads in flight per thread here, four output features per wave and step below, instead of one load per round trip)
    for (int c = tid; c < C; c += nt) {
        float s = 0.0f;
        for (int p0 = 0; p0 < P; p0 += 8) {
            float xv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = p0 + j < P ? x[(size_t)(p0 + j) * C + c] : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (p0 + j < P) {
                    const float v = fmaxf(xv[j] * invn[p0 + j], eps);
                    s += cube ? v * v * v : powf(v, pw);
                }
            }
        }
        g[c] = powf(s * invP, ip);
    }
    __syncthreads();
    for (int d0 = wave * 4; d0 < Dout; d0 += nw * 4) {                 // Linear (network.py:27): four output features per wave and step
        float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = lane; c < C4; c += 64) {
            const float4 gv = *(const float4 *)(g + 4 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (d0 + j < Dout) {
                    const float4 w = ((const float4 *)(W + (size_t)(d0 + j) * C))[c];
                    s4[j] += w.x * gv.x + w.y * gv.y + w.z * gv.z + w.w * gv.w;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = wave_sum_f32(s4[j]);
            if (lane == 0 && d0 + j < Dout) o[d0 + j] = t + (bias ? bias[d0 + j] : 0.0f);
        }
    }
    __syncthreads();
    float s = 0.0f;
    for (int d = tid; d < Dout; d += nt) s += o[d] * o[d];
    float nrm = sqrtf(block_sum_f32(s, red));
    float sc = 1.0f / fmaxf(nrm, 1e-12f);
    for (int d = tid; d < Dout; d += nt) out[(size_t)blockIdx.x * Dout + d] = o[d] * sc;
}

CSLAM_API int cslam_gem_fc_head_nhwc_dev(const float *d_feat, float p, float eps, const float *d_W,
                                         const float *d_b, int B, int C, int P, int Dout,
                                         float *d_out, void *stream) {
    PTR_DEVICE(d_feat);
    ARG_CHECK(d_feat && d_W && d_out, "NULL argument");
    ARG_CHECK(B >= 0 && C >= 4 && (C % 4) == 0 && P >= 1 && Dout >= 1, "bad sizes (C must be a multiple of 4)");
    size_t lds = (size_t)(P + C + Dout + 16) * 4;
    ARG_CHECK(lds <= 150 * 1024, "C + P + Dout too large for one workgroup's LDS");
    if (B == 0) return CSLAM_OK;
    HIP_TRY(hipFuncSetAttribute((const void *)gem_fc_nhwc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(gem_fc_nhwc_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, d_feat, p, eps, d_W, d_b, C,
                       P, Dout, d_out);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

// ------------------------------------------------------------ image transform ----
// Pillow's antialiased resampling (Resample.c, 8 bits per channel), restated:
//   coefficients: precompute_coeffs() in double, bicubic a = -0.5, support = 2 * max(scale, 1),
//                 normalised per output pixel, then fixed point with 22 fractional bits
//                 (normalize_coeffs_8bpc); horizontal pass first, result clipped to uint8,
//                 then the vertical pass on that uint8 image; both round with + 2^21.
// (Pillow is a third-party dependency of the reference via torchvision.transforms; pinned by
//  tests/golden/heads_g.npz produced with Pillow in the build container.)
#define PREC_BITS 22

static double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

static int precompute_coeffs(int in_size, double in0, double in1, int out_size, std::vector<int> &bounds,
                             std::vector<int> &kk) {
    double scale = (in1 - in0) / out_size, filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> k((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        double center = in0 + (xx + 0.5) * scale, ww = 0.0, ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        int x;
        for (x = 0; x < xmax; ++x) {
            double w = bicubic_filter((x + xmin - center + 0.5) * ss);
            k[x] = w; ww += w;
        }
        for (x = 0; x < xmax; ++x) if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; ++x) k[x] = 0.0;
        for (x = 0; x < ksize; ++x)
            kk[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PREC_BITS))
                                                  : (int)(0.5 + k[x] * (1 << PREC_BITS));
        bounds[xx * 2] = xmin; bounds[xx * 2 + 1] = xmax;
    }
    return ksize;
}

__device__ __forceinline__ int clip8(int v) {
    v >>= PREC_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Rows rlo .. rlo + nrows - 1 of frame b's crop window into LDS (`in_row_bytes` per row), zero-filled where the window
// hangs over a frame smaller than the crop (torchvision pads, then crops).
__device__ __forceinline__ void pp_load_rows(const uint8_t *__restrict__ img, uint8_t *s_in, int b, int H, int W, int crop, int top,
                                             int left, int ptop, int pleft, int rlo, int nrows, int in_row_bytes) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const bool padded = (ptop | pleft) != 0 || H < crop || W < crop;
    const size_t row0 = padded ? 0 : ((size_t)b * H + top + rlo) * W * 3 + (size_t)left * 3;
    const int row_bytes = crop * 3;
    const bool aligned = !padded && ((((size_t)img + row0) & 3) == 0) && (((size_t)W * 3) % 4 == 0) && (row_bytes % 4 == 0);
    // all loops below: one wave per row (or per (channel, output row) pair), lanes along the row --
    // no runtime integer divisions on the per-element path
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    if (aligned) {
        // dword e = i*nt + tid of the tile lives at (row e / ndw, dword e % ndw): walk it incrementally,
        // 8 independent global loads in flight per thread before the LDS stores
        const int ndw = row_bytes >> 2, total = nrows * ndw;
        const int dq = nt / ndw, dr = nt - dq * ndw;
        int r = tid / ndw, c = tid - r * ndw;
        for (int base = 0; base < total; base += nt * 8) {
            uint32_t v[8]; int rr[8], cc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                rr[j] = r; cc[j] = c;
                v[j] = (base + j * nt + tid < total) ? *(const uint32_t *)(img + row0 + (size_t)r * W * 3 + (size_t)c * 4) : 0u;
                r += dq; c += dr;
                if (c >= ndw) { c -= ndw; ++r; }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (base + j * nt + tid < total) ((uint32_t *)(s_in + (size_t)rr[j] * in_row_bytes))[cc[j]] = v[j];
        }
    } else if (!padded) {
        for (int r = wave; r < nrows; r += nw)
            for (int c = lane; c < row_bytes; c += 64)
                s_in[(size_t)r * in_row_bytes + c] = img[row0 + (size_t)r * W * 3 + c];
    } else {
        // CenterCrop of a frame smaller than the crop: zero fill outside the frame (torchvision pads, then crops)
        const uint8_t *frame = img + (size_t)b * H * W * 3;
        for (int r = wave; r < nrows; r += nw) {
            const int sr = top + rlo + r - ptop;
            for (int c = lane; c < row_bytes; c += 64) {
                const int sc = left * 3 + c - pleft * 3;
                const bool in = sr >= 0 && sr < H && sc >= 0 && sc < W * 3;
                s_in[(size_t)r * in_row_bytes + c] = in ? frame[(size_t)sr * W * 3 + sc] : (uint8_t)0;
            }
        }
    }
}

// Fused crop + horizontal pass + vertical pass + ToTensor + Normalize.  One workgroup = one image x
// PP_TY output rows: the input rows those outputs need (about 1.7*PP_TY + 8 at 376 -> 224) are
// read from HBM once with 4-byte loads into LDS, resized horizontally to uint8 in LDS (Pillow
// rounds and clips to 8 bits between the passes), then vertically, and stored as float32 CHW with
// consecutive lanes on consecutive x.  HBM traffic per frame ~ crop*crop*3 (x1.3 row overlap between
// tiles, absorbed by L2) + 3*out*out*4 bytes; the old two-kernel version moved the uint8
// intermediate through memory and read single bytes.
// `ty` (PP_TY_MAX = 16 at the reference's 376 -> 224; smaller when a larger crop would not fit the 160 KiB of LDS) is a
// launch parameter.  A frame smaller than the crop is zero-padded like torchvision's CenterCrop (`ptop`, `pleft` rows /
// pixels of padding before the frame; `top`, `left` then address the padded frame).
#define PP_TY_MAX 16
__global__ __launch_bounds__(256) void preprocess_fused_kernel(
    const uint8_t *__restrict__ img, int H, int W, int crop, int top, int left, int ptop, int pleft, int ty,
    int out_hw, int ksize, int max_rows, const int *__restrict__ bounds, const int *__restrict__ kk,
    float m0, float m1, float m2, float s0, float s1, float s2, float *__restrict__ out, int nhwc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int in_row_bytes = (crop * 3 + 3) & ~3;        // padded to dwords
    const int tmp_row_bytes = out_hw * 3;
    int *s_bounds = (int *)smem;                                     // [out_hw][2]
    int *s_kk = s_bounds + out_hw * 2;                               // [out_hw][ksize]
    uint8_t *s_in = (uint8_t *)(s_kk + out_hw * ksize);              // [max_rows][in_row_bytes]
    uint8_t *s_tmp = s_in + (size_t)max_rows * in_row_bytes;         // [max_rows][tmp_row_bytes]
    const int tid = threadIdx.x, nt = blockDim.x;
    const int b = blockIdx.y, y0 = blockIdx.x * ty;
    const int ny = out_hw - y0 < ty ? out_hw - y0 : ty;
    for (int e = tid; e < out_hw * 2; e += nt) s_bounds[e] = bounds[e];
    for (int e = tid; e < out_hw * ksize; e += nt) s_kk[e] = kk[e];
    const int rlo = bounds[y0 * 2];
    const int ylast = y0 + ny - 1;
    const int rhi = bounds[ylast * 2] + bounds[ylast * 2 + 1];
    const int nrows = rhi - rlo;
    // ---- load the input rows (crop window) into LDS
    pp_load_rows(img, s_in, b, H, W, crop, top, left, ptop, pleft, rlo, nrows, in_row_bytes);
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    __syncthreads();
    // ---- horizontal pass (uint8 result, rounded + clipped like ImagingResampleHorizontal_8bpc);
    //      a lane owns one output x and produces its three channels with one read of the taps
    for (int r = wave; r < nrows; r += nw) {
        const uint8_t *rowp = s_in + (size_t)r * in_row_bytes;
        uint8_t *dst = s_tmp + (size_t)r * tmp_row_bytes;
        for (int xo = lane; xo < out_hw; xo += 64) {
            const int xmin = s_bounds[xo * 2], xn = s_bounds[xo * 2 + 1];
            const int *k = s_kk + xo * ksize;
            const uint8_t *src = rowp + xmin * 3;
            int a0 = 1 << (PREC_BITS - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < xn; ++x) {
                const int kx = k[x];
                a0 += (int)src[x * 3] * kx; a1 += (int)src[x * 3 + 1] * kx; a2 += (int)src[x * 3 + 2] * kx;
            }
            dst[xo * 3] = (uint8_t)clip8(a0); dst[xo * 3 + 1] = (uint8_t)clip8(a1); dst[xo * 3 + 2] = (uint8_t)clip8(a2);
        }
    }
    __syncthreads();
    // ---- vertical pass + ToTensor + Normalize: one wave per output row, lanes along x, the three
    //      channel planes written as three coalesced rows
    for (int yo = wave; yo < ny; yo += nw) {
        const int y = y0 + yo;
        const int ymin = s_bounds[y * 2], yn = s_bounds[y * 2 + 1];
        const int *k = s_kk + y * ksize;
        const uint8_t *base = s_tmp + (size_t)(ymin - rlo) * tmp_row_bytes;
        // planar [B,3,h,w]: three coalesced rows; nhwc [B,h,w,3]: the same three pointers one float apart, pixel pitch 3
        float *o0 = nhwc ? out + ((size_t)b * out_hw + y) * out_hw * 3 : out + (((size_t)b * 3 + 0) * out_hw + y) * out_hw;
        const size_t plane = nhwc ? 1 : (size_t)out_hw * out_hw;
        const int xs = nhwc ? 3 : 1;
        float *o1 = o0 + plane, *o2 = o1 + plane;
        for (int xo = lane; xo < out_hw; xo += 64) {
            const uint8_t *src = base + xo * 3;
            int a0 = 1 << (PREC_BITS - 1), a1 = a0, a2 = a0;
            for (int j = 0; j < yn; ++j) {
                const int kj = k[j];
                const uint8_t *q = src + (size_t)j * tmp_row_bytes;
                a0 += (int)q[0] * kj; a1 += (int)q[1] * kj; a2 += (int)q[2] * kj;
            }
            o0[xo * xs] = ((float)clip8(a0) / 255.0f - m0) / s0;        // ToTensor, Normalize
            o1[xo * xs] = ((float)clip8(a1) / 255.0f - m1) / s1;
            o2[xo * xs] = ((float)clip8(a2) / 255.0f - m2) / s2;
        }
    }
}

// The same transform with far fewer LDS instructions (the form above spends one per byte and per tap: 72 a pixel, and is
// bound by them at 1.1 us a frame), for the tap counts that occur in practice (KS = 5 .. 13: scale factors up to 3):
//   horizontal  a lane owns output columns xo, xo + 64, ..: their KS taps sit in registers; per input row the 3 KS bytes
//               under the taps arrive as (3 KS + 3) / 4 + 1 aligned dwords, shifted into place with v_alignbyte
//   vertical    a lane owns FOUR consecutive bytes (a dword column) of the interleaved uint8 rows; the row's taps are
//               wave-uniform (scalar loads); one dword read per tap feeds four accumulators
//   store       the uint8 results of a row go through LDS once more so that the three float planes are written with
//               consecutive lanes on consecutive x.
// Integer arithmetic as above (sums of the same products: the order is immaterial), so the result is the same bit for bit.
// Taps past a window's end are zero in `kk` (precompute_coeffs pads them): what the extra reads hit does not matter, they stay
// inside the workgroup's LDS.
template <int KS>
__global__ __launch_bounds__(512) void preprocess_tile_kernel(
    const uint8_t *__restrict__ img, int H, int W, int crop, int top, int left, int ptop, int pleft, int ty,
    int out_hw, int max_rows, const int *__restrict__ bounds, const int *__restrict__ kk,
    float m0, float m1, float m2, float s0, float s1, float s2, float *__restrict__ out, int nhwc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int in_row_bytes = (crop * 3 + 3) & ~3;
    const int tmp_pitch = (out_hw * 3 + 3) & ~3;
    uint8_t *s_in = (uint8_t *)smem;                                 // [max_rows][in_row_bytes]
    uint8_t *s_tmp = s_in + (size_t)max_rows * in_row_bytes;         // [max_rows][tmp_pitch]   horizontal pass, uint8
    uint8_t *s_out = s_tmp + (size_t)max_rows * tmp_pitch;           // [ty][tmp_pitch]         vertical pass, uint8
    float *s_lut = (float *)(s_out + (size_t)ty * tmp_pitch);        // [3][256]                ToTensor + Normalize of every uint8 value
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
    const int b = blockIdx.y, y0 = blockIdx.x * ty;
    const int ny = out_hw - y0 < ty ? out_hw - y0 : ty;
    const int rlo = bounds[y0 * 2];
    const int ylast = y0 + ny - 1;
    const int nrows = bounds[ylast * 2] + bounds[ylast * 2 + 1] - rlo;
    pp_load_rows(img, s_in, b, H, W, crop, top, left, ptop, pleft, rlo, nrows, in_row_bytes);
    // the two IEEE divisions of ToTensor + Normalize, once per (channel, uint8 value) instead of once per output element
    for (int e = tid; e < 768; e += blockDim.x) {
        const int c = e >> 8;
        s_lut[e] = ((float)(e & 255) / 255.0f - (c == 0 ? m0 : c == 1 ? m1 : m2)) / (c == 0 ? s0 : c == 1 ? s1 : s2);
    }
    __syncthreads();
    // ---- horizontal pass (uint8 result, rounded + clipped like ImagingResampleHorizontal_8bpc)
    constexpr int NE = (3 * KS + 3) / 4;                             // dwords holding the 3 KS bytes once aligned
    const int in_pitch4 = in_row_bytes >> 2;
    for (int xo = lane; xo < out_hw; xo += 64) {
        int k[KS];
#pragma unroll
        for (int j = 0; j < KS; ++j) k[j] = kk[xo * KS + j];
        const int boff = bounds[xo * 2] * 3, sh = boff & 3;
        const uint32_t *src = (const uint32_t *)(s_in + (boff & ~3)) + wave * in_pitch4;
        uint8_t *dst = s_tmp + (size_t)wave * tmp_pitch + xo * 3;
        for (int r = wave; r < nrows; r += nw, src += nw * in_pitch4, dst += nw * tmp_pitch) {
            uint32_t d[NE + 1], e[NE];
#pragma unroll
            for (int i = 0; i <= NE; ++i) d[i] = src[i];
#pragma unroll
            for (int i = 0; i < NE; ++i) e[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
            int a[3] = {1 << (PREC_BITS - 1), 1 << (PREC_BITS - 1), 1 << (PREC_BITS - 1)};
#pragma unroll
            for (int x = 0; x < KS; ++x)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int idx = 3 * x + c;
                    a[c] += __mul24((int)((e[idx >> 2] >> (8 * (idx & 3))) & 0xffu), k[x]);    // |k| < 2^23 (checked on the host)
                }
            dst[0] = (uint8_t)clip8(a[0]); dst[1] = (uint8_t)clip8(a[1]); dst[2] = (uint8_t)clip8(a[2]);
        }
    }
    __syncthreads();
    // ---- vertical pass + ToTensor + Normalize: one wave per output row
    const int pitch4 = tmp_pitch >> 2;
    for (int yo = wave; yo < ny; yo += nw) {
        const int y = y0 + yo;
        const int r0 = bounds[y * 2] - rlo;
        int kj[KS], rj[KS];
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            kj[j] = kk[y * KS + j];
            rj[j] = (r0 + j < nrows ? r0 + j : nrows - 1) * pitch4;   // zero taps past the window: any row will do
        }
        uint32_t *orow = (uint32_t *)(s_out + (size_t)yo * tmp_pitch);
        for (int dc = lane; dc < pitch4; dc += 64) {
            int a[4] = {1 << (PREC_BITS - 1), 1 << (PREC_BITS - 1), 1 << (PREC_BITS - 1), 1 << (PREC_BITS - 1)};
#pragma unroll
            for (int j = 0; j < KS; ++j) {
                const uint32_t v = ((const uint32_t *)s_tmp)[rj[j] + dc];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] += __mul24((int)((v >> (8 * q)) & 0xffu), kj[j]);
            }
            // (the four clipped values are made opaque before packing: left to itself the compiler turns the low pair into
            //  gfx950's v_ashr_pk_u8_i32 and ORs the other two onto a register whose upper half that instruction does not clear --
            //  measured: bytes 2 and 3 of every dword wrong)
            int c4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { c4[q] = clip8(a[q]); asm volatile("" : "+v"(c4[q])); }
            orow[dc] = (uint32_t)c4[0] | ((uint32_t)c4[1] << 8) | ((uint32_t)c4[2] << 16) | ((uint32_t)c4[3] << 24);
        }
        // the row was written by this wave and is read by this wave: LDS operations of a wave complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint8_t *q = s_out + (size_t)yo * tmp_pitch;
        if (nhwc) {                                                   // [B,h,w,3]: the row is 3 w consecutive floats, byte j -> float j
            float *o = out + ((size_t)b * out_hw + y) * out_hw * 3;
            for (int j = lane; j < out_hw * 3; j += 64) o[j] = s_lut[(j % 3) * 256 + q[j]];
            continue;
        }
        float *o0 = out + (((size_t)b * 3 + 0) * out_hw + y) * out_hw;
        float *o1 = o0 + (size_t)out_hw * out_hw, *o2 = o1 + (size_t)out_hw * out_hw;
        for (int xo = lane; xo < out_hw; xo += 64) {
            o0[xo] = s_lut[q[xo * 3]];                                // ToTensor, Normalize
            o1[xo] = s_lut[256 + q[xo * 3 + 1]];
            o2[xo] = s_lut[512 + q[xo * 3 + 2]];
        }
    }
}

struct PreprocCache {
    int device, crop, out_hw, ksize, max_rows, ty;
    int max_rows2, ty2;                 // preprocess_tile_kernel's tile (its LDS holds no tables, but the output rows); ty2 = 0: not usable
    int *d_bounds, *d_kk;
};
static std::mutex g_pp_mutex;          // extractors on several threads share the tables
// Coefficient tables per (device, crop, output size).  Entries are never freed or moved once built: the online
// path captures this launch in a hipGraph, and a table pointer baked into a graph must stay valid when another
// extractor with a different crop is used in between.
static std::vector<PreprocCache *> g_pp_all;

static int preprocess_launch(const uint8_t *d_img, int B, int H, int W, int crop, int out_hw,
                             const float mean[3], const float std_[3], float *d_out, int nhwc, void *stream) {
    PTR_DEVICE(d_img);
    ARG_CHECK(d_img && d_out && mean && std_, "NULL argument");
    ARG_CHECK(B >= 0 && crop >= 1 && out_hw >= 1, "bad sizes");
    ARG_CHECK(H >= 1 && W >= 1, "empty frame");
    if (B == 0) return CSLAM_OK;
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const size_t in_row_bytes = ((size_t)crop * 3 + 3) & ~(size_t)3;
    PreprocCache *pp = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_pp_mutex);
        for (PreprocCache *c : g_pp_all)
            if (c->device == dev && c->crop == crop && c->out_hw == out_hw) pp = c;
        if (!pp) {
            std::vector<int> bounds, kk;
            int ksize = precompute_coeffs(crop, 0.0, (double)crop, out_hw, bounds, kk);
            // largest row tile whose input rows + uint8 intermediate fit the 160 KiB of LDS
            int ty = PP_TY_MAX, max_rows = 0;
            for (;; ty >>= 1) {
                max_rows = 0;
                for (int y0 = 0; y0 < out_hw; y0 += ty) {
                    int yl = y0 + ty - 1 < out_hw - 1 ? y0 + ty - 1 : out_hw - 1;
                    int span = bounds[yl * 2] + bounds[yl * 2 + 1] - bounds[y0 * 2];
                    if (span > max_rows) max_rows = span;
                }
                size_t need = (size_t)out_hw * 2 * 4 + (size_t)out_hw * ksize * 4 +
                              (size_t)max_rows * (in_row_bytes + (size_t)out_hw * 3);
                if (need <= 160 * 1024 || ty == 1) break;
            }
            // preprocess_tile_kernel: the largest row tile that leaves room for two workgroups per CU (80 KiB), else for one
            const size_t tmp_pitch = ((size_t)out_hw * 3 + 3) & ~(size_t)3;
            int ty2 = PP_TY_MAX, max_rows2 = 0;
            for (int pass = 0; pass < 2; ++pass) {
                const size_t limit = pass == 0 ? 80 * 1024 : 160 * 1024;
                bool ok = false;
                for (ty2 = PP_TY_MAX; ty2 >= (pass == 0 ? 4 : 1); ty2 >>= 1) {
                    max_rows2 = 0;
                    for (int y0 = 0; y0 < out_hw; y0 += ty2) {
                        int yl = y0 + ty2 - 1 < out_hw - 1 ? y0 + ty2 - 1 : out_hw - 1;
                        int span = bounds[yl * 2] + bounds[yl * 2 + 1] - bounds[y0 * 2];
                        if (span > max_rows2) max_rows2 = span;
                    }
                    if ((size_t)max_rows2 * (in_row_bytes + tmp_pitch) + (size_t)ty2 * tmp_pitch + 3072 <= limit) { ok = true; break; }
                }
                if (ok) break;
                if (pass == 1) ty2 = 0;                                  // does not fit: the table form decides
            }
            for (int v : kk)
                if (v >= (1 << 23) || v <= -(1 << 23)) ty2 = 0;          // its 24-bit multiplies need |tap| < 2^23 (a tap is <= ~1.1 x 2^22)
            pp = new PreprocCache{dev, crop, out_hw, ksize, max_rows, ty, max_rows2, ty2, nullptr, nullptr};
            HIP_TRY(hipMalloc((void **)&pp->d_bounds, bounds.size() * 4));
            HIP_TRY(hipMalloc((void **)&pp->d_kk, kk.size() * 4));
            HIP_TRY(hipMemcpy(pp->d_bounds, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(pp->d_kk, kk.data(), kk.size() * 4, hipMemcpyHostToDevice));
            g_pp_all.push_back(pp);
        }
    }
    const PreprocCache &g_pp = *pp;
    // torchvision CenterCrop: a frame smaller than the crop is zero-padded first ((crop - H) / 2 rows on top, the
    // odd row at the bottom), then top = round((H' - crop) / 2), left = round((W' - crop) / 2) on the padded frame
    const int ptop = H < crop ? (crop - H) / 2 : 0, pleft = W < crop ? (crop - W) / 2 : 0;
    const int Hp = H < crop ? crop : H, Wp = W < crop ? crop : W;
    const int top = (int)lrint((Hp - crop) / 2.0), left = (int)lrint((Wp - crop) / 2.0);
    if (g_pp.ty2 > 0 && g_pp.ksize >= 5 && g_pp.ksize <= 13 && (g_pp.ksize & 1)) {
        const size_t tmp_pitch = ((size_t)out_hw * 3 + 3) & ~(size_t)3;
        const size_t lds2 = (size_t)g_pp.max_rows2 * (in_row_bytes + tmp_pitch) + (size_t)g_pp.ty2 * tmp_pitch + 3072;   // + the [3][256] table
        const dim3 grid((out_hw + g_pp.ty2 - 1) / g_pp.ty2, B);
#define PP_TILE(KS_)                                                                                                          \
    case KS_:                                                                                                                 \
        HIP_TRY(hipFuncSetAttribute((const void *)preprocess_tile_kernel<KS_>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                    (int)lds2));                                                                              \
        hipLaunchKernelGGL(preprocess_tile_kernel<KS_>, grid, dim3(512), lds2, st, d_img, H, W, crop, top, left, ptop, pleft, \
                           g_pp.ty2, out_hw, g_pp.max_rows2, g_pp.d_bounds, g_pp.d_kk, mean[0], mean[1], mean[2], std_[0],    \
                           std_[1], std_[2], d_out, nhwc);                                                                    \
        break;
        switch (g_pp.ksize) {
            PP_TILE(5) PP_TILE(7) PP_TILE(9) PP_TILE(11) PP_TILE(13)
        }
#undef PP_TILE
        HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    const size_t lds = (size_t)out_hw * 2 * 4 + (size_t)out_hw * g_pp.ksize * 4 +
                       (size_t)g_pp.max_rows * (in_row_bytes + (size_t)out_hw * 3);
    ARG_CHECK(lds <= 160 * 1024, "crop too large for the fused transform: one output row's input rows exceed the LDS");
    HIP_TRY(hipFuncSetAttribute((const void *)preprocess_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    hipLaunchKernelGGL(preprocess_fused_kernel, dim3((out_hw + g_pp.ty - 1) / g_pp.ty, B), dim3(256), lds, st, d_img, H,
                       W, crop, top, left, ptop, pleft, g_pp.ty, out_hw, g_pp.ksize, g_pp.max_rows, g_pp.d_bounds,
                       g_pp.d_kk, mean[0], mean[1], mean[2], std_[0], std_[1], std_[2], d_out, nhwc);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}
CSLAM_API int cslam_preprocess_dev(const uint8_t *d_img, int B, int H, int W, int crop, int out_hw,
                                   const float mean[3], const float std_[3], float *d_out, void *stream) {
    return preprocess_launch(d_img, B, H, W, crop, out_hw, mean, std_, d_out, 0, stream);
}
/* the same transform with the output as [B, out_hw, out_hw, 3] (what the trunks' first convolution reads: channels_last storage) */
CSLAM_API int cslam_preprocess_nhwc_dev(const uint8_t *d_img, int B, int H, int W, int crop, int out_hw,
                                        const float mean[3], const float std_[3], float *d_out, void *stream) {
    return preprocess_launch(d_img, B, H, W, crop, out_hw, mean, std_, d_out, 1, stream);
}
