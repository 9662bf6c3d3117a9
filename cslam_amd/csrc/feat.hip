// feat.hip -- what a visual keyframe carries, from the image (gfx950): corners, steered BRIEF-32 descriptors, 3D points.
//
// Replaces RGBDHandler::compute_local_descriptors of src/front_end/rgbd_handler.cpp:266-312 (grey conversion, depth mask,
// rtabmap's Feature2D::generateKeypoints / generateDescriptors / generateKeypoints3D) for a ragged batch of images.  rtabmap
// and OpenCV are third party and were not available to compare against, and OpenCV's learned ORB / BRIEF sampling tables
// are not ours to restate: parity with rtabmap's features is unpinned.  The algorithm is the one stated in
// include/cslam_hip.h and feat.h; tests/feat_reference.py restates it in integer numpy, and the two agree bit for bit.
//
//   feat_gray_kernel     : a thread per pixel; 1 channel is copied, 3 (BGR) are weighted in integers.
//   feat_response_kernel : a 16 x 16 tile of output pixels per workgroup.  The grey tile plus a 2-pixel halo in LDS, from it
//                          Ix, Iy (int16) of the tile plus a 1-pixel halo, where a halo position outside the image holds the
//                          derivative of its REFLECTED position (reflecting the grey image instead would flip the sign of
//                          one derivative and with it of b).  Box sums in int32, the response in int64, the maximum of
//                          an image by a wave reduction and one integer atomicMax per wave.
//   feat_cand_kernel     : a thread per pixel: the candidate rule into a state map (0 none, 1 undecided candidate).
//   feat_round_kernel    : a round of the greedy rule on the state map, a thread per pixel: an undecided candidate is
//                          rejected when a higher-priority neighbour nearer than min_distance is accepted, accepted when all
//                          of them are rejected (2 accepted, 3 rejected).  Both are final facts of the sequential rule, so
//                          reading a state another wave has just written, or a stale one, changes no outcome, and the
//                          highest-priority undecided candidate is decided in every round.  FEAT_WIDE_ROUNDS launches of it
//                          use the whole chip; they leave few candidates undecided, and only long dependency chains.
//   feat_select_kernel   : one workgroup of 512 per image.  (1) the candidates not yet rejected, in pixel order (prefix
//                          counts over runs of 16 pixels per thread); (2) the remaining rounds, until none is undecided;
//                          (3) the accepted ones in pixel order as
//                          (Rmax - R) << 32 | pixel; (4) a stable LSD radix sort of the upper half, 4 bits per pass,
//                          each thread a contiguous run, as many passes as the largest Rmax - R has digits: stable on a list
//                          in pixel order is the index tie rule; (5) the first max_features.
//                          The capacity of every list is H W: there is no overflow path.
//   feat_describe_kernel : one wave per keypoint: the 37 x 37 grey patch in LDS, the moments over the disc of radius 15 by an
//                          integer wave reduction, the bin, the separable binomial blur as unnormalised integer sums, the 256
//                          tests 64 at a time with the bytes taken from __ballot.
//   feat_points_kernel   : a thread per keypoint, float64.
//   feat_stereo_kernel   : the stereo frame's depth (stereo_handler.cpp:148-227 in place of the depth image at rgbd_handler.cpp:309):
//                          one wave per keypoint.  The 3 x 15 left window and the right strip of the whole disparity range in
//                          LDS, a disparity per lane and round (at most 5), the costs kept in LDS, the best by a wave minimum
//                          of (cost << 9 | d), the second best by another with the neighbours of the best masked out; for
//                          the left-right check the right window and the mirrored left strip take the same buffers.  The
//                          rules are stereo.h's.  No atomics; a keypoint's result depends on nothing else in the batch.
//   feat_pyr_level_kernel : the scale pyramid (feat_pyr.h): one launch per level, the frame on grid.y; a thread makes 4 consecutive
//                          bytes of the level image from the 2 x 2 footprints in the level below and stores them as one word,
//                          and the level's validity map in the same pass when a depth image is given.
//   feat_pyr_merge_kernel : a thread per output row of a frame: the levels' rows, each cut at its budget, one after another; the
//                          position is the exclusive sum of the (at most 8) counts of the frame, added up per thread.  No atomics.
//   feat_pyr_subpix_kernel: the sub-pixel offsets (feat_pyr.h): a thread per keypoint reads the response map at it and at its four
//                          neighbours; the merge then writes the refined level-0 coordinates and takes X and Y from them.
// A batch of n images occupies n workgroups in the selection, so a small batch leaves most of the chip idle there (accepted
// as for the PnP kernel: DESIGN.md).
#include "common.h"
#include "feat.h"
#include "feat_pyr.h"
#include "stereo.h"
#include "feat_args.h"             // FEAT_TILE, FEAT_MAX_PIXELS, StereoParams and the argument checks

#define FEAT_SEL_BLOCK 512
#define FEAT_SEL_WAVES (FEAT_SEL_BLOCK / 64)
#define FEAT_SEL_RUN 16
#define FEAT_WINDOW_RUN 16
#define FEAT_MAX_DISTANCE 1024
#define FEAT_WIDE_ROUNDS 4        // rounds of the greedy rule run over the whole chip before one workgroup per image finishes

typedef unsigned long long u64;

__constant__ FeatPattern c_feat_pattern = feat_make_pattern();

struct FeatImage { int64_t base; int H, W; };

__device__ __forceinline__ FeatImage feat_image(const int64_t *off, const int32_t *hw, int c) {
    FeatImage im = {off[c], hw[2 * c], hw[2 * c + 1]};
    return im;
}

// ---- grey ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feat_gray_kernel(const uint8_t *__restrict__ src, const int64_t *__restrict__ src_off,
                                                        const int64_t *__restrict__ off, uint8_t *__restrict__ gray) {
    const int c = blockIdx.y;
    const int64_t n = off[c + 1] - off[c], i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = src + src_off[c];
    if (src_off[c + 1] - src_off[c] == n) gray[off[c] + i] = s[i];
    else gray[off[c] + i] = (uint8_t)feat_gray(s[3 * i], s[3 * i + 1], s[3 * i + 2]);
}

// ---- response ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int feat_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(FEAT_TILE * FEAT_TILE) void feat_response_kernel(const uint8_t *__restrict__ gray, const int64_t *__restrict__ off,
                                                                              const int32_t *__restrict__ hw, int32_t *__restrict__ R,
                                                                              int32_t *__restrict__ rmax) {
    constexpr int G = FEAT_TILE + 4, D = FEAT_TILE + 2;
    __shared__ uint8_t s_g[G * G];
    __shared__ int16_t s_ix[D * D], s_iy[D * D];
    const int c = blockIdx.z, t = threadIdx.x;
    const FeatImage im = feat_image(off, hw, c);
    const int H = im.H, W = im.W, y0 = blockIdx.y * FEAT_TILE, x0 = blockIdx.x * FEAT_TILE;
    if (y0 >= H || x0 >= W) return;                        // the whole workgroup leaves
    for (int e = t; e < G * G; e += FEAT_TILE * FEAT_TILE) {
        const int yy = y0 - 2 + e / G, xx = x0 - 2 + e % G;
        s_g[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? gray[im.base + (int64_t)yy * W + xx] : (uint8_t)0;
    }
    __syncthreads();
    for (int e = t; e < D * D; e += FEAT_TILE * FEAT_TILE) {
        const int py = y0 - 1 + e / D, px = x0 - 1 + e % D;
        if (py < -1 || py > H || px < -1 || px > W) continue;             // no output pixel of the image reads it
        const int qy = feat_reflect(py, H), qx = feat_reflect(px, W);
        // rows and columns qy - 1 .. qy + 1 reflected into the image all lie inside the grey tile (H, W >= 2)
        const int r0 = feat_reflect(qy - 1, H) - (y0 - 2), r1 = qy - (y0 - 2), r2 = feat_reflect(qy + 1, H) - (y0 - 2);
        const int c0 = feat_reflect(qx - 1, W) - (x0 - 2), c1 = qx - (x0 - 2), c2 = feat_reflect(qx + 1, W) - (x0 - 2);
        const int g00 = s_g[r0 * G + c0], g01 = s_g[r0 * G + c1], g02 = s_g[r0 * G + c2];
        const int g10 = s_g[r1 * G + c0], g12 = s_g[r1 * G + c2];
        const int g20 = s_g[r2 * G + c0], g21 = s_g[r2 * G + c1], g22 = s_g[r2 * G + c2];
        s_ix[e] = (int16_t)((g02 + 2 * g12 + g22) - (g00 + 2 * g10 + g20));
        s_iy[e] = (int16_t)((g20 + 2 * g21 + g22) - (g00 + 2 * g01 + g02));
    }
    __syncthreads();
    const int ty = t / FEAT_TILE, tx = t % FEAT_TILE, y = y0 + ty, x = x0 + tx;
    int32_t r = 0;
    if (y < H && x < W) {
        int32_t a = 0, b = 0, cc = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = s_ix[(ty + dy) * D + tx + dx], iy = s_iy[(ty + dy) * D + tx + dx];
                a += ix * ix; b += ix * iy; cc += iy * iy;
            }
        r = feat_response(a, b, cc);
        R[im.base + (int64_t)y * W + x] = r;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t v = __shfl_xor(r, o, 64); r = v > r ? v : r; }
    if ((t & 63) == 0) atomicMax(&rmax[c], r);
}

// ---- candidates ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool feat_depth_valid(float d) { return d > 0.0f && d <= 3.4028234663852886e38f; }   // false for NaN, inf

__global__ __launch_bounds__(256) void feat_cand_kernel(const int32_t *__restrict__ R, const int32_t *__restrict__ rmax,
                                                        const uint8_t *__restrict__ valid, const float *__restrict__ depth,
                                                        const int64_t *__restrict__ off, const int32_t *__restrict__ hw, double quality,
                                                        int border, uint8_t *__restrict__ state) {
    const int c = blockIdx.y;
    const FeatImage im = feat_image(off, hw, c);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)im.H * im.W) return;
    const int H = im.H, W = im.W, y = (int)(i / W), x = (int)(i % W);
    const int32_t *Rc = R + im.base;
    const int32_t r = Rc[i];
    bool ok = y >= border && y <= H - 1 - border && x >= border && x <= W - 1 - border;
    ok = ok && (double)r > quality * (double)rmax[c];
    if (ok && valid) ok = valid[im.base + i] != 0;
    if (ok && depth) ok = feat_depth_valid(depth[im.base + i]);
    for (int dy = -1; dy <= 1 && ok; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            const int32_t v = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? Rc[(int64_t)yy * W + xx] : -1;
            ok = ok && r >= v;
        }
    state[im.base + i] = ok ? 1 : 0;
}

// ---- selection -----------------------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup in thread order; *total = the sum.  s_w: FEAT_SEL_WAVES ints.
__device__ __forceinline__ int feat_block_exscan(int v, int *s_w, int t, int *total) {
    const int lane = t & 63, wave = t >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
    __syncthreads();                                       // s_w of the previous call has been read
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0, sum = 0;
    for (int w = 0; w < FEAT_SEL_WAVES; ++w) { if (w < wave) before += s_w[w]; sum += s_w[w]; }
    *total = sum;
    return before + inc - v;
}

// The state map (0 none, 1 undecided, 2 accepted, 3 rejected) is read while other waves write it: relaxed atomics of the
// scope the readers share.  A stale 1 only postpones a decision.
template <int SCOPE> __device__ __forceinline__ int feat_state_load(const uint8_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE> __device__ __forceinline__ void feat_state_store(uint8_t *p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }

// One step of the greedy rule for the undecided candidate `pix`: rejected when a candidate that comes before it (larger R,
// then lower index) and lies nearer than md is accepted, accepted when all of those are rejected.  Both are final facts of
// the sequential rule whenever they are read.  Returns true when it stays undecided.
template <int SCOPE> __device__ __forceinline__ bool feat_decide(const int32_t *R, uint8_t *state, int H, int W, int md, int pix) {
    const int y = pix / W, x = pix % W;
    const int32_t r = R[pix];
    bool blocked = false;
    const int ya = y - (md - 1) < 0 ? 0 : y - (md - 1), yb = y + (md - 1) > H - 1 ? H - 1 : y + (md - 1);
    const int xa = x - (md - 1) < 0 ? 0 : x - (md - 1), xb = x + (md - 1) > W - 1 ? W - 1 : x + (md - 1);
    for (int yy = ya; yy <= yb; ++yy)
        for (int x0 = xa; x0 <= xb; x0 += FEAT_WINDOW_RUN) {
            int s[FEAT_WINDOW_RUN];                        // a run of states loaded side by side, then looked at: one latency
#pragma unroll
            for (int e = 0; e < FEAT_WINDOW_RUN; ++e) s[e] = x0 + e <= xb ? feat_state_load<SCOPE>(state + yy * W + x0 + e) : 0;
#pragma unroll
            for (int e = 0; e < FEAT_WINDOW_RUN; ++e) {
                if (s[e] != 1 && s[e] != 2) continue;
                const int dy = yy - y, dx = x0 + e - x, j = yy * W + x0 + e;
                if (j == pix || dx * dx + dy * dy >= md * md) continue;
                const int32_t rj = R[j];
                if (!(rj > r || (rj == r && j < pix))) continue;              // j does not come before pix
                if (s[e] == 2) { feat_state_store<SCOPE>(state + pix, 3); return false; }
                blocked = true;
            }
        }
    if (!blocked) feat_state_store<SCOPE>(state + pix, 2);
    return blocked;
}

// a round over the whole image, a thread per pixel
__global__ __launch_bounds__(256) void feat_round_kernel(const int32_t *__restrict__ R, const int64_t *__restrict__ off,
                                                         const int32_t *__restrict__ hw, int md, uint8_t *state) {
    const int c = blockIdx.y;
    const FeatImage im = feat_image(off, hw, c);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)im.H * im.W) return;
    if (feat_state_load<__HIP_MEMORY_SCOPE_AGENT>(state + im.base + i) != 1) return;
    (void)feat_decide<__HIP_MEMORY_SCOPE_AGENT>(R + im.base, state + im.base, im.H, im.W, md, (int)i);
}

struct FeatSelArgs {
    const int32_t *R; const int32_t *rmax; const int64_t *off; const int32_t *hw;
    uint8_t *state; int32_t *cand; u64 *ka, *kb;           // scratch, [total pixels] each
    int min_distance, max_features;
    int32_t *count, *kp, *resp;                            // [n], [n, max_features, 2], [n, max_features]
};

__global__ __launch_bounds__(FEAT_SEL_BLOCK) void feat_select_kernel(FeatSelArgs A) {
    __shared__ int s_w[FEAT_SEL_WAVES];
    __shared__ int s_max;
    __shared__ uint32_t s_h[16 * FEAT_SEL_BLOCK];
    const int c = blockIdx.x, t = threadIdx.x;
    const FeatImage im = feat_image(A.off, A.hw, c);
    const int H = im.H, W = im.W, npix = H * W, md = A.min_distance;
    const int32_t *R = A.R + im.base;
    uint8_t *state = A.state + im.base;
    int32_t *cand = A.cand + im.base;
    const int32_t Rmax = A.rmax[c];

    // (1) the candidates the rounds before have not rejected, in pixel order
    int ncand = 0;
    for (int p0 = 0; p0 < npix; p0 += FEAT_SEL_BLOCK * FEAT_SEL_RUN) {
        const int p = p0 + t * FEAT_SEL_RUN;
        int m = 0;
        for (int e = 0; e < FEAT_SEL_RUN; ++e)
            if (p + e < npix && (state[p + e] == 1 || state[p + e] == 2)) m |= 1 << e;
        int tot;
        int at = ncand + feat_block_exscan(__popc(m), s_w, t, &tot);
        for (int e = 0; e < FEAT_SEL_RUN; ++e)
            if (m >> e & 1) cand[at++] = p + e;
        ncand += tot;
    }
    __threadfence_block();
    __syncthreads();

    // (2) the remaining rounds of the greedy rule; every round decides a candidate, so ncand rounds are never exceeded
    for (int round = 0; round <= ncand; ++round) {
        int open = 0;
        for (int k = t; k < ncand; k += FEAT_SEL_BLOCK) {
            const int pix = cand[k];
            if (feat_state_load<__HIP_MEMORY_SCOPE_WORKGROUP>(state + pix) != 1) continue;
            if (feat_decide<__HIP_MEMORY_SCOPE_WORKGROUP>(R, state, H, W, md, pix)) open = 1;
        }
        __threadfence_block();
        if (!__syncthreads_or(open)) break;
    }

    // (3) the accepted ones in pixel order
    int n_acc = 0;
    if (t == 0) s_max = 0;
    for (int k0 = 0; k0 < ncand; k0 += FEAT_SEL_BLOCK) {
        const int k = k0 + t;
        int pix = -1;
        if (k < ncand) { pix = cand[k]; if (feat_state_load<__HIP_MEMORY_SCOPE_WORKGROUP>(state + pix) != 2) pix = -1; }
        int tot;
        const int at = n_acc + feat_block_exscan(pix >= 0 ? 1 : 0, s_w, t, &tot);
        if (pix >= 0) {
            const int key = Rmax - R[pix];
            A.ka[im.base + at] = ((u64)(uint32_t)key << 32) | (u64)(uint32_t)pix;
            atomicMax(&s_max, key);
        }
        n_acc += tot;
    }
    __threadfence_block();
    __syncthreads();

    // (4) stable radix sort of the upper half
    u64 *src = A.ka + im.base, *dst = A.kb + im.base;
    const int per = (n_acc + FEAT_SEL_BLOCK - 1) / FEAT_SEL_BLOCK;
    const int i0 = t * per < n_acc ? t * per : n_acc, i1 = i0 + per < n_acc ? i0 + per : n_acc;
    const int key_max = s_max;
    for (int shift = 32; shift < 64 && (key_max >> (shift - 32)) != 0; shift += 4) {
        for (int d = 0; d < 16; ++d) s_h[d * FEAT_SEL_BLOCK + t] = 0;
        for (int i = i0; i < i1; ++i) s_h[(int)((src[i] >> shift) & 15) * FEAT_SEL_BLOCK + t] += 1;
        __syncthreads();
        int sum = 0;
        for (int e = 0; e < 16; ++e) sum += (int)s_h[16 * t + e];
        int tot;
        int at = feat_block_exscan(sum, s_w, t, &tot);
        for (int e = 0; e < 16; ++e) { const int v = (int)s_h[16 * t + e]; s_h[16 * t + e] = (uint32_t)at; at += v; }
        __syncthreads();
        for (int i = i0; i < i1; ++i) {
            const u64 key = src[i];
            dst[s_h[(int)((key >> shift) & 15) * FEAT_SEL_BLOCK + t]++] = key;
        }
        __threadfence_block();
        __syncthreads();
        u64 *sw = src; src = dst; dst = sw;
    }

    // (5) the first max_features
    const int n_out = n_acc < A.max_features ? n_acc : A.max_features;
    for (int k = t; k < n_out; k += FEAT_SEL_BLOCK) {
        const u64 key = src[k];
        const int pix = (int)(uint32_t)key;
        const int64_t o = (int64_t)c * A.max_features + k;
        A.kp[2 * o] = pix % W;
        A.kp[2 * o + 1] = pix / W;
        A.resp[o] = Rmax - (int32_t)(key >> 32);
    }
    if (t == 0) A.count[c] = n_out;
}

// ---- keypoints of a batch: ragged (kp_off) or a fixed stride with counts --------------------------------------------
struct FeatKeypoints { const int32_t *kp; const int64_t *kp_off; const int32_t *count; int stride; };

__device__ __forceinline__ bool feat_keypoint_row(const FeatKeypoints &K, int c, int64_t k, int64_t *row) {
    const int64_t n = K.kp_off ? K.kp_off[c + 1] - K.kp_off[c] : (int64_t)(K.count[c] < K.stride ? K.count[c] : K.stride);
    *row = (K.kp_off ? K.kp_off[c] : (int64_t)c * K.stride) + k;
    return k < n;
}

// ---- orientation and descriptors -----------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void feat_describe_kernel(const uint8_t *__restrict__ gray, const int64_t *__restrict__ off,
                                                           const int32_t *__restrict__ hw, FeatKeypoints K, int32_t *__restrict__ bins,
                                                           uint8_t *__restrict__ desc) {
    constexpr int P = 2 * FEAT_MIN_BORDER + 1, B = 2 * FEAT_PATCH_RADIUS + 1, RAD = FEAT_PATCH_RADIUS;
    __shared__ uint8_t s_p[P * P];
    __shared__ uint16_t s_hb[P * B];
    __shared__ int32_t s_b[B * B];
    const int c = blockIdx.y, lane = threadIdx.x;
    int64_t row;
    if (!feat_keypoint_row(K, c, blockIdx.x, &row)) return;
    const FeatImage im = feat_image(off, hw, c);
    const int x = K.kp[2 * row], y = K.kp[2 * row + 1];
    if (x < FEAT_MIN_BORDER || x > im.W - 1 - FEAT_MIN_BORDER || y < FEAT_MIN_BORDER || y > im.H - 1 - FEAT_MIN_BORDER) {
        if (lane == 0) bins[row] = -1;                     // the patch would leave the image: nothing is read
        if (lane < FEAT_DESC_BYTES) desc[FEAT_DESC_BYTES * row + lane] = 0;
        return;
    }
    for (int e = lane; e < P * P; e += 64)
        s_p[e] = gray[im.base + (int64_t)(y - FEAT_MIN_BORDER + e / P) * im.W + (x - FEAT_MIN_BORDER + e % P)];
    __syncthreads();
    int m10 = 0, m01 = 0;
    for (int e = lane; e < B * B; e += 64) {
        const int dy = e / B - RAD, dx = e % B - RAD;
        if (dx * dx + dy * dy > RAD * RAD) continue;
        const int I = s_p[(dy + FEAT_MIN_BORDER) * P + dx + FEAT_MIN_BORDER];
        m10 += dx * I;
        m01 += dy * I;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { m10 += __shfl_xor(m10, o, 64); m01 += __shfl_xor(m01, o, 64); }
    const int bin = feat_bin(m10, m01);
    for (int e = lane; e < P * B; e += 64) {
        const uint8_t *p = s_p + (e / B) * P + e % B;
        s_hb[e] = (uint16_t)(p[0] + 6 * p[1] + 15 * p[2] + 20 * p[3] + 15 * p[4] + 6 * p[5] + p[6]);
    }
    __syncthreads();
    for (int e = lane; e < B * B; e += 64) {
        const uint16_t *p = s_hb + e;
        s_b[e] = p[0] + 6 * p[B] + 15 * p[2 * B] + 20 * p[3 * B] + 15 * p[4 * B] + 6 * p[5 * B] + p[6 * B];
    }
    __syncthreads();
    for (int r = 0; r < FEAT_PAIRS / 64; ++r) {
        const int8_t *pq = c_feat_pattern.v[r * 64 + lane];
        int px, py, qx, qy;
        feat_rotate(pq[0], pq[1], bin, &px, &py);
        feat_rotate(pq[2], pq[3], bin, &qx, &qy);
        const u64 m = __ballot(s_b[(py + RAD) * B + px + RAD] < s_b[(qy + RAD) * B + qx + RAD]);
        if (lane < 8) desc[FEAT_DESC_BYTES * row + 8 * r + lane] = (uint8_t)(m >> (8 * lane));
    }
    if (lane == 0) bins[row] = bin;
}

// ---- 3D points -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feat_points_kernel(const float *__restrict__ depth, const int64_t *__restrict__ off,
                                                          const int32_t *__restrict__ hw, FeatKeypoints K, const double *__restrict__ cams,
                                                          double *__restrict__ pts) {
    const int c = blockIdx.y;
    int64_t row;
    if (!feat_keypoint_row(K, c, (int64_t)blockIdx.x * 256 + threadIdx.x, &row)) return;
    const FeatImage im = feat_image(off, hw, c);
    const int u = K.kp[2 * row], v = K.kp[2 * row + 1];
    const double fx = cams[4 * c], fy = cams[4 * c + 1], cx = cams[4 * c + 2], cy = cams[4 * c + 3];
    double X = NAN, Y = NAN, Z = NAN;
    if (u >= 0 && u < im.W && v >= 0 && v < im.H) {
        const float d = depth[im.base + (int64_t)v * im.W + u];
        if (feat_depth_valid(d)) {
            Z = (double)d;
            X = (((double)u - cx) * Z) / fx;
            Y = (((double)v - cy) * Z) / fy;
        }
    }
    pts[3 * row] = X; pts[3 * row + 1] = Y; pts[3 * row + 2] = Z;
}

// ---- sparse stereo -------------------------------------------------------------------------------------------------
#define STEREO_WIN_STRIDE 16
#define STEREO_STRIP_STRIDE 272    // >= STEREO_STRIP_W
#define STEREO_NO_KEY 0x7fffffff

__device__ __forceinline__ int32_t stereo_wave_min(int32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int32_t w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}

// The costs of the window against the `count` windows of the strip, entry i for the disparity d_lo + i, into s_cost; the
// wave's smallest key.  Window i of the strip starts at its column i, or at count - 1 - i when `mirrored` (the right strip:
// a larger disparity lies further left).
__device__ __forceinline__ int32_t stereo_search(const uint8_t *s_win, const uint8_t *s_strip, int count, int d_lo, bool mirrored,
                                                 int32_t *s_cost, int lane) {
    int w[STEREO_WIN_H * STEREO_WIN_W];
#pragma unroll
    for (int e = 0; e < STEREO_WIN_H * STEREO_WIN_W; ++e) w[e] = s_win[(e / STEREO_WIN_W) * STEREO_WIN_STRIDE + e % STEREO_WIN_W];
    int32_t best = STEREO_NO_KEY;
    for (int i = lane; i < count; i += 64) {
        const uint8_t *p = s_strip + (mirrored ? count - 1 - i : i);
        int32_t cost = 0;
#pragma unroll
        for (int e = 0; e < STEREO_WIN_H * STEREO_WIN_W; ++e) {
            const int diff = w[e] - (int)p[(e / STEREO_WIN_W) * STEREO_STRIP_STRIDE + e % STEREO_WIN_W];
            cost += diff * diff;
        }
        s_cost[i] = cost;
        const int32_t key = stereo_key(cost, d_lo + i);
        best = key < best ? key : best;
    }
    return stereo_wave_min(best);
}

// rows v - 1 .. v + 1, columns x0 .. x0 + width - 1 of an image into LDS rows of `stride` bytes
__device__ __forceinline__ void stereo_stage(const uint8_t *img, int W, int v, int x0, int width, uint8_t *s, int stride, int lane) {
    for (int e = lane; e < STEREO_WIN_H * width; e += 64) {
        const int r = e / width, x = e % width;
        s[r * stride + x] = img[(int64_t)(v - STEREO_HALF_H + r) * W + x0 + x];
    }
}

__global__ __launch_bounds__(64) void feat_stereo_kernel(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right,
                                                         const int64_t *__restrict__ off, const int32_t *__restrict__ hw, FeatKeypoints K,
                                                         const double *__restrict__ cams, StereoParams P, double *__restrict__ disparity,
                                                         int32_t *__restrict__ status, int32_t *__restrict__ best, double *__restrict__ pts) {
    __shared__ uint8_t s_win[STEREO_WIN_H * STEREO_WIN_STRIDE];
    __shared__ uint8_t s_strip[STEREO_WIN_H * STEREO_STRIP_STRIDE];
    __shared__ int32_t s_cost[STEREO_MAX_RANGE];
    const int c = blockIdx.y, lane = threadIdx.x;
    int64_t row;
    if (!feat_keypoint_row(K, c, blockIdx.x, &row)) return;
    const FeatImage im = feat_image(off, hw, c);
    const int W = im.W, u = K.kp[2 * row], v = K.kp[2 * row + 1];
    int st = STEREO_ACCEPTED, ds = -1, d_lo = 0, d_hi = 0;
    int32_t ca = -1, cb = -1, cc = -1;
    // every branch below is taken by the whole wave: u, v and the reduced keys are the same in all lanes
    if (!stereo_inside(u, v, im.H, W)) st = STEREO_OUTSIDE;
    else if (!stereo_range(u, P.min_disparity, P.max_disparity, &d_lo, &d_hi)) st = STEREO_NO_RANGE;
    else {
        const uint8_t *L = left + im.base, *R = right + im.base;
        const int count = d_hi - d_lo + 1;                 // 3 .. 257
        stereo_stage(L, W, v, u - STEREO_HALF_W, STEREO_WIN_W, s_win, STEREO_WIN_STRIDE, lane);
        // columns u - d_hi - 7 >= 0 .. u - d_lo + 7 <= W - 1
        stereo_stage(R, W, v, u - d_hi - STEREO_HALF_W, count - 1 + STEREO_WIN_W, s_strip, STEREO_STRIP_STRIDE, lane);
        __syncthreads();
        const int32_t key = stereo_search(s_win, s_strip, count, d_lo, true, s_cost, lane);
        __syncthreads();
        ds = stereo_key_d(key);
        cb = stereo_key_cost(key);
        if (ds > d_lo) ca = s_cost[ds - 1 - d_lo];
        if (ds < d_hi) cc = s_cost[ds + 1 - d_lo];
        if (ds == d_lo || ds == d_hi) st = STEREO_EDGE;
        else {
            int32_t second = STEREO_NO_KEY;
            for (int i = lane; i < count; i += 64) {
                const int dd = d_lo + i - ds;
                if (dd >= 2 || dd <= -2) second = s_cost[i] < second ? s_cost[i] : second;
            }
            second = stereo_wave_min(second);
            if (second != STEREO_NO_KEY && stereo_not_unique(second, cb, P.uniqueness)) st = STEREO_NOT_UNIQUE;
            else if (P.lr_tolerance >= 0) {
                // back from the right column ur: its window is window d_hi - ds of the strip, the left strip takes the strip's place
                const int ur = u - ds, e_hi = stereo_range_back(ur, W, P.max_disparity), count2 = e_hi - d_lo + 1;      // ds in it
                uint8_t wv = 0;
                if (lane < STEREO_WIN_H * STEREO_WIN_W)
                    wv = s_strip[(lane / STEREO_WIN_W) * STEREO_STRIP_STRIDE + d_hi - ds + lane % STEREO_WIN_W];
                __syncthreads();                           // the strip and the costs have been read
                if (lane < STEREO_WIN_H * STEREO_WIN_W) s_win[(lane / STEREO_WIN_W) * STEREO_WIN_STRIDE + lane % STEREO_WIN_W] = wv;
                // columns ur + d_lo - 7 >= 1 (ds < d_hi <= u - 7) .. ur + e_hi + 7 <= W - 1
                stereo_stage(L, W, v, ur + d_lo - STEREO_HALF_W, count2 - 1 + STEREO_WIN_W, s_strip, STEREO_STRIP_STRIDE, lane);
                __syncthreads();
                const int es = stereo_key_d(stereo_search(s_win, s_strip, count2, d_lo, false, s_cost, lane));
                const int apart = es > ds ? es - ds : ds - es;
                if (apart > P.lr_tolerance) st = STEREO_LEFT_RIGHT;
            }
        }
    }
    if (lane != 0) return;
    double d = NAN, p[3] = {NAN, NAN, NAN};
    if (st == STEREO_ACCEPTED) {
        const double *cam = cams + 5 * c;
        d = stereo_parabola(ds, ca, cb, cc);
        stereo_point(u, v, d, cam[0], cam[1], cam[2], cam[3], cam[4], p);
    }
    disparity[row] = d;
    status[row] = st;
    if (best) { best[4 * row] = ds; best[4 * row + 1] = ca; best[4 * row + 2] = cb; best[4 * row + 3] = cc; }
    pts[3 * row] = p[0]; pts[3 * row + 1] = p[1]; pts[3 * row + 2] = p[2];
}

// ---- scale pyramid -------------------------------------------------------------------------------------------------
// A frame becomes `levels` images of the batch: level l of frame c is image l * n + c of the level layout (level-major: a
// launch of the level kernel reads one contiguous stretch and writes the next; frame-major measured the same times),
// whose offsets are multiples of FEAT_PYR_RUN so that a thread's run is one aligned word.  The rules are feat_pyr.h's.
#define FEAT_PYR_RUN 4             // output bytes per thread, stored as one word
#define FEAT_PYR_BLOCK 256         // threads: a workgroup covers 1024 consecutive bytes of a level image

struct FeatPyrLevelArgs {
    const uint8_t *src; const int64_t *src_off; const int32_t *src_hw; int src_at;               // source image src_at + c
    uint8_t *dst; const int64_t *lvl_off; const int32_t *lvl_hw; int levels, level;
    const float *depth; const int64_t *off; const int32_t *hw; uint8_t *valid;                    // level 0: depth NULL = no maps
};

// Level `level` of every frame from the level below it (level 0: from the grey batch, which the rule copies).  A thread
// walks FEAT_PYR_RUN consecutive pixels of the flat level image, across a row end if need be.
__global__ __launch_bounds__(FEAT_PYR_BLOCK) void feat_pyr_level_kernel(FeatPyrLevelArgs A) {
    const int c = blockIdx.y, n = gridDim.y;
    const FeatImage out = feat_image(A.lvl_off, A.lvl_hw, A.level * n + c);
    const int npix = out.H * out.W;                        // <= 2^30
    const int64_t first = ((int64_t)blockIdx.x * FEAT_PYR_BLOCK + threadIdx.x) * FEAT_PYR_RUN;
    if (first >= npix) return;
    const int p0 = (int)first;
    const FeatImage in = feat_image(A.src_off, A.src_hw, A.src_at + c);
    const uint8_t *g = A.src + in.base;
    const int H0 = A.hw[2 * c], W0 = A.hw[2 * c + 1];
    const float *depth = A.depth ? A.depth + A.off[c] : nullptr;
    int y = p0 / out.W, x = p0 % out.W;
    int r0, r1, b;
    feat_pyr_tap(y, out.H, in.H, &r0, &r1, &b);
    int py = depth ? feat_pyr_base_pixel(y, H0, out.H) : 0;
    uint32_t word = 0, vword = 0;
#pragma unroll
    for (int e = 0; e < FEAT_PYR_RUN; ++e) {
        if (p0 + e >= npix) break;
        int c0, c1, a;
        feat_pyr_tap(x, out.W, in.W, &c0, &c1, &a);
        const int v = feat_pyr_blend(g[(int64_t)r0 * in.W + c0], g[(int64_t)r0 * in.W + c1], g[(int64_t)r1 * in.W + c0],
                                     g[(int64_t)r1 * in.W + c1], a, b);
        word |= (uint32_t)v << (8 * e);
        if (depth && feat_depth_valid(depth[(int64_t)py * W0 + feat_pyr_base_pixel(x, W0, out.W)])) vword |= 1u << (8 * e);
        if (++x == out.W) {
            x = 0;
            ++y;
            if (y < out.H) {
                feat_pyr_tap(y, out.H, in.H, &r0, &r1, &b);
                if (depth) py = feat_pyr_base_pixel(y, H0, out.H);
            }
        }
    }
    *reinterpret_cast<uint32_t *>(A.dst + out.base + p0) = word;          // the layout pads every image to whole words
    if (depth) *reinterpret_cast<uint32_t *>(A.valid + out.base + p0) = vword;
}

struct FeatPyrMergeArgs {
    const int32_t *lcount, *lkp, *lresp, *lbins; const uint8_t *ldesc; int stride;   // per level image: [n L], [n L, stride, ..]
    const double *z;                                       // [n L, stride], or NULL: Z from the depth image
    const float *depth; const int64_t *off; const int32_t *hw, *lvl_hw;
    const double *cams; int levels, max_features;
    int budget[FEAT_PYR_MAX_LEVELS];
    int32_t *count; double *kp; int32_t *level_kp, *level, *base_px, *resp, *bins; uint8_t *desc; double *pts;   // base_px, pts: may be NULL
    const double *loff; double *offs;                      // sub-pixel offsets [n L, stride, 2] -> [n, max_features, 2], or both NULL
};

// Row k of frame c: the levels' rows one after another, level 0 first, each level cut at its budget.  The position of a
// level's rows is the exclusive sum of the counts before it, which every thread adds up for itself: no atomics.
__global__ __launch_bounds__(256) void feat_pyr_merge_kernel(FeatPyrMergeArgs A) {
    const int c = blockIdx.y, frames = gridDim.y, k = blockIdx.x * 256 + threadIdx.x;
    int at = 0, l = -1, j = 0;
    for (int e = 0; e < A.levels; ++e) {
        int n = A.lcount[e * frames + c];
        n = n < A.budget[e] ? n : A.budget[e];
        n = n < A.stride ? n : A.stride;
        if (l < 0 && k < at + n) { l = e; j = k - at; }
        at += n;
    }
    if (k == 0) A.count[c] = at;
    if (l < 0) return;
    const int im = l * frames + c;
    const int64_t src = (int64_t)im * A.stride + j, row = (int64_t)c * A.max_features + k;
    const int H0 = A.hw[2 * c], W0 = A.hw[2 * c + 1], Hl = A.lvl_hw[2 * im], Wl = A.lvl_hw[2 * im + 1];
    const int x = A.lkp[2 * src], y = A.lkp[2 * src + 1];
    double kx = feat_pyr_base_coord(x, W0, Wl), ky = feat_pyr_base_coord(y, H0, Hl);
    if (A.loff) {                                          // the refined coordinates; the pixel under the keypoint stays
        const double ox = A.loff[2 * src], oy = A.loff[2 * src + 1];
        kx = feat_pyr_subpix_coord(x, ox, W0, Wl);
        ky = feat_pyr_subpix_coord(y, oy, H0, Hl);
        A.offs[2 * row] = ox; A.offs[2 * row + 1] = oy;
    }
    const int px = feat_pyr_base_pixel(x, W0, Wl), py = feat_pyr_base_pixel(y, H0, Hl);
    A.kp[2 * row] = kx; A.kp[2 * row + 1] = ky;
    A.level_kp[2 * row] = x; A.level_kp[2 * row + 1] = y;
    A.level[row] = l;
    A.resp[row] = A.lresp[src];
    A.bins[row] = A.lbins[src];
    const uint4 *d = reinterpret_cast<const uint4 *>(A.ldesc + FEAT_DESC_BYTES * src);
    uint4 *o = reinterpret_cast<uint4 *>(A.desc + FEAT_DESC_BYTES * row);
    o[0] = d[0]; o[1] = d[1];
    if (A.base_px) { A.base_px[2 * row] = px; A.base_px[2 * row + 1] = py; }
    if (A.pts) {
        double Z = NAN, p[3];
        if (A.z) Z = A.z[src];
        else { const float dz = A.depth[A.off[c] + (int64_t)py * W0 + px]; if (feat_depth_valid(dz)) Z = (double)dz; }
        feat_pyr_point(kx, ky, Z, A.cams[4 * c], A.cams[4 * c + 1], A.cams[4 * c + 2], A.cams[4 * c + 3], p);
        A.pts[3 * row] = p[0]; A.pts[3 * row + 1] = p[1]; A.pts[3 * row + 2] = p[2];
    }
}

// The sub-pixel offsets of the keypoints of a batch of response maps (the rule: feat_pyr_subpix): a thread per keypoint,
// five loads of R.
__global__ __launch_bounds__(256) void feat_pyr_subpix_kernel(const int32_t *__restrict__ R, const int64_t *__restrict__ off,
                                                              const int32_t *__restrict__ hw, FeatKeypoints K, double *__restrict__ offs) {
    const int c = blockIdx.y;
    int64_t row;
    if (!feat_keypoint_row(K, c, (int64_t)blockIdx.x * 256 + threadIdx.x, &row)) return;
    const FeatImage im = feat_image(off, hw, c);
    double o[2];
    feat_pyr_subpix(R + im.base, im.H, im.W, K.kp[2 * row], K.kp[2 * row + 1], o);
    offs[2 * row] = o[0]; offs[2 * row + 1] = o[1];
}

// The merge's point rule on the Z the stereo kernel left in the rows (cams: five numbers per frame): X and Y move from the
// integer pixel the stereo rule ran at to the keypoint's level-0 coordinates; a rejected keypoint keeps its NaN row.
__global__ __launch_bounds__(256) void feat_pyr_repoint_kernel(const double *__restrict__ kp, const int32_t *__restrict__ count,
                                                               const double *__restrict__ cams, int max_features, double *__restrict__ pts) {
    const int c = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count[c]) return;
    const int64_t row = (int64_t)c * max_features + k;
    double p[3];
    feat_pyr_point(kp[2 * row], kp[2 * row + 1], pts[3 * row + 2], cams[5 * c], cams[5 * c + 1], cams[5 * c + 2], cams[5 * c + 3], p);
    pts[3 * row] = p[0]; pts[3 * row + 1] = p[1]; pts[3 * row + 2] = p[2];
}

// ---- host side -----------------------------------------------------------------------------------------------------
static StreamScratch g_feat_scratch;

static int feat_select_checks(double quality, int min_distance, int border, int max_features) {
    ARG_CHECK(quality >= 0.0 && quality <= 1.0, "quality_level must be in [0, 1]");
    ARG_CHECK(min_distance >= 1 && min_distance <= FEAT_MAX_DISTANCE, "min_distance must be in [1, 1024]");
    ARG_CHECK(border >= FEAT_MIN_BORDER, "border must be at least 18 (patch radius 15 plus blur radius 3)");
    ARG_CHECK(max_features >= 1 && max_features <= 65535, "max_features must be in [1, 65535]");
    return CSLAM_OK;
}

static int feat_kp_shape(const int64_t *h_kp_off, int n, RaggedShape *s) {
    ARG_CHECK(h_kp_off != nullptr, "h_kp_off is required");
    int rc = offsets_check(h_kp_off, n, s);
    if (rc) return rc;
    ARG_CHECK(s->largest <= 0x7fffffffll, "too many keypoints in one image");
    return CSLAM_OK;
}

struct FeatSelScratch { uint8_t *state; int32_t *cand; u64 *ka, *kb; };
static void feat_sel_carve(Carver &cv, size_t total, FeatSelScratch *s) {
    s->state = cv.take<uint8_t>(total);
    s->cand = cv.take<int32_t>(total);
    s->ka = cv.take<u64>(total);
    s->kb = cv.take<u64>(total);
}

static void feat_launch_gray(const uint8_t *src, const int64_t *src_off, const int64_t *off, int n, const FeatShape &sh, uint8_t *gray,
                             hipStream_t st) {
    hipLaunchKernelGGL(feat_gray_kernel, dim3((unsigned)ceil_div64(sh.px.largest, 256), (unsigned)n), dim3(256), 0, st, src, src_off, off, gray);
}

static int feat_launch_response(const uint8_t *gray, const int64_t *off, const int32_t *hw, int n, const FeatShape &sh, int32_t *R,
                                int32_t *rmax, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(rmax, 0, sizeof(int32_t) * (size_t)n, st));
    hipLaunchKernelGGL(feat_response_kernel, dim3((unsigned)ceil_div64(sh.max_w, FEAT_TILE), (unsigned)ceil_div64(sh.max_h, FEAT_TILE), (unsigned)n),
                       dim3(FEAT_TILE * FEAT_TILE), 0, st, gray, off, hw, R, rmax);
    return CSLAM_OK;
}

static void feat_launch_select(const int32_t *R, const int32_t *rmax, const uint8_t *valid, const float *depth, const int64_t *off,
                               const int32_t *hw, int n, const FeatShape &sh, double quality, int min_distance, int border, int max_features,
                               const FeatSelScratch &s, int32_t *count, int32_t *kp, int32_t *resp, hipStream_t st) {
    hipLaunchKernelGGL(feat_cand_kernel, dim3((unsigned)ceil_div64(sh.px.largest, 256), (unsigned)n), dim3(256), 0, st, R, rmax, valid, depth, off,
                       hw, quality, border, s.state);
    for (int round = 0; round < FEAT_WIDE_ROUNDS; ++round)
        hipLaunchKernelGGL(feat_round_kernel, dim3((unsigned)ceil_div64(sh.px.largest, 256), (unsigned)n), dim3(256), 0, st, R, off, hw, min_distance,
                           s.state);
    FeatSelArgs a = {R, rmax, off, hw, s.state, s.cand, s.ka, s.kb, min_distance, max_features, count, kp, resp};
    hipLaunchKernelGGL(feat_select_kernel, dim3((unsigned)n), dim3(FEAT_SEL_BLOCK), 0, st, a);
}

static void feat_launch_describe(const uint8_t *gray, const int64_t *off, const int32_t *hw, int n, const FeatKeypoints &K, int64_t most,
                                 int32_t *bins, uint8_t *desc, hipStream_t st) {
    if (most > 0)
        hipLaunchKernelGGL(feat_describe_kernel, dim3((unsigned)most, (unsigned)n), dim3(64), 0, st, gray, off, hw, K, bins, desc);
}

static void feat_launch_points(const float *depth, const int64_t *off, const int32_t *hw, int n, const FeatKeypoints &K, int64_t most,
                               const double *cams, double *pts, hipStream_t st) {
    if (most > 0)
        hipLaunchKernelGGL(feat_points_kernel, dim3((unsigned)ceil_div64(most, 256), (unsigned)n), dim3(256), 0, st, depth, off, hw, K, cams, pts);
}

static void feat_launch_subpix(const int32_t *R, const int64_t *off, const int32_t *hw, int n, const FeatKeypoints &K, int64_t most,
                               double *offs, hipStream_t st) {
    if (most > 0)
        hipLaunchKernelGGL(feat_pyr_subpix_kernel, dim3((unsigned)ceil_div64(most, 256), (unsigned)n), dim3(256), 0, st, R, off, hw, K, offs);
}

static void feat_launch_stereo(const uint8_t *left, const uint8_t *right, const int64_t *off, const int32_t *hw, int n, const FeatKeypoints &K,
                               int64_t most, const double *cams, const StereoParams &P, double *disparity, int32_t *status, int32_t *best,
                               double *pts, hipStream_t st) {
    if (most > 0)
        hipLaunchKernelGGL(feat_stereo_kernel, dim3((unsigned)most, (unsigned)n), dim3(64), 0, st, left, right, off, hw, K, cams, P, disparity,
                           status, best, pts);
}

CSLAM_API int cslam_feat_gray_dev(const uint8_t *d_src, const int64_t *d_src_off, const int64_t *d_off, const int32_t *d_hw, int n,
                                  uint8_t *d_gray, const int64_t *h_src_off, const int64_t *h_off, const int32_t *h_hw, void *stream) {
    FeatShape sh;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_src_check(h_src_off, h_off, n))) return rc;
    ARG_CHECK(d_src && d_src_off && d_off && d_hw && d_gray, "NULL argument");
    PTR_DEVICE(d_src);
    feat_launch_gray(d_src, d_src_off, d_off, n, sh, d_gray, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_response_dev(const uint8_t *d_gray, const int64_t *d_off, const int32_t *d_hw, int n, int32_t *d_R,
                                      int32_t *d_rmax, const int64_t *h_off, const int32_t *h_hw, void *stream) {
    FeatShape sh;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    ARG_CHECK(d_gray && d_off && d_hw && d_R && d_rmax, "NULL argument");
    PTR_DEVICE(d_gray);
    if ((rc = feat_launch_response(d_gray, d_off, d_hw, n, sh, d_R, d_rmax, (hipStream_t)stream))) return rc;
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_select_dev(const int32_t *d_R, const int32_t *d_rmax, const uint8_t *d_valid, const int64_t *d_off,
                                    const int32_t *d_hw, int n, double quality_level, int min_distance, int border, int max_features,
                                    int32_t *d_count, int32_t *d_kp, int32_t *d_resp, const int64_t *h_off, const int32_t *h_hw,
                                    void *stream) {
    FeatShape sh;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_select_checks(quality_level, min_distance, border, max_features))) return rc;
    ARG_CHECK(d_R && d_rmax && d_off && d_hw && d_count && d_kp && d_resp, "NULL argument");
    PTR_DEVICE(d_R);
    hipStream_t st = (hipStream_t)stream;
    FeatSelScratch s;
    auto layout = [&](Carver &cv) { feat_sel_carve(cv, (size_t)sh.px.total, &s); };
    SCRATCH_CARVE(g_feat_scratch, st, (size_t)1 << 20, layout);
    feat_launch_select(d_R, d_rmax, d_valid, nullptr, d_off, d_hw, n, sh, quality_level, min_distance, border, max_features, s, d_count, d_kp,
                       d_resp, st);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_describe_dev(const uint8_t *d_gray, const int64_t *d_off, const int32_t *d_hw, int n, const int32_t *d_kp,
                                      const int64_t *d_kp_off, int32_t *d_bins, uint8_t *d_desc, const int64_t *h_off,
                                      const int32_t *h_hw, const int64_t *h_kp_off, void *stream) {
    FeatShape sh;
    RaggedShape ks;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_kp_shape(h_kp_off, n, &ks))) return rc;
    ARG_CHECK(d_gray && d_off && d_hw && d_kp && d_kp_off && d_bins && d_desc, "NULL argument");
    PTR_DEVICE(d_gray);
    FeatKeypoints K = {d_kp, d_kp_off, nullptr, 0};
    feat_launch_describe(d_gray, d_off, d_hw, n, K, ks.largest, d_bins, d_desc, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_points_dev(const float *d_depth, const int64_t *d_off, const int32_t *d_hw, int n, const int32_t *d_kp,
                                    const int64_t *d_kp_off, const double *d_cameras, double *d_points, const int64_t *h_off,
                                    const int32_t *h_hw, const int64_t *h_kp_off, void *stream) {
    FeatShape sh;
    RaggedShape ks;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_kp_shape(h_kp_off, n, &ks))) return rc;
    ARG_CHECK(d_depth && d_off && d_hw && d_kp && d_kp_off && d_cameras && d_points, "NULL argument");
    PTR_DEVICE(d_depth);
    FeatKeypoints K = {d_kp, d_kp_off, nullptr, 0};
    feat_launch_points(d_depth, d_off, d_hw, n, K, ks.largest, d_cameras, d_points, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_subpixel_dev(const int32_t *d_R, const int64_t *d_off, const int32_t *d_hw, int n, const int32_t *d_kp,
                                      const int64_t *d_kp_off, double *d_offsets, const int64_t *h_off, const int32_t *h_hw,
                                      const int64_t *h_kp_off, void *stream) {
    FeatShape sh;
    RaggedShape ks;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_kp_shape(h_kp_off, n, &ks))) return rc;
    ARG_CHECK(d_R && d_off && d_hw && d_kp && d_kp_off && d_offsets, "NULL argument");
    PTR_DEVICE(d_R);
    FeatKeypoints K = {d_kp, d_kp_off, nullptr, 0};
    feat_launch_subpix(d_R, d_off, d_hw, n, K, ks.largest, d_offsets, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_extract_dev(const uint8_t *d_src, const int64_t *d_src_off, const float *d_depth, const int64_t *d_off,
                                     const int32_t *d_hw, const double *d_cameras, int n, double quality_level, int min_distance,
                                     int border, int max_features, int depth_as_mask, int32_t *d_count, int32_t *d_kp, int32_t *d_resp,
                                     int32_t *d_bins, uint8_t *d_desc, double *d_points, const int64_t *h_src_off, const int64_t *h_off,
                                     const int32_t *h_hw, void *stream) {
    FeatShape sh;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_src_check(h_src_off, h_off, n))) return rc;
    if ((rc = feat_select_checks(quality_level, min_distance, border, max_features))) return rc;
    ARG_CHECK(d_src && d_src_off && d_depth && d_off && d_hw && d_cameras && d_count && d_kp && d_resp && d_bins && d_desc && d_points,
              "NULL argument");
    PTR_DEVICE(d_src);
    hipStream_t st = (hipStream_t)stream;
    FeatSelScratch s;
    uint8_t *gray;
    int32_t *R, *rmax;
    auto layout = [&](Carver &cv) {
        gray = cv.take<uint8_t>((size_t)sh.px.total);
        R = cv.take<int32_t>((size_t)sh.px.total);
        rmax = cv.take<int32_t>((size_t)n);
        feat_sel_carve(cv, (size_t)sh.px.total, &s);
    };
    SCRATCH_CARVE(g_feat_scratch, st, (size_t)1 << 20, layout);
    feat_launch_gray(d_src, d_src_off, d_off, n, sh, gray, st);
    if ((rc = feat_launch_response(gray, d_off, d_hw, n, sh, R, rmax, st))) return rc;
    feat_launch_select(R, rmax, nullptr, depth_as_mask ? d_depth : nullptr, d_off, d_hw, n, sh, quality_level, min_distance, border,
                       max_features, s, d_count, d_kp, d_resp, st);
    FeatKeypoints K = {d_kp, nullptr, d_count, max_features};
    feat_launch_describe(gray, d_off, d_hw, n, K, max_features, d_bins, d_desc, st);
    feat_launch_points(d_depth, d_off, d_hw, n, K, max_features, d_cameras, d_points, st);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_stereo_dev(const uint8_t *d_left, const uint8_t *d_right, const int64_t *d_off, const int32_t *d_hw, int n,
                                    const int32_t *d_kp, const int64_t *d_kp_off, const double *d_cameras, int min_disparity,
                                    int max_disparity, int uniqueness, int lr_tolerance, double *d_disparity, int32_t *d_status,
                                    int32_t *d_best, double *d_points, const int64_t *h_off, const int32_t *h_hw, const int64_t *h_kp_off,
                                    const double *h_cameras, void *stream) {
    FeatShape sh;
    RaggedShape ks;
    const StereoParams P = {min_disparity, max_disparity, uniqueness, lr_tolerance};
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_kp_shape(h_kp_off, n, &ks))) return rc;
    if ((rc = feat_stereo_checks(P, h_cameras, n))) return rc;
    ARG_CHECK(d_left && d_right && d_off && d_hw && d_kp && d_kp_off && d_cameras && d_disparity && d_status && d_best && d_points,
              "NULL argument");
    PTR_DEVICE(d_left);
    FeatKeypoints K = {d_kp, d_kp_off, nullptr, 0};
    feat_launch_stereo(d_left, d_right, d_off, d_hw, n, K, ks.largest, d_cameras, P, d_disparity, d_status, d_best, d_points,
                       (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_extract_stereo_dev(const uint8_t *d_left, const int64_t *d_left_off, const uint8_t *d_right,
                                            const int64_t *d_right_off, const int64_t *d_off, const int32_t *d_hw, const double *d_cameras,
                                            int n, double quality_level, int min_distance, int border, int max_features, int min_disparity,
                                            int max_disparity, int uniqueness, int lr_tolerance, int32_t *d_count, int32_t *d_kp,
                                            int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc, double *d_points, double *d_disparity,
                                            int32_t *d_status, const int64_t *h_left_off, const int64_t *h_right_off, const int64_t *h_off,
                                            const int32_t *h_hw, const double *h_cameras, void *stream) {
    FeatShape sh;
    const StereoParams P = {min_disparity, max_disparity, uniqueness, lr_tolerance};
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_src_check(h_left_off, h_off, n))) return rc;
    if ((rc = feat_src_check(h_right_off, h_off, n))) return rc;
    if ((rc = feat_select_checks(quality_level, min_distance, border, max_features))) return rc;
    if ((rc = feat_stereo_checks(P, h_cameras, n))) return rc;
    ARG_CHECK(d_left && d_left_off && d_right && d_right_off && d_off && d_hw && d_cameras && d_count && d_kp && d_resp && d_bins && d_desc &&
                  d_points && d_disparity && d_status,
              "NULL argument");
    PTR_DEVICE(d_left);
    hipStream_t st = (hipStream_t)stream;
    FeatSelScratch s;
    uint8_t *gray_l, *gray_r;
    int32_t *R, *rmax;
    auto layout = [&](Carver &cv) {
        gray_l = cv.take<uint8_t>((size_t)sh.px.total);
        gray_r = cv.take<uint8_t>((size_t)sh.px.total);
        R = cv.take<int32_t>((size_t)sh.px.total);
        rmax = cv.take<int32_t>((size_t)n);
        feat_sel_carve(cv, (size_t)sh.px.total, &s);
    };
    SCRATCH_CARVE(g_feat_scratch, st, (size_t)1 << 20, layout);
    feat_launch_gray(d_left, d_left_off, d_off, n, sh, gray_l, st);
    feat_launch_gray(d_right, d_right_off, d_off, n, sh, gray_r, st);
    if ((rc = feat_launch_response(gray_l, d_off, d_hw, n, sh, R, rmax, st))) return rc;
    feat_launch_select(R, rmax, nullptr, nullptr, d_off, d_hw, n, sh, quality_level, min_distance, border, max_features, s, d_count, d_kp,
                       d_resp, st);                        // a stereo frame has no depth image, so no mask
    FeatKeypoints K = {d_kp, nullptr, d_count, max_features};
    feat_launch_describe(gray_l, d_off, d_hw, n, K, max_features, d_bins, d_desc, st);
    feat_launch_stereo(gray_l, gray_r, d_off, d_hw, n, K, max_features, d_cameras, P, d_disparity, d_status, nullptr, d_points, st);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

// ---- scale pyramid: host side --------------------------------------------------------------------------------------
// The level layout of a batch, from the host sizes: image l * n + c = level l of frame c, every offset a multiple of
// FEAT_PYR_RUN.  The caller passes the same layout on the device and on the host, as it passes d_off and h_off.
struct FeatPyrLayout {
    std::vector<int64_t> off;
    std::vector<int32_t> hw;
    FeatShape sh;                                          // of the n * levels level images
    int budget[FEAT_PYR_MAX_LEVELS];
};

static int feat_pyr_layout(const int32_t *h_hw, int n, int levels, int min_side, const int64_t *h_lvl_off, const int32_t *h_lvl_hw,
                           FeatPyrLayout *P) {
    ARG_CHECK(levels >= 1 && levels <= FEAT_PYR_MAX_LEVELS, "levels must be in [1, 8]");
    ARG_CHECK((int64_t)n * levels <= 65535, "n * levels must be at most 65535");
    ARG_CHECK(h_lvl_off != nullptr && h_lvl_hw != nullptr, "h_lvl_off and h_lvl_hw are required");
    P->off.assign((size_t)n * levels + 1, 0);
    P->hw.assign((size_t)n * levels * 2, 0);
    P->sh.px.largest = 0;
    P->sh.px.smallest = INT64_MAX;
    P->sh.max_h = P->sh.max_w = 0;
    for (int l = 0; l < levels; ++l)
        for (int c = 0; c < n; ++c) {
            const int H = h_hw[2 * c], W = h_hw[2 * c + 1];
            ARG_CHECK(H <= FEAT_PYR_MAX_SIDE && W <= FEAT_PYR_MAX_SIDE, "a pyramid image has at most 2^20 rows and columns");
            const int i = l * n + c, Hl = feat_pyr_size(H, l), Wl = feat_pyr_size(W, l);
            ARG_CHECK(Hl >= min_side && Wl >= min_side, "a frame is too small for its top level (every level: at least 2 x 2, and 2 * border + 1 on each side)");
            const int64_t px = (int64_t)Hl * Wl;
            P->hw[2 * i] = Hl;
            P->hw[2 * i + 1] = Wl;
            P->off[i + 1] = P->off[i] + round_up64(px, FEAT_PYR_RUN);
            if (px > P->sh.px.largest) P->sh.px.largest = px;
            if (px < P->sh.px.smallest) P->sh.px.smallest = px;
            if (Hl > P->sh.max_h) P->sh.max_h = Hl;
            if (Wl > P->sh.max_w) P->sh.max_w = Wl;
        }
    P->sh.px.total = P->off[(size_t)n * levels];
    for (size_t i = 0; i < P->off.size(); ++i) ARG_CHECK(h_lvl_off[i] == P->off[i], "h_lvl_off is not the level layout of h_hw");
    for (size_t i = 0; i < P->hw.size(); ++i) ARG_CHECK(h_lvl_hw[i] == P->hw[i], "h_lvl_hw is not the level layout of h_hw");
    return CSLAM_OK;
}

// level 0 from the grey batch, every further level from the one below; the maps in the same passes when depth is given
static void feat_launch_pyramid(const uint8_t *gray, const int64_t *off, const int32_t *hw, int n, int levels, const float *depth,
                                const int64_t *lvl_off, const int32_t *lvl_hw, const FeatPyrLayout &P, uint8_t *lvl_gray, uint8_t *lvl_valid,
                                hipStream_t st) {
    for (int l = 0; l < levels; ++l) {
        int64_t largest = 0;
        for (int c = 0; c < n; ++c) {
            const int64_t px = (int64_t)P.hw[2 * (l * n + c)] * P.hw[2 * (l * n + c) + 1];
            if (px > largest) largest = px;
        }
        FeatPyrLevelArgs a = {l ? lvl_gray : gray, l ? lvl_off : off, l ? lvl_hw : hw, l ? (l - 1) * n : 0,
                              lvl_gray, lvl_off, lvl_hw, levels, l, depth, off, hw, lvl_valid};
        hipLaunchKernelGGL(feat_pyr_level_kernel, dim3((unsigned)ceil_div64(largest, FEAT_PYR_BLOCK * FEAT_PYR_RUN), (unsigned)n),
                           dim3(FEAT_PYR_BLOCK), 0, st, a);
    }
}

static void feat_launch_merge(FeatPyrMergeArgs &a, const FeatPyrLayout &P, int n, hipStream_t st) {
    for (int l = 0; l < FEAT_PYR_MAX_LEVELS; ++l) a.budget[l] = l < a.levels ? P.budget[l] : 0;
    hipLaunchKernelGGL(feat_pyr_merge_kernel, dim3((unsigned)ceil_div64(a.max_features, 256), (unsigned)n), dim3(256), 0, st, a);
}

CSLAM_API int cslam_feat_pyramid_dev(const uint8_t *d_gray, const int64_t *d_off, const int32_t *d_hw, int n, int levels,
                                     const float *d_depth, const int64_t *d_lvl_off, const int32_t *d_lvl_hw, uint8_t *d_lvl_gray,
                                     uint8_t *d_lvl_valid, const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off,
                                     const int32_t *h_lvl_hw, void *stream) {
    FeatShape sh;
    FeatPyrLayout P;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_pyr_layout(h_hw, n, levels, 2, h_lvl_off, h_lvl_hw, &P))) return rc;
    ARG_CHECK(d_gray && d_off && d_hw && d_lvl_off && d_lvl_hw && d_lvl_gray, "NULL argument");
    ARG_CHECK((d_depth != nullptr) == (d_lvl_valid != nullptr), "d_lvl_valid goes with d_depth");
    ARG_CHECK((uintptr_t)d_lvl_gray % FEAT_PYR_RUN == 0 && (uintptr_t)d_lvl_valid % FEAT_PYR_RUN == 0, "the level images start on a 4-byte boundary");
    PTR_DEVICE(d_gray);
    feat_launch_pyramid(d_gray, d_off, d_hw, n, levels, d_depth, d_lvl_off, d_lvl_hw, P, d_lvl_gray, d_lvl_valid, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_pyramid_merge_dev(const int32_t *d_lvl_count, const int32_t *d_lvl_kp, const int32_t *d_lvl_resp,
                                           const int32_t *d_lvl_bins, const uint8_t *d_lvl_desc, const double *d_lvl_z, int stride,
                                           const int32_t *d_hw, const int32_t *d_lvl_hw, const double *d_cameras, int n, int levels,
                                           int max_features, int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels,
                                           int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc, double *d_points, const int32_t *h_hw,
                                           const int64_t *h_lvl_off, const int32_t *h_lvl_hw, void *stream) {
    FeatPyrLayout P;
    BATCH_COUNT_CHECK(n);
    ARG_CHECK(h_hw != nullptr, "h_hw is required");
    for (int c = 0; c < n; ++c) ARG_CHECK(h_hw[2 * c] >= 2 && h_hw[2 * c + 1] >= 2, "an image is at least 2 x 2");
    int rc = feat_pyr_layout(h_hw, n, levels, 2, h_lvl_off, h_lvl_hw, &P);
    if (rc) return rc;
    ARG_CHECK(max_features >= 1 && max_features <= 65535, "max_features must be in [1, 65535]");
    ARG_CHECK(stride >= 1 && stride <= 65535, "stride must be in [1, 65535]");
    ARG_CHECK(d_lvl_count && d_lvl_kp && d_lvl_resp && d_lvl_bins && d_lvl_desc && d_lvl_z && d_hw && d_lvl_hw && d_cameras && d_count && d_kp &&
                  d_level_kp && d_levels && d_resp && d_bins && d_desc && d_points,
              "NULL argument");
    ARG_CHECK((uintptr_t)d_lvl_desc % 16 == 0 && (uintptr_t)d_desc % 16 == 0, "the descriptors start on a 16-byte boundary");
    PTR_DEVICE(d_lvl_kp);
    feat_pyr_budgets(max_features, levels, P.budget);
    FeatPyrMergeArgs a = {d_lvl_count, d_lvl_kp, d_lvl_resp, d_lvl_bins, d_lvl_desc, stride, d_lvl_z, nullptr, nullptr, d_hw, d_lvl_hw,
                          d_cameras, levels, max_features, {0}, d_count, d_kp, d_level_kp, d_levels, nullptr, d_resp, d_bins, d_desc, d_points};
    feat_launch_merge(a, P, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

// what both pyramid chains share up to the per-level rows: level images (and maps), response, selection with the largest
// budget (a level's first rows are its selection at any smaller one), bins and descriptors on the level images
struct FeatPyrRows { uint8_t *gray; int32_t *count, *kp, *resp, *bins; uint8_t *desc; int stride; double *loff; };   // loff: NULL = integer keypoints

static int feat_pyr_rows(const uint8_t *gray0, const float *mask_depth, const int64_t *d_off, const int32_t *d_hw, int n, int levels,
                         const int64_t *d_lvl_off, const int32_t *d_lvl_hw, const FeatPyrLayout &P, double quality, int min_distance,
                         int border, uint8_t *lvl_valid, int32_t *R, int32_t *rmax, const FeatSelScratch &s, const FeatPyrRows &rows,
                         hipStream_t st) {
    const int nl = n * levels;
    feat_launch_pyramid(gray0, d_off, d_hw, n, levels, mask_depth, d_lvl_off, d_lvl_hw, P, rows.gray, lvl_valid, st);
    int rc = feat_launch_response(rows.gray, d_lvl_off, d_lvl_hw, nl, P.sh, R, rmax, st);
    if (rc) return rc;
    feat_launch_select(R, rmax, mask_depth ? lvl_valid : nullptr, nullptr, d_lvl_off, d_lvl_hw, nl, P.sh, quality, min_distance, border,
                       rows.stride, s, rows.count, rows.kp, rows.resp, st);
    FeatKeypoints K = {rows.kp, nullptr, rows.count, rows.stride};
    feat_launch_describe(rows.gray, d_lvl_off, d_lvl_hw, nl, K, rows.stride, rows.bins, rows.desc, st);
    if (rows.loff) feat_launch_subpix(R, d_lvl_off, d_lvl_hw, nl, K, rows.stride, rows.loff, st);
    return CSLAM_OK;
}

static void feat_pyr_rows_carve(Carver &cv, const FeatPyrLayout &P, int nl, bool maps, bool subpixel, uint8_t **lvl_valid, int32_t **R,
                                int32_t **rmax, FeatSelScratch *s, FeatPyrRows *rows) {
    const size_t total = (size_t)P.sh.px.total, r = (size_t)nl * rows->stride;
    rows->gray = cv.take<uint8_t>(total);
    *lvl_valid = maps ? cv.take<uint8_t>(total) : nullptr;
    *R = cv.take<int32_t>(total);
    *rmax = cv.take<int32_t>((size_t)nl);
    feat_sel_carve(cv, total, s);
    rows->count = cv.take<int32_t>((size_t)nl);
    rows->kp = cv.take<int32_t>(2 * r);
    rows->resp = cv.take<int32_t>(r);
    rows->bins = cv.take<int32_t>(r);
    rows->desc = cv.take<uint8_t>(FEAT_DESC_BYTES * r);
    rows->loff = subpixel ? cv.take<double>(2 * r) : nullptr;
}

// both pyramid chains, with and without sub-pixel keypoints: d_offsets NULL = the integer keypoints
static int feat_extract_pyramid(const uint8_t *d_src, const int64_t *d_src_off, const float *d_depth, const int64_t *d_off,
                                const int32_t *d_hw, const double *d_cameras, int n, int levels, const int64_t *d_lvl_off,
                                const int32_t *d_lvl_hw, double quality_level, int min_distance, int border, int max_features,
                                int depth_as_mask, int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels, int32_t *d_resp,
                                int32_t *d_bins, uint8_t *d_desc, double *d_points, double *d_offsets, const int64_t *h_src_off,
                                const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw, void *stream) {
    FeatShape sh;
    FeatPyrLayout P;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_src_check(h_src_off, h_off, n))) return rc;
    if ((rc = feat_select_checks(quality_level, min_distance, border, max_features))) return rc;
    if ((rc = feat_pyr_layout(h_hw, n, levels, 2 * border + 1, h_lvl_off, h_lvl_hw, &P))) return rc;
    ARG_CHECK(d_src && d_src_off && d_depth && d_off && d_hw && d_cameras && d_lvl_off && d_lvl_hw && d_count && d_kp && d_level_kp && d_levels &&
                  d_resp && d_bins && d_desc && d_points,
              "NULL argument");
    ARG_CHECK((uintptr_t)d_desc % 16 == 0, "the descriptors start on a 16-byte boundary");
    PTR_DEVICE(d_src);
    hipStream_t st = (hipStream_t)stream;
    feat_pyr_budgets(max_features, levels, P.budget);
    FeatSelScratch s;
    FeatPyrRows rows = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, P.budget[0]};
    uint8_t *gray, *lvl_valid;
    int32_t *R, *rmax;
    auto layout = [&](Carver &cv) {
        gray = cv.take<uint8_t>((size_t)sh.px.total);
        feat_pyr_rows_carve(cv, P, n * levels, depth_as_mask != 0, d_offsets != nullptr, &lvl_valid, &R, &rmax, &s, &rows);
    };
    SCRATCH_CARVE(g_feat_scratch, st, (size_t)1 << 20, layout);
    feat_launch_gray(d_src, d_src_off, d_off, n, sh, gray, st);
    if ((rc = feat_pyr_rows(gray, depth_as_mask ? d_depth : nullptr, d_off, d_hw, n, levels, d_lvl_off, d_lvl_hw, P, quality_level, min_distance,
                            border, lvl_valid, R, rmax, s, rows, st)))
        return rc;
    FeatPyrMergeArgs a = {rows.count, rows.kp, rows.resp, rows.bins, rows.desc, rows.stride, nullptr, d_depth, d_off, d_hw, d_lvl_hw,
                          d_cameras, levels, max_features, {0}, d_count, d_kp, d_level_kp, d_levels, nullptr, d_resp, d_bins, d_desc, d_points,
                          rows.loff, d_offsets};
    feat_launch_merge(a, P, n, st);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_extract_pyramid_dev(const uint8_t *d_src, const int64_t *d_src_off, const float *d_depth, const int64_t *d_off,
                                             const int32_t *d_hw, const double *d_cameras, int n, int levels, const int64_t *d_lvl_off,
                                             const int32_t *d_lvl_hw, double quality_level, int min_distance, int border, int max_features,
                                             int depth_as_mask, int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels,
                                             int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc, double *d_points, const int64_t *h_src_off,
                                             const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw,
                                             void *stream) {
    return feat_extract_pyramid(d_src, d_src_off, d_depth, d_off, d_hw, d_cameras, n, levels, d_lvl_off, d_lvl_hw, quality_level, min_distance,
                                border, max_features, depth_as_mask, d_count, d_kp, d_level_kp, d_levels, d_resp, d_bins, d_desc, d_points,
                                nullptr, h_src_off, h_off, h_hw, h_lvl_off, h_lvl_hw, stream);
}

CSLAM_API int cslam_feat_extract_pyramid_subpix_dev(const uint8_t *d_src, const int64_t *d_src_off, const float *d_depth,
                                                    const int64_t *d_off, const int32_t *d_hw, const double *d_cameras, int n, int levels,
                                                    const int64_t *d_lvl_off, const int32_t *d_lvl_hw, double quality_level,
                                                    int min_distance, int border, int max_features, int depth_as_mask, int32_t *d_count,
                                                    double *d_kp, int32_t *d_level_kp, int32_t *d_levels, int32_t *d_resp, int32_t *d_bins,
                                                    uint8_t *d_desc, double *d_points, double *d_offsets, const int64_t *h_src_off,
                                                    const int64_t *h_off, const int32_t *h_hw, const int64_t *h_lvl_off,
                                                    const int32_t *h_lvl_hw, void *stream) {
    ARG_CHECK(d_offsets != nullptr, "NULL argument");
    return feat_extract_pyramid(d_src, d_src_off, d_depth, d_off, d_hw, d_cameras, n, levels, d_lvl_off, d_lvl_hw, quality_level, min_distance,
                                border, max_features, depth_as_mask, d_count, d_kp, d_level_kp, d_levels, d_resp, d_bins, d_desc, d_points,
                                d_offsets, h_src_off, h_off, h_hw, h_lvl_off, h_lvl_hw, stream);
}

static int feat_extract_stereo_pyramid(const uint8_t *d_left, const int64_t *d_left_off, const uint8_t *d_right, const int64_t *d_right_off,
                                       const int64_t *d_off, const int32_t *d_hw, const double *d_cameras, int n, int levels,
                                       const int64_t *d_lvl_off, const int32_t *d_lvl_hw, double quality_level, int min_distance, int border,
                                       int max_features, int min_disparity, int max_disparity, int uniqueness, int lr_tolerance,
                                       int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels, int32_t *d_resp,
                                       int32_t *d_bins, uint8_t *d_desc, double *d_points, double *d_disparity, int32_t *d_status,
                                       double *d_offsets, const int64_t *h_left_off, const int64_t *h_right_off, const int64_t *h_off,
                                       const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw, const double *h_cameras,
                                       void *stream) {
    FeatShape sh;
    FeatPyrLayout P;
    const StereoParams SP = {min_disparity, max_disparity, uniqueness, lr_tolerance};
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_src_check(h_left_off, h_off, n))) return rc;
    if ((rc = feat_src_check(h_right_off, h_off, n))) return rc;
    if ((rc = feat_select_checks(quality_level, min_distance, border, max_features))) return rc;
    if ((rc = feat_stereo_checks(SP, h_cameras, n))) return rc;
    if ((rc = feat_pyr_layout(h_hw, n, levels, 2 * border + 1, h_lvl_off, h_lvl_hw, &P))) return rc;
    ARG_CHECK(d_left && d_left_off && d_right && d_right_off && d_off && d_hw && d_cameras && d_lvl_off && d_lvl_hw && d_count && d_kp &&
                  d_level_kp && d_levels && d_resp && d_bins && d_desc && d_points && d_disparity && d_status,
              "NULL argument");
    ARG_CHECK((uintptr_t)d_desc % 16 == 0, "the descriptors start on a 16-byte boundary");
    PTR_DEVICE(d_left);
    hipStream_t st = (hipStream_t)stream;
    feat_pyr_budgets(max_features, levels, P.budget);
    FeatSelScratch s;
    FeatPyrRows rows = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, P.budget[0]};
    uint8_t *gray_l, *gray_r, *lvl_valid;
    int32_t *R, *rmax, *base_px;
    auto layout = [&](Carver &cv) {
        gray_l = cv.take<uint8_t>((size_t)sh.px.total);
        gray_r = cv.take<uint8_t>((size_t)sh.px.total);
        base_px = cv.take<int32_t>((size_t)n * max_features * 2);
        feat_pyr_rows_carve(cv, P, n * levels, false, d_offsets != nullptr, &lvl_valid, &R, &rmax, &s, &rows);
    };
    SCRATCH_CARVE(g_feat_scratch, st, (size_t)1 << 20, layout);
    feat_launch_gray(d_left, d_left_off, d_off, n, sh, gray_l, st);
    feat_launch_gray(d_right, d_right_off, d_off, n, sh, gray_r, st);
    if ((rc = feat_pyr_rows(gray_l, nullptr, d_off, d_hw, n, levels, d_lvl_off, d_lvl_hw, P, quality_level, min_distance, border, lvl_valid, R,
                            rmax, s, rows, st)))
        return rc;
    FeatPyrMergeArgs a = {rows.count, rows.kp, rows.resp, rows.bins, rows.desc, rows.stride, nullptr, nullptr, d_off, d_hw, d_lvl_hw,
                          d_cameras, levels, max_features, {0}, d_count, d_kp, d_level_kp, d_levels, base_px, d_resp, d_bins, d_desc, nullptr,
                          rows.loff, d_offsets};
    feat_launch_merge(a, P, n, st);
    // the stereo rule at the level-0 pixels under the keypoints, then X and Y of its rows at the keypoints' own coordinates
    FeatKeypoints K = {base_px, nullptr, d_count, max_features};
    feat_launch_stereo(gray_l, gray_r, d_off, d_hw, n, K, max_features, d_cameras, SP, d_disparity, d_status, nullptr, d_points, st);
    hipLaunchKernelGGL(feat_pyr_repoint_kernel, dim3((unsigned)ceil_div64(max_features, 256), (unsigned)n), dim3(256), 0, st, d_kp, d_count,
                       d_cameras, max_features, d_points);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feat_extract_stereo_pyramid_dev(const uint8_t *d_left, const int64_t *d_left_off, const uint8_t *d_right,
                                                    const int64_t *d_right_off, const int64_t *d_off, const int32_t *d_hw,
                                                    const double *d_cameras, int n, int levels, const int64_t *d_lvl_off,
                                                    const int32_t *d_lvl_hw, double quality_level, int min_distance, int border,
                                                    int max_features, int min_disparity, int max_disparity, int uniqueness, int lr_tolerance,
                                                    int32_t *d_count, double *d_kp, int32_t *d_level_kp, int32_t *d_levels, int32_t *d_resp,
                                                    int32_t *d_bins, uint8_t *d_desc, double *d_points, double *d_disparity, int32_t *d_status,
                                                    const int64_t *h_left_off, const int64_t *h_right_off, const int64_t *h_off,
                                                    const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw,
                                                    const double *h_cameras, void *stream) {
    return feat_extract_stereo_pyramid(d_left, d_left_off, d_right, d_right_off, d_off, d_hw, d_cameras, n, levels, d_lvl_off, d_lvl_hw,
                                       quality_level, min_distance, border, max_features, min_disparity, max_disparity, uniqueness,
                                       lr_tolerance, d_count, d_kp, d_level_kp, d_levels, d_resp, d_bins, d_desc, d_points, d_disparity,
                                       d_status, nullptr, h_left_off, h_right_off, h_off, h_hw, h_lvl_off, h_lvl_hw, h_cameras, stream);
}

CSLAM_API int cslam_feat_extract_stereo_pyramid_subpix_dev(const uint8_t *d_left, const int64_t *d_left_off, const uint8_t *d_right,
                                                           const int64_t *d_right_off, const int64_t *d_off, const int32_t *d_hw,
                                                           const double *d_cameras, int n, int levels, const int64_t *d_lvl_off,
                                                           const int32_t *d_lvl_hw, double quality_level, int min_distance, int border,
                                                           int max_features, int min_disparity, int max_disparity, int uniqueness,
                                                           int lr_tolerance, int32_t *d_count, double *d_kp, int32_t *d_level_kp,
                                                           int32_t *d_levels, int32_t *d_resp, int32_t *d_bins, uint8_t *d_desc,
                                                           double *d_points, double *d_disparity, int32_t *d_status, double *d_offsets,
                                                           const int64_t *h_left_off, const int64_t *h_right_off, const int64_t *h_off,
                                                           const int32_t *h_hw, const int64_t *h_lvl_off, const int32_t *h_lvl_hw,
                                                           const double *h_cameras, void *stream) {
    ARG_CHECK(d_offsets != nullptr, "NULL argument");
    return feat_extract_stereo_pyramid(d_left, d_left_off, d_right, d_right_off, d_off, d_hw, d_cameras, n, levels, d_lvl_off, d_lvl_hw,
                                       quality_level, min_distance, border, max_features, min_disparity, max_disparity, uniqueness,
                                       lr_tolerance, d_count, d_kp, d_level_kp, d_levels, d_resp, d_bins, d_desc, d_points, d_disparity,
                                       d_status, d_offsets, h_left_off, h_right_off, h_off, h_hw, h_lvl_off, h_lvl_hw, h_cameras, stream);
}
