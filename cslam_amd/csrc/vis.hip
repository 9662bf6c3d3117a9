// vis.hip -- geometric verification of a visual loop closure (gfx950): binary keypoint matching and 3D -> 2D PnP RANSAC.
//
// Replaces the `registration_.computeTransformation(from, to, ...)` calls of src/front_end/rgbd_handler.cpp:433-469
// (receive_local_keyframe_match) and :493-554 (receive_local_image_descriptors) for a batch of keyframe pairs that carry 2D
// keypoints, their 3D points and 32-byte binary descriptors (:471-491).  Behind that call is rtabmap's visual registration,
// which is third party and was not available to compare against: parity with rtabmap / OpenCV is unpinned.  The algorithm is
// the one stated in include/cslam_hip.h and pnp.h; tests/vis_reference.py restates it in float64 numpy.
//
//   vis_match_kernel   : one workgroup per (pair, 256 "from" rows).  A lane keeps its descriptor in 8 registers; the "to"
//                        descriptors go through LDS in chunks of 256 rows (8 KiB) and every lane reads the same row at a
//                        time (a broadcast).  8 x (xor, popcount) per distance; nearest, second nearest and the nearest
//                        index per lane, the lowest index on ties.  A row that passes the ratio test claims its "to" row by
//                        an integer atomicMin on (distance << 32 | from row).
//   vis_compact_kernel : one workgroup per pair: the claims that held, ascending in the from row (ballot + prefix counts).
//   vis_pnp_kernel     : one workgroup of 256 threads per pair; the usable correspondences live in LDS as float64 SoA
//                        (5 x 2048 x 8 = 80 KiB, plus their source index and inlier flag: 90 KiB of the CU's 160).
//                        A: a hypothesis per lane (sample, P3P, selection by the fourth point; pnp.h), looped over
//                        `iterations`; B: the same lane scores it over all correspondences by broadcast LDS reads;
//                        C: the best (inlier count, then lowest h) by a packed integer max; D: rounds of Gauss-Newton on
//                        the inlier set and a recount: lanes stride over the points, a fixed shuffle tree per wave, the
//                        waves added in wave order by thread 0, which solves and broadcasts.
//                        vis_pnp_kernel<true> is the level-aware form (pnp.h): sigma2 of each correspondence's "to" level
//                        lies beside it in LDS as a float64 (16 KiB more: 106 KiB), which scales its inlier threshold and
//                        divides its Gauss-Newton terms; vis_pnp_kernel<false> compiles to what it was without the form.
// No float atomics; every floating sum has a fixed order: a pair's bytes are the same alone or in any batch.  A batch of P
// pairs occupies P workgroups in the PnP kernel, so a small batch leaves most of the chip idle (accepted: DESIGN.md).
#include "common.h"
#include "pnp.h"

#define VIS_DESC_BYTES 32
#define VIS_MATCH_BLOCK 256
#define VIS_MATCH_CHUNK 256
#define VIS_MAX_CORR 2048
#define VIS_BLOCK 256
#define VIS_WAVES (VIS_BLOCK / 64)
#define VIS_GN_TOL 1e-10
#define VIS_PNP_LDS (5 * VIS_MAX_CORR * 8 + VIS_MAX_CORR * 4 + VIS_MAX_CORR)
#define VIS_PNP_LEVELS_LDS (VIS_PNP_LDS + VIS_MAX_CORR * 8)

typedef unsigned long long u64;

// ---- matching ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIS_MATCH_BLOCK) void vis_match_kernel(const uint32_t *__restrict__ da, const int64_t *__restrict__ a_off,
                                                                   const uint32_t *__restrict__ db, const int64_t *__restrict__ b_off,
                                                                   double nndr, int32_t *__restrict__ nn, u64 *__restrict__ claim) {
    __shared__ uint32_t s_d[VIS_MATCH_CHUNK * 8];
    const int p = blockIdx.y, t = threadIdx.x;
    const int64_t a0 = a_off[p], na = a_off[p + 1] - a0, b0 = b_off[p], nb = b_off[p + 1] - b0;
    const int64_t i0 = (int64_t)blockIdx.x * VIS_MATCH_BLOCK;
    if (i0 >= na) return;                                  // the whole workgroup leaves
    const int64_t i = i0 + t;
    const bool live = i < na;
    uint32_t q[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) q[w] = live ? da[8 * (a0 + i) + w] : 0u;
    int d1 = 0x7fffffff, d2 = 0x7fffffff, i1 = -1;
    for (int64_t c0 = 0; c0 < nb; c0 += VIS_MATCH_CHUNK) {
        const int cm = nb - c0 < VIS_MATCH_CHUNK ? (int)(nb - c0) : VIS_MATCH_CHUNK;
        __syncthreads();                                   // the previous chunk has been consumed
        for (int e = t; e < 8 * cm; e += VIS_MATCH_BLOCK) s_d[e] = db[8 * (b0 + c0) + e];
        __syncthreads();
        for (int r = 0; r < cm; ++r) {
            int d = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w) d += __popc(q[w] ^ s_d[8 * r + w]);
            if (d < d1) { d2 = d1; d1 = d; i1 = (int)(c0 + r); }
            else if (d < d2) d2 = d;
        }
    }
    if (!live) return;
    const bool match = nb >= 2 && (double)d1 <= nndr * (double)d2;
    nn[2 * (a0 + i)] = match ? i1 : -1;
    nn[2 * (a0 + i) + 1] = d1;
    if (match) atomicMin(&claim[b0 + i1], ((u64)d1 << 32) | (u64)i);
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_compact_kernel(const int64_t *__restrict__ a_off, const int64_t *__restrict__ b_off,
                                                               const int32_t *__restrict__ nn, const u64 *__restrict__ claim,
                                                               int32_t *__restrict__ rows, int32_t *__restrict__ count) {
    __shared__ int s_w[VIS_WAVES];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t a0 = a_off[p], na = a_off[p + 1] - a0, b0 = b_off[p];
    int base = 0;
    for (int64_t c0 = 0; c0 < na; c0 += VIS_BLOCK) {
        const int64_t i = c0 + t;
        int j = -1;
        if (i < na) {
            j = nn[2 * (a0 + i)];
            if (j >= 0 && claim[b0 + j] != (((u64)nn[2 * (a0 + i) + 1] << 32) | (u64)i)) j = -1;
        }
        const u64 m = __ballot(j >= 0);
        __syncthreads();                                   // s_w of the previous chunk has been read
        if (lane == 0) s_w[wave] = (int)__popcll(m);
        __syncthreads();
        int at = base + (int)__popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) at += s_w[w];
        if (j >= 0) { rows[2 * (a0 + at)] = (int32_t)i; rows[2 * (a0 + at) + 1] = j; }
        for (int w = 0; w < VIS_WAVES; ++w) base += s_w[w];
    }
    if (t == 0) count[p] = base;
}

// ---- PnP RANSAC ----------------------------------------------------------------------------------------------------
struct VisPnpArgs {
    const double *pts; const int64_t *pts_off;             // "from" 3D points [., 3]
    const double *pix; const int64_t *pix_off;             // "to" pixels [., 2]
    const int32_t *rows; const int64_t *row_off; const int32_t *count;      // correspondences (from row, to row), pair-local
    const double *cams;                                    // [n_pairs, 4]
    int iterations, min_inliers, refine_iterations, refine_rounds;
    double thr2;
    u64 seed;
    double *T; int32_t *info; int32_t *flags;              // [n_pairs, 16], [n_pairs, 8], [total rows]
    double *hyp_pose; int32_t *hyp_info;                   // NULL, or [n_pairs, iterations, 12] and [n_pairs, iterations, 2]
    const int32_t *lvl;                                    // the level-aware form: the level of every "to" row, in the layout of pix
};

__device__ __forceinline__ int vis_block_count(bool x, int *s_w, int t) {
    const u64 m = __ballot(x);
    __syncthreads();
    if ((t & 63) == 0) s_w[t >> 6] = (int)__popcll(m);
    __syncthreads();
    int n = 0;
    for (int w = 0; w < VIS_WAVES; ++w) n += s_w[w];
    return n;
}

// the inlier rule of correspondence k; sW: sigma2 per correspondence (the level-aware form only)
template <bool LEVELS>
__device__ __forceinline__ bool vis_inlier(const double *R, const double *t, const double *cam, const double *x, double u, double v,
                                           double thr2, const double *sW, int k) {
    if constexpr (LEVELS) return pnp_inlier_level(R, t, cam, x, u, v, thr2, sW[k]);
    else return pnp_inlier(R, t, cam, x, u, v, thr2);
}

template <bool LEVELS> __global__ __launch_bounds__(VIS_BLOCK) void vis_pnp_kernel(VisPnpArgs A) {
    extern __shared__ __attribute__((aligned(16))) char vis_smem[];
    double *sX = (double *)vis_smem, *sY = sX + VIS_MAX_CORR, *sZ = sY + VIS_MAX_CORR, *sU = sZ + VIS_MAX_CORR, *sV = sU + VIS_MAX_CORR;
    int32_t *s_src = (int32_t *)(sV + VIS_MAX_CORR);
    uint8_t *s_inl = (uint8_t *)(s_src + VIS_MAX_CORR);
    double *sW = LEVELS ? (double *)(s_inl + VIS_MAX_CORR) : nullptr;      // sigma2 per correspondence; the uniform form has no room for it
    __shared__ int s_w[VIS_WAVES];
    __shared__ u64 s_key[VIS_WAVES];
    __shared__ double s_sum[VIS_WAVES][PNP_NSUM];
    __shared__ double s_pose[12];
    __shared__ int s_flag;

    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t r0 = A.row_off[p], cap = A.row_off[p + 1] - r0;
    int64_t given = A.count ? (int64_t)A.count[p] : cap;
    given = given < 0 ? 0 : (given > cap ? cap : given);
    const int64_t p0 = A.pts_off[p], np_ = A.pts_off[p + 1] - p0, x0 = A.pix_off[p], nx_ = A.pix_off[p + 1] - x0;
    double cam[4];
    for (int e = 0; e < 4; ++e) cam[e] = A.cams[4 * (int64_t)p + e];

    // usable correspondences, in order, into LDS; the rest are counted
    int M = 0;
    for (int64_t c0 = 0; c0 < given; c0 += VIS_BLOCK) {
        const int64_t k = c0 + t;
        bool ok = false;
        double x[3] = {0.0, 0.0, 0.0}, u = 0.0, v = 0.0;
        int lv = 0;
        if (k < given) {
            A.flags[r0 + k] = 0;
            const int64_t i = A.rows[2 * (r0 + k)], j = A.rows[2 * (r0 + k) + 1];
            if (i >= 0 && i < np_ && j >= 0 && j < nx_) {  // a row that points outside its keyframes is dropped
                for (int a = 0; a < 3; ++a) x[a] = A.pts[3 * (p0 + i) + a];
                u = A.pix[2 * (x0 + j)]; v = A.pix[2 * (x0 + j) + 1];
                if constexpr (LEVELS) lv = A.lvl[x0 + j];
                ok = pnp_finite(x[0]) && pnp_finite(x[1]) && pnp_finite(x[2]) && pnp_finite(u) && pnp_finite(v);
            }
        }
        const u64 m = __ballot(ok);
        __syncthreads();
        if (lane == 0) s_w[wave] = (int)__popcll(m);
        __syncthreads();
        int at = M + (int)__popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) at += s_w[w];
        if (ok && at < VIS_MAX_CORR) { sX[at] = x[0]; sY[at] = x[1]; sZ[at] = x[2]; sU[at] = u; sV[at] = v; s_src[at] = (int)k; }
        // The host refused levels outside 0 .. PNP_MAX_LEVEL on h_levels_to; the device copy is trusted to equal that checked copy,
        // and the clamp only bounds the loop of pnp_level_sigma2 should a caller break that.
        if constexpr (LEVELS)
            if (ok && at < VIS_MAX_CORR) sW[at] = pnp_level_sigma2(lv < 0 ? 0 : (lv > PNP_MAX_LEVEL ? PNP_MAX_LEVEL : lv));
        for (int w = 0; w < VIS_WAVES; ++w) M += s_w[w];
    }
    __syncthreads();

    double *Tp = A.T + 16 * (int64_t)p;
    int32_t *info = A.info + 8 * (int64_t)p;
    const int need = A.min_inliers > 4 ? A.min_inliers : 4;
    if (M > VIS_MAX_CORR || M < need) {                    // not attempted: the identity
        if (t < 16) Tp[t] = t % 5 == 0 ? 1.0 : 0.0;
        if (t == 0) {
            info[0] = M > VIS_MAX_CORR ? 3 : 2; info[1] = (int)given; info[2] = M; info[3] = (int)(given - M);
            info[4] = 0; info[5] = -1; info[6] = 0; info[7] = 0;
        }
        if (A.hyp_info)
            for (int h = t; h < A.iterations; h += VIS_BLOCK) {
                A.hyp_info[2 * ((int64_t)p * A.iterations + h)] = 0;
                A.hyp_info[2 * ((int64_t)p * A.iterations + h) + 1] = 0;
                for (int e = 0; e < 12; ++e) A.hyp_pose[12 * ((int64_t)p * A.iterations + h) + e] = 0.0;
            }
        return;
    }

    // A + B: a hypothesis per lane, scored by the lane
    u64 best_key = 0;
    double bR[9], bt[3];
    bool best_valid = false;
    for (int e = 0; e < 9; ++e) bR[e] = e % 4 == 0 ? 1.0 : 0.0;
    for (int e = 0; e < 3; ++e) bt[e] = 0.0;
    for (int h = t; h < A.iterations; h += VIS_BLOCK) {
        int idx[4];
        pnp_sample(A.seed, (uint32_t)h, M, idx);
        double X4[12], uv4[8], R[9], tt[3];
        for (int j = 0; j < 4; ++j) {
            X4[3 * j] = sX[idx[j]]; X4[3 * j + 1] = sY[idx[j]]; X4[3 * j + 2] = sZ[idx[j]];
            uv4[2 * j] = sU[idx[j]]; uv4[2 * j + 1] = sV[idx[j]];
        }
        const bool valid = pnp_hypothesis(X4, uv4, cam, R, tt);
        int cnt = 0;
        if (valid)
            for (int k = 0; k < M; ++k) {
                const double x[3] = {sX[k], sY[k], sZ[k]};
                cnt += vis_inlier<LEVELS>(R, tt, cam, x, sU[k], sV[k], A.thr2, sW, k) ? 1 : 0;
            }
        const u64 key = ((u64)cnt << 32) | (u64)(0x7fffffff - h);
        if (key > best_key) {
            best_key = key; best_valid = valid;
            for (int e = 0; e < 9; ++e) bR[e] = valid ? R[e] : (e % 4 == 0 ? 1.0 : 0.0);
            for (int e = 0; e < 3; ++e) bt[e] = valid ? tt[e] : 0.0;
        }
        if (A.hyp_info) {
            const int64_t o = (int64_t)p * A.iterations + h;
            A.hyp_info[2 * o] = valid ? 1 : 0;
            A.hyp_info[2 * o + 1] = cnt;
            for (int e = 0; e < 9; ++e) A.hyp_pose[12 * o + e] = valid ? R[e] : 0.0;
            for (int e = 0; e < 3; ++e) A.hyp_pose[12 * o + 9 + e] = valid ? tt[e] : 0.0;
        }
    }
    // C: the best key over the workgroup; its lane publishes the pose
    u64 wk = best_key;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const u64 y = __shfl_xor(wk, o, 64); wk = y > wk ? y : wk; }
    if (lane == 0) s_key[wave] = wk;
    __syncthreads();
    for (int w = 0; w < VIS_WAVES; ++w) wk = s_key[w] > wk ? s_key[w] : wk;
    if (best_key == wk) {                                  // keys are distinct: every h belongs to one lane
        for (int e = 0; e < 9; ++e) s_pose[e] = bR[e];
        for (int e = 0; e < 3; ++e) s_pose[9 + e] = bt[e];
        s_flag = best_valid ? 1 : 0;
    }
    __syncthreads();
    const int best_h = 0x7fffffff - (int)(wk & 0xffffffffull), best_cnt = (int)(wk >> 32);
    const bool have = s_flag != 0;
    double R[9], tt[3];
    for (int e = 0; e < 9; ++e) R[e] = s_pose[e];
    for (int e = 0; e < 3; ++e) tt[e] = s_pose[9 + e];

    // D: the inlier set of the best hypothesis, then rounds of Gauss-Newton and a recount
    int inliers = 0, steps = 0;
    for (int k0 = 0; k0 < M; k0 += VIS_BLOCK) {
        const int k = k0 + t;
        bool in = false;
        if (k < M && have) {
            const double x[3] = {sX[k], sY[k], sZ[k]};
            in = vis_inlier<LEVELS>(R, tt, cam, x, sU[k], sV[k], A.thr2, sW, k);
        }
        if (k < M) s_inl[k] = in ? 1 : 0;
        inliers += vis_block_count(in, s_w, t);
    }
    for (int round = 0; round < A.refine_rounds && have; ++round) {
        for (int it = 0; it < A.refine_iterations; ++it) {
            double s[PNP_NSUM];
#pragma unroll
            for (int e = 0; e < PNP_NSUM; ++e) s[e] = 0.0;
            for (int k = t; k < M; k += VIS_BLOCK)
                if (s_inl[k]) {
                    const double x[3] = {sX[k], sY[k], sZ[k]};
                    if constexpr (LEVELS) pnp_gn_accumulate_level(R, tt, cam, x, sU[k], sV[k], 1.0 / sW[k], s);
                    else pnp_gn_accumulate(R, tt, cam, x, sU[k], sV[k], s);
                }
#pragma unroll
            for (int e = 0; e < PNP_NSUM; ++e) {
                double x = s[e];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
                if (lane == 0) s_sum[wave][e] = x;
            }
            __syncthreads();
            if (t == 0) {
                double tot[PNP_NSUM], delta[6];
                for (int e = 0; e < PNP_NSUM; ++e) {
                    double a = s_sum[0][e];
                    for (int w = 1; w < VIS_WAVES; ++w) a += s_sum[w][e];
                    tot[e] = a;
                }
                int stop = 1;
                if (pnp_gn_solve(tot, delta)) {
                    double Rn[9], tn[3];
                    for (int e = 0; e < 9; ++e) Rn[e] = R[e];
                    for (int e = 0; e < 3; ++e) tn[e] = tt[e];
                    const double nd = pnp_gn_apply(delta, Rn, tn);
                    bool fin = pnp_finite(nd);
                    for (int e = 0; e < 9; ++e) fin = fin && pnp_finite(Rn[e]);
                    for (int e = 0; e < 3; ++e) fin = fin && pnp_finite(tn[e]);
                    if (fin) {
                        for (int e = 0; e < 9; ++e) s_pose[e] = Rn[e];
                        for (int e = 0; e < 3; ++e) s_pose[9 + e] = tn[e];
                        stop = nd < VIS_GN_TOL ? 2 : 0;    // 2: the step is taken, then the round ends
                    }
                }
                s_flag = stop;
            }
            __syncthreads();
            const int stop = s_flag;
            if (stop != 1) {
                for (int e = 0; e < 9; ++e) R[e] = s_pose[e];
                for (int e = 0; e < 3; ++e) tt[e] = s_pose[9 + e];
                ++steps;
            }
            __syncthreads();                               // s_flag, s_pose and s_sum have been read
            if (stop) break;
        }
        inliers = 0;
        for (int k0 = 0; k0 < M; k0 += VIS_BLOCK) {
            const int k = k0 + t;
            bool in = false;
            if (k < M) {
                const double x[3] = {sX[k], sY[k], sZ[k]};
                in = vis_inlier<LEVELS>(R, tt, cam, x, sU[k], sV[k], A.thr2, sW, k);
                s_inl[k] = in ? 1 : 0;
            }
            inliers += vis_block_count(in, s_w, t);
        }
    }
    __syncthreads();
    for (int k = t; k < M; k += VIS_BLOCK) A.flags[r0 + s_src[k]] = s_inl[k];
    if (t == 0) {
        pose_store(R, tt, Tp);
        info[0] = inliers >= A.min_inliers ? 0 : 1; info[1] = (int)given; info[2] = M; info[3] = (int)(given - M);
        info[4] = inliers; info[5] = best_h; info[6] = best_cnt; info[7] = steps;
    }
}

__global__ void vis_identity_rows_kernel(const int64_t *__restrict__ off, int32_t *__restrict__ rows) {
    const int p = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n = off[p + 1] - off[p];
    if (k >= n) return;
    rows[2 * (off[p] + k)] = (int32_t)k;
    rows[2 * (off[p] + k) + 1] = (int32_t)k;
}

// ---- host side -----------------------------------------------------------------------------------------------------
static StreamScratch g_vis_scratch;

// the host copy of the offsets is required here; then the shared rule and this family's limits
static int vis_shape(const int64_t *h_off, int n_pairs, const char *what, RaggedShape *s) {
    ARG_CHECK(h_off != nullptr, what);
    int rc = offsets_check(h_off, n_pairs, s);
    if (rc) return rc;
    ARG_CHECK(s->total <= 0x7fffffffll / 16, "too many rows in one call");
    ARG_CHECK(s->largest <= (int64_t)65535 * VIS_MATCH_BLOCK, "too many rows in one pair");
    return CSLAM_OK;
}

static int vis_match_checks(int n_pairs, int desc_bytes, double nndr) {
    BATCH_COUNT_CHECK(n_pairs);
    ARG_CHECK(desc_bytes == VIS_DESC_BYTES, "descriptors must be 32 bytes wide (ORB / BRIEF-32)");
    ARG_CHECK(nndr >= 0.0 && nndr <= 1.0, "nndr must be in [0, 1]");
    return CSLAM_OK;
}

static int vis_pnp_checks(int n_pairs, int iterations, double reproj_error, int min_inliers, int refine_iterations, int refine_rounds) {
    BATCH_COUNT_CHECK(n_pairs);
    ARG_CHECK(iterations >= 1 && iterations <= (1 << 24), "iterations must be in [1, 2^24]");
    ARG_CHECK(reproj_error > 0.0 && reproj_error < INFINITY, "reproj_error must be positive and finite");
    ARG_CHECK(min_inliers >= 1, "min_inliers must be at least 1");
    ARG_CHECK(refine_iterations >= 0 && refine_rounds >= 0, "refine_iterations and refine_rounds must not be negative");
    return CSLAM_OK;
}

static int vis_launch_match(const uint8_t *da, const int64_t *a_off, const uint8_t *db, const int64_t *b_off, int n_pairs,
                            const RaggedShape &a, const RaggedShape &b, double nndr, int32_t *rows, int32_t *count, hipStream_t st) {
    u64 *claim;
    int32_t *nn;
    auto layout = [&](Carver &cv) { claim = cv.take<u64>((size_t)b.total, 8); nn = cv.take<int32_t>(2 * (size_t)a.total, 8); };
    SCRATCH_CARVE(g_vis_scratch, st, (size_t)1 << 20, layout);
    HIP_TRY(hipMemsetAsync(claim, 0xff, (size_t)((char *)nn - (char *)claim), st));     // the whole piece
    if (a.largest > 0)
        hipLaunchKernelGGL(vis_match_kernel, dim3((unsigned)ceil_div64(a.largest, VIS_MATCH_BLOCK), (unsigned)n_pairs), dim3(VIS_MATCH_BLOCK), 0,
                           st, (const uint32_t *)da, a_off, (const uint32_t *)db, b_off, nndr, nn, claim);
    hipLaunchKernelGGL(vis_compact_kernel, dim3((unsigned)n_pairs), dim3(VIS_BLOCK), 0, st, a_off, b_off, nn, claim, rows, count);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

template <bool LEVELS> static int vis_launch_pnp_form(const VisPnpArgs &a, int n_pairs, hipStream_t st) {
    constexpr int lds = LEVELS ? VIS_PNP_LEVELS_LDS : VIS_PNP_LDS;
    static DeviceOnce once;
    int dev;
    if (once.todo(&dev)) {
        HIP_TRY(hipFuncSetAttribute((const void *)vis_pnp_kernel<LEVELS>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        once.done(dev);
    }
    hipLaunchKernelGGL(vis_pnp_kernel<LEVELS>, dim3((unsigned)n_pairs), dim3(VIS_BLOCK), lds, st, a);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

static int vis_launch_pnp(const VisPnpArgs &a, int n_pairs, hipStream_t st) {
    return a.lvl ? vis_launch_pnp_form<true>(a, n_pairs, st) : vis_launch_pnp_form<false>(a, n_pairs, st);
}

// the levels of the "to" rows on the host: each in 0 .. PNP_MAX_LEVEL, refused before any launch
static int vis_levels_check(const int32_t *h_levels_to, const int64_t *h_to_off, int n_pairs) {
    ARG_CHECK(h_levels_to != nullptr && h_to_off != nullptr, "h_levels_to and the host offsets of the \"to\" rows are required");
    for (int64_t i = 0; i < h_to_off[n_pairs]; ++i)
        ARG_CHECK(h_levels_to[i] >= 0 && h_levels_to[i] <= PNP_MAX_LEVEL, "levels must be in [0, 7]");
    return CSLAM_OK;
}

CSLAM_API int cslam_vis_match_dev(const uint8_t *d_desc_from, const int64_t *d_from_off, const uint8_t *d_desc_to,
                                  const int64_t *d_to_off, int n_pairs, int desc_bytes, double nndr, int32_t *d_rows,
                                  int32_t *d_count, const int64_t *h_from_off, const int64_t *h_to_off, void *stream) {
    int rc = vis_match_checks(n_pairs, desc_bytes, nndr);
    if (rc) return rc;
    ARG_CHECK(d_desc_from && d_from_off && d_desc_to && d_to_off && d_rows && d_count, "NULL argument");
    RaggedShape from, to;
    if ((rc = vis_shape(h_from_off, n_pairs, "h_from_off is required", &from))) return rc;
    if ((rc = vis_shape(h_to_off, n_pairs, "h_to_off is required", &to))) return rc;
    PTR_DEVICE(d_desc_from);
    return vis_launch_match(d_desc_from, d_from_off, d_desc_to, d_to_off, n_pairs, from, to, nndr, d_rows, d_count, (hipStream_t)stream);
}

CSLAM_API int cslam_vis_pnp_dev(const double *d_points, const int64_t *d_points_off, const double *d_pixels,
                                const int64_t *d_pixels_off, const int32_t *d_rows, const int64_t *d_row_off,
                                const int32_t *d_count, const double *d_cameras, int n_pairs, int iterations, double reproj_error,
                                int min_inliers, int refine_iterations, int refine_rounds, uint64_t seed, double *d_T,
                                int32_t *d_info, int32_t *d_flags, void *stream) {
    int rc = vis_pnp_checks(n_pairs, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds);
    if (rc) return rc;
    ARG_CHECK(d_points && d_points_off && d_pixels && d_pixels_off && d_rows && d_row_off && d_cameras && d_T && d_info && d_flags,
              "NULL argument");
    PTR_DEVICE(d_points);
    VisPnpArgs a = {d_points, d_points_off, d_pixels, d_pixels_off, d_rows, d_row_off, d_count, d_cameras, iterations, min_inliers,
                    refine_iterations, refine_rounds, reproj_error * reproj_error, (u64)seed, d_T, d_info, d_flags, nullptr, nullptr};
    return vis_launch_pnp(a, n_pairs, (hipStream_t)stream);
}

CSLAM_API int cslam_vis_pnp_levels_dev(const double *d_points, const int64_t *d_points_off, const double *d_pixels,
                                       const int64_t *d_pixels_off, const int32_t *d_levels_to, const int32_t *d_rows,
                                       const int64_t *d_row_off, const int32_t *d_count, const double *d_cameras, int n_pairs,
                                       int iterations, double reproj_error, int min_inliers, int refine_iterations, int refine_rounds,
                                       uint64_t seed, double *d_T, int32_t *d_info, int32_t *d_flags, const int64_t *h_pixels_off,
                                       const int32_t *h_levels_to, void *stream) {
    int rc = vis_pnp_checks(n_pairs, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds);
    if (rc) return rc;
    ARG_CHECK(d_points && d_points_off && d_pixels && d_pixels_off && d_levels_to && d_rows && d_row_off && d_cameras && d_T && d_info &&
              d_flags, "NULL argument");
    RaggedShape to;
    if ((rc = vis_shape(h_pixels_off, n_pairs, "h_pixels_off is required", &to))) return rc;
    if ((rc = vis_levels_check(h_levels_to, h_pixels_off, n_pairs))) return rc;
    PTR_DEVICE(d_points);
    VisPnpArgs a = {d_points, d_points_off, d_pixels, d_pixels_off, d_rows, d_row_off, d_count, d_cameras, iterations, min_inliers,
                    refine_iterations, refine_rounds, reproj_error * reproj_error, (u64)seed, d_T, d_info, d_flags, nullptr, nullptr,
                    d_levels_to};
    return vis_launch_pnp(a, n_pairs, (hipStream_t)stream);
}

// match, then PnP on the matches, chained without a host wait; d_levels_to NULL = the uniform form
static int vis_register(const uint8_t *d_desc_from, const double *d_points_from, const int64_t *d_from_off, const uint8_t *d_desc_to,
                        const double *d_pixels_to, const int64_t *d_to_off, const int32_t *d_levels_to, const double *d_cameras,
                        int n_pairs, int desc_bytes, double nndr, int iterations, double reproj_error, int min_inliers,
                        int refine_iterations, int refine_rounds, uint64_t seed, int32_t *d_rows, int32_t *d_count, double *d_T,
                        int32_t *d_info, int32_t *d_flags, const int64_t *h_from_off, const int64_t *h_to_off, const int32_t *h_levels_to,
                        void *stream) {
    int rc = vis_match_checks(n_pairs, desc_bytes, nndr);
    if (rc) return rc;
    if ((rc = vis_pnp_checks(n_pairs, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds))) return rc;
    ARG_CHECK(d_desc_from && d_points_from && d_from_off && d_desc_to && d_pixels_to && d_to_off && d_cameras && d_rows && d_count &&
              d_T && d_info && d_flags, "NULL argument");
    RaggedShape from, to;
    if ((rc = vis_shape(h_from_off, n_pairs, "h_from_off is required", &from))) return rc;
    if ((rc = vis_shape(h_to_off, n_pairs, "h_to_off is required", &to))) return rc;
    if (d_levels_to && (rc = vis_levels_check(h_levels_to, h_to_off, n_pairs))) return rc;
    PTR_DEVICE(d_desc_from);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = vis_launch_match(d_desc_from, d_from_off, d_desc_to, d_to_off, n_pairs, from, to, nndr, d_rows, d_count, st))) return rc;
    VisPnpArgs a = {d_points_from, d_from_off, d_pixels_to, d_to_off, d_rows, d_from_off, d_count, d_cameras, iterations, min_inliers,
                    refine_iterations, refine_rounds, reproj_error * reproj_error, (u64)seed, d_T, d_info, d_flags, nullptr, nullptr,
                    d_levels_to};
    return vis_launch_pnp(a, n_pairs, st);
}

CSLAM_API int cslam_vis_register_dev(const uint8_t *d_desc_from, const double *d_points_from, const int64_t *d_from_off,
                                     const uint8_t *d_desc_to, const double *d_pixels_to, const int64_t *d_to_off,
                                     const double *d_cameras, int n_pairs, int desc_bytes, double nndr, int iterations,
                                     double reproj_error, int min_inliers, int refine_iterations, int refine_rounds, uint64_t seed,
                                     int32_t *d_rows, int32_t *d_count, double *d_T, int32_t *d_info, int32_t *d_flags,
                                     const int64_t *h_from_off, const int64_t *h_to_off, void *stream) {
    return vis_register(d_desc_from, d_points_from, d_from_off, d_desc_to, d_pixels_to, d_to_off, nullptr, d_cameras, n_pairs, desc_bytes,
                        nndr, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed, d_rows, d_count, d_T, d_info,
                        d_flags, h_from_off, h_to_off, nullptr, stream);
}

CSLAM_API int cslam_vis_register_levels_dev(const uint8_t *d_desc_from, const double *d_points_from, const int64_t *d_from_off,
                                            const uint8_t *d_desc_to, const double *d_pixels_to, const int64_t *d_to_off,
                                            const int32_t *d_levels_to, const double *d_cameras, int n_pairs, int desc_bytes, double nndr,
                                            int iterations, double reproj_error, int min_inliers, int refine_iterations, int refine_rounds,
                                            uint64_t seed, int32_t *d_rows, int32_t *d_count, double *d_T, int32_t *d_info,
                                            int32_t *d_flags, const int64_t *h_from_off, const int64_t *h_to_off,
                                            const int32_t *h_levels_to, void *stream) {
    ARG_CHECK(d_levels_to != nullptr && h_levels_to != nullptr, "d_levels_to and h_levels_to are required");
    return vis_register(d_desc_from, d_points_from, d_from_off, d_desc_to, d_pixels_to, d_to_off, d_levels_to, d_cameras, n_pairs,
                        desc_bytes, nndr, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed, d_rows, d_count,
                        d_T, d_info, d_flags, h_from_off, h_to_off, h_levels_to, stream);
}

CSLAM_API int cslam_vis_hypotheses_dev(const double *d_points, const double *d_pixels, const int64_t *d_off, const double *d_cameras,
                                       int n_pairs, int iterations, double reproj_error, uint64_t seed, double *d_hyp_pose,
                                       int32_t *d_hyp_info, double *d_T, int32_t *d_info, int32_t *d_flags, const int64_t *h_off,
                                       void *stream) {
    int rc = vis_pnp_checks(n_pairs, iterations, reproj_error, 1, 0, 0);
    if (rc) return rc;
    ARG_CHECK(d_points && d_pixels && d_off && d_cameras && d_hyp_pose && d_hyp_info && d_T && d_info && d_flags, "NULL argument");
    RaggedShape sh;
    if ((rc = vis_shape(h_off, n_pairs, "h_off is required", &sh))) return rc;
    PTR_DEVICE(d_points);
    hipStream_t st = (hipStream_t)stream;
    SCRATCH_HERE(base, g_vis_scratch, st, (size_t)sh.total * 8 + 256, (size_t)1 << 20);
    int32_t *rows = (int32_t *)base;
    if (sh.largest > 0)
        hipLaunchKernelGGL(vis_identity_rows_kernel, dim3((unsigned)ceil_div64(sh.largest, 256), (unsigned)n_pairs), dim3(256), 0, st, d_off, rows);
    // min_inliers 1: a pair of four correspondences or more is attempted, as the staged tests need
    VisPnpArgs a = {d_points, d_off, d_pixels, d_off, rows, d_off, nullptr, d_cameras, iterations, 1, 0, 0, reproj_error * reproj_error,
                    (u64)seed, d_T, d_info, d_flags, d_hyp_pose, d_hyp_info};
    return vis_launch_pnp(a, n_pairs, st);
}
