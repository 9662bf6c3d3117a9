// vis_ba.hip -- two-view bundle adjustment after the PnP fit of a visual loop closure (gfx950).
//
// Serves the `registration_.computeTransformation(from, to, ...)` calls of src/front_end/rgbd_handler.cpp:443-445 and :519-520:
// rtabmap's visual registration does not stop at PnP at its defaults but follows it with a local bundle adjustment over the two
// views.  rtabmap and g2o are third party and were not available to compare against: parity with them is unpinned.  The rule
// is the one stated in include/cslam_hip.h and ba.h; tests/vis_ba_reference.py restates it in float64 numpy.
//
//   vis_ba_kernel : one workgroup of 256 threads per pair.  The adjusted set (the correspondences PnP flagged, in row order, at
//                   most 2048) lives in LDS as float64 SoA: (u, v, 1 / Z) of both views = 6 x 2048 x 8 = 96 KiB, plus the source
//                   row (8 KiB), both levels as bytes (4 KiB) and the membership byte (2 KiB): 110 KiB of the CU's 160, so the
//                   workgroup is alone on its CU.  Correspondence k belongs to thread k mod 256 in every pass; its point Y_k
//                   lives in a per-pair piece of the stream's scratch (SoA, 3 x rows x 8 bytes, and as much again for the copy
//                   a discarded round goes back to), read and written by its owner only.  A step is: every thread eliminates
//                   its points and adds their 27 reduced terms (ba_accumulate), a fixed shuffle tree per wave, the waves added
//                   in wave order by thread 0, which solves (pnp_gn_solve) and broadcasts delta; every thread then rebuilds
//                   its points' blocks at the same linearisation point and back-substitutes (ba_back_substitute): nothing
//                   per point is kept between the two passes but Y_k itself, at the price of computing the blocks twice.
// No float atomics; every floating sum has a fixed order: a pair's bytes are the same alone, in any batch, in any order.
#include "common.h"
#include "ba.h"

#define BA_BLOCK 256
#define BA_WAVES (BA_BLOCK / 64)
#define BA_LDS (6 * BA_MAX_CORR * 8 + BA_MAX_CORR * 4 + 3 * BA_MAX_CORR)

typedef unsigned long long u64;

struct VisBaArgs {
    const double *kp_a, *pts_a; const int64_t *a_off;      // "from": keypoints [., 2], points [., 3]
    const double *kp_b, *pts_b; const int64_t *b_off;      // "to"
    const int32_t *lvl_a, *lvl_b;                          // NULL: every level 0
    const double *cams_a, *cams_b, *baselines;             // [n_pairs, 4], [n_pairs, 4], [n_pairs, 2]
    const int32_t *rows; const int64_t *row_off; const int32_t *count;
    const double *T0; const int32_t *info0; const int32_t *flags0;          // what PnP wrote
    double thr2;
    int min_inliers, iterations, rounds;
    double *T; int32_t *info; int32_t *flags; double *points; double *cost;
    double *Y, *Ysave;                                     // scratch, [3 * total rows] each
};

__device__ __forceinline__ int ba_block_count(int x, int *s_w, int t) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
    __syncthreads();
    if ((t & 63) == 0) s_w[t >> 6] = x;
    __syncthreads();
    int n = 0;
    for (int w = 0; w < BA_WAVES; ++w) n += s_w[w];
    return n;
}

// the sum of x over the workgroup in the fixed order (shuffle tree per wave, waves in wave order); every thread gets it
__device__ __forceinline__ double ba_block_sum(double x, double *s_c, int t) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
    __syncthreads();
    if ((t & 63) == 0) s_c[t >> 6] = x;
    __syncthreads();
    double a = s_c[0];
    for (int w = 1; w < BA_WAVES; ++w) a += s_c[w];
    return a;
}

__global__ __launch_bounds__(BA_BLOCK) void vis_ba_kernel(VisBaArgs A) {
    extern __shared__ __attribute__((aligned(16))) char ba_smem[];
    double *sUa = (double *)ba_smem, *sVa = sUa + BA_MAX_CORR, *sIa = sVa + BA_MAX_CORR, *sUb = sIa + BA_MAX_CORR, *sVb = sUb + BA_MAX_CORR,
           *sIb = sVb + BA_MAX_CORR;
    int32_t *s_src = (int32_t *)(sIb + BA_MAX_CORR);
    uint8_t *s_la = (uint8_t *)(s_src + BA_MAX_CORR), *s_lb = s_la + BA_MAX_CORR, *s_in = s_lb + BA_MAX_CORR;
    __shared__ int s_w[BA_WAVES];
    __shared__ double s_c[BA_WAVES];
    __shared__ double s_sum[BA_WAVES][PNP_NSUM];
    __shared__ double s_pose[12], s_delta[6], s_sig[PNP_MAX_LEVEL + 1];
    __shared__ int s_flag;

    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t r0 = A.row_off[p], cap = A.row_off[p + 1] - r0;
    int64_t given = A.count ? (int64_t)A.count[p] : cap;
    given = given < 0 ? 0 : (given > cap ? cap : given);
    const int64_t a0 = A.a_off[p], na = A.a_off[p + 1] - a0, b0 = A.b_off[p], nb = A.b_off[p + 1] - b0;
    const int pnp_status = A.info0[8 * (int64_t)p];
    double *Tp = A.T + 16 * (int64_t)p;
    int32_t *info = A.info + 8 * (int64_t)p;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (t <= PNP_MAX_LEVEL) s_sig[t] = pnp_level_sigma2(t);

    // every row of the pair: no refined point yet; the flags PnP wrote
    for (int64_t k = t; k < cap; k += BA_BLOCK) {
        for (int a = 0; a < 3; ++a) A.points[3 * (r0 + k) + a] = nan;
        A.flags[r0 + k] = A.flags0[r0 + k];
    }

    // the adjusted set, in row order, into LDS
    const bool adjust = pnp_status == 0 && A.rounds > 0 && A.iterations > 0;
    int M = 0;
    for (int64_t c0 = 0; c0 < given && adjust; c0 += BA_BLOCK) {
        const int64_t k = c0 + t;
        bool ok = false;
        double ua = 0.0, va = 0.0, ia = 0.0, ub = 0.0, vb = 0.0, ib = 0.0;
        int la = 0, lb = 0;
        if (k < given && A.flags0[r0 + k] != 0) {
            const int64_t i = A.rows[2 * (r0 + k)], j = A.rows[2 * (r0 + k) + 1];
            if (i >= 0 && i < na && j >= 0 && j < nb) {
                ua = A.kp_a[2 * (a0 + i)]; va = A.kp_a[2 * (a0 + i) + 1];
                ub = A.kp_b[2 * (b0 + j)]; vb = A.kp_b[2 * (b0 + j) + 1];
                const double xa = A.pts_a[3 * (a0 + i)], ya = A.pts_a[3 * (a0 + i) + 1];
                ia = ba_inv_depth(A.pts_a[3 * (a0 + i) + 2]);
                ib = ba_inv_depth(A.pts_b[3 * (b0 + j) + 2]);
                if (A.lvl_a) la = A.lvl_a[a0 + i];
                if (A.lvl_b) lb = A.lvl_b[b0 + j];
                // the host refused levels outside 0 .. PNP_MAX_LEVEL; the clamp only bounds the index should a caller break that
                la = la < 0 ? 0 : (la > PNP_MAX_LEVEL ? PNP_MAX_LEVEL : la);
                lb = lb < 0 ? 0 : (lb > PNP_MAX_LEVEL ? PNP_MAX_LEVEL : lb);
                ok = pnp_finite(ua) && pnp_finite(va) && pnp_finite(ub) && pnp_finite(vb) && pnp_finite(xa) && pnp_finite(ya) && ia != 0.0;
            }
            if (!ok) A.flags[r0 + k] = 0;                  // flagged by PnP but not adjustable: it leaves the set (row k is this thread's above too)
        }
        const u64 m = __ballot(ok);
        __syncthreads();
        if (lane == 0) s_w[wave] = (int)__popcll(m);
        __syncthreads();
        int at = M + (int)__popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) at += s_w[w];
        if (ok && at < BA_MAX_CORR) {
            sUa[at] = ua; sVa[at] = va; sIa[at] = ia; sUb[at] = ub; sVb[at] = vb; sIb[at] = ib;
            s_src[at] = (int)k; s_la[at] = (uint8_t)la; s_lb[at] = (uint8_t)lb; s_in[at] = 1;
        }
        for (int w = 0; w < BA_WAVES; ++w) M += s_w[w];
    }
    __syncthreads();

    if (!adjust || M > BA_MAX_CORR) {                      // not adjusted: what PnP wrote
        if (t < 16) Tp[t] = A.T0[16 * (int64_t)p + t];
        // a set above the cap cannot follow a PnP status 0 of the chained call; a staged caller gets status 3 and PnP's pose and flags
        if (adjust)
            for (int64_t k = t; k < cap; k += BA_BLOCK) A.flags[r0 + k] = A.flags0[r0 + k];
        if (t == 0) {
            const int n0 = A.info0[8 * (int64_t)p + 4];
            info[0] = adjust ? 3 : pnp_status; info[1] = adjust ? M : n0; info[2] = adjust ? M : n0; info[3] = 0; info[4] = 0; info[5] = 0;
            info[6] = pnp_status; info[7] = 0;
            A.cost[2 * (int64_t)p] = nan; A.cost[2 * (int64_t)p + 1] = nan;
        }
        return;
    }

    BaView ca, cb;
    {
        const double *c = A.cams_a + 4 * (int64_t)p, *d = A.cams_b + 4 * (int64_t)p;
        ca.fx = c[0]; ca.fy = c[1]; ca.cx = c[2]; ca.cy = c[3]; ca.w = c[0] * A.baselines[2 * (int64_t)p];
        cb.fx = d[0]; cb.fy = d[1]; cb.cx = d[2]; cb.cy = d[3]; cb.w = d[0] * A.baselines[2 * (int64_t)p + 1];
    }
    double R[9], tt[3];
    pose_load(A.T0 + 16 * (int64_t)p, R, tt);
    double *Yx = A.Y + 3 * r0, *Yy = Yx + cap, *Yz = Yy + cap;
    double *Sx = A.Ysave + 3 * r0, *Sy = Sx + cap, *Sz = Sy + cap;
    // the points start at the "from" keyframe's; from here on Y[k] is its owner's alone
    for (int k = t; k < M; k += BA_BLOCK) {
        const int64_t i = A.rows[2 * (r0 + s_src[k])];
        Yx[k] = A.pts_a[3 * (a0 + i)]; Yy[k] = A.pts_a[3 * (a0 + i) + 1]; Yz[k] = A.pts_a[3 * (a0 + i) + 2];
    }
#define BA_OBS(k) BaObs o = {sUa[k], sVa[k], sIa[k], sUb[k], sVb[k], sIb[k], 1.0 / s_sig[s_la[k]], 1.0 / s_sig[s_lb[k]]}

    int kept = M, steps = 0, discarded = 0, held = 0;
    double cost_first = 0.0, cost_last = 0.0;
    for (int round = 0; round < A.rounds; ++round) {
        double R0[9], t0[3];
        for (int e = 0; e < 9; ++e) R0[e] = R[e];
        for (int e = 0; e < 3; ++e) t0[e] = tt[e];
        double c = 0.0;
        for (int k = t; k < M; k += BA_BLOCK)
            if (s_in[k]) {
                BA_OBS(k);
                const double Y[3] = {Yx[k], Yy[k], Yz[k]};
                Sx[k] = Y[0]; Sy[k] = Y[1]; Sz[k] = Y[2];
                c += ba_cost(R, tt, ca, cb, o, Y);
            }
        const double cost0 = ba_block_sum(c, s_c, t);
        if (round == 0) cost_first = cost0;
        for (int it = 0; it < A.iterations; ++it) {
            double s[PNP_NSUM];
#pragma unroll
            for (int e = 0; e < PNP_NSUM; ++e) s[e] = 0.0;
            int h = 0;
            for (int k = t; k < M; k += BA_BLOCK)
                if (s_in[k]) {
                    BA_OBS(k);
                    const double Y[3] = {Yx[k], Yy[k], Yz[k]};
                    h += ba_accumulate(R, tt, ca, cb, o, Y, s) == BA_HELD ? 1 : 0;
                }
#pragma unroll
            for (int e = 0; e < PNP_NSUM; ++e) {
                double x = s[e];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
                if (lane == 0) s_sum[wave][e] = x;
            }
            held += ba_block_count(h, s_w, t);             // its barriers also publish s_sum
            if (t == 0) {
                double tot[PNP_NSUM], delta[6], Rn[9], tn[3];
                for (int e = 0; e < PNP_NSUM; ++e) {
                    double a = s_sum[0][e];
                    for (int w = 1; w < BA_WAVES; ++w) a += s_sum[w][e];
                    tot[e] = a;
                }
                const int stop = ba_pose_step(tot, R, tt, delta, Rn, tn);
                if (stop != 1) {
                    for (int e = 0; e < 9; ++e) s_pose[e] = Rn[e];
                    for (int e = 0; e < 3; ++e) s_pose[9 + e] = tn[e];
                    for (int e = 0; e < 6; ++e) s_delta[e] = delta[e];
                }
                s_flag = stop;
            }
            __syncthreads();
            const int stop = s_flag;
            if (stop != 1) {
                double delta[6];
                for (int e = 0; e < 6; ++e) delta[e] = s_delta[e];
                for (int k = t; k < M; k += BA_BLOCK)
                    if (s_in[k]) {
                        BA_OBS(k);
                        double Y[3] = {Yx[k], Yy[k], Yz[k]};
                        if (ba_back_substitute(R, tt, ca, cb, o, delta, Y) == BA_FREE) { Yx[k] = Y[0]; Yy[k] = Y[1]; Yz[k] = Y[2]; }
                    }
                for (int e = 0; e < 9; ++e) R[e] = s_pose[e];
                for (int e = 0; e < 3; ++e) tt[e] = s_pose[9 + e];
                ++steps;
            }
            __syncthreads();                               // s_flag, s_pose, s_delta and s_sum have been read
            if (stop) break;
        }
        // the guard: the cost over the round's starting set must be finite and must not have risen (ba_round_rejected)
        c = 0.0;
        for (int k = t; k < M; k += BA_BLOCK)
            if (s_in[k]) {
                BA_OBS(k);
                const double Y[3] = {Yx[k], Yy[k], Yz[k]};
                c += ba_cost(R, tt, ca, cb, o, Y);
            }
        double cost1 = ba_block_sum(c, s_c, t);
        if (ba_round_rejected(cost0, cost1)) {
            for (int e = 0; e < 9; ++e) R[e] = R0[e];
            for (int e = 0; e < 3; ++e) tt[e] = t0[e];
            for (int k = t; k < M; k += BA_BLOCK)
                if (s_in[k]) { Yx[k] = Sx[k]; Yy[k] = Sy[k]; Yz[k] = Sz[k]; }
            ++discarded;
            cost1 = cost0;
        }
        cost_last = cost1;
        // the recount: the set only shrinks
        int n = 0;
        for (int k = t; k < M; k += BA_BLOCK)
            if (s_in[k]) {
                BA_OBS(k);
                const double Y[3] = {Yx[k], Yy[k], Yz[k]};
                const bool in = ba_keep(R, tt, ca, cb, o, Y, A.thr2, s_sig[s_la[k]], s_sig[s_lb[k]]);
                s_in[k] = in ? 1 : 0;
                n += in ? 1 : 0;
            }
        kept = ba_block_count(n, s_w, t);
    }
#undef BA_OBS
    __syncthreads();
    for (int k = t; k < M; k += BA_BLOCK) {
        const int64_t row = r0 + s_src[k];
        A.flags[row] = s_in[k];
        if (s_in[k]) { A.points[3 * row] = Yx[k]; A.points[3 * row + 1] = Yy[k]; A.points[3 * row + 2] = Yz[k]; }
    }
    if (t == 0) {
        pose_store(R, tt, Tp);
        info[0] = kept >= A.min_inliers ? 0 : 1; info[1] = M; info[2] = kept; info[3] = steps; info[4] = discarded; info[5] = held;
        info[6] = pnp_status; info[7] = 0;
        A.cost[2 * (int64_t)p] = cost_first; A.cost[2 * (int64_t)p + 1] = cost_last;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
static StreamScratch g_ba_scratch;

static int ba_shape(const int64_t *h_off, int n_pairs, const char *what, RaggedShape *s) {
    ARG_CHECK(h_off != nullptr, what);
    int rc = offsets_check(h_off, n_pairs, s);
    if (rc) return rc;
    ARG_CHECK(s->total <= 0x7fffffffll / 16, "too many rows in one call");
    return CSLAM_OK;
}

static int ba_levels_check(const int32_t *h_levels, const int64_t *h_off, int n_pairs, const char *what) {
    ARG_CHECK(h_levels != nullptr, what);
    for (int64_t i = 0; i < h_off[n_pairs]; ++i) ARG_CHECK(h_levels[i] >= 0 && h_levels[i] <= PNP_MAX_LEVEL, "levels must be in [0, 7]");
    return CSLAM_OK;
}

// everything that can be refused on the host, before any launch
static int ba_checks(int n_pairs, double reproj_error, int min_inliers, int ba_iterations, int ba_rounds, const int32_t *d_levels_from,
                     const int32_t *d_levels_to, const int64_t *h_from_off, const int64_t *h_to_off, const int64_t *h_row_off,
                     const int32_t *h_levels_from, const int32_t *h_levels_to, const double *h_baselines, RaggedShape *rows) {
    BATCH_COUNT_CHECK(n_pairs);
    ARG_CHECK(reproj_error > 0.0 && reproj_error < INFINITY, "reproj_error must be positive and finite");
    ARG_CHECK(min_inliers >= 1, "min_inliers must be at least 1");
    ARG_CHECK(ba_iterations >= 0 && ba_rounds >= 0, "ba_iterations and ba_rounds must not be negative");
    RaggedShape from, to;
    int rc;
    if ((rc = ba_shape(h_from_off, n_pairs, "h_from_off is required", &from))) return rc;
    if ((rc = ba_shape(h_to_off, n_pairs, "h_to_off is required", &to))) return rc;
    if ((rc = ba_shape(h_row_off, n_pairs, "h_row_off is required", rows))) return rc;
    if (d_levels_from && (rc = ba_levels_check(h_levels_from, h_from_off, n_pairs, "h_levels_from is required with d_levels_from"))) return rc;
    if (d_levels_to && (rc = ba_levels_check(h_levels_to, h_to_off, n_pairs, "h_levels_to is required with d_levels_to"))) return rc;
    ARG_CHECK(h_baselines != nullptr, "h_baselines is required");
    for (int64_t i = 0; i < 2 * (int64_t)n_pairs; ++i)
        ARG_CHECK(h_baselines[i] > 0.0 && h_baselines[i] < INFINITY, "baselines must be positive and finite");
    return CSLAM_OK;
}

static int ba_launch(VisBaArgs a, int n_pairs, const RaggedShape &rows, hipStream_t st) {
    auto layout = [&](Carver &cv) { a.Y = cv.take<double>(3 * (size_t)rows.total, 8); a.Ysave = cv.take<double>(3 * (size_t)rows.total, 8); };
    SCRATCH_CARVE(g_ba_scratch, st, (size_t)1 << 20, layout);
    return launch_lds<vis_ba_kernel>(dim3((unsigned)n_pairs), dim3(BA_BLOCK), BA_LDS, st, a);
}

CSLAM_API int cslam_vis_ba_dev(const double *d_kp_from, const double *d_points_from, const int64_t *d_from_off, const double *d_kp_to,
                               const double *d_points_to, const int64_t *d_to_off, const int32_t *d_levels_from,
                               const int32_t *d_levels_to, const double *d_cameras_from, const double *d_cameras_to,
                               const double *d_baselines, const int32_t *d_rows, const int64_t *d_row_off, const int32_t *d_count,
                               const double *d_T0, const int32_t *d_info0, const int32_t *d_flags0, int n_pairs, double reproj_error,
                               int min_inliers, int ba_iterations, int ba_rounds, double *d_T, int32_t *d_info, int32_t *d_flags,
                               double *d_points, double *d_cost, const int64_t *h_from_off, const int64_t *h_to_off,
                               const int64_t *h_row_off, const int32_t *h_levels_from, const int32_t *h_levels_to,
                               const double *h_baselines, void *stream) {
    RaggedShape rows;
    int rc = ba_checks(n_pairs, reproj_error, min_inliers, ba_iterations, ba_rounds, d_levels_from, d_levels_to, h_from_off, h_to_off,
                       h_row_off, h_levels_from, h_levels_to, h_baselines, &rows);
    if (rc) return rc;
    ARG_CHECK(d_kp_from && d_points_from && d_from_off && d_kp_to && d_points_to && d_to_off && d_cameras_from && d_cameras_to &&
              d_baselines && d_rows && d_row_off && d_T0 && d_info0 && d_flags0 && d_T && d_info && d_flags && d_points && d_cost,
              "NULL argument");
    ARG_CHECK((const double *)d_T != d_T0 && (const int32_t *)d_info != d_info0 && (const int32_t *)d_flags != d_flags0,
              "the outputs must not be the arrays PnP wrote");
    PTR_DEVICE(d_kp_from);
    VisBaArgs a = {d_kp_from, d_points_from, d_from_off, d_kp_to, d_points_to, d_to_off, d_levels_from, d_levels_to, d_cameras_from,
                   d_cameras_to, d_baselines, d_rows, d_row_off, d_count, d_T0, d_info0, d_flags0, reproj_error * reproj_error,
                   min_inliers, ba_iterations, ba_rounds, d_T, d_info, d_flags, d_points, d_cost, nullptr, nullptr};
    return ba_launch(a, n_pairs, rows, (hipStream_t)stream);
}

CSLAM_API int cslam_vis_register_ba_dev(const uint8_t *d_desc_from, const double *d_kp_from, const double *d_points_from,
                                        const int64_t *d_from_off, const uint8_t *d_desc_to, const double *d_kp_to,
                                        const double *d_points_to, const int64_t *d_to_off, const int32_t *d_levels_from,
                                        const int32_t *d_levels_to, const double *d_cameras_from, const double *d_cameras_to,
                                        const double *d_baselines, int n_pairs, int desc_bytes, double nndr, int iterations,
                                        double reproj_error, int min_inliers, int refine_iterations, int refine_rounds, uint64_t seed,
                                        int ba_iterations, int ba_rounds, int32_t *d_rows, int32_t *d_count, double *d_T0,
                                        int32_t *d_info0, int32_t *d_flags0, double *d_T, int32_t *d_info, int32_t *d_flags,
                                        double *d_points, double *d_cost, const int64_t *h_from_off, const int64_t *h_to_off,
                                        const int32_t *h_levels_from, const int32_t *h_levels_to, const double *h_baselines,
                                        void *stream) {
    RaggedShape rows;
    int rc = ba_checks(n_pairs, reproj_error, min_inliers, ba_iterations, ba_rounds, d_levels_from, d_levels_to, h_from_off, h_to_off,
                       h_from_off, h_levels_from, h_levels_to, h_baselines, &rows);
    if (rc) return rc;
    ARG_CHECK(d_kp_from && d_points_to && d_cameras_from && d_baselines && d_T0 && d_info0 && d_flags0 && d_T && d_info && d_flags &&
              d_points && d_cost, "NULL argument");
    ARG_CHECK(d_T != d_T0 && d_info != d_info0 && d_flags != d_flags0, "the adjusted outputs must not be the arrays PnP writes");
    // match and PnP as the entry points without the adjustment run them (their own checks included), then the adjustment on
    // the same stream: no host wait anywhere
    if (d_levels_to)
        rc = cslam_vis_register_levels_dev(d_desc_from, d_points_from, d_from_off, d_desc_to, d_kp_to, d_to_off, d_levels_to, d_cameras_to,
                                           n_pairs, desc_bytes, nndr, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds,
                                           seed, d_rows, d_count, d_T0, d_info0, d_flags0, h_from_off, h_to_off, h_levels_to, stream);
    else
        rc = cslam_vis_register_dev(d_desc_from, d_points_from, d_from_off, d_desc_to, d_kp_to, d_to_off, d_cameras_to, n_pairs, desc_bytes,
                                    nndr, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed, d_rows, d_count,
                                    d_T0, d_info0, d_flags0, h_from_off, h_to_off, stream);
    if (rc) return rc;
    PTR_DEVICE(d_kp_from);
    VisBaArgs a = {d_kp_from, d_points_from, d_from_off, d_kp_to, d_points_to, d_to_off, d_levels_from, d_levels_to, d_cameras_from,
                   d_cameras_to, d_baselines, d_rows, d_from_off, d_count, d_T0, d_info0, d_flags0, reproj_error * reproj_error,
                   min_inliers, ba_iterations, ba_rounds, d_T, d_info, d_flags, d_points, d_cost, nullptr, nullptr};
    return ba_launch(a, n_pairs, rows, (hipStream_t)stream);
}
