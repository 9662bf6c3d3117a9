// icp.hip -- batched ICP for lidar loop closures (gfx950): point-to-point, and point-to-plane as a compile-time form.
//
// Replaces the refinement step of cslam/lidar_pr/icp_utils.py:126-134 (open3d `registration_icp` with
// TransformationEstimationPointToPoint and ICPConvergenceCriteria(max_iteration=100)) for a batch of
// (source, target) cloud pairs.  All arithmetic is float64; the nearest neighbour is brute force, as the
// ring-key search of scancontext.hip is, in place of open3d's per-target KD-tree.
//
// One ROUND evaluates every pair at its current transform and, unless the pair has finished, updates it:
//   icp_nn_kernel    : one thread per source point, p = T . src_i from the ORIGINAL cloud; the target goes through
//                      LDS in chunks of ICP_CHUNK points that every lane reads at the same address (broadcast);
//                      grid = (source blocks, target chunk lanes, pairs) so that one pair fills the device.
//                      Output: a partial (d^2, index) per source point and chunk lane.
//   icp_merge_kernel : minimum over the chunk lanes, ties -> lower target index (argmin); a correspondence is kept
//                      iff d^2 <= r^2; n, sum p, sum q, sum q p^T, sum d^2 per block by a fixed shuffle tree, p and q
//                      taken relative to the pair's origin (horn.h icp_sum_origin: its first target point rounded to
//                      a 1024 m grid, zero for a cloud around the frame origin).
//   icp_solve_kernel : one wave per pair: block partials added in block order, fitness = n / |src|,
//                      inlier_rmse = sqrt(sum d^2 / n), open3d's stopping rule, else the rigid update without scale
//                      (Horn's quaternion form of the Umeyama solution: largest eigenvector of a symmetric 4 x 4 by
//                      cyclic Jacobi -- a proper rotation by construction, which is what the det = -1 fix of the SVD
//                      form restores) of the shifted sets, the translation moved back to the frame, and T <- U . T.
// Point-to-plane (cslam_icp_register_plane_dev; open3d's TransformationEstimationPointToPlane) differs in the update only:
// icp_merge_kernel<true> sums the 29 terms of plane.h (n, d^2, J J^T, J r with J = [(p - o) x n, n], n the target's normal at
// q) through the same tree, icp_solve_kernel<true> solves the 6 x 6 (lane 0; identity for a singular system) and composes
// as above.  The <false> instantiations are the point-to-point kernels, instruction for instruction.
// Coordinate range: the uncentred sums lose (distance of the centroid from the sums' origin / spread)^2 of the precision;
// with the origin at most 512 m per axis from the first target point that leaves the moved points within a few ulp of the
// largest coordinate of the centred fit, wherever the clouds lie (map-frame, UTM or ENU coordinates included; tested up
// to 2^20 m).  What remains is the rounding of T . p itself: one ulp of the coordinates per round.
// No float atomics: every sum has one order that depends on the pair's own sizes only, so a pair's result is the same
// bits alone or in any batch.  A per-pair `done` flag in device memory turns the kernels of later rounds into
// immediate returns; the host enqueues max_iteration + 1 rounds per stage without waiting.
#include "common.h"
#include "horn.h"
#include "plane.h"

#define ICP_BLOCK 256        // source points per workgroup (4 waves)
#define ICP_CHUNK 1024       // target points per LDS chunk: 24 KiB, 6 workgroups per CU
#define ICP_MAX_LANES 64     // chunk lanes (grid.y); a lane walks chunks lane, lane + lanes, ...
#define ICP_NSUM 17          // n, p[3], q[3], q p^T [9], d^2
#define ICP_MAX_STAGES 16

// p = T[0:3, :] . (x, y, z, 1), one fixed fma chain per row (both kernels must produce the same bits)
__device__ __forceinline__ void icp_apply(const double *T, double x, double y, double z, double *p) {
    p[0] = fma(T[0], x, fma(T[1], y, fma(T[2], z, T[3])));
    p[1] = fma(T[4], x, fma(T[5], y, fma(T[6], z, T[7])));
    p[2] = fma(T[8], x, fma(T[9], y, fma(T[10], z, T[11])));
}

__device__ __forceinline__ void icp_load_point(const double *src, const double *T, int p, int64_t row, double *out) {
    const double x = src[3 * row], y = src[3 * row + 1], z = src[3 * row + 2];
    if (T) icp_apply(T + 16 * (int64_t)p, x, y, z, out);
    else { out[0] = x; out[1] = y; out[2] = z; }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_nn_kernel(const double *__restrict__ src, const int64_t *__restrict__ src_off,
                                                          const double *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                          const double *__restrict__ T, const int *__restrict__ done,
                                                          int64_t total_src, double *__restrict__ part_d2,
                                                          int *__restrict__ part_idx) {
    __shared__ double s_q[3 * ICP_CHUNK];
    const int p = blockIdx.z, t = threadIdx.x;
    if (done && done[p]) return;
    const int64_t s0 = src_off[p], ns = src_off[p + 1] - s0;
    const int64_t i0 = (int64_t)blockIdx.x * ICP_BLOCK;
    if (i0 >= ns) return;
    const int64_t d0 = dst_off[p], nd = dst_off[p + 1] - d0;
    const int nchunks = (int)((nd + ICP_CHUNK - 1) / ICP_CHUNK);
    if ((int)blockIdx.y >= nchunks) return;
    const bool live = i0 + t < ns;
    double pt[3] = {0.0, 0.0, 0.0};
    if (live) icp_load_point(src, T, p, s0 + i0 + t, pt);
    double best = INFINITY;
    int bi = -1;
    for (int c = blockIdx.y; c < nchunks; c += gridDim.y) {
        const int64_t q0 = (int64_t)c * ICP_CHUNK;
        const int m = (int)(nd - q0 < ICP_CHUNK ? nd - q0 : ICP_CHUNK);
        __syncthreads();                                   // the previous chunk has been consumed
        const double *g = dst + 3 * (d0 + q0);
        for (int e = t; e < 3 * m; e += ICP_BLOCK) s_q[e] = g[e];
        __syncthreads();
        const int base = (int)q0;
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const double dx = pt[0] - s_q[3 * j], dy = pt[1] - s_q[3 * j + 1], dz = pt[2] - s_q[3 * j + 2];
            const double d = fma(dz, dz, fma(dy, dy, __dmul_rn(dx, dx)));
            if (d < best) { best = d; bi = base + j; }     // strict: the first (lowest) index of equal distances stays
        }
    }
    if (live) {
        const int64_t o = (int64_t)blockIdx.y * total_src + s0 + i0 + t;
        part_d2[o] = best;
        part_idx[o] = bi;
    }
}

// fixed-order sum over the 64 lanes; lane 0 holds the result
__device__ __forceinline__ double icp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// PLANE: the 29 sums of plane.h (dst_nrm: the targets' normals, rows as dst) in place of the 17 of the rigid fit; a
// compile-time choice, so that the point-to-point kernel is the code it was.
template <bool PLANE>
__global__ __launch_bounds__(ICP_BLOCK) void icp_merge_kernel(const double *__restrict__ src, const int64_t *__restrict__ src_off,
                                                             const double *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                             const double *__restrict__ T, const int *__restrict__ done,
                                                             int64_t total_src, int lanes, const double *__restrict__ part_d2,
                                                             const int *__restrict__ part_idx, double r2,
                                                             int *__restrict__ corr_idx, double *__restrict__ corr_d2,
                                                             double *__restrict__ bsums, int max_blocks,
                                                             const double *__restrict__ dst_nrm) {
    constexpr int NSUM = PLANE ? ICP_PLANE_NSUM : ICP_NSUM;
    __shared__ double s_w[ICP_BLOCK / 64][NSUM];
    const int p = blockIdx.y, t = threadIdx.x;
    if (done && done[p]) return;
    const int64_t s0 = src_off[p], ns = src_off[p + 1] - s0;
    const int64_t i0 = (int64_t)blockIdx.x * ICP_BLOCK;
    if (i0 >= ns) return;
    const int64_t d0 = dst_off[p], nd = dst_off[p + 1] - d0;
    const int64_t nchunks = (nd + ICP_CHUNK - 1) / ICP_CHUNK;
    const int ny = (int)(nchunks < lanes ? nchunks : lanes);
    const bool live = i0 + t < ns;
    const int64_t row = s0 + i0 + t;
    double best = INFINITY;
    int bi = -1;
    if (live) {
        for (int y = 0; y < ny; ++y) {
            const double d = part_d2[(int64_t)y * total_src + row];
            const int i = part_idx[(int64_t)y * total_src + row];
            if (d < best || (d == best && i < bi)) { best = d; bi = i; }
        }
    }
    const bool keep = live && bi >= 0 && best <= r2;
    if (live && corr_idx) {
        corr_idx[row] = keep ? bi : -1;
        corr_d2[row] = best;
    }
    if (!bsums) return;
    double v[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) v[k] = 0.0;
    if (keep) {
        double pt[3], o[3];
        icp_load_point(src, T, p, row, pt);
        icp_sum_origin(dst + 3 * d0, o);
        const double *q = dst + 3 * (d0 + bi);
        if constexpr (PLANE) {
            const double *nq = dst_nrm + 3 * (d0 + bi);
            const double ps[3] = {pt[0] - o[0], pt[1] - o[1], pt[2] - o[2]}, dq[3] = {pt[0] - q[0], pt[1] - q[1], pt[2] - q[2]};
            const double nr[3] = {nq[0], nq[1], nq[2]};
            icp_plane_terms(ps, dq, nr, best, v);
        } else {
            v[0] = 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) { v[1 + a] = pt[a] - o[a]; v[4 + a] = q[a] - o[a]; }
#pragma unroll
            for (int b = 0; b < 3; ++b)
#pragma unroll
                for (int a = 0; a < 3; ++a) v[7 + 3 * b + a] = __dmul_rn(v[4 + b], v[1 + a]);
            v[16] = best;
        }
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        const double w = icp_wave_sum(v[k]);
        if ((t & 63) == 0) s_w[t >> 6][k] = w;
    }
    __syncthreads();
    if (t < NSUM) {
        double a = s_w[0][t];
#pragma unroll
        for (int w = 1; w < ICP_BLOCK / 64; ++w) a += s_w[w][t];
        bsums[((int64_t)p * max_blocks + blockIdx.x) * NSUM + t] = a;
    }
}

// open3d's loop (RegistrationICP): evaluate at init; for i = 1 .. max_iteration: update, re-evaluate, stop when both
// |delta fitness| < relative_fitness and |delta inlier_rmse| < relative_rmse.  Round r is the evaluation after r updates.
// PLANE: the 29 sums and the update of plane.h; everything else -- fitness, inlier_rmse, the stopping rule -- is the same.
template <bool PLANE>
__global__ __launch_bounds__(64) void icp_solve_kernel(const int64_t *__restrict__ src_off, const double *__restrict__ dst,
                                                      const int64_t *__restrict__ dst_off, const double *__restrict__ bsums,
                                                      int max_blocks, int round, int max_iter, double rel_fitness,
                                                      double rel_rmse, double *__restrict__ T, double *__restrict__ stats,
                                                      int *__restrict__ done) {
    constexpr int NSUM = PLANE ? ICP_PLANE_NSUM : ICP_NSUM, SUM_D2 = PLANE ? 1 : 16;
    __shared__ double s[NSUM];
    const int p = blockIdx.x, t = threadIdx.x;
    if (done[p]) return;
    const int64_t ns = src_off[p + 1] - src_off[p];
    const int nb = (int)((ns + ICP_BLOCK - 1) / ICP_BLOCK);
    if (t < NSUM) {
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += bsums[((int64_t)p * max_blocks + b) * NSUM + t];
        s[t] = a;
    }
    __syncthreads();
    if (t != 0) return;
    const double n = s[0];
    const double fitness = n > 0.0 ? n / (double)ns : 0.0;
    const double rmse = n > 0.0 ? sqrt(s[SUM_D2] / n) : 0.0;
    double *st = stats + 4 * (int64_t)p;
    const double prev_f = st[0], prev_r = st[1];
    st[0] = fitness; st[1] = rmse; st[2] = n; st[3] = (double)round;
    if (round >= max_iter || (round >= 1 && fabs(prev_f - fitness) < rel_fitness && fabs(prev_r - rmse) < rel_rmse)) {
        done[p] = 1;
        return;
    }
    if (n <= 0.0) return;                                  // no correspondences: the update is the identity
    double U[12], Tn[12], o[3];
    icp_sum_origin(dst + 3 * dst_off[p], o);
    if constexpr (PLANE) {
        if (!icp_plane_update_from_shifted_sums(s, o, U)) return;      // a singular system: the update is the identity
    } else {
        icp_rigid_from_shifted_sums(s, o, U);
    }
    double *Tp = T + 16 * (int64_t)p;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b)
            Tn[4 * a + b] = U[4 * a] * Tp[b] + U[4 * a + 1] * Tp[4 + b] + U[4 * a + 2] * Tp[8 + b] + (b == 3 ? U[4 * a + 3] : 0.0);
    for (int e = 0; e < 12; ++e) Tp[e] = Tn[e];
}

__global__ void icp_init_kernel(const double *__restrict__ init, int n_pairs, double *__restrict__ T, double *__restrict__ stats) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < 16 * n_pairs) T[e] = init ? init[e] : ((e & 15) % 5 == 0 ? 1.0 : 0.0);
    if (e < 4 * n_pairs) stats[e] = 0.0;
}

// ---- host side ---------------------------------------------------------------------------------
struct IcpShape {
    int64_t total_src;
    int src_blocks, lanes;
};

// offsets come from device memory: both arrays in one wait, then every size is checked before anything is launched
static int icp_read_shape(const int64_t *d_src_off, const int64_t *d_dst_off, int n_pairs, hipStream_t st, IcpShape *sh) {
    std::vector<int64_t> so, dofs;
    int rc;
    if ((rc = read_back_async(so, d_src_off, (size_t)n_pairs + 1, st)) || (rc = read_back_async(dofs, d_dst_off, (size_t)n_pairs + 1, st)))
        return rc;
    HIP_TRY(hipStreamSynchronize(st));
    RaggedShape src, dst;
    if ((rc = offsets_check(so.data(), n_pairs, &src, "offsets must start at a row >= 0")) ||
        (rc = offsets_check(dofs.data(), n_pairs, &dst, "offsets must start at a row >= 0")))
        return rc;
    ARG_CHECK(src.smallest >= 1 && dst.smallest >= 1, "offsets must increase: every source and target cloud needs at least one point");
    ARG_CHECK(dst.largest <= 0x7fffffffll - ICP_CHUNK, "a target cloud has more points than an int32 index addresses");
    ARG_CHECK(src.largest <= (int64_t)ICP_BLOCK * 0x7fffffffll, "a source cloud is too large");
    sh->total_src = src.total;
    sh->src_blocks = (int)ceil_div64(src.largest, ICP_BLOCK);
    const int64_t chunks = ceil_div64(dst.largest, ICP_CHUNK);
    sh->lanes = (int)(chunks < ICP_MAX_LANES ? chunks : ICP_MAX_LANES);
    return CSLAM_OK;
}

struct IcpScratch {
    double *part_d2, *bsums;
    int *part_idx, *done;
};

static StreamScratch g_icp_scratch;

static int icp_scratch(const IcpShape &sh, int n_pairs, int nsum, hipStream_t st, IcpScratch *ws) {
    const size_t n_part = (size_t)sh.lanes * (size_t)sh.total_src;
    auto layout = [&](Carver &cv) {
        ws->part_d2 = cv.take<double>(n_part);
        ws->bsums = cv.take<double>((size_t)n_pairs * sh.src_blocks * nsum);
        ws->part_idx = cv.take<int>(n_part);
        ws->done = cv.take<int>((size_t)n_pairs);
    };
    SCRATCH_CARVE(g_icp_scratch, st, (size_t)1 << 20, layout);
    return CSLAM_OK;
}

static int icp_common_checks(const double *d_src, const int64_t *d_src_off, const double *d_dst, const int64_t *d_dst_off,
                             int n_pairs) {
    ARG_CHECK(d_src && d_src_off && d_dst && d_dst_off, "NULL argument");
    BATCH_COUNT_CHECK(n_pairs);
    return CSLAM_OK;
}

// one evaluation of every unfinished pair at T: nearest neighbours, then the merge (+ sums when bsums is given: the 29 of
// plane.h with the targets' normals, else the 17 of the rigid fit)
static void icp_launch_eval(const double *d_src, const int64_t *d_src_off, const double *d_dst, const int64_t *d_dst_off,
                            int n_pairs, const IcpShape &sh, const IcpScratch &ws, const double *d_T, const int *d_done,
                            double r2, int *d_idx, double *d_dist2, double *bsums, const double *d_nrm, hipStream_t st) {
    hipLaunchKernelGGL(icp_nn_kernel, dim3((unsigned)sh.src_blocks, (unsigned)sh.lanes, (unsigned)n_pairs), dim3(ICP_BLOCK), 0, st,
                       d_src, d_src_off, d_dst, d_dst_off, d_T, d_done, sh.total_src, ws.part_d2, ws.part_idx);
    auto merge = d_nrm ? icp_merge_kernel<true> : icp_merge_kernel<false>;
    hipLaunchKernelGGL(merge, dim3((unsigned)sh.src_blocks, (unsigned)n_pairs), dim3(ICP_BLOCK), 0, st, d_src, d_src_off, d_dst,
                       d_dst_off, d_T, d_done, sh.total_src, sh.lanes, ws.part_d2, ws.part_idx, r2, d_idx, d_dist2, bsums,
                       sh.src_blocks, d_nrm);
}

CSLAM_API int cslam_icp_correspondences_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst,
                                            const int64_t *d_dst_off, int n_pairs, const double *d_T, double max_dist,
                                            int32_t *d_idx, double *d_dist2, void *stream) {
    int rc = icp_common_checks(d_src, d_src_off, d_dst, d_dst_off, n_pairs);
    if (rc) return rc;
    ARG_CHECK(d_idx && d_dist2, "NULL output");
    ARG_CHECK(max_dist > 0.0 && max_dist < INFINITY, "max_dist must be positive and finite");
    PTR_DEVICE(d_src);
    hipStream_t st = (hipStream_t)stream;
    IcpShape sh;
    if ((rc = icp_read_shape(d_src_off, d_dst_off, n_pairs, st, &sh))) return rc;
    IcpScratch ws;
    if ((rc = icp_scratch(sh, n_pairs, ICP_NSUM, st, &ws))) return rc;
    icp_launch_eval(d_src, d_src_off, d_dst, d_dst_off, n_pairs, sh, ws, d_T, nullptr, max_dist * max_dist, d_idx, d_dist2,
                    nullptr, nullptr, st);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

// both estimators: d_nrm = the targets' normals for point-to-plane, NULL for point-to-point
static int icp_register(const double *d_src, const int64_t *d_src_off, const double *d_dst, const int64_t *d_dst_off, int n_pairs,
                        const double *d_init, const double *max_dist, const int *max_iter, int n_stages, double rel_fitness,
                        double rel_rmse, double *d_T_out, double *d_stats_out, const double *d_nrm, hipStream_t st) {
    ARG_CHECK(d_T_out && d_stats_out && max_dist && max_iter, "NULL argument");
    ARG_CHECK(n_stages >= 1 && n_stages <= ICP_MAX_STAGES, "n_stages must be in [1, 16]");
    for (int s = 0; s < n_stages; ++s) {
        ARG_CHECK(max_dist[s] > 0.0 && max_dist[s] < INFINITY, "max_dist must be positive and finite");
        ARG_CHECK(max_iter[s] >= 0 && max_iter[s] <= 100000, "max_iter must be in [0, 100000]");
    }
    ARG_CHECK(rel_fitness == rel_fitness && rel_rmse == rel_rmse, "relative_fitness / relative_rmse is NaN");
    PTR_DEVICE(d_src);
    int rc;
    IcpShape sh;
    if ((rc = icp_read_shape(d_src_off, d_dst_off, n_pairs, st, &sh))) return rc;
    IcpScratch ws;
    if ((rc = icp_scratch(sh, n_pairs, d_nrm ? ICP_PLANE_NSUM : ICP_NSUM, st, &ws))) return rc;
    hipLaunchKernelGGL(icp_init_kernel, dim3((unsigned)ceil_div64(16 * (int64_t)n_pairs, 256)), dim3(256), 0, st, d_init, n_pairs,
                       d_T_out, d_stats_out);
    auto solve = d_nrm ? icp_solve_kernel<true> : icp_solve_kernel<false>;
    for (int s = 0; s < n_stages; ++s) {
        HIP_TRY(hipMemsetAsync(ws.done, 0, (size_t)n_pairs * sizeof(int), st));
        const double r2 = max_dist[s] * max_dist[s];
        for (int round = 0; round <= max_iter[s]; ++round) {
            icp_launch_eval(d_src, d_src_off, d_dst, d_dst_off, n_pairs, sh, ws, d_T_out, ws.done, r2, nullptr, nullptr, ws.bsums,
                            d_nrm, st);
            hipLaunchKernelGGL(solve, dim3((unsigned)n_pairs), dim3(64), 0, st, d_src_off, d_dst, d_dst_off, ws.bsums, sh.src_blocks,
                               round, max_iter[s], rel_fitness, rel_rmse, d_T_out, d_stats_out, ws.done);
        }
    }
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_icp_register_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst,
                                     const int64_t *d_dst_off, int n_pairs, const double *d_init, const double *max_dist,
                                     const int *max_iter, int n_stages, double rel_fitness, double rel_rmse, double *d_T_out,
                                     double *d_stats_out, void *stream) {
    int rc = icp_common_checks(d_src, d_src_off, d_dst, d_dst_off, n_pairs);
    if (rc) return rc;
    return icp_register(d_src, d_src_off, d_dst, d_dst_off, n_pairs, d_init, max_dist, max_iter, n_stages, rel_fitness, rel_rmse,
                        d_T_out, d_stats_out, nullptr, (hipStream_t)stream);
}

CSLAM_API int cslam_icp_register_plane_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst,
                                           const int64_t *d_dst_off, const double *d_dst_normals, int n_pairs,
                                           const double *d_init, const double *max_dist, const int *max_iter, int n_stages,
                                           double rel_fitness, double rel_rmse, double *d_T_out, double *d_stats_out,
                                           void *stream) {
    int rc = icp_common_checks(d_src, d_src_off, d_dst, d_dst_off, n_pairs);
    if (rc) return rc;
    ARG_CHECK(d_dst_normals, "d_dst_normals is NULL");
    return icp_register(d_src, d_src_off, d_dst, d_dst_off, n_pairs, d_init, max_dist, max_iter, n_stages, rel_fitness, rel_rmse,
                        d_T_out, d_stats_out, d_dst_normals, (hipStream_t)stream);
}
