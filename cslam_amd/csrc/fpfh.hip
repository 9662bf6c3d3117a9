// fpfh.hip -- FPFH features and mutual nearest neighbours in feature space for lidar loop closures (gfx950).
//
// Replaces `extract_fpfh` (cslam/lidar_pr/icp_utils.py:26-37: open3d's estimate_normals with KDTreeSearchParamHybrid,
// then compute_fpfh_feature) and `find_knn_cpu` / `find_correspondences` (icp_utils.py:40-65: cKDTree queries in
// feature space and the mutual filter) for a batch of clouds / of feature-array pairs.  The structure is open3d's
// EstimateNormals.cpp and Feature.cpp; what those leave to a KD-tree's visiting order, a hash map or an eigen-solver is
// fixed here (the rules are spelled out in include/cslam_hip.h).  All arithmetic is float64 and nothing is contracted:
// an fma is an fma only where it is written.
//
//   fp_knn_kernel      : one wave per query point, four per workgroup.  The cloud goes through LDS in chunks of KNN_CHUNK
//                        points; a lane takes one point of 64, the in-radius ones are compacted by ballot into the wave's
//                        candidate buffer (KNN_CAND entries of (d^2, j), in index order).  When the next 64 might not
//                        fit, the buffer is cut to its max_nn - 1 best by rank counting on the total order (d^2, j) and
//                        the scan goes on: the best of everything are among the best so far and the rest.  The same
//                        ranks write the result: the query itself first, then ascending (d^2, j).
//   fp_normals_kernel  : one thread per point: mean and covariance of the neighbours relative to the query, both summed in
//                        list order, cyclic Jacobi on the 3 x 3, the eigenvector of the smallest eigenvalue, the sign
//                        towards the viewpoint.  It reads a PREFIX of a list: the first max_nn entries with d^2 <= r^2,
//                        which is the list a search at (r, max_nn) returns, because lists are in ascending d^2.
//   fp_spfh_kernel     : one wave per point, a lane per neighbour: open3d's ComputePairFeatures, three bins, integer LDS
//                        atomics (a count does not depend on the order it is taken in), scaled once by 100 / (k - 1).
//   fp_fpfh_kernel     : one wave per point, a lane per bin: the neighbours' SPFH rows weighted by 1 / d^2, one after
//                        another in list order; the group sums in ascending bin order.
//   fp_match_kernel    : one thread per query row, the query block transposed in LDS, the target rows through LDS in
//                        chunks of FM_CHUNK that all lanes read at one address; FM_GROUP targets at a time share a query
//                        read.  Both directions and the chunk lanes are one launch (grid.z), as in icp_nn_kernel;
//                        fp_match_merge_kernel takes the minimum over the lanes (ties -> the lower index, so the result
//                        does not depend on the number of lanes).
//   fp_mutual_kernel   : one workgroup per pair: nn10[nn01[i]] == i, the kept rows compacted by ballot in ascending i.
// No float atomics and no sum whose order depends on scheduling: a cloud's (a pair's) output is the same bits alone or
// in any batch.
#include "common.h"

#pragma clang fp contract(off)

#define KNN_BLOCK 256        // four waves = four query points per workgroup
#define KNN_CHUNK 1024       // cloud points per LDS chunk: 24 KiB
#define KNN_CAND 512         // candidate buffer per wave: (d^2, j), 6 KiB
#define KNN_MAX_NN 256       // widest list; KNN_MAX_NN - 1 + 64 <= KNN_CAND: a cut buffer takes the next 64 points
#define FPFH_BINS 33
#define FPFH_BLOCK 256       // threads per workgroup of the normals, SPFH and FPFH kernels
#define FM_BLOCK 64          // query rows per workgroup of the matching kernel: one wave
#define FM_CHUNK 32          // target rows per LDS chunk; (FM_BLOCK + FM_CHUNK) * dim * 8 bytes: 25 KiB at dim 33, 48 KiB at 64
#define FM_GROUP 8           // target rows that share one read of the query; divides FM_CHUNK
#define FM_MAX_LANES 16      // chunk lanes (grid.z / 2); a target of more chunks than lanes is walked lane-strided
#define FM_MAX_DIM 64
#define FM_MUTUAL_BLOCK 256

// the cloud with off[c] <= i < off[c + 1]: the last c with off[c] <= i (clouds may be empty)
__device__ __forceinline__ int fp_cloud_of(const int64_t *__restrict__ off, int n_clouds, int64_t i) {
    int lo = 0, hi = n_clouds;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool fp_before(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }

// Ranks of the wave's m candidates in the order (d^2, j): lane l holds those of entries l, l + 64, ... in rk[], with
// their values in cd[] / cj[].  Every lane has read what it needs when this returns, so the caller may overwrite the buffer.
__device__ __forceinline__ void fp_knn_ranks(const double *c_d2, const int *c_j, int m, int lane, double *cd, int *cj, int *rk) {
#pragma unroll
    for (int s = 0; s < KNN_CAND / 64; ++s) {
        const int e = s * 64 + lane;
        cd[s] = e < m ? c_d2[e] : INFINITY;
        cj[s] = e < m ? c_j[e] : 0x7fffffff;
        rk[s] = 0;
    }
    for (int o = 0; o < m; ++o) {                          // every lane reads the same entry: a broadcast
        const double od = c_d2[o];
        const int oj = c_j[o];
#pragma unroll
        for (int s = 0; s < KNN_CAND / 64; ++s) rk[s] += fp_before(od, oj, cd[s], cj[s]) ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(KNN_BLOCK) void fp_knn_kernel(const double *__restrict__ pts, const int64_t *__restrict__ off, double r2,
                                                          int max_nn, int32_t *__restrict__ out_idx, double *__restrict__ out_d2,
                                                          int32_t *__restrict__ out_count) {
    __shared__ double s_p[3 * KNN_CHUNK];
    __shared__ double s_d2[KNN_BLOCK / 64][KNN_CAND];
    __shared__ int s_j[KNN_BLOCK / 64][KNN_CAND];
    const int c = blockIdx.y, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int64_t base = off[c], n = off[c + 1] - base;
    const int64_t q0 = (int64_t)blockIdx.x * (KNN_BLOCK / 64);
    if (q0 >= n) return;                                   // the whole workgroup leaves: no barrier is left waiting
    const int64_t qi = q0 + w;
    const bool live = qi < n;                              // a wave without a query still helps to load the chunks
    const int keep = max_nn - 1;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) { qx = pts[3 * (base + qi)]; qy = pts[3 * (base + qi) + 1]; qz = pts[3 * (base + qi) + 2]; }
    double *c_d2 = s_d2[w];
    int *c_j = s_j[w];
    double cd[KNN_CAND / 64];
    int cj[KNN_CAND / 64], rk[KNN_CAND / 64];
    int m = 0;                                             // wave-uniform: candidates in the buffer
    for (int64_t p0 = 0; p0 < n; p0 += KNN_CHUNK) {
        const int cm = (int)(n - p0 < KNN_CHUNK ? n - p0 : KNN_CHUNK);
        __syncthreads();                                   // the previous chunk has been consumed
        const double *g = pts + 3 * (base + p0);
        for (int e = t; e < 3 * cm; e += KNN_BLOCK) s_p[e] = g[e];
        __syncthreads();
        if (!live || keep == 0) continue;
        for (int j0 = 0; j0 < cm; j0 += 64) {
            if (m + 64 > KNN_CAND) {                       // the next 64 might not fit: cut to the best `keep`
                fp_knn_ranks(c_d2, c_j, m, lane, cd, cj, rk);
#pragma unroll
                for (int s = 0; s < KNN_CAND / 64; ++s)
                    if (rk[s] < keep && s * 64 + lane < m) { c_d2[rk[s]] = cd[s]; c_j[rk[s]] = cj[s]; }
                __builtin_amdgcn_wave_barrier();
                m = keep;                                  // m > KNN_CAND - 64 >= keep here
            }
            const int j = j0 + lane;
            bool in = false;
            double d = 0.0;
            if (j < cm) {
                const double dx = s_p[3 * j] - qx, dy = s_p[3 * j + 1] - qy, dz = s_p[3 * j + 2] - qz;
                d = fma(dz, dz, fma(dy, dy, __dmul_rn(dx, dx)));
                in = d <= r2 && p0 + j != qi;              // the query is entry 0 by rule, whatever coincides with it
            }
            const unsigned long long mask = __ballot(in);
            if (mask) {
                const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                if (in) { c_d2[m + below] = d; c_j[m + below] = (int)(p0 + j); }
                m += (int)__popcll(mask);
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (!live) return;
    fp_knn_ranks(c_d2, c_j, m, lane, cd, cj, rk);
    const int others = m < keep ? m : keep;
    int32_t *o_idx = out_idx + (base + qi) * max_nn;
    double *o_d2 = out_d2 + (base + qi) * max_nn;
#pragma unroll
    for (int s = 0; s < KNN_CAND / 64; ++s)
        if (rk[s] < keep && s * 64 + lane < m) { o_idx[1 + rk[s]] = cj[s]; o_d2[1 + rk[s]] = cd[s]; }
    for (int e = 1 + others + lane; e < max_nn; e += 64) { o_idx[e] = -1; o_d2[e] = INFINITY; }
    if (lane == 0) {
        o_idx[0] = (int)qi;
        o_d2[0] = 0.0;
        out_count[base + qi] = 1 + others;
    }
}

// Eigenvector of the smallest eigenvalue of the symmetric A (cyclic Jacobi; equal eigenvalues -> the lower index)
__device__ static void fp_smallest_eigenvector(double A[3][3], double *nrm) {
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 60; ++sweep) {
        double offd = 0.0, diag = 0.0;
        for (int i = 0; i < 3; ++i) {
            diag += A[i][i] * A[i][i];
            for (int j = i + 1; j < 3; ++j) offd += A[i][j] * A[i][j];
        }
        if (offd <= 1e-34 * diag || offd == 0.0) break;
        for (int i = 0; i < 2; ++i)
            for (int j = i + 1; j < 3; ++j) {
                const double aij = A[i][j];
                if (aij == 0.0) continue;
                const double theta = (A[j][j] - A[i][i]) / (2.0 * aij);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                for (int k = 0; k < 3; ++k) {               // A <- A J  (columns i, j)
                    const double aki = A[k][i], akj = A[k][j];
                    A[k][i] = cs * aki - sn * akj;
                    A[k][j] = sn * aki + cs * akj;
                }
                for (int k = 0; k < 3; ++k) {               // A <- J^T A (rows i, j)
                    const double aik = A[i][k], ajk = A[j][k];
                    A[i][k] = cs * aik - sn * ajk;
                    A[j][k] = sn * aik + cs * ajk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vki = V[k][i], vkj = V[k][j];
                    V[k][i] = cs * vki - sn * vkj;
                    V[k][j] = sn * vki + cs * vkj;
                }
            }
    }
    int best = 0;
    for (int k = 1; k < 3; ++k)
        if (A[k][k] < A[best][best]) best = k;
    const double x = V[0][best], y = V[1][best], z = V[2][best];
    const double inv = 1.0 / sqrt(x * x + y * y + z * z);
    nrm[0] = x * inv; nrm[1] = y * inv; nrm[2] = z * inv;
}

__global__ __launch_bounds__(FPFH_BLOCK) void fp_normals_kernel(const double *__restrict__ pts, const int64_t *__restrict__ off,
                                                               int n_clouds, int64_t total, const int32_t *__restrict__ idx,
                                                               const double *__restrict__ d2, const int32_t *__restrict__ count,
                                                               int width, double r2, int max_nn, double vx, double vy, double vz,
                                                               double *__restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * FPFH_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int64_t base = off[fp_cloud_of(off, n_clouds, i)];
    const int32_t *li = idx + i * width;
    const double *ld = d2 + i * width;
    int k = count[i] < max_nn ? count[i] : max_nn;
    k = k < width ? k : width;
    for (int e = 1; e < k; ++e)                            // ascending d^2 after the query: the first one beyond r ends the prefix
        if (!(ld[e] <= r2)) { k = e; break; }
    const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    double nrm[3] = {0.0, 0.0, 1.0};
    if (k >= 3) {
        double mx = 0.0, my = 0.0, mz = 0.0;
        for (int e = 0; e < k; ++e) {
            const int64_t j = base + li[e];
            mx += pts[3 * j] - px; my += pts[3 * j + 1] - py; mz += pts[3 * j + 2] - pz;
        }
        const double kk = (double)k;
        mx /= kk; my /= kk; mz /= kk;
        double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
        for (int e = 0; e < k; ++e) {
            const int64_t j = base + li[e];
            const double x = (pts[3 * j] - px) - mx, y = (pts[3 * j + 1] - py) - my, z = (pts[3 * j + 2] - pz) - mz;
            cxx += x * x; cxy += x * y; cxz += x * z; cyy += y * y; cyz += y * z; czz += z * z;
        }
        double A[3][3] = {{cxx / kk, cxy / kk, cxz / kk}, {cxy / kk, cyy / kk, cyz / kk}, {cxz / kk, cyz / kk, czz / kk}};
        fp_smallest_eigenvector(A, nrm);
    }
    const double dot = nrm[0] * (vx - px) + nrm[1] * (vy - py) + nrm[2] * (vz - pz);
    bool flip = dot < 0.0;
    if (dot == 0.0) {                                      // no side to choose: the component of largest magnitude is made positive
        int big = 0;
        for (int a = 1; a < 3; ++a)
            if (fabs(nrm[a]) > fabs(nrm[big])) big = a;
        flip = nrm[big] < 0.0;
    }
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = flip ? -nrm[a] : nrm[a];
}

__device__ __forceinline__ double fp_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// open3d's ComputePairFeatures (Feature.cpp): f[0] = atan2(w . n2, n1 . n2), f[1] = v . n2, f[2] = n1 . d / |d| after
// the swap that makes point 1 the one whose normal is closer to the connecting line; zeros for a degenerate pair
__device__ static void fp_pair_features(const double *p1, const double *n1, const double *p2, const double *n2, double *f) {
    f[0] = f[1] = f[2] = 0.0;
    double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double len = sqrt(fp_dot(d, d));
    if (len == 0.0) return;
    const double a1 = fp_dot(n1, d) / len, a2 = fp_dot(n2, d) / len;
    const double *m1 = n1, *m2 = n2;
    double f2;
    if (acos(fabs(a1)) > acos(fabs(a2))) {
        m1 = n2; m2 = n1;
        d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2];
        f2 = -a2;
    } else {
        f2 = a1;
    }
    double v[3] = {d[1] * m1[2] - d[2] * m1[1], d[2] * m1[0] - d[0] * m1[2], d[0] * m1[1] - d[1] * m1[0]};
    const double vn = sqrt(fp_dot(v, v));
    if (vn == 0.0) return;
    v[0] /= vn; v[1] /= vn; v[2] /= vn;
    const double w[3] = {m1[1] * v[2] - m1[2] * v[1], m1[2] * v[0] - m1[0] * v[2], m1[0] * v[1] - m1[1] * v[0]};
    f[2] = f2;
    f[1] = fp_dot(v, m2);
    f[0] = atan2(fp_dot(w, m2), fp_dot(m1, m2));
}

__device__ __forceinline__ int fp_bin(double x) {
    const double b = floor(x);
    return !(b >= 0.0) ? 0 : (b >= 10.0 ? 10 : (int)b);    // clamped to [0, 10]; a NaN goes to bin 0
}

__global__ __launch_bounds__(FPFH_BLOCK) void fp_spfh_kernel(const double *__restrict__ pts, const double *__restrict__ normals,
                                                            const int64_t *__restrict__ off, int n_clouds, int64_t total,
                                                            const int32_t *__restrict__ idx, const int32_t *__restrict__ count,
                                                            int width, double *__restrict__ spfh) {
    __shared__ int s_h[FPFH_BLOCK / 64][FPFH_BINS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (FPFH_BLOCK / 64) + w;
    if (i >= total) return;                                // whole waves leave; there is no workgroup barrier below
    if (lane < FPFH_BINS) s_h[w][lane] = 0;
    __builtin_amdgcn_wave_barrier();
    const int64_t base = off[fp_cloud_of(off, n_clouds, i)];
    const int k = count[i] < width ? count[i] : width;
    const double p1[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const double n1[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    for (int e = 1 + lane; e < k; e += 64) {
        const int64_t j = base + idx[i * width + e];
        const double p2[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
        const double n2[3] = {normals[3 * j], normals[3 * j + 1], normals[3 * j + 2]};
        double f[3];
        fp_pair_features(p1, n1, p2, n2, f);
        atomicAdd(&s_h[w][fp_bin(11.0 * (f[0] + M_PI) / (2.0 * M_PI))], 1);
        atomicAdd(&s_h[w][11 + fp_bin(11.0 * (f[1] + 1.0) / 2.0)], 1);
        atomicAdd(&s_h[w][22 + fp_bin(11.0 * (f[2] + 1.0) / 2.0)], 1);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < FPFH_BINS) spfh[i * FPFH_BINS + lane] = k > 1 ? (double)s_h[w][lane] * (100.0 / (double)(k - 1)) : 0.0;
}

__global__ __launch_bounds__(FPFH_BLOCK) void fp_fpfh_kernel(const double *__restrict__ spfh, const int64_t *__restrict__ off,
                                                            int n_clouds, int64_t total, const int32_t *__restrict__ idx,
                                                            const double *__restrict__ d2, const int32_t *__restrict__ count,
                                                            int width, double *__restrict__ fpfh) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (FPFH_BLOCK / 64) + w;
    if (i >= total) return;
    const int64_t base = off[fp_cloud_of(off, n_clouds, i)];
    const int k = count[i] < width ? count[i] : width;
    const int bin = lane < FPFH_BINS ? lane : FPFH_BINS - 1;   // the upper lanes repeat the last bin and write nothing
    double acc = 0.0;
    for (int e = 1; e < k; ++e) {
        const double dist = d2[i * width + e];
        if (dist == 0.0) continue;                         // wave-uniform
        acc += spfh[(base + idx[i * width + e]) * FPFH_BINS + bin] / dist;
    }
    double s = 0.0;                                        // the sum of this lane's group, in ascending bin order
    const int g0 = bin / 11 * 11;
    for (int b = 0; b < 11; ++b) s += __shfl(acc, g0 + b, 64);
    const double scaled = s != 0.0 ? acc * (100.0 / s) : acc;
    if (lane < FPFH_BINS) fpfh[i * FPFH_BINS + lane] = scaled + spfh[i * FPFH_BINS + lane];
}

// One thread per query row and chunk lane.  grid = (query blocks, pairs, 2 * lanes): z & 1 = direction (0: rows of a
// against b -> nn01, 1: rows of b against a -> nn10), z >> 1 = the lane, which walks the target chunks lane, lane + lanes, ...
// Output: a partial (distance, index) per query row and lane; fp_match_merge_kernel takes their minimum.
__global__ __launch_bounds__(FM_BLOCK) void fp_match_kernel(const double *__restrict__ a, const int64_t *__restrict__ a_off,
                                                           const double *__restrict__ b, const int64_t *__restrict__ b_off, int dim,
                                                           int64_t total_a, int64_t total_b, int lanes, double *__restrict__ part_d,
                                                           int *__restrict__ part_i) {
    extern __shared__ __align__(16) double s_fm[];
    double *s_q = s_fm;                                    // [dim][FM_BLOCK]: lane t reads its own column
    double *s_t = s_fm + (size_t)dim * FM_BLOCK;           // [FM_CHUNK][dim]: every lane reads the same address
    const int p = blockIdx.y, t = threadIdx.x, y = blockIdx.z >> 1;
    const bool fwd = (blockIdx.z & 1) == 0;
    const double *q = fwd ? a : b, *tg = fwd ? b : a;
    const int64_t *q_off = fwd ? a_off : b_off, *t_off = fwd ? b_off : a_off;
    const int64_t qb = q_off[p], nq = q_off[p + 1] - qb, tb = t_off[p], nt = t_off[p + 1] - tb;
    const int64_t i0 = (int64_t)blockIdx.x * FM_BLOCK;
    if (i0 >= nq) return;
    const int nchunks = (int)((nt + FM_CHUNK - 1) / FM_CHUNK);
    if (y >= nchunks) return;                              // the merge reads min(lanes, chunks) partials
    const int mq = (int)(nq - i0 < FM_BLOCK ? nq - i0 : FM_BLOCK);
    for (int e = t; e < FM_BLOCK * dim; e += FM_BLOCK) {   // e = row * dim + d of the block; absent rows are zeros
        const int r = e / dim, d = e - r * dim;
        s_q[d * FM_BLOCK + r] = r < mq ? q[(qb + i0) * dim + e] : 0.0;
    }
    double best = INFINITY;
    int bi = -1;
    for (int c = y; c < nchunks; c += lanes) {
        const int64_t c0 = (int64_t)c * FM_CHUNK;
        const int m = (int)(nt - c0 < FM_CHUNK ? nt - c0 : FM_CHUNK);
        __syncthreads();                                   // the previous chunk has been consumed (and s_q is written)
        const double *g = tg + (tb + c0) * dim;
        for (int e = t; e < FM_CHUNK * dim; e += FM_BLOCK) s_t[e] = e < m * dim ? g[e] : 0.0;
        __syncthreads();
        for (int j = 0; j < m; j += FM_GROUP) {            // FM_GROUP targets share each read of the query; rows >= m are zeros
            double acc[FM_GROUP];
#pragma unroll
            for (int v = 0; v < FM_GROUP; ++v) acc[v] = 0.0;
            const double *row = s_t + j * dim;
#pragma unroll 2
            for (int d = 0; d < dim; ++d) {
                const double x = s_q[d * FM_BLOCK + t];
#pragma unroll
                for (int v = 0; v < FM_GROUP; ++v) {
                    const double df = x - row[v * dim + d];
                    acc[v] += df * df;
                }
            }
#pragma unroll
            for (int v = 0; v < FM_GROUP; ++v)
                if (j + v < m && acc[v] < best) { best = acc[v]; bi = (int)c0 + j + v; }    // strict: the lower index of equals stays
        }
    }
    if (t < mq) {
        const int64_t o = (fwd ? 0 : (int64_t)lanes * total_a) + (int64_t)y * (fwd ? total_a : total_b) + qb + i0 + t;
        part_d[o] = best;
        part_i[o] = bi;
    }
}

// minimum over the chunk lanes, ties -> the lower target index; rows 0 .. total_a - 1 are nn01, the rest nn10
__global__ __launch_bounds__(256) void fp_match_merge_kernel(const int64_t *__restrict__ a_off, const int64_t *__restrict__ b_off,
                                                            int n_pairs, int64_t total_a, int64_t total_b, int lanes,
                                                            const double *__restrict__ part_d, const int *__restrict__ part_i,
                                                            int32_t *__restrict__ nn01, int32_t *__restrict__ nn10) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= total_a + total_b) return;
    const bool fwd = r < total_a;
    const int64_t row = fwd ? r : r - total_a, total_q = fwd ? total_a : total_b;
    const int p = fp_cloud_of(fwd ? a_off : b_off, n_pairs, row);
    const int64_t *t_off = fwd ? b_off : a_off;
    const int64_t nchunks = (t_off[p + 1] - t_off[p] + FM_CHUNK - 1) / FM_CHUNK;
    const int ny = (int)(nchunks < lanes ? nchunks : lanes);
    const int64_t base = (fwd ? 0 : (int64_t)lanes * total_a) + row;
    double best = INFINITY;
    int bi = -1;
    for (int y = 0; y < ny; ++y) {
        const double d = part_d[base + (int64_t)y * total_q];
        const int i = part_i[base + (int64_t)y * total_q];
        if (i >= 0 && (bi < 0 || d < best || (d == best && i < bi))) { best = d; bi = i; }
    }
    (fwd ? nn01 : nn10)[row] = bi;
}

__global__ __launch_bounds__(FM_MUTUAL_BLOCK) void fp_mutual_kernel(const int64_t *__restrict__ a_off, const int64_t *__restrict__ b_off,
                                                                   const int32_t *__restrict__ nn01, const int32_t *__restrict__ nn10,
                                                                   int32_t *__restrict__ pairs, int32_t *__restrict__ pair_count) {
    __shared__ int s_w[FM_MUTUAL_BLOCK / 64];
    const int p = blockIdx.x, t = threadIdx.x, w = t >> 6;
    const int64_t ab = a_off[p], na = a_off[p + 1] - ab, bb = b_off[p];
    int done = 0;                                          // kept rows so far: the same in every thread
    for (int64_t i0 = 0; i0 < na; i0 += FM_MUTUAL_BLOCK) {
        const int64_t i = i0 + t;
        int j = -1;
        bool keep = false;
        if (i < na) {
            j = nn01[ab + i];
            keep = j >= 0 && (int64_t)nn10[bb + j] == i;
        }
        const unsigned long long mask = __ballot(keep);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        __syncthreads();                                   // s_w of the previous round has been read
        if ((t & 63) == 0) s_w[w] = (int)__popcll(mask);
        __syncthreads();
        int before = done, all = 0;
        for (int v = 0; v < FM_MUTUAL_BLOCK / 64; ++v) {
            if (v < w) before += s_w[v];
            all += s_w[v];
        }
        if (keep) {
            pairs[2 * (ab + before + below)] = (int32_t)i;
            pairs[2 * (ab + before + below) + 1] = j;
        }
        done += all;
    }
    if (t == 0) pair_count[p] = done;
}

// ---- host side ---------------------------------------------------------------------------------
static StreamScratch g_fpfh_scratch;

// The shared offsets rule and this family's limits.  An entry point checks the caller's host copy before anything touches
// HIP (fp_host_shape); without one it makes one small read-back and one wait and checks then (fp_read_shape).
static int fp_host_shape(const int64_t *h_off, int n, bool may_be_empty, RaggedShape *s) {
    if (!h_off) return CSLAM_OK;
    int rc = offsets_check(h_off, n, s);
    if (rc) return rc;
    ARG_CHECK(may_be_empty || s->smallest > 0, "every feature array needs at least one row");
    ARG_CHECK(s->largest <= 0x7fffffffll - KNN_CHUNK, "a cloud has more points than an int32 index addresses");
    return CSLAM_OK;
}

static int fp_read_shape(const int64_t *h_off, const int64_t *d_off, int n, bool may_be_empty, hipStream_t st, RaggedShape *s) {
    if (h_off) return CSLAM_OK;
    std::vector<int64_t> own;
    int rc = read_back_async(own, d_off, (size_t)n + 1, st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return fp_host_shape(own.data(), n, may_be_empty, s);
}

static int fp_list_checks(const int32_t *d_idx, const int32_t *d_count, int width) {
    ARG_CHECK(d_idx && d_count, "NULL neighbour list");
    ARG_CHECK(width >= 1 && width <= KNN_MAX_NN, "the width of a neighbour list must be in [1, 256]");
    return CSLAM_OK;
}

CSLAM_API int cslam_knn_radius_dev(const double *d_points, const int64_t *d_offsets, int n_clouds, double radius, int max_nn,
                                   int32_t *d_idx, double *d_d2, int32_t *d_count, const int64_t *h_offsets, void *stream) {
    ARG_CHECK(radius > 0.0 && radius < INFINITY, "radius must be positive and finite");
    ARG_CHECK(max_nn >= 1 && max_nn <= KNN_MAX_NN, "max_nn must be in [1, 256]");
    BATCH_COUNT_CHECK(n_clouds);
    ARG_CHECK(d_points && d_offsets && d_idx && d_d2 && d_count, "NULL argument");
    RaggedShape off;
    int rc = fp_host_shape(h_offsets, n_clouds, true, &off);
    if (rc) return rc;
    PTR_DEVICE(d_points);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = fp_read_shape(h_offsets, d_offsets, n_clouds, true, st, &off))) return rc;
    if (off.total == 0) return CSLAM_OK;
    hipLaunchKernelGGL(fp_knn_kernel, dim3((unsigned)ceil_div64(off.largest, KNN_BLOCK / 64), (unsigned)n_clouds), dim3(KNN_BLOCK), 0, st,
                       d_points, d_offsets, radius * radius, max_nn, d_idx, d_d2, d_count);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_normals_dev(const double *d_points, const int64_t *d_offsets, int n_clouds, const int32_t *d_idx,
                                const double *d_d2, const int32_t *d_count, int list_width, double radius, int max_nn,
                                const double *viewpoint, double *d_normals, const int64_t *h_offsets, void *stream) {
    ARG_CHECK(radius > 0.0 && radius < INFINITY, "radius must be positive and finite");
    ARG_CHECK(max_nn >= 1, "max_nn must be at least 1");
    BATCH_COUNT_CHECK(n_clouds);
    ARG_CHECK(d_points && d_offsets && d_d2 && d_normals, "NULL argument");
    int rc = fp_list_checks(d_idx, d_count, list_width);
    if (rc) return rc;
    double v[3] = {0.0, 0.0, 0.0};
    if (viewpoint)
        for (int a = 0; a < 3; ++a) {
            ARG_CHECK(fabs(viewpoint[a]) < INFINITY, "the viewpoint must be finite");
            v[a] = viewpoint[a];
        }
    RaggedShape off;
    if ((rc = fp_host_shape(h_offsets, n_clouds, true, &off))) return rc;
    PTR_DEVICE(d_points);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = fp_read_shape(h_offsets, d_offsets, n_clouds, true, st, &off))) return rc;
    if (off.total == 0) return CSLAM_OK;
    hipLaunchKernelGGL(fp_normals_kernel, dim3((unsigned)ceil_div64(off.total, FPFH_BLOCK)), dim3(FPFH_BLOCK), 0, st, d_points, d_offsets,
                       n_clouds, off.total, d_idx, d_d2, d_count, list_width, radius * radius, max_nn, v[0], v[1], v[2], d_normals);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_fpfh_dev(const double *d_points, const double *d_normals, const int64_t *d_offsets, int n_clouds,
                             const int32_t *d_idx, const double *d_d2, const int32_t *d_count, int list_width, double *d_fpfh,
                             double *d_spfh, const int64_t *h_offsets, void *stream) {
    BATCH_COUNT_CHECK(n_clouds);
    ARG_CHECK(d_points && d_normals && d_offsets && d_d2 && d_fpfh, "NULL argument");
    int rc = fp_list_checks(d_idx, d_count, list_width);
    if (rc) return rc;
    RaggedShape off;
    if ((rc = fp_host_shape(h_offsets, n_clouds, true, &off))) return rc;
    PTR_DEVICE(d_points);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = fp_read_shape(h_offsets, d_offsets, n_clouds, true, st, &off))) return rc;
    if (off.total == 0) return CSLAM_OK;
    if (!d_spfh) {
        SCRATCH_HERE(base, g_fpfh_scratch, st, (size_t)off.total * FPFH_BINS * 8, (size_t)1 << 20);
        d_spfh = (double *)base;
    }
    const unsigned blocks = (unsigned)ceil_div64(off.total, FPFH_BLOCK / 64);
    hipLaunchKernelGGL(fp_spfh_kernel, dim3(blocks), dim3(FPFH_BLOCK), 0, st, d_points, d_normals, d_offsets, n_clouds, off.total, d_idx,
                       d_count, list_width, d_spfh);
    hipLaunchKernelGGL(fp_fpfh_kernel, dim3(blocks), dim3(FPFH_BLOCK), 0, st, d_spfh, d_offsets, n_clouds, off.total, d_idx, d_d2, d_count,
                       list_width, d_fpfh);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_feature_match_dev(const double *d_a, const int64_t *d_a_off, const double *d_b, const int64_t *d_b_off,
                                      int n_pairs, int dim, int32_t *d_nn01, int32_t *d_nn10, int32_t *d_pairs,
                                      int32_t *d_pair_count, const int64_t *h_a_off, const int64_t *h_b_off, void *stream) {
    ARG_CHECK(dim >= 1 && dim <= FM_MAX_DIM, "dim must be in [1, 64]");
    BATCH_COUNT_CHECK(n_pairs);
    ARG_CHECK(d_a && d_a_off && d_b && d_b_off && d_nn01 && d_nn10, "NULL argument");
    ARG_CHECK((d_pairs == nullptr) == (d_pair_count == nullptr), "d_pairs and d_pair_count go together");
    RaggedShape oa, ob;
    int rc;
    if ((rc = fp_host_shape(h_a_off, n_pairs, false, &oa)) || (rc = fp_host_shape(h_b_off, n_pairs, false, &ob))) return rc;
    PTR_DEVICE(d_a);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = fp_read_shape(h_a_off, d_a_off, n_pairs, false, st, &oa)) || (rc = fp_read_shape(h_b_off, d_b_off, n_pairs, false, st, &ob))) return rc;
    const size_t lds = (size_t)(FM_BLOCK + FM_CHUNK) * dim * sizeof(double);      // 48 KiB at dim 64
    const int64_t largest = oa.largest > ob.largest ? oa.largest : ob.largest;
    const int64_t qblocks = ceil_div64(largest, FM_BLOCK), chunks = ceil_div64(largest, FM_CHUNK);
    // chunk lanes until the launch has about 16 one-wave workgroups per compute unit: one pair fills the device
    const int64_t want = 16 * (int64_t)(cslam_cu_count() > 0 ? cslam_cu_count() : 256);
    int64_t lanes = ceil_div64(want, 2 * qblocks * n_pairs);
    lanes = lanes > FM_MAX_LANES ? FM_MAX_LANES : lanes;
    lanes = lanes > chunks ? chunks : lanes;
    const size_t n_part = (size_t)lanes * (size_t)(oa.total + ob.total);
    double *part_d;
    int *part_i;
    auto layout = [&](Carver &cv) { part_d = cv.take<double>(n_part); part_i = cv.take<int>(n_part); };
    SCRATCH_CARVE(g_fpfh_scratch, st, (size_t)1 << 20, layout);
    hipLaunchKernelGGL(fp_match_kernel, dim3((unsigned)qblocks, (unsigned)n_pairs, (unsigned)(2 * lanes)), dim3(FM_BLOCK), lds, st, d_a,
                       d_a_off, d_b, d_b_off, dim, oa.total, ob.total, (int)lanes, part_d, part_i);
    hipLaunchKernelGGL(fp_match_merge_kernel, dim3((unsigned)ceil_div64(oa.total + ob.total, 256)), dim3(256), 0, st, d_a_off, d_b_off,
                       n_pairs, oa.total, ob.total, (int)lanes, part_d, part_i, d_nn01, d_nn10);
    if (d_pairs)
        hipLaunchKernelGGL(fp_mutual_kernel, dim3((unsigned)n_pairs), dim3(FM_MUTUAL_BLOCK), 0, st, d_a_off, d_b_off, d_nn01, d_nn10, d_pairs,
                           d_pair_count);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}
