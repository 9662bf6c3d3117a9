// Pose-graph back end: GNC-TLS around Levenberg-Marquardt on SE(3), the algorithm of the reference's
// DecentralizedPGO::optimize (src/back_end/decentralized_pgo.cpp:797-845: GncOptimizer<GncParams<LevenbergMarquardtParams>>
// over BetweenFactor<Pose3> with diagonal noise and one prior), restated; GTSAM itself is third party and not available
// to compare against, tests/pgo_reference.py is the float64 yardstick.
//   host    pgo_plan.h: junctions / segments / index lists; the LM and GNC loops (one cost read-back per trial step)
//   device  linearise per factor + gather per pose and per pair in ascending factor order (no floating-point atomics
//           anywhere: two runs agree bit for bit), block-tridiagonal elimination of every segment (one wave per segment),
//           dense blocked Cholesky of the junction system, back substitution per pose, retraction, cost, GNC weights
// Everything is float64.  The workspace is grow-only and kept between calls; cslam_pgo_release frees it.
#include <algorithm>
#include <mutex>
#include <vector>
#include "common.h"
#define POSE_HD __host__ __device__ static inline
#include "pose.h"
#include "pgo_plan.h"

#define PGO_FAC_STRIDE 120        // per-factor scratch: Hii 36, Hjj 36, Hij 36, gi 6, gj 6
#define PGO_Y_COLS 19             // per interior slot: z (1), the two junction couplings (6 + 6), W = L^-1 U (6)
#define PGO_CON_STRIDE 120        // per segment: AA 36, AB 36, BB 36, ra 6, rb 6
#define PGO_CHOL_NB 48            // panel width of the dense Cholesky: 8 junction blocks, 18 KB of LDS
#define PGO_SUM_BLOCK 256

#define PGO_STATUS_OK 0
#define PGO_STATUS_PIVOT 1        // a non-positive pivot in a segment or in the junction factor: the step is rejected

namespace {

// ---- linearise ---------------------------------------------------------------------------------------------------------------
// one thread per factor k (k == nf: the prior).  E[k] = 1/2 sum (e / sigma)^2; with F the whitened (sqrt(w) / sigma) products
__global__ __launch_bounds__(64) void pgo_linearize_kernel(int nf, const int32_t *__restrict__ ei, const int32_t *__restrict__ ej, int prior,
                                                           const double *__restrict__ poses, const double *__restrict__ meas,
                                                           const double *__restrict__ sig, const double *__restrict__ w,
                                                           double *__restrict__ E, double *__restrict__ F) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nf) return;
    const bool is_prior = k == nf;
    const int i = is_prior ? -1 : ei[k], j = is_prior ? prior : ej[k];
    double e[6], Ai[36], Aj[36];
    pgo_between_residual(is_prior ? nullptr : poses + 16 * (int64_t)i, poses + 16 * (int64_t)j, meas + 16 * (int64_t)k, e,
                         F && !is_prior ? Ai : nullptr, F ? Aj : nullptr);
    double s[6], err = 0.0;
    for (int r = 0; r < 6; ++r) {
        const double q = e[r] / sig[6 * (int64_t)k + r];
        err += q * q;
    }
    E[k] = 0.5 * err;
    if (!F) return;
    const double sw = sqrt(w[k]);
    for (int r = 0; r < 6; ++r) {
        s[r] = sw / sig[6 * (int64_t)k + r];
        e[r] *= s[r];
        for (int c = 0; c < 6; ++c) {
            Aj[6 * r + c] *= s[r];
            if (!is_prior) Ai[6 * r + c] *= s[r];
        }
    }
    double *f = F + (int64_t)k * PGO_FAC_STRIDE;
    for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) {
            double hii = 0.0, hjj = 0.0, hij = 0.0;
            for (int r = 0; r < 6; ++r) {
                hjj += Aj[6 * r + a] * Aj[6 * r + b];
                if (!is_prior) { hii += Ai[6 * r + a] * Ai[6 * r + b]; hij += Ai[6 * r + a] * Aj[6 * r + b]; }
            }
            f[6 * a + b] = hii; f[36 + 6 * a + b] = hjj; f[72 + 6 * a + b] = hij;
        }
        double gi = 0.0, gj = 0.0;
        for (int r = 0; r < 6; ++r) {
            gj += Aj[6 * r + a] * e[r];
            if (!is_prior) gi += Ai[6 * r + a] * e[r];
        }
        f[108 + a] = gi; f[114 + a] = gj;
    }
}

// per pose: diagonal block [36] and gradient [6]; per pair: the block (row pa, column pb).  Sums run in ascending factor index.
__global__ __launch_bounds__(256) void pgo_gather_kernel(int64_t n, int64_t P, const int32_t *__restrict__ pose_ptr, const int32_t *__restrict__ pose_fac,
                                                         const int32_t *__restrict__ pair_ptr, const int32_t *__restrict__ pair_fac,
                                                         const double *__restrict__ F, double *__restrict__ Hdiag, double *__restrict__ g,
                                                         double *__restrict__ Hoff) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * 42) {
        const int64_t v = t / 42;
        const int e = (int)(t % 42);
        double acc = 0.0;
        for (int q = pose_ptr[v]; q < pose_ptr[v + 1]; ++q) {
            const int role = pose_fac[q] & 3;
            const double *f = F + (int64_t)(pose_fac[q] >> 2) * PGO_FAC_STRIDE;
            acc += e < 36 ? f[(role == 0 ? 0 : 36) + e] : f[(role == 0 ? 108 : 114) + e - 36];
        }
        if (e < 36) Hdiag[v * 36 + e] = acc; else g[v * 6 + e - 36] = acc;
    } else if (t < n * 42 + P * 36) {
        const int64_t u = t - n * 42, p = u / 36;
        const int e = (int)(u % 36), r = e / 6, c = e % 6;
        double acc = 0.0;
        for (int q = pair_ptr[p]; q < pair_ptr[p + 1]; ++q) {
            const double *f = F + (int64_t)(pair_fac[q] >> 1) * PGO_FAC_STRIDE + 72;
            acc += (pair_fac[q] & 1) ? f[6 * c + r] : f[6 * r + c];
        }
        Hoff[p * 36 + e] = acc;
    }
}

// ---- segment elimination --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pgo_load_block(const double *__restrict__ Hoff, int link, double *X) {
    const double *src = Hoff + (int64_t)(link >> 1) * 36;
    const bool tr = link & 1;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) X[6 * r + c] = tr ? src[6 * c + r] : src[6 * r + c];
}

// in-place lower Cholesky of a 6 x 6 (row-major, the lower triangle is read and written); false on a non-positive pivot
__device__ __forceinline__ bool pgo_chol6(double *L) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double d = L[7 * k];
#pragma unroll
        for (int q = 0; q < k; ++q) d -= L[6 * k + q] * L[6 * k + q];
        if (!(d > 0.0)) { ok = false; d = 1.0; }
        d = sqrt(d);
        L[7 * k] = d;
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double v = L[6 * i + k];
#pragma unroll
            for (int q = 0; q < k; ++q) v -= L[6 * i + q] * L[6 * k + q];
            L[6 * i + k] = v / d;
        }
    }
    return ok;
}
__device__ __forceinline__ void pgo_chol6_solve(const double *L, double *b) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = b[k];
#pragma unroll
        for (int q = 0; q < k; ++q) v -= L[6 * k + q] * b[q];
        b[k] = v / L[7 * k];
    }
#pragma unroll
    for (int k = 5; k >= 0; --k) {
        double v = b[k];
#pragma unroll
        for (int q = k + 1; q < 6; ++q) v -= L[6 * q + k] * b[q];
        b[k] = v / L[7 * k];
    }
}

// One wave per segment.  The interior (D_k + lambda I on the diagonal, U_k above it) is eliminated by the block recurrence
//   L_k = D_k + lambda I - U_{k-1}^T W_{k-1},  W_k = L_k^-1 U_k,  z_k = L_k^-1 (rhs_k - U_{k-1}^T z_{k-1}),  y_k = z_k - W_k y_{k+1}
// with 13 right-hand sides at once, one per lane: -g, the six columns of the coupling C_a to junction a (first row only) and the
// six of C_b (last row only).  Lanes 13 .. 18 carry the columns of W_k; every lane factors the 6 x 6 L_k itself.  Y keeps y_k
// and W_k per slot; `con` gets the Schur contribution C^T Y to the two end junctions.
__global__ __launch_bounds__(64) void pgo_segment_kernel(const int32_t *__restrict__ seg_ptr, const int32_t *__restrict__ seg_first,
                                                         const int32_t *__restrict__ slot_pose, const int32_t *__restrict__ slot_link,
                                                         const double *__restrict__ Hdiag, const double *__restrict__ Hoff,
                                                         const double *__restrict__ g, double lambda, double *__restrict__ Y,
                                                         double *__restrict__ con, int *__restrict__ status) {
    const int s = blockIdx.x, lane = threadIdx.x, col = lane < PGO_Y_COLS ? lane : PGO_Y_COLS - 1;
    const int s0 = seg_ptr[s], m = seg_ptr[s + 1] - s0;
    double Ca[36], U[36], Uprev[36], Wprev[36], L[36], z[6];
    pgo_load_block(Hoff, seg_first[s], Ca);
#pragma unroll
    for (int q = 0; q < 6; ++q) z[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 36; ++q) { Uprev[q] = 0.0; Wprev[q] = 0.0; }
    bool ok = true;
    for (int k = 0; k < m; ++k) {
        const int slot = s0 + k;
        const int64_t pose = slot_pose[slot];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = Hdiag[pose * 36 + 6 * r + c] + (r == c ? lambda : 0.0);
#pragma unroll
                for (int q = 0; q < 6; ++q) v -= Uprev[6 * q + r] * Wprev[6 * q + c];      // zero at k == 0
                L[6 * r + c] = v;
            }
        ok = pgo_chol6(L) && ok;
        pgo_load_block(Hoff, slot_link[slot], U);
        double b[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            double v = 0.0;
            if (col == 0) v = -g[pose * 6 + q];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (k == 0 && col == 1 + c) v = Ca[6 * q + c];
                if (k == m - 1 && col == 7 + c) v = U[6 * q + c];
                if (k < m - 1 && col == 13 + c) v = U[6 * q + c];
            }
            if (col < 13) {
#pragma unroll
                for (int p = 0; p < 6; ++p) v -= Uprev[6 * p + q] * z[p];
            }
            b[q] = v;
        }
        pgo_chol6_solve(L, b);
#pragma unroll
        for (int q = 0; q < 6; ++q) z[q] = b[q];
        if (lane < PGO_Y_COLS)
#pragma unroll
            for (int q = 0; q < 6; ++q) Y[((int64_t)slot * PGO_Y_COLS + col) * 6 + q] = z[q];
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int c = 0; c < 6; ++c) Wprev[6 * q + c] = __shfl(z[q], 13 + c, 64);
#pragma unroll
        for (int q = 0; q < 36; ++q) Uprev[q] = U[q];
    }
    if (!ok && lane == 0) *status = PGO_STATUS_PIVOT;
    __syncthreads();
    // back substitution over the slots; z is y of the last slot already
    for (int k = m - 2; k >= 0; --k) {
        const int64_t slot = s0 + k;
        double y[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            double v = Y[(slot * PGO_Y_COLS + col) * 6 + q];
#pragma unroll
            for (int c = 0; c < 6; ++c) v -= Y[(slot * PGO_Y_COLS + 13 + c) * 6 + q] * z[c];
            y[q] = v;
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) z[q] = y[q];
        if (lane < 13)
#pragma unroll
            for (int q = 0; q < 6; ++q) Y[(slot * PGO_Y_COLS + col) * 6 + q] = z[q];
    }
    __syncthreads();
    // C_a^T Y_first and C_b^T Y_last; U still holds C_b
    const double *Y1 = Y + (int64_t)s0 * PGO_Y_COLS * 6, *Ym = Y + (int64_t)(s0 + m - 1) * PGO_Y_COLS * 6;
    for (int e = lane; e < PGO_CON_STRIDE; e += 64) {
        const bool from_b = (e >= 72 && e < 108) || e >= 114;
        int r, ycol;
        if (e < 36) { r = e / 6; ycol = 1 + e % 6; }
        else if (e < 72) { r = (e - 36) / 6; ycol = 7 + (e - 36) % 6; }
        else if (e < 108) { r = (e - 72) / 6; ycol = 7 + (e - 72) % 6; }
        else if (e < 114) { r = e - 108; ycol = 0; }
        else { r = e - 114; ycol = 0; }
        const double *Yx = (from_b ? Ym : Y1) + ycol * 6;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            double cv = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c)
                if (c == r) cv = from_b ? U[6 * q + c] : Ca[6 * q + c];
            acc += cv * Yx[q];
        }
        con[(int64_t)s * PGO_CON_STRIDE + e] = acc;
    }
}

// ---- junction system: S [N x N] row-major, the lower triangle (whole diagonal blocks), rhs [N] ---------------------------------------
__global__ __launch_bounds__(256) void pgo_junction_set_kernel(int64_t J, int64_t nJJ, const int32_t *__restrict__ jl, const int32_t *__restrict__ jidx,
                                                               const int32_t *__restrict__ jj_pair, const int32_t *__restrict__ pa,
                                                               const int32_t *__restrict__ pb, const double *__restrict__ Hdiag,
                                                               const double *__restrict__ Hoff, const double *__restrict__ g, double lambda,
                                                               double *__restrict__ S, double *__restrict__ rhs) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, N = 6 * J;
    if (t < J * 42) {
        const int64_t j = t / 42, pose = jl[j];
        const int e = (int)(t % 42);
        if (e < 36) {
            const int r = e / 6, c = e % 6;
            S[(6 * j + r) * N + 6 * j + c] = Hdiag[pose * 36 + e] + (r == c ? lambda : 0.0);
        } else rhs[6 * j + e - 36] = -g[pose * 6 + e - 36];
    } else if (t < J * 42 + nJJ * 36) {
        const int64_t u = t - J * 42, p = jj_pair[u / 36];
        const int e = (int)(u % 36), r = e / 6, c = e % 6;
        const int64_t ja = jidx[pa[p]], jb = jidx[pb[p]];                  // ja < jb: block (row jb, column ja) is the pair's transposed
        S[(6 * jb + r) * N + 6 * ja + c] = Hoff[p * 36 + 6 * c + r];
    }
}

__global__ __launch_bounds__(256) void pgo_junction_add_kernel(int64_t nT, int64_t J, const int32_t *__restrict__ tgt_r, const int32_t *__restrict__ tgt_c,
                                                               const int32_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt_ent,
                                                               const double *__restrict__ con, double *__restrict__ S, double *__restrict__ rhs) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, N = 6 * J;
    if (t >= nT * 42) return;
    const int64_t T = t / 42, jr = tgt_r[T], jc = tgt_c[T];
    const int e = (int)(t % 42);
    if (e >= 36 && jr != jc) return;
    const int r = e < 36 ? e / 6 : e - 36, c = e % 6;
    double *dst = e < 36 ? S + (6 * jr + r) * N + 6 * jc + c : rhs + 6 * jr + r;
    double v = *dst;
    for (int q = tgt_ptr[T]; q < tgt_ptr[T + 1]; ++q) {                      // segment order
        const double *cs = con + (int64_t)(tgt_ent[q] >> 2) * PGO_CON_STRIDE;
        const int kind = tgt_ent[q] & 3;
        if (e < 36) {
            if (kind == PGO_KIND_AA) v -= cs[e];
            else if (kind == PGO_KIND_BB) v -= cs[72 + e];
            else if (kind == PGO_KIND_AB) v -= cs[36 + e];
            else v -= cs[36 + 6 * c + r];
        } else {
            if (kind == PGO_KIND_AA) v -= cs[108 + r];
            else if (kind == PGO_KIND_BB) v -= cs[114 + r];
        }
    }
    *dst = v;
}

// ---- dense Cholesky, right-looking, panels of PGO_CHOL_NB columns ----------------------------------------------------------------------
// the diagonal block of the panel, one workgroup, in LDS
__global__ __launch_bounds__(256) void pgo_chol_diag_kernel(double *__restrict__ S, int64_t N, int64_t k0, int *__restrict__ status) {
    __shared__ double D[PGO_CHOL_NB][PGO_CHOL_NB + 1];
    const int tid = threadIdx.x;
    const int nb = (int)(N - k0 < PGO_CHOL_NB ? N - k0 : PGO_CHOL_NB);
    for (int e = tid; e < nb * nb; e += 256) {
        const int r = e / nb, c = e % nb;
        D[r][c] = c <= r ? S[(k0 + r) * N + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < nb; ++k) {
        if (tid == 0) {
            double d = D[k][k];
            if (!(d > 0.0)) { d = 1.0; *status = PGO_STATUS_PIVOT; }
            D[k][k] = sqrt(d);
        }
        __syncthreads();
        const double dk = D[k][k];
        if (tid > k && tid < nb) D[tid][k] /= dk;
        __syncthreads();
        const int cnt = nb - k - 1;
        for (int e = tid; e < cnt * cnt; e += 256) {
            const int i = k + 1 + e / cnt, j = k + 1 + e % cnt;
            if (j <= i) D[i][j] -= D[i][k] * D[j][k];
        }
        __syncthreads();
    }
    for (int e = tid; e < nb * nb; e += 256) {
        const int r = e / nb, c = e % nb;
        if (c <= r) S[(k0 + r) * N + k0 + c] = D[r][c];
    }
}

// the rows below the panel's diagonal block: X L^T = A, one thread per row, the factored block in LDS
__global__ __launch_bounds__(256) void pgo_chol_rows_kernel(double *__restrict__ S, int64_t N, int64_t k0, int nb) {
    __shared__ double D[PGO_CHOL_NB][PGO_CHOL_NB + 1];
    const int tid = threadIdx.x;
    for (int e = tid; e < nb * nb; e += 256) D[e / nb][e % nb] = S[(k0 + e / nb) * N + k0 + e % nb];
    __syncthreads();
    const int64_t row = k0 + nb + (int64_t)blockIdx.x * 256 + tid;
    if (row < N) {
        double x[PGO_CHOL_NB];
        double *a = S + row * N + k0;
        for (int j = 0; j < nb; ++j) {
            double v = a[j];
            for (int q = 0; q < j; ++q) v -= x[q] * D[j][q];
            x[j] = v / D[j][j];
        }
        for (int j = 0; j < nb; ++j) a[j] = x[j];
    }
}

// trailing update: C[i][j] -= sum_q P[i][q] P[j][q] over the panel's columns, lower tiles only; 16 x 16 threads, 3 x 3 each
__global__ __launch_bounds__(256) void pgo_chol_update_kernel(double *__restrict__ S, int64_t N, int64_t k0, int nb) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    __shared__ double Pi[PGO_CHOL_NB][PGO_CHOL_NB + 1], Pj[PGO_CHOL_NB][PGO_CHOL_NB + 1];
    const int64_t t0 = k0 + nb, i0 = t0 + (int64_t)ti * PGO_CHOL_NB, j0 = t0 + (int64_t)tj * PGO_CHOL_NB;
    const int tid = threadIdx.x;
    for (int e = tid; e < PGO_CHOL_NB * PGO_CHOL_NB; e += 256) {
        const int r = e / PGO_CHOL_NB, c = e % PGO_CHOL_NB;
        Pi[r][c] = (i0 + r < N && c < nb) ? S[(i0 + r) * N + k0 + c] : 0.0;
        Pj[r][c] = (j0 + r < N && c < nb) ? S[(j0 + r) * N + k0 + c] : 0.0;
    }
    __syncthreads();
    const int tr = tid / 16, tc = tid % 16;
    double acc[3][3] = {};
    for (int q = 0; q < PGO_CHOL_NB; ++q)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[a][b] += Pi[3 * tr + a][q] * Pj[3 * tc + b][q];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int64_t i = i0 + 3 * tr + a, j = j0 + 3 * tc + b;
            if (i < N && j <= i) S[i * N + j] -= acc[a][b];
        }
}

// L y = b then L^T x = y, one workgroup, panel by panel: the triangle of the panel in LDS, the rest one row / column per thread
__global__ __launch_bounds__(256) void pgo_trisolve_kernel(const double *__restrict__ S, int64_t N, double *__restrict__ rhs) {
    __shared__ double D[PGO_CHOL_NB][PGO_CHOL_NB + 1], y[PGO_CHOL_NB];
    const int tid = threadIdx.x;
    for (int64_t k0 = 0; k0 < N; k0 += PGO_CHOL_NB) {
        const int nb = (int)(N - k0 < PGO_CHOL_NB ? N - k0 : PGO_CHOL_NB);
        for (int e = tid; e < nb * nb; e += 256) D[e / nb][e % nb] = S[(k0 + e / nb) * N + k0 + e % nb];
        if (tid < nb) y[tid] = rhs[k0 + tid];
        __syncthreads();
        for (int q = 0; q < nb; ++q) {
            if (tid == 0) y[q] /= D[q][q];
            __syncthreads();
            if (tid > q && tid < nb) y[tid] -= D[tid][q] * y[q];
            __syncthreads();
        }
        if (tid < nb) rhs[k0 + tid] = y[tid];
        for (int64_t i = k0 + nb + tid; i < N; i += 256) {
            double acc = rhs[i];
            for (int q = 0; q < nb; ++q) acc -= S[i * N + k0 + q] * y[q];
            rhs[i] = acc;
        }
        __syncthreads();
    }
    for (int64_t k0 = (N - 1) / PGO_CHOL_NB * PGO_CHOL_NB; k0 >= 0; k0 -= PGO_CHOL_NB) {
        const int nb = (int)(N - k0 < PGO_CHOL_NB ? N - k0 : PGO_CHOL_NB);
        for (int e = tid; e < nb * nb; e += 256) D[e / nb][e % nb] = S[(k0 + e / nb) * N + k0 + e % nb];
        if (tid < nb) y[tid] = rhs[k0 + tid];
        __syncthreads();
        for (int q = nb - 1; q >= 0; --q) {
            if (tid == 0) y[q] /= D[q][q];
            __syncthreads();
            if (tid < q) y[tid] -= D[q][tid] * y[q];
            __syncthreads();
        }
        if (tid < nb) rhs[k0 + tid] = y[tid];
        for (int64_t i = tid; i < k0; i += 256) {
            double acc = rhs[i];
            for (int q = 0; q < nb; ++q) acc -= S[(k0 + q) * N + i] * y[q];
            rhs[i] = acc;
        }
        __syncthreads();
    }
}

// ---- back substitution, model, retraction, sums, weights ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pgo_backsub_kernel(int64_t n, const int32_t *__restrict__ jidx, const int32_t *__restrict__ pose_slot,
                                                          const int32_t *__restrict__ slot_seg, const int32_t *__restrict__ seg_a,
                                                          const int32_t *__restrict__ seg_b, const double *__restrict__ Y,
                                                          const double *__restrict__ xj, double *__restrict__ delta) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 6) return;
    const int64_t v = t / 6;
    const int r = (int)(t % 6);
    if (jidx[v] >= 0) { delta[t] = xj[6 * (int64_t)jidx[v] + r]; return; }
    const int64_t slot = pose_slot[v];
    const int s = slot_seg[slot];
    const double *xa = xj + 6 * (int64_t)seg_a[s], *xb = xj + 6 * (int64_t)seg_b[s], *y = Y + slot * PGO_Y_COLS * 6;
    double acc = y[r];
    for (int c = 0; c < 6; ++c) acc -= y[(1 + c) * 6 + r] * xa[c];
    for (int c = 0; c < 6; ++c) acc -= y[(7 + c) * 6 + r] * xb[c];
    delta[t] = acc;
}

// q[v] = g_v . d_v + 1/2 d_v . (H d)_v: the quadratic model's change is their sum
__global__ __launch_bounds__(256) void pgo_model_kernel(int64_t n, const int32_t *__restrict__ adj_ptr, const int32_t *__restrict__ adj_nbr,
                                                        const int32_t *__restrict__ adj_pair, const double *__restrict__ Hdiag,
                                                        const double *__restrict__ Hoff, const double *__restrict__ g,
                                                        const double *__restrict__ delta, double *__restrict__ q) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double hd[6], d[6];
    for (int r = 0; r < 6; ++r) d[r] = delta[v * 6 + r];
    for (int r = 0; r < 6; ++r) {
        double acc = 0.0;
        for (int c = 0; c < 6; ++c) acc += Hdiag[v * 36 + 6 * r + c] * d[c];
        hd[r] = acc;
    }
    for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) {
        const int64_t u = adj_nbr[k];
        const double *B = Hoff + (int64_t)adj_pair[k] * 36;
        const bool tr = u < v;                                               // stored block is (row min, column max)
        for (int r = 0; r < 6; ++r) {
            double acc = 0.0;
            for (int c = 0; c < 6; ++c) acc += (tr ? B[6 * c + r] : B[6 * r + c]) * delta[u * 6 + c];
            hd[r] += acc;
        }
    }
    double acc = 0.0;
    for (int r = 0; r < 6; ++r) acc += g[v * 6 + r] * d[r] + 0.5 * d[r] * hd[r];
    q[v] = acc;
}

__global__ __launch_bounds__(256) void pgo_retract_kernel(int64_t n, const double *__restrict__ poses, const double *__restrict__ delta,
                                                          double *__restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double R[9], t[3], Rd[9], td[3], Ro[9], to[3], T[16];
    pose_load(poses + 16 * v, R, t);
    se3_exp(delta + 6 * v, Rd, td);
    se3_mul(R, t, Rd, td, Ro, to);
    pose_store(Ro, to, T);
    for (int k = 0; k < 16; ++k) out[16 * v + k] = T[k];
}

// sum of w[k] x[k] (w NULL: of x[k]): per block a fixed tree over 256 values, then the block partials in block order
__global__ __launch_bounds__(PGO_SUM_BLOCK) void pgo_cost_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ w,
                                                                 double *__restrict__ partial) {
    __shared__ double sh[PGO_SUM_BLOCK];
    const int64_t k = (int64_t)blockIdx.x * PGO_SUM_BLOCK + threadIdx.x;
    sh[threadIdx.x] = k < n ? (w ? w[k] * x[k] : x[k]) : 0.0;
    __syncthreads();
    for (int off = PGO_SUM_BLOCK / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ void pgo_cost_final_kernel(int64_t nblocks, const double *__restrict__ partial, double *__restrict__ out) {
    double acc = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) acc += partial[b];
    *out = acc;
}

// GNC-TLS weights (Yang, Antonante, Tzoumas, Carlone 2020, eq. 14): 0 at E >= up, 1 at E <= lo, between them
// sqrt(barc2 mu (mu + 1) / E) - mu; a known inlier keeps 1
__global__ __launch_bounds__(256) void pgo_weights_kernel(int64_t nfac, const double *__restrict__ E, double mu, double barc2,
                                                          const uint8_t *__restrict__ known, double *__restrict__ w) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nfac) return;
    const double up = (mu + 1.0) / mu * barc2, lo = mu / (mu + 1.0) * barc2, e = E[k];
    double v;
    if (known && known[k]) v = 1.0;
    else if (e >= up) v = 0.0;
    else if (e <= lo) v = 1.0;
    else v = sqrt(barc2 * mu * (mu + 1.0) / e) - mu;
    w[k] = v;
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------
struct PgoBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return CSLAM_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipMalloc(&p, want) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            cslam_set_error("cslam_pgo: hipMalloc of %zu bytes failed", want);
            return CSLAM_E_NOMEM;
        }
        cap = want;
        return CSLAM_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct PgoWs {
    int device = -1;
    bool planned = false;
    PgoPlan plan;
    PgoBuf ints, dbl, dense, io, word;            // word: the status of cslam_pgo_dense_solve_dev, which has no plan to keep it in
    // device views into `ints`
    int32_t *ei, *ej, *pa, *pb, *pair_ptr, *pair_fac, *pose_ptr, *pose_fac, *adj_ptr, *adj_nbr, *adj_pair, *jl, *jidx, *seg_ptr, *seg_a,
        *seg_b, *seg_first, *slot_pose, *slot_link, *pose_slot, *slot_seg, *jj_pair, *tgt_r, *tgt_c, *tgt_ptr, *tgt_ent, *status;
    // device views into `dbl`
    double *F, *Hdiag, *g, *Hoff, *E, *Y, *con, *rhs, *delta, *q, *partial, *scalar;
    std::vector<int32_t> trace;                   // accept (1) / reject (0) of every trial step of the last cslam_pgo_optimize
    void release() { ints.release(); dbl.release(); dense.release(); io.release(); word.release(); planned = false; device = -1; }
} g_pgo;
std::mutex g_pgo_mu;

// the workspace lives on the current device: buffers left on another one are freed there first
int pgo_bind_device() {
    PgoWs &w = g_pgo;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (w.device != dev) { if (w.device >= 0) { DeviceGuard guard(w.device); w.release(); } w.device = dev; }
    return CSLAM_OK;
}

int pgo_set_plan(int64_t n, int64_t nf, const int32_t *h_ei, const int32_t *h_ej, int64_t prior, hipStream_t st) {
    PgoWs &w = g_pgo;
    w.planned = false;
    const int prc = pgo_make_plan(n, nf, h_ei, h_ej, prior, &w.plan);
    if (prc == PGO_PLAN_E_LIMIT) {
        cslam_set_error("cslam_pgo: %lld junctions, the dense junction system holds at most %d", (long long)w.plan.J(), PGO_MAX_JUNCTIONS);
        return CSLAM_E_LIMIT;
    }
    ARG_CHECK(prc == 0, "cslam_pgo: pose index out of range, an edge with i == j, or a prior outside the poses");
    int rc = pgo_bind_device();
    if (rc) return rc;
    const PgoPlan &p = w.plan;
    const int64_t J = p.J(), S = p.S(), M = p.M(), P = p.P(), N = 6 * J;
    std::vector<int32_t> slot_seg(M);
    for (int64_t s = 0; s < S; ++s)
        for (int32_t q = p.seg_ptr[s]; q < p.seg_ptr[s + 1]; ++q) slot_seg[q] = (int32_t)s;
    std::vector<int32_t> vei(h_ei, h_ei + nf), vej(h_ej, h_ej + nf), vstatus(1, 0);
    struct Up { int32_t **dst; const std::vector<int32_t> *src; };
    const Up ups[] = {{&w.ei, &vei}, {&w.ej, &vej}, {&w.pa, &p.pa}, {&w.pb, &p.pb}, {&w.pair_ptr, &p.pair_ptr}, {&w.pair_fac, &p.pair_fac},
                      {&w.pose_ptr, &p.pose_ptr}, {&w.pose_fac, &p.pose_fac}, {&w.adj_ptr, &p.adj_ptr}, {&w.adj_nbr, &p.adj_nbr},
                      {&w.adj_pair, &p.adj_pair}, {&w.jl, &p.jl}, {&w.jidx, &p.jidx}, {&w.seg_ptr, &p.seg_ptr}, {&w.seg_a, &p.seg_a},
                      {&w.seg_b, &p.seg_b}, {&w.seg_first, &p.seg_first}, {&w.slot_pose, &p.slot_pose}, {&w.slot_link, &p.slot_link},
                      {&w.pose_slot, &p.pose_slot}, {&w.slot_seg, &slot_seg}, {&w.jj_pair, &p.jj_pair}, {&w.tgt_r, &p.tgt_r},
                      {&w.tgt_c, &p.tgt_c}, {&w.tgt_ptr, &p.tgt_ptr}, {&w.tgt_ent, &p.tgt_ent}, {&w.status, &vstatus}};
    auto ints_layout = [&](Carver &cv) {
        for (const Up &u : ups) *u.dst = cv.take<int32_t>(u.src->size(), 256);
    };
    Carver isize;
    ints_layout(isize);
    std::vector<char> stage(isize.at, 0);
    rc = w.ints.ensure(isize.at);
    if (rc) return rc;
    Carver iplace(w.ints.p);
    ints_layout(iplace);
    for (const Up &u : ups)
        if (!u.src->empty()) memcpy(stage.data() + ((char *)*u.dst - (char *)w.ints.p), u.src->data(), u.src->size() * 4);
    HIP_TRY(hipMemcpyAsync(w.ints.p, stage.data(), isize.at, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                                      // `stage` leaves scope
    const int64_t nfac = nf + 1, nsum = ceil_div64(std::max(nfac, n), PGO_SUM_BLOCK);
    const size_t counts[] = {(size_t)nfac * PGO_FAC_STRIDE, (size_t)n * 36, (size_t)n * 6, (size_t)std::max<int64_t>(P, 1) * 36, (size_t)nfac,
                             (size_t)std::max<int64_t>(M, 1) * PGO_Y_COLS * 6, (size_t)std::max<int64_t>(S, 1) * PGO_CON_STRIDE, (size_t)N,
                             (size_t)n * 6, (size_t)n, (size_t)nsum, 4};
    double **views[] = {&w.F, &w.Hdiag, &w.g, &w.Hoff, &w.E, &w.Y, &w.con, &w.rhs, &w.delta, &w.q, &w.partial, &w.scalar};
    auto dbl_layout = [&](Carver &cv) {
        for (int k = 0; k < 12; ++k) *views[k] = cv.take<double>(counts[k]);
    };
    Carver dsize;
    dbl_layout(dsize);
    rc = w.dbl.ensure(dsize.at);
    if (rc) return rc;
    Carver dplace(w.dbl.p);
    dbl_layout(dplace);
    rc = w.dense.ensure((size_t)N * N * 8);
    if (rc) return rc;
    w.planned = true;
    return CSLAM_OK;
}

static inline unsigned pgo_grid(int64_t threads, int block) { return (unsigned)std::max<int64_t>(1, ceil_div64(threads, block)); }

// E [nf + 1] at `poses`; with d_w the system (Hdiag, g, Hoff) as well
int pgo_linearize(const double *d_poses, const double *d_meas, const double *d_sig, const double *d_w, double *d_E, hipStream_t st) {
    PgoWs &w = g_pgo;
    const PgoPlan &p = w.plan;
    const int64_t nfac = p.nf + 1;
    hipLaunchKernelGGL(pgo_linearize_kernel, dim3(pgo_grid(nfac, 64)), dim3(64), 0, st, (int)p.nf, w.ei, w.ej, (int)p.prior, d_poses, d_meas,
                       d_sig, d_w, d_E, d_w ? w.F : nullptr);
    if (d_w)
        hipLaunchKernelGGL(pgo_gather_kernel, dim3(pgo_grid(p.n * 42 + p.P() * 36, 256)), dim3(256), 0, st, p.n, p.P(), w.pose_ptr, w.pose_fac,
                           w.pair_ptr, w.pair_fac, w.F, w.Hdiag, w.g, w.Hoff);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

int pgo_sum(const double *d_x, const double *d_w, int64_t count, double *h_out, hipStream_t st) {
    PgoWs &w = g_pgo;
    const int64_t nb = ceil_div64(count, PGO_SUM_BLOCK);
    hipLaunchKernelGGL(pgo_cost_kernel, dim3((unsigned)nb), dim3(PGO_SUM_BLOCK), 0, st, count, d_x, d_w, w.partial);
    hipLaunchKernelGGL(pgo_cost_final_kernel, dim3(1), dim3(1), 0, st, nb, w.partial, w.scalar);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_out, w.scalar, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CSLAM_OK;
}

// S x = rhs by the panelled factor and the two triangular solves, launches only: the lower triangle of Sd becomes the factor, rhs the
// solution, *d_status PGO_STATUS_PIVOT on a non-positive pivot (the caller zeroes it).  The one statement of this sequence: pgo_solve
// and cslam_pgo_dense_solve_dev both run it.
void pgo_dense_solve(double *Sd, int64_t N, double *d_rhs, int *d_status, hipStream_t st) {
    for (int64_t k0 = 0; k0 < N; k0 += PGO_CHOL_NB) {
        const int nb = (int)std::min<int64_t>(PGO_CHOL_NB, N - k0);
        const int64_t below = N - k0 - nb;
        hipLaunchKernelGGL(pgo_chol_diag_kernel, dim3(1), dim3(256), 0, st, Sd, N, k0, d_status);
        if (below > 0) {
            hipLaunchKernelGGL(pgo_chol_rows_kernel, dim3(pgo_grid(below, 256)), dim3(256), 0, st, Sd, N, k0, nb);
            const unsigned tiles = (unsigned)ceil_div64(below, PGO_CHOL_NB);
            hipLaunchKernelGGL(pgo_chol_update_kernel, dim3(tiles, tiles), dim3(256), 0, st, Sd, N, k0, nb);
        }
    }
    hipLaunchKernelGGL(pgo_trisolve_kernel, dim3(1), dim3(256), 0, st, Sd, N, d_rhs);
}

// (H + lambda I) delta = -g on the system of the last pgo_linearize; *h_predicted = -(g . delta + 1/2 delta . H delta)
int pgo_solve(double lambda, double *d_delta, int *h_status, double *h_predicted, hipStream_t st) {
    PgoWs &w = g_pgo;
    const PgoPlan &p = w.plan;
    const int64_t J = p.J(), S = p.S(), N = 6 * J, nT = (int64_t)p.tgt_r.size(), nJJ = (int64_t)p.jj_pair.size();
    double *Sd = (double *)w.dense.p;
    HIP_TRY(hipMemsetAsync(w.status, 0, 4, st));
    HIP_TRY(hipMemsetAsync(Sd, 0, (size_t)N * N * 8, st));
    if (S)
        hipLaunchKernelGGL(pgo_segment_kernel, dim3((unsigned)S), dim3(64), 0, st, w.seg_ptr, w.seg_first, w.slot_pose, w.slot_link, w.Hdiag,
                           w.Hoff, w.g, lambda, w.Y, w.con, w.status);
    hipLaunchKernelGGL(pgo_junction_set_kernel, dim3(pgo_grid(J * 42 + nJJ * 36, 256)), dim3(256), 0, st, J, nJJ, w.jl, w.jidx, w.jj_pair, w.pa,
                       w.pb, w.Hdiag, w.Hoff, w.g, lambda, Sd, w.rhs);
    if (nT)
        hipLaunchKernelGGL(pgo_junction_add_kernel, dim3(pgo_grid(nT * 42, 256)), dim3(256), 0, st, nT, J, w.tgt_r, w.tgt_c, w.tgt_ptr, w.tgt_ent,
                           w.con, Sd, w.rhs);
    pgo_dense_solve(Sd, N, w.rhs, w.status, st);
    hipLaunchKernelGGL(pgo_backsub_kernel, dim3(pgo_grid(p.n * 6, 256)), dim3(256), 0, st, p.n, w.jidx, w.pose_slot, w.slot_seg, w.seg_a, w.seg_b,
                       w.Y, w.rhs, d_delta);
    hipLaunchKernelGGL(pgo_model_kernel, dim3(pgo_grid(p.n, 256)), dim3(256), 0, st, p.n, w.adj_ptr, w.adj_nbr, w.adj_pair, w.Hdiag, w.Hoff, w.g,
                       d_delta, w.q);
    HIP_TRY(hipGetLastError());
    double model = 0.0;
    int rc = pgo_sum(w.q, nullptr, p.n, &model, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h_status, w.status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *h_predicted = -model;
    return CSLAM_OK;
}

#define PGO_NEED_PLAN() \
    do { if (!g_pgo.planned) { cslam_set_error("cslam_pgo: no plan (call cslam_pgo_plan first)"); return CSLAM_E_INVALID; } } while (0)

struct PgoParams {
    double lambda0 = 1e-5, factor = 10.0, lambda_max = 1e5;
    int max_iter = 100;
    double rel_tol = 1e-5, abs_tol = 1e-5, fidelity = 1e-3;
    int gnc_max_rounds = 100;
    double mu_step = 1.4, gnc_cost_tol = 1e-5, weights_tol = 1e-4, barc2 = 0.5 * 16.811893829770927, mu_floor = 1e-6;
};

struct PgoCounters { int64_t lm_iterations = 0, solves = 0; double lambda = 0.0; int status = PGO_STATUS_OK; };

// Levenberg-Marquardt with the lambda I damping from d_x (updated in place; d_try is the trial estimate); *cost = sum w E at the result
int pgo_lm(const PgoParams &P, double *d_x, double *d_try, const double *d_meas, const double *d_sig, const double *d_w, double *cost,
           PgoCounters *cnt, hipStream_t st) {
    PgoWs &w = g_pgo;
    const int64_t n = w.plan.n, nfac = w.plan.nf + 1;
    double lambda = P.lambda0, c = 0.0;
    int rc = pgo_linearize(d_x, d_meas, d_sig, d_w, w.E, st);
    if (rc) return rc;
    rc = pgo_sum(w.E, d_w, nfac, &c, st);
    if (rc) return rc;
    bool stop = false;
    for (int it = 0; it < P.max_iter && !stop; ++it) {
        if (it) { rc = pgo_linearize(d_x, d_meas, d_sig, d_w, w.E, st); if (rc) return rc; }
        double c_accepted = c;
        for (;;) {
            int status = 0;
            double predicted = 0.0, c_new = 0.0;
            rc = pgo_solve(lambda, w.delta, &status, &predicted, st);
            if (rc) return rc;
            ++cnt->solves;
            bool accept = false;
            if (status == PGO_STATUS_OK && predicted > 0.0) {
                hipLaunchKernelGGL(pgo_retract_kernel, dim3(pgo_grid(n, 256)), dim3(256), 0, st, n, d_x, w.delta, d_try);
                rc = pgo_linearize(d_try, d_meas, d_sig, nullptr, w.E, st);
                if (rc) return rc;
                rc = pgo_sum(w.E, d_w, nfac, &c_new, st);
                if (rc) return rc;
                accept = (c - c_new) / predicted > P.fidelity;
            } else if (status != PGO_STATUS_OK) cnt->status = status;
            w.trace.push_back(accept ? 1 : 0);
            if (accept) {
                HIP_TRY(hipMemcpyAsync(d_x, d_try, (size_t)n * 16 * 8, hipMemcpyDeviceToDevice, st));
                c_accepted = c_new;
                lambda /= P.factor;
                break;
            }
            lambda *= P.factor;
            if (lambda > P.lambda_max) { stop = true; break; }
        }
        if (stop) break;
        ++cnt->lm_iterations;
        const double decrease = c - c_accepted;
        if (decrease < P.abs_tol || decrease / c < P.rel_tol) stop = true;
        c = c_accepted;
    }
    cnt->lambda = lambda;
    *cost = c;
    return CSLAM_OK;
}

}  // namespace

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
CSLAM_API int cslam_pgo_release(void) {
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    if (g_pgo.device >= 0) { DeviceGuard guard(g_pgo.device); g_pgo.release(); }
    return CSLAM_OK;
}

CSLAM_API int cslam_pgo_plan(int64_t n, int64_t nf, const int32_t *h_ei, const int32_t *h_ej, int64_t prior, int64_t *h_info) {
    ARG_CHECK((h_ei && h_ej) || nf == 0, "cslam_pgo_plan: NULL edge arrays");
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    // the structure pass comes before anything touches HIP: argument errors and the junction cap need no device
    const int rc = pgo_set_plan(n, nf, h_ei, h_ej, prior, nullptr);
    if (rc) return rc;
    if (h_info) {
        const PgoPlan &p = g_pgo.plan;
        h_info[0] = p.J(); h_info[1] = p.S(); h_info[2] = p.M(); h_info[3] = p.P(); h_info[4] = p.n_cut;
        int64_t longest = 0;
        for (int64_t s = 0; s < p.S(); ++s) longest = std::max<int64_t>(longest, p.seg_ptr[s + 1] - p.seg_ptr[s]);
        h_info[5] = longest; h_info[6] = PGO_SEG_MAX; h_info[7] = PGO_MAX_JUNCTIONS;
    }
    return CSLAM_OK;
}

CSLAM_API int cslam_pgo_linearize_dev(const double *d_poses, const double *d_meas, const double *d_sigmas, const double *d_weights,
                                      double *d_E, void *stream) {
    ARG_CHECK(d_poses && d_meas && d_sigmas && d_weights && d_E, "cslam_pgo_linearize_dev: NULL argument");
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    PGO_NEED_PLAN();
    return pgo_linearize(d_poses, d_meas, d_sigmas, d_weights, d_E, (hipStream_t)stream);
}

CSLAM_API int cslam_pgo_system_host(double *h_Hdiag, double *h_g, double *h_Hoff, int32_t *h_pa, int32_t *h_pb, void *stream) {
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    PGO_NEED_PLAN();
    const PgoPlan &p = g_pgo.plan;
    hipStream_t st = (hipStream_t)stream;
    if (h_Hdiag) HIP_TRY(hipMemcpyAsync(h_Hdiag, g_pgo.Hdiag, (size_t)p.n * 36 * 8, hipMemcpyDeviceToHost, st));
    if (h_g) HIP_TRY(hipMemcpyAsync(h_g, g_pgo.g, (size_t)p.n * 6 * 8, hipMemcpyDeviceToHost, st));
    if (h_Hoff && p.P()) HIP_TRY(hipMemcpyAsync(h_Hoff, g_pgo.Hoff, (size_t)p.P() * 36 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_pa && p.P()) memcpy(h_pa, p.pa.data(), (size_t)p.P() * 4);
    if (h_pb && p.P()) memcpy(h_pb, p.pb.data(), (size_t)p.P() * 4);
    return CSLAM_OK;
}

CSLAM_API int cslam_pgo_solve_dev(double lambda, double *d_delta, int *h_status, double *h_predicted, void *stream) {
    ARG_CHECK(d_delta && h_status && h_predicted, "cslam_pgo_solve_dev: NULL argument");
    ARG_CHECK(lambda >= 0.0 && lambda == lambda, "cslam_pgo_solve_dev: lambda must be >= 0");
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    PGO_NEED_PLAN();
    return pgo_solve(lambda, d_delta, h_status, h_predicted, (hipStream_t)stream);
}

CSLAM_API int cslam_pgo_dense_solve_dev(double *d_S, int64_t N, double *d_rhs, int *h_status, void *stream) {
    ARG_CHECK(d_S && d_rhs && h_status, "cslam_pgo_dense_solve_dev: NULL argument");
    ARG_CHECK(N >= 1 && N <= 6 * (int64_t)PGO_MAX_JUNCTIONS, "cslam_pgo_dense_solve_dev: N must be in [1, 6 x the junction cap]");
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    hipStream_t st = (hipStream_t)stream;
    int rc = pgo_bind_device();
    if (rc) return rc;
    rc = g_pgo.word.ensure(4);
    if (rc) return rc;
    int *d_status = (int *)g_pgo.word.p;
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, st));
    pgo_dense_solve(d_S, N, d_rhs, d_status, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_status, d_status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CSLAM_OK;
}

CSLAM_API int cslam_pgo_retract_dev(const double *d_poses, const double *d_delta, int64_t n, double *d_out, void *stream) {
    ARG_CHECK(d_poses && d_delta && d_out && n >= 1, "cslam_pgo_retract_dev: NULL argument or n < 1");
    hipLaunchKernelGGL(pgo_retract_kernel, dim3(pgo_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n, d_poses, d_delta, d_out);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_pgo_cost_dev(const double *d_poses, const double *d_meas, const double *d_sigmas, const double *d_weights, double *d_E,
                                 double *h_cost, void *stream) {
    ARG_CHECK(d_poses && d_meas && d_sigmas && d_weights && d_E && h_cost, "cslam_pgo_cost_dev: NULL argument");
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    PGO_NEED_PLAN();
    const int rc = pgo_linearize(d_poses, d_meas, d_sigmas, nullptr, d_E, (hipStream_t)stream);
    if (rc) return rc;
    return pgo_sum(d_E, d_weights, g_pgo.plan.nf + 1, h_cost, (hipStream_t)stream);
}

CSLAM_API int cslam_pgo_weights_dev(const double *d_E, int64_t nfac, double mu, double barc2, const uint8_t *d_known, double *d_w,
                                    void *stream) {
    ARG_CHECK(d_E && d_w && nfac >= 1, "cslam_pgo_weights_dev: NULL argument or nfac < 1");
    ARG_CHECK(mu > 0.0 && barc2 > 0.0, "cslam_pgo_weights_dev: mu and barc2 must be positive");
    hipLaunchKernelGGL(pgo_weights_kernel, dim3(pgo_grid(nfac, 256)), dim3(256), 0, (hipStream_t)stream, nfac, d_E, mu, barc2, d_known, d_w);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_pgo_trace(int32_t *h_out, int64_t cap, int64_t *h_count) {
    ARG_CHECK(h_count, "cslam_pgo_trace: NULL count");
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    *h_count = (int64_t)g_pgo.trace.size();
    for (int64_t k = 0; h_out && k < cap && k < *h_count; ++k) h_out[k] = g_pgo.trace[k];
    return CSLAM_OK;
}

CSLAM_API int cslam_pgo_optimize(int64_t n, int64_t nf, const int32_t *h_ei, const int32_t *h_ej, int64_t prior, double *h_poses,
                                 const double *h_meas, const double *h_sigmas, const uint8_t *h_known, const double *h_params,
                                 double *h_weights, double *h_info) {
    ARG_CHECK(h_poses && h_meas && h_sigmas && h_weights && h_info, "cslam_pgo_optimize: NULL argument");
    ARG_CHECK((h_ei && h_ej) || nf == 0, "cslam_pgo_optimize: NULL edge arrays");
    ARG_CHECK(n >= 1 && nf >= 0, "cslam_pgo_optimize: n < 1 or nf < 0");
    const int64_t nfac = nf + 1;
    for (int64_t k = 0; k < nfac * 6; ++k) ARG_CHECK(h_sigmas[k] > 0.0 && h_sigmas[k] < INFINITY, "cslam_pgo_optimize: sigmas must be positive and finite");
    PgoParams P;
    if (h_params) {
        P.lambda0 = h_params[0]; P.factor = h_params[1]; P.lambda_max = h_params[2]; P.max_iter = (int)h_params[3];
        P.rel_tol = h_params[4]; P.abs_tol = h_params[5]; P.fidelity = h_params[6]; P.gnc_max_rounds = (int)h_params[7];
        P.mu_step = h_params[8]; P.gnc_cost_tol = h_params[9]; P.weights_tol = h_params[10]; P.barc2 = h_params[11];
        ARG_CHECK(P.lambda0 > 0.0 && P.factor > 1.0 && P.lambda_max >= P.lambda0 && P.max_iter >= 0 && P.gnc_max_rounds >= 0 && P.mu_step > 1.0 &&
                  P.barc2 > 0.0, "cslam_pgo_optimize: parameters out of range");
    }
    std::lock_guard<std::mutex> lock(g_pgo_mu);
    hipStream_t st = nullptr;
    int rc = pgo_set_plan(n, nf, h_ei, h_ej, prior, st);
    if (rc) return rc;
    PgoWs &w = g_pgo;
    w.trace.clear();
    // poses, trial poses, measurements, sigmas, weights, the mask
    const size_t b_pose = ((size_t)n * 16 * 8 + 255) & ~(size_t)255, b_meas = ((size_t)nfac * 16 * 8 + 255) & ~(size_t)255,
                 b_sig = ((size_t)nfac * 6 * 8 + 255) & ~(size_t)255, b_w = ((size_t)nfac * 8 + 255) & ~(size_t)255,
                 b_known = ((size_t)nfac + 255) & ~(size_t)255;
    rc = w.io.ensure(2 * b_pose + b_meas + b_sig + b_w + b_known);
    if (rc) return rc;
    char *base = (char *)w.io.p;
    double *d_x = (double *)base, *d_try = (double *)(base + b_pose), *d_meas = (double *)(base + 2 * b_pose),
           *d_sig = (double *)(base + 2 * b_pose + b_meas), *d_w = (double *)(base + 2 * b_pose + b_meas + b_sig);
    uint8_t *d_known = h_known ? (uint8_t *)(base + 2 * b_pose + b_meas + b_sig + b_w) : nullptr;
    HIP_TRY(hipMemcpyAsync(d_x, h_poses, (size_t)n * 16 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_meas, h_meas, (size_t)nfac * 16 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_sig, h_sigmas, (size_t)nfac * 6 * 8, hipMemcpyHostToDevice, st));
    if (h_known) HIP_TRY(hipMemcpyAsync(d_known, h_known, (size_t)nfac, hipMemcpyHostToDevice, st));
    std::vector<double> hw(nfac, 1.0), hE(nfac);
    HIP_TRY(hipMemcpyAsync(d_w, hw.data(), (size_t)nfac * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));

    PgoCounters cnt;
    double cost = 0.0;
    int rounds = 0;
    rc = pgo_lm(P, d_x, d_try, d_meas, d_sig, d_w, &cost, &cnt, st);
    if (rc) return rc;
    // mu_0 from the largest residual of the free factors (w.E holds E at the result: pgo_lm ends on an evaluation of it)
    rc = pgo_linearize(d_x, d_meas, d_sig, nullptr, w.E, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(hE.data(), w.E, (size_t)nfac * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double r = -1.0;
    for (int64_t k = 0; k < nfac; ++k)
        if (!(h_known && h_known[k])) r = std::max(r, hE[k] / P.barc2);
    if (r >= 0.0 && 2.0 * r - 1.0 > 0.0) {
        double mu = std::max(1.0 / (2.0 * r - 1.0), P.mu_floor), prev = cost;
        for (int round = 0; round < P.gnc_max_rounds; ++round) {
            rc = pgo_linearize(d_x, d_meas, d_sig, nullptr, w.E, st);
            if (rc) return rc;
            hipLaunchKernelGGL(pgo_weights_kernel, dim3(pgo_grid(nfac, 256)), dim3(256), 0, st, nfac, w.E, mu, P.barc2, d_known, d_w);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(hw.data(), d_w, (size_t)nfac * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            rc = pgo_lm(P, d_x, d_try, d_meas, d_sig, d_w, &cost, &cnt, st);
            if (rc) return rc;
            ++rounds;
            bool binary = true;
            for (int64_t k = 0; k < nfac; ++k) binary = binary && (fabs(hw[k]) <= P.weights_tol || fabs(hw[k] - 1.0) <= P.weights_tol);
            if (binary) break;
            if (fabs(cost - prev) / std::max(prev, 1e-7) < P.gnc_cost_tol) break;
            prev = cost;
            mu *= P.mu_step;
        }
    }
    HIP_TRY(hipMemcpyAsync(h_poses, d_x, (size_t)n * 16 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t k = 0; k < nfac; ++k) h_weights[k] = hw[k];
    h_info[0] = (double)rounds; h_info[1] = (double)cnt.lm_iterations; h_info[2] = (double)cnt.solves; h_info[3] = cost;
    h_info[4] = cnt.lambda; h_info[5] = (double)cnt.status; h_info[6] = (double)w.plan.J(); h_info[7] = (double)w.plan.S();
    return CSLAM_OK;
}
