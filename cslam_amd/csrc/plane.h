// plane.h -- the point-to-plane update of icp.hip (open3d's TransformationEstimationPointToPlane), float64 throughout.
//
// For the kept correspondences of a round (p = T . src_i, q its nearest target point, n the target's normal at q):
//   r = (p - q) . n,   J = [(p - o) x n, n] (six entries),   A = sum J J^T,   b = sum J r,   x = -A^-1 b,
// o the pair's sum origin (horn.h icp_sum_origin: zero for clouds around the frame origin, where the sums are open3d's as
// written).  The cross product is taken relative to o because p x n of frame coordinates far from the origin couples the
// rotation and the translation columns of A: condition 2.8e3 at the origin and 7.8e18 for the same clouds moved by
// (2^17, -2^16, 1024) m.  det A does not change with o, so the determinant test below is the same test in both frames.
//
// The 29 sums: s[0] = n, s[1] = sum d^2, s[2 .. 22] = the upper triangle of A row by row, s[23 .. 28] = b.
//
// Solve: an unpivoted LDL^T of the symmetric 6 x 6, det A = the product of D.  The update is the IDENTITY when
//   * fewer than six correspondences were kept (A has rank < 6: det A is 0 in exact arithmetic, and the factorisation of a
//     rank-deficient A would end in rounding noise; answered directly, as horn.h answers one correspondence itself),
//   * a pivot is exactly 0, or det A is NaN, infinite or |det A| < 1e-6 (the determinant check of open3d's
//     SolveLinearSystemPSD, restated from memory: parity with open3d is not pinned),
//   * or the solution has a non-finite entry.
// The threshold is ABSOLUTE, as open3d's is: a scene with ONE sliding direction (two plane families that share a line) has
// a computed determinant far above it and takes whatever step the solve gives.  That is open3d's behaviour and it is kept.
//
// Compose: U' = (Rz(x2) . Ry(x1) . Rx(x0), (x3, x4, x5)) (open3d's TransformVector6dToMatrix4d) acts on coordinates relative
// to o; in the frame the translation is t = t' + o - R o.
#pragma once

#define ICP_PLANE_NSUM 29
#define ICP_PLANE_MIN_DET 1e-6

__host__ __device__ static bool icp_plane_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// The 29 terms of one kept correspondence: ps = p - o, dq = p - q, nr the normal at q, d2 = |p - q|^2 as the search gave it.
__host__ __device__ static void icp_plane_terms(const double *ps, const double *dq, const double *nr, double d2, double *v) {
    double J[6];
    J[0] = ps[1] * nr[2] - ps[2] * nr[1];
    J[1] = ps[2] * nr[0] - ps[0] * nr[2];
    J[2] = ps[0] * nr[1] - ps[1] * nr[0];
    J[3] = nr[0]; J[4] = nr[1]; J[5] = nr[2];
    const double r = dq[0] * nr[0] + dq[1] * nr[1] + dq[2] * nr[2];
    v[0] = 1.0;
    v[1] = d2;
    int k = 2;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) v[k++] = J[i] * J[j];
    for (int i = 0; i < 6; ++i) v[23 + i] = J[i] * r;
}

// x = -A^-1 b from the 29 sums; *det = det A as computed (0 for fewer than six correspondences or a zero pivot).  False,
// and x = 0, where the rule above says identity.
__host__ __device__ static bool icp_plane_solve(const double *s, double *x, double *det) {
    double A[6][6], L[6][6], D[6];
    for (int i = 0; i < 6; ++i) x[i] = 0.0;
    *det = 0.0;
    if (!(s[0] >= 6.0)) return false;
    int k = 2;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = s[k++];
    double prod = 1.0;
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int m = 0; m < j; ++m) d -= L[j][m] * L[j][m] * D[m];
        if (d == 0.0) return false;
        D[j] = d;
        prod *= d;
        for (int i = j + 1; i < 6; ++i) {
            double a = A[i][j];
            for (int m = 0; m < j; ++m) a -= L[i][m] * L[j][m] * D[m];
            L[i][j] = a / d;
        }
    }
    *det = prod;
    if (!icp_plane_finite(prod) || fabs(prod) < ICP_PLANE_MIN_DET) return false;
    double y[6];
    for (int i = 0; i < 6; ++i) {                                // L y = -b
        double a = -s[23 + i];
        for (int m = 0; m < i; ++m) a -= L[i][m] * y[m];
        y[i] = a;
    }
    for (int i = 0; i < 6; ++i) y[i] /= D[i];
    for (int i = 5; i >= 0; --i) {                               // L^T x = y
        double a = y[i];
        for (int m = i + 1; m < 6; ++m) a -= L[m][i] * x[m];
        x[i] = a;
    }
    bool ok = true;
    for (int i = 0; i < 6; ++i) ok = ok && icp_plane_finite(x[i]);
    if (!ok)
        for (int i = 0; i < 6; ++i) x[i] = 0.0;
    return ok;
}

// U' (3 x 4, row-major) of the six-vector: rotation Rz(x2) . Ry(x1) . Rx(x0), translation (x3, x4, x5).
__host__ __device__ static void icp_plane_vector_to_matrix(const double *x, double *U) {
    const double sx = sin(x[0]), cx = cos(x[0]), sy = sin(x[1]), cy = cos(x[1]), sz = sin(x[2]), cz = cos(x[2]);
    U[0] = cz * cy; U[1] = cz * sy * sx - sz * cx; U[2] = cz * sy * cx + sz * sx; U[3] = x[3];
    U[4] = sz * cy; U[5] = sz * sy * sx + cz * cx; U[6] = sz * sy * cx - cz * sx; U[7] = x[4];
    U[8] = -sy;     U[9] = cy * sx;                U[10] = cy * cx;               U[11] = x[5];
}

// The update U (3 x 4, row-major, frame coordinates) from sums taken relative to o.  False, and U = the identity, where the
// rule says so.
__host__ __device__ static bool icp_plane_update_from_shifted_sums(const double *s, const double *o, double *U) {
    double x[6], det;
    if (!icp_plane_solve(s, x, &det)) {
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 4; ++b) U[4 * a + b] = a == b ? 1.0 : 0.0;
        return false;
    }
    icp_plane_vector_to_matrix(x, U);
    if (o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0) return true;
    for (int a = 0; a < 3; ++a) U[4 * a + 3] += o[a] - (U[4 * a] * o[0] + U[4 * a + 1] * o[1] + U[4 * a + 2] * o[2]);
    return true;
}
