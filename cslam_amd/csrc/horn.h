// horn.h -- the rigid fit without scale shared by icp.hip (every ICP update) and robust.hip (the rotation of the robust fit).
//
// Accuracy.  icp_rigid_from_sums forms the covariance from UNCENTRED sums, (sum q p^T - sum q . mean p) / n, which loses
// (|mean| / spread)^2 of the float64 precision.  It is therefore fed coordinates relative to an origin near the clouds:
// icp.hip takes its sums relative to icp_sum_origin(first target point of the pair) and calls icp_rigid_from_shifted_sums,
// which fits the shifted sets and moves the translation back.  With that the moved points are within a few ulp of the
// largest input coordinate of the centred extended-precision fit for clouds of lidar size (a few hundred metres) anywhere
// float64 represents them to the millimetre (tested to 2^20 m); robust.hip passes differences of points and zero means,
// which no origin enters.
#pragma once

// The origin of a pair's sums: its first target point rounded to the multiples of ICP_ORIGIN_GRID per axis.  It depends on
// the pair alone (so do the sums: alone or in any batch, the same bits), it is exact in float64, and it is zero for a
// cloud that starts within half a grid step of the frame origin: sensor-frame clouds are summed as they are.
#define ICP_ORIGIN_GRID 1024.0
__host__ __device__ static void icp_sum_origin(const double *q0, double *o) {
    for (int a = 0; a < 3; ++a) o[a] = ICP_ORIGIN_GRID * rint(q0[a] / ICP_ORIGIN_GRID);
}

// Rigid update without scale from the 17 sums: U (3 x 4, row-major) with q ~ R p + t in the least-squares sense.
// Horn's closed form: the unit quaternion of R is the eigenvector of the largest eigenvalue of the symmetric 4 x 4
// N(M), M = sum (p - mean p)(q - mean q)^T.  A zero M leaves the Jacobi basis at the identity and the first largest
// eigenvalue picks q = (1, 0, 0, 0): R = I, as the SVD form gives.  The M of ONE correspondence is zero only where the
// difference below is not contracted: the device build fuses it, keeps the rounding error of q p and turns that noise into
// a rotation.  icp_rigid_from_shifted_sums therefore answers one correspondence itself.
__host__ __device__ static void icp_rigid_from_sums(const double *s, double *U) {
    const double n = s[0];
    double mp[3], mq[3], M[3][3];
    for (int a = 0; a < 3; ++a) { mp[a] = s[1 + a] / n; mq[a] = s[4 + a] / n; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[a][b] = (s[7 + 3 * b + a] - s[4 + b] * mp[a]) / n;
    double A[4][4], V[4][4];
    A[0][0] = M[0][0] + M[1][1] + M[2][2];
    A[1][1] = M[0][0] - M[1][1] - M[2][2];
    A[2][2] = -M[0][0] + M[1][1] - M[2][2];
    A[3][3] = -M[0][0] - M[1][1] + M[2][2];
    A[0][1] = A[1][0] = M[1][2] - M[2][1];
    A[0][2] = A[2][0] = M[2][0] - M[0][2];
    A[0][3] = A[3][0] = M[0][1] - M[1][0];
    A[1][2] = A[2][1] = M[0][1] + M[1][0];
    A[1][3] = A[3][1] = M[2][0] + M[0][2];
    A[2][3] = A[3][2] = M[1][2] + M[2][1];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 4; ++i) {
            diag += A[i][i] * A[i][i];
            for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
        }
        if (off <= 1e-34 * diag || off == 0.0) break;
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 4; ++j) {
                const double aij = A[i][j];
                if (aij == 0.0) continue;
                const double theta = (A[j][j] - A[i][i]) / (2.0 * aij);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
                for (int k = 0; k < 4; ++k) {               // A <- A J  (columns i, j)
                    const double aki = A[k][i], akj = A[k][j];
                    A[k][i] = c * aki - sn * akj;
                    A[k][j] = sn * aki + c * akj;
                }
                for (int k = 0; k < 4; ++k) {               // A <- J^T A (rows i, j)
                    const double aik = A[i][k], ajk = A[j][k];
                    A[i][k] = c * aik - sn * ajk;
                    A[j][k] = sn * aik + c * ajk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vki = V[k][i], vkj = V[k][j];
                    V[k][i] = c * vki - sn * vkj;
                    V[k][j] = sn * vki + c * vkj;
                }
            }
    }
    int best = 0;
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > A[best][best]) best = k;
    double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
    const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= inv; x *= inv; y *= inv; z *= inv;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - w * z); R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z); R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y); R[2][1] = 2.0 * (y * z + w * x); R[2][2] = 1.0 - 2.0 * (x * x + y * y);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) U[4 * a + b] = R[a][b];
        U[4 * a + 3] = mq[a] - (R[a][0] * mp[0] + R[a][1] * mp[1] + R[a][2] * mp[2]);
    }
}

// The same from sums of (p - o) and (q - o): the fit of the shifted sets is U' = (R, t'), and q ~ R p + t' + o - R o.
// One correspondence: R = I exactly and t = q - p.
__host__ __device__ static void icp_rigid_from_shifted_sums(const double *s, const double *o, double *U) {
    if (s[0] == 1.0) {
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) U[4 * a + b] = a == b ? 1.0 : 0.0;
            U[4 * a + 3] = s[4 + a] - s[1 + a];
        }
        return;
    }
    icp_rigid_from_sums(s, U);
    if (o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0) return;
    for (int a = 0; a < 3; ++a) U[4 * a + 3] += o[a] - (U[4 * a] * o[0] + U[4 * a + 1] * o[1] + U[4 * a + 2] * o[2]);
}
