// SE(3) in float64 for the pose-graph back end (pgo.hip), shared by the kernels and the host tests (compiled for the host
// with __host__ / __device__ defined away, as horn.h and plane.h are).
//   tangent order   GTSAM's Pose3: xi = [omega, v], rotation first
//   pose            R [9] row-major and t [3]; poses in memory are 4 x 4 row-major (16 doubles)
//   retraction      T <- T . Exp(delta)                              (full SE(3) exponential, Pose3::Expmap)
//   Jr_inv          inverse right Jacobian of SE(3) (Pose3::LogmapDerivative), closed form with Barfoot's Q matrix
//                   (State Estimation for Robotics, eq. 7.86), Jr_inv(xi) = Jl_inv(-xi)
// Every coefficient has a closed form that cancels near theta = 0; below POSE_SERIES_THETA the Taylor series through
// theta^4 is taken instead (truncation theta^6 / 362880 < 3e-18 at the threshold; the closed forms lose about
// eps / theta^k there, which the theta^k of the matrix power they multiply gives back).
#pragma once
#include <math.h>

#ifndef POSE_HD
#define POSE_HD __host__ __device__ static inline
#endif

#define POSE_SERIES_THETA 1e-2      // below: Taylor series of the trigonometric coefficients
#define POSE_LOG_SMALL_SIN 1e-10    // |vector part| of the unit quaternion below which theta / sin(theta / 2) is taken as 2

POSE_HD void pose_m3_mul(const double *A, const double *B, double *C) {         // C = A B (C distinct from A, B)
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
POSE_HD void pose_m3_mul_tn(const double *A, const double *B, double *C) {      // C = A^T B
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
POSE_HD void pose_m3_vec(const double *A, const double *x, double *y) {
    for (int r = 0; r < 3; ++r) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
POSE_HD void pose_skew(const double *w, double *W) {
    W[0] = 0.0; W[1] = -w[2]; W[2] = w[1];
    W[3] = w[2]; W[4] = 0.0; W[5] = -w[0];
    W[6] = -w[1]; W[7] = w[0]; W[8] = 0.0;
}

// coefficients of theta (th2 = theta^2):
//   a = sin t / t               b = (1 - cos t) / t^2            c = (t - sin t) / t^3
//   d = 1/t^2 - (1 + cos t) / (2 t sin t)                        (inverse Jacobian of SO(3): I -+ W/2 + d W^2)
//   q2 = (t^2/2 + cos t - 1) / t^4                               q3 = (2t + t cos t - 3 sin t) / (2 t^5)
struct PoseCoef { double a, b, c, d, q2, q3; };
POSE_HD PoseCoef pose_coef(double th2) {
    PoseCoef k;
    if (th2 < POSE_SERIES_THETA * POSE_SERIES_THETA) {
        const double t4 = th2 * th2;
        k.a = 1.0 - th2 / 6.0 + t4 / 120.0;
        k.b = 0.5 - th2 / 24.0 + t4 / 720.0;
        k.c = 1.0 / 6.0 - th2 / 120.0 + t4 / 5040.0;
        k.d = 1.0 / 12.0 + th2 / 720.0 + t4 / 30240.0;
        k.q2 = 1.0 / 24.0 - th2 / 720.0 + t4 / 40320.0;
        k.q3 = 1.0 / 120.0 - th2 / 2520.0 + t4 / 120960.0;
    } else {
        const double t = sqrt(th2), s = sin(t), c = cos(t);
        // 1 - cos t as 2 sin^2(t / 2): no cancellation at any angle
        const double sh = sin(0.5 * t), omc = 2.0 * sh * sh;
        k.a = s / t;
        k.b = omc / th2;
        k.c = (t - s) / (th2 * t);
        // (1 + cos t) / sin t = cot(t / 2) = cos(t / 2) / sin(t / 2): finite up to and at pi
        k.d = (1.0 - 0.5 * t * cos(0.5 * t) / sh) / th2;
        k.q2 = (0.5 * th2 - omc) / (th2 * th2);
        k.q3 = (2.0 * t + t * c - 3.0 * s) / (2.0 * th2 * th2 * t);
    }
    return k;
}

// Exp: R = I + a W + b W^2, t = (I + b W + c W^2) v
POSE_HD void se3_exp(const double *xi, double *R, double *t) {
    const double *w = xi, *v = xi + 3;
    const PoseCoef k = pose_coef(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double W[9], W2[9];
    pose_skew(w, W);
    pose_m3_mul(W, W, W2);
    double V[9];
    for (int e = 0; e < 9; ++e) {
        const double id = (e % 4 == 0) ? 1.0 : 0.0;
        R[e] = id + k.a * W[e] + k.b * W2[e];
        V[e] = id + k.b * W[e] + k.c * W2[e];
    }
    pose_m3_vec(V, v, t);
}

// Log of a rotation through the unit quaternion (Shepperd's branch on the largest of trace and diagonal): accurate at every
// angle, pi included, where acos of the trace loses half the digits
POSE_HD void so3_log(const double *R, double *w) {
    const double tr = R[0] + R[4] + R[8];
    double qw, qx, qy, qz;
    if (tr > 0.0) {
        const double s = 2.0 * sqrt(tr + 1.0);
        qw = 0.25 * s; qx = (R[7] - R[5]) / s; qy = (R[2] - R[6]) / s; qz = (R[3] - R[1]) / s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        qw = (R[7] - R[5]) / s; qx = 0.25 * s; qy = (R[1] + R[3]) / s; qz = (R[2] + R[6]) / s;
    } else if (R[4] >= R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        qw = (R[2] - R[6]) / s; qx = (R[1] + R[3]) / s; qy = 0.25 * s; qz = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        qw = (R[3] - R[1]) / s; qx = (R[2] + R[6]) / s; qy = (R[5] + R[7]) / s; qz = 0.25 * s;
    }
    if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    const double n = sqrt(qx * qx + qy * qy + qz * qz);
    const double f = n < POSE_LOG_SMALL_SIN ? 2.0 / qw : 2.0 * atan2(n, qw) / n;
    w[0] = f * qx; w[1] = f * qy; w[2] = f * qz;
}

// Log: omega = Log(R), v = (I - W/2 + d W^2) t
POSE_HD void se3_log(const double *R, const double *t, double *xi) {
    so3_log(R, xi);
    const PoseCoef k = pose_coef(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    double W[9], W2[9], Vi[9];
    pose_skew(xi, W);
    pose_m3_mul(W, W, W2);
    for (int e = 0; e < 9; ++e) Vi[e] = ((e % 4 == 0) ? 1.0 : 0.0) - 0.5 * W[e] + k.d * W2[e];
    pose_m3_vec(Vi, t, xi + 3);
}

POSE_HD void se3_inv(const double *R, const double *t, double *Ri, double *ti) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ri[3 * r + c] = R[3 * c + r];
    for (int r = 0; r < 3; ++r) ti[r] = -(Ri[3 * r] * t[0] + Ri[3 * r + 1] * t[1] + Ri[3 * r + 2] * t[2]);
}
// (Ra, ta)^-1 (Rb, tb)
POSE_HD void se3_between(const double *Ra, const double *ta, const double *Rb, const double *tb, double *R, double *t) {
    pose_m3_mul_tn(Ra, Rb, R);
    const double d[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
    for (int r = 0; r < 3; ++r) t[r] = Ra[r] * d[0] + Ra[3 + r] * d[1] + Ra[6 + r] * d[2];
}
POSE_HD void se3_mul(const double *Ra, const double *ta, const double *Rb, const double *tb, double *R, double *t) {
    pose_m3_mul(Ra, Rb, R);
    pose_m3_vec(Ra, tb, t);
    for (int r = 0; r < 3; ++r) t[r] += ta[r];
}

// Ad_T [36] row-major: [[R, 0], [[t]x R, R]]
POSE_HD void se3_adjoint(const double *R, const double *t, double *A) {
    double Tx[9], TR[9];
    pose_skew(t, Tx);
    pose_m3_mul(Tx, R, TR);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            A[6 * r + c] = R[3 * r + c];
            A[6 * r + 3 + c] = 0.0;
            A[6 * (r + 3) + c] = TR[3 * r + c];
            A[6 * (r + 3) + 3 + c] = R[3 * r + c];
        }
}

// Jr_inv(xi) [36] row-major = Jl_inv(-xi) = [[Ji, 0], [-Ji Q Ji, Ji]] with W = [-omega]x, V = [-v]x,
//   Ji = I - W/2 + d W^2
//   Q  = V/2 + c (WV + VW + WVW) + q2 (WWV + VWW - 3 WVW) + q3 (WVWW + WWVW)
POSE_HD void se3_jr_inv(const double *xi, double *J) {
    const double w[3] = {-xi[0], -xi[1], -xi[2]}, v[3] = {-xi[3], -xi[4], -xi[5]};
    const PoseCoef k = pose_coef(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double W[9], V[9], W2[9], WV[9], VW[9], WVW[9], WWV[9], VWW[9], WVWW[9], WWVW[9], Ji[9], Q[9], T1[9], T2[9];
    pose_skew(w, W);
    pose_skew(v, V);
    pose_m3_mul(W, W, W2);
    pose_m3_mul(W, V, WV);
    pose_m3_mul(V, W, VW);
    pose_m3_mul(WV, W, WVW);
    pose_m3_mul(W, WV, WWV);
    pose_m3_mul(VW, W, VWW);
    pose_m3_mul(WVW, W, WVWW);
    pose_m3_mul(W, WVW, WWVW);
    for (int e = 0; e < 9; ++e) {
        Ji[e] = ((e % 4 == 0) ? 1.0 : 0.0) - 0.5 * W[e] + k.d * W2[e];
        Q[e] = 0.5 * V[e] + k.c * (WV[e] + VW[e] + WVW[e]) + k.q2 * (WWV[e] + VWW[e] - 3.0 * WVW[e]) + k.q3 * (WVWW[e] + WWVW[e]);
    }
    pose_m3_mul(Ji, Q, T1);
    pose_m3_mul(T1, Ji, T2);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            J[6 * r + c] = Ji[3 * r + c];
            J[6 * r + 3 + c] = 0.0;
            J[6 * (r + 3) + c] = -T2[3 * r + c];
            J[6 * (r + 3) + 3 + c] = Ji[3 * r + c];
        }
}

// 4 x 4 row-major <-> (R, t)
POSE_HD void pose_load(const double *T, double *R, double *t) {
    for (int r = 0; r < 3; ++r) {
        R[3 * r] = T[4 * r]; R[3 * r + 1] = T[4 * r + 1]; R[3 * r + 2] = T[4 * r + 2];
        t[r] = T[4 * r + 3];
    }
}
POSE_HD void pose_store(const double *R, const double *t, double *T) {
    for (int r = 0; r < 3; ++r) {
        T[4 * r] = R[3 * r]; T[4 * r + 1] = R[3 * r + 1]; T[4 * r + 2] = R[3 * r + 2];
        T[4 * r + 3] = t[r];
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

// One factor of the pose graph: e = Log(Z^-1 Ti^-1 Tj) with Aj = Jr_inv(e), Ai = -Jr_inv(e) Ad(h^-1), h = Ti^-1 Tj
// (the prior: Ti = identity, only Aj).  e [6], Ai / Aj [36] row-major (either may be NULL).
POSE_HD void pgo_between_residual(const double *Ti, const double *Tj, const double *Z, double *e, double *Ai, double *Aj) {
    double Rj[9], tj[3], Rz[9], tz[3], Rh[9], th[3], Re[9], te[3];
    pose_load(Tj, Rj, tj);
    pose_load(Z, Rz, tz);
    if (Ti) {
        double Ri[9], ti[3];
        pose_load(Ti, Ri, ti);
        se3_between(Ri, ti, Rj, tj, Rh, th);
    } else {
        for (int k = 0; k < 9; ++k) Rh[k] = Rj[k];
        for (int k = 0; k < 3; ++k) th[k] = tj[k];
    }
    se3_between(Rz, tz, Rh, th, Re, te);
    se3_log(Re, te, e);
    if (!Aj && !Ai) return;
    double J[36];
    se3_jr_inv(e, J);
    if (Aj) for (int k = 0; k < 36; ++k) Aj[k] = J[k];
    if (Ai) {
        double Rhi[9], thi[3], Ad[36];
        se3_inv(Rh, th, Rhi, thi);
        se3_adjoint(Rhi, thi, Ad);
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                double s = 0.0;
                for (int q = 0; q < 6; ++q) s += J[6 * r + q] * Ad[6 * q + c];
                Ai[6 * r + c] = -s;
            }
    }
}
