// pnp.h -- 3D -> 2D pose from point correspondences in float64, shared by the kernels of vis.hip and the host tests
// (compiled for the host with __host__ / __device__ defined away, as horn.h, plane.h and pose.h are).
//
// Convention: T = (R, t) maps points of the "from" camera frame into the "to" camera frame.  The 3D points come from
// "from", the pixels and the intrinsics cam = (fx, fy, cx, cy) from "to": pinhole, rectified, no distortion.
//
//   sampler     pnp_sample(seed, h, M, idx): slot j of hypothesis h = splitmix64(splitmix64(seed) + (h << 6 | j << 4 | a))
//               mod M with attempt a = 0; re-drawn with a + 1 while it repeats an earlier slot; after 16 attempts the lowest
//               index no earlier slot holds.  Integer only, no state, nothing about the pair's place in a batch.
//   P3P         Lambda Twist (Persson and Nordberg, ECCV 2018): the distances l1, l2, l3 along the three unit bearings obey
//               li^2 + lj^2 + bij li lj = aij (bij = -2 yi.yj, aij = |xi - xj|^2).  With D1 = a23 M12 - a12 M23 and
//               D2 = a23 M13 - a13 M23 both quadratic forms vanish at the solution; g is a real root of
//               det(D1 - g D2) = 0 (Newton on the monic cubic from a start left or right of its stationary points), so that
//               A = D1 - g D2 has rank 2: A = L0 v0 v0^T + L1 v1 v1^T with L0 >= 0 >= L1 is a pair of planes
//               v0.l = +- s v1.l, s = sqrt(-L1 / L0).  Each plane gives l1 = w0 l2 + w1 l3, a quadratic in tau = l3 / l2
//               from a13 eq12 - a12 eq13 and l2 from eq23.  Roots with tau > 0 and l1 >= 0 are kept, polished by
//               PNP_P3P_POLISH Gauss-Newton steps on the three equations, and turned into (R, t) by
//               R [x1 - x2, x1 - x3, n] = [l1 y1 - l2 y2, l1 y1 - l3 y3, n'], t = l1 y1 - R x1.
//               Only + - * / and sqrt: host and device differ by contraction at most.  Collinear or coincident points
//               (|d12 x d13|^2 <= PNP_COLLINEAR a12 a13) give 0 roots; a root with a non-finite entry is dropped.
//   selection   pnp_select: the root with the smallest squared reprojection error of a fourth correspondence (infinite where
//               its depth is not positive); the lowest root index wins ties.
//   inlier      depth > 0 and squared pixel error <= reproj_error^2.
//   refinement  left perturbation T <- Exp(delta) T through se3_exp of pose.h, delta = [omega, v]:
//               J = Jpi [-[p]x, I] (2 x 6), r = projection - pixel; the 27 sums s[0 .. 20] = upper triangle of sum J^T J row
//               by row, s[21 .. 26] = sum J^T r; delta = -A^-1 b by an unpivoted LDL^T.  The 6 x 6 solve of plane.h does not
//               fit: it wants six correspondences and tests det A against an ABSOLUTE 1e-6, which in pixel units (entries
//               of A near 1e5) the rounding noise of a rank-deficient A exceeds by many orders.  Here: singular, and
//               delta = 0, where a pivot is not above PNP_PIVOT_REL times its diagonal entry or anything is non-finite.
//   levels      the level-aware form (keypoints of a scale pyramid): sigma2[l] = (double)36^l / (double)25^l for l = 0 .. 7,
//               exact integers and one division.  A correspondence whose "to" keypoint has level l is an inlier iff its depth
//               is positive and e2 <= thr2 sigma2[l], in hypothesis scoring, in the inlier set of the best hypothesis and in
//               every recount; each of its 27 Gauss-Newton terms is multiplied by 1 / sigma2[l].  Sampler, P3P, selection
//               by the fourth point, the best key, the stopping rule and the status rules are those above.
#pragma once
#include <math.h>
#include <stdint.h>
#include "pose.h"

#ifndef PNP_HD
#define PNP_HD __host__ __device__ static inline
#endif

#define PNP_SAMPLE_ATTEMPTS 16
#define PNP_P3P_NEWTON 50          // most Newton steps on the cubic
#define PNP_P3P_POLISH 3           // Gauss-Newton steps on the three distance equations per root
#define PNP_COLLINEAR 1e-20        // |d12 x d13|^2 <= this * a12 * a13: no solution attempted
#define PNP_PIVOT_REL 1e-11        // an LDL^T pivot at or below this share of its diagonal entry: singular
#define PNP_NSUM 27
#define PNP_MAX_LEVEL 7

PNP_HD bool pnp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

PNP_HD uint64_t pnp_mix64(uint64_t z) {                    // splitmix64's output function after its increment
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// four distinct indices in [0, M), M >= 4
PNP_HD void pnp_sample(uint64_t seed, uint32_t h, int M, int *idx) {
    const uint64_t s = pnp_mix64(seed);
    for (int j = 0; j < 4; ++j) {
        int pick = -1;
        for (int a = 0; a < PNP_SAMPLE_ATTEMPTS && pick < 0; ++a) {
            const int c = (int)(pnp_mix64(s + (((uint64_t)h << 6) | ((uint64_t)j << 4) | (uint64_t)a)) % (uint64_t)M);
            bool rep = false;
            for (int q = 0; q < j; ++q) rep = rep || idx[q] == c;
            if (!rep) pick = c;
        }
        for (int c = 0; pick < 0; ++c) {                   // the lowest unused index
            bool rep = false;
            for (int q = 0; q < j; ++q) rep = rep || idx[q] == c;
            if (!rep) pick = c;
        }
        idx[j] = pick;
    }
}

PNP_HD void pnp_cross(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
PNP_HD double pnp_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// symmetric 3 x 3 as (m00, m01, m02, m11, m12, m22): its adjugate in the same order, and its determinant
PNP_HD void pnp_sym_adj(const double *m, double *a) {
    a[0] = m[3] * m[5] - m[4] * m[4];
    a[1] = m[2] * m[4] - m[1] * m[5];
    a[2] = m[1] * m[4] - m[2] * m[3];
    a[3] = m[0] * m[5] - m[2] * m[2];
    a[4] = m[1] * m[2] - m[0] * m[4];
    a[5] = m[0] * m[3] - m[1] * m[1];
}
PNP_HD double pnp_sym_trace_prod(const double *a, const double *b) {    // trace(A B) of two symmetric matrices
    return a[0] * b[0] + a[3] * b[3] + a[5] * b[5] + 2.0 * (a[1] * b[1] + a[2] * b[2] + a[4] * b[4]);
}

// a real root of r^3 + b r^2 + c r + d
PNP_HD double pnp_cubic_root(double b, double c, double d) {
    double r;
    const double disc = b * b - 3.0 * c;
    if (disc >= 0.0) {                                     // two stationary points t1 <= t2
        const double v = sqrt(disc), t1 = (-b - v) / 3.0;
        double k = ((t1 + b) * t1 + c) * t1 + d;
        if (k > 0.0) {
            r = t1 - sqrt(-k / (3.0 * t1 + b));            // the root left of t1; h'' (t1) = 2 (3 t1 + b) <= 0
        } else {
            const double t2 = (-b + v) / 3.0;
            k = ((t2 + b) * t2 + c) * t2 + d;
            r = k < 0.0 ? t2 + sqrt(-k / (3.0 * t2 + b)) : -b / 3.0;
        }
        if (!pnp_finite(r)) r = -b / 3.0;
    } else {
        r = -b / 3.0;
        if (fabs((3.0 * r + 2.0 * b) * r + c) < 1e-4) r += 1.0;
    }
    for (int it = 0; it < PNP_P3P_NEWTON; ++it) {
        const double fx = ((r + b) * r + c) * r + d, fpx = (3.0 * r + 2.0 * b) * r + c;
        if (fx == 0.0 || fpx == 0.0) break;
        const double step = fx / fpx;
        if (!pnp_finite(step)) break;
        r -= step;
        if (fabs(step) <= 1e-15 * fabs(r)) break;
    }
    return r;
}

// unit eigenvector of the symmetric m (order as above) for the eigenvalue lam: the largest cross product of two rows of
// m - lam I.  False when all three vanish.
PNP_HD bool pnp_eigvec(const double *m, double lam, double *v) {
    const double r0[3] = {m[0] - lam, m[1], m[2]}, r1[3] = {m[1], m[3] - lam, m[4]}, r2[3] = {m[2], m[4], m[5] - lam};
    double c0[3], c1[3], c2[3];
    pnp_cross(r0, r1, c0);
    pnp_cross(r0, r2, c1);
    pnp_cross(r1, r2, c2);
    const double n0 = pnp_dot(c0, c0), n1 = pnp_dot(c1, c1), n2 = pnp_dot(c2, c2);
    const double *c = c0;
    double n = n0;
    if (n1 > n) { c = c1; n = n1; }
    if (n2 > n) { c = c2; n = n2; }
    if (!(n > 0.0) || !pnp_finite(n)) return false;
    const double s = 1.0 / sqrt(n);
    v[0] = c[0] * s; v[1] = c[1] * s; v[2] = c[2] * s;
    return true;
}

// Three correspondences: X [9] the 3D points row by row, Yb [9] their bearings (any positive length; normalised here).
// Up to four (R [9] row-major, t [3]) to Rs [36], ts [12]; returns their number.
PNP_HD int pnp_p3p(const double *X, const double *Yb, double *Rs, double *ts) {
    double y[9];
    for (int i = 0; i < 3; ++i) {
        const double n = sqrt(pnp_dot(Yb + 3 * i, Yb + 3 * i));
        if (!(n > 0.0) || !pnp_finite(n)) return 0;
        for (int a = 0; a < 3; ++a) y[3 * i + a] = Yb[3 * i + a] / n;
    }
    double d12[3], d13[3], d23[3], nx[3];
    for (int a = 0; a < 3; ++a) { d12[a] = X[a] - X[3 + a]; d13[a] = X[a] - X[6 + a]; d23[a] = X[3 + a] - X[6 + a]; }
    pnp_cross(d12, d13, nx);
    const double a12 = pnp_dot(d12, d12), a13 = pnp_dot(d13, d13), a23 = pnp_dot(d23, d23), nn = pnp_dot(nx, nx);
    if (!pnp_finite(a12) || !pnp_finite(a13) || !pnp_finite(a23) || !pnp_finite(nn)) return 0;
    if (!(nn > PNP_COLLINEAR * a12 * a13) || !(a23 > 0.0)) return 0;
    const double b12 = -2.0 * pnp_dot(y, y + 3), b13 = -2.0 * pnp_dot(y, y + 6), b23 = -2.0 * pnp_dot(y + 3, y + 6);
    // D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23
    const double D1[6] = {a23, 0.5 * a23 * b12, 0.0, a23 - a12, -0.5 * a12 * b23, -a12};
    const double D2[6] = {a23, 0.0, 0.5 * a23 * b13, -a13, -0.5 * a13 * b23, a23 - a13};
    double J1[6], J2[6];
    pnp_sym_adj(D1, J1);
    pnp_sym_adj(D2, J2);
    // det(D1 - g D2) = det D1 - g tr(adj(D1) D2) + g^2 tr(D1 adj(D2)) - g^3 det D2
    const double k0 = (D1[0] * J1[0] + D1[1] * J1[1] + D1[2] * J1[2]);
    const double k3 = -(D2[0] * J2[0] + D2[1] * J2[1] + D2[2] * J2[2]);
    const double k1 = -pnp_sym_trace_prod(J1, D2), k2 = pnp_sym_trace_prod(D1, J2);
    if (k3 == 0.0) return 0;
    const double g = pnp_cubic_root(k2 / k3, k1 / k3, k0 / k3);
    if (!pnp_finite(g)) return 0;
    double A[6];
    for (int e = 0; e < 6; ++e) A[e] = D1[e] - g * D2[e];
    // eigenvalues: 0 and the roots of L^2 - tr L + (sum of the principal 2 x 2 minors)
    const double tr = A[0] + A[3] + A[5];
    const double mn = (A[0] * A[3] - A[1] * A[1]) + (A[0] * A[5] - A[2] * A[2]) + (A[3] * A[5] - A[4] * A[4]);
    const double dq = tr * tr - 4.0 * mn;
    if (!(dq >= 0.0)) return 0;
    const double sq = sqrt(dq);
    // the root of larger magnitude first, the other from the product: no cancellation
    const double big = tr >= 0.0 ? 0.5 * (tr + sq) : 0.5 * (tr - sq);
    if (big == 0.0) return 0;
    const double small = mn / big;
    const double L0 = big > small ? big : small, L1 = big > small ? small : big;      // L0 >= L1
    if (!(L0 > 0.0)) return 0;
    double v0[3], v1[3];
    if (!pnp_eigvec(A, L0, v0) || !pnp_eigvec(A, L1, v1)) return 0;
    const double ratio = -L1 / L0;
    const double sv = ratio > 0.0 ? sqrt(ratio) : 0.0;
    double Ls[12];
    int nl = 0;
    for (int sgn = 0; sgn < 2; ++sgn) {
        const double s = sgn ? -sv : sv;
        const double w2 = 1.0 / (s * v1[0] - v0[0]);
        const double w0 = (v0[1] - s * v1[1]) * w2, w1 = (v0[2] - s * v1[2]) * w2;
        const double a = 1.0 / ((a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12);
        const double b = (a13 * b12 * w1 - a12 * b13 * w0 - 2.0 * w0 * w1 * (a12 - a13)) * a;
        const double c = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * a;
        const double disc = b * b - 4.0 * c;
        if (!(disc >= 0.0) || !pnp_finite(disc)) continue;
        const double q = sqrt(disc);
        const double r1 = b >= 0.0 ? 0.5 * (-b - q) : 0.5 * (-b + q);   // larger magnitude
        const double taus[2] = {r1, r1 != 0.0 ? c / r1 : 0.0};
        for (int k = 0; k < 2; ++k) {
            const double tau = taus[k];
            if (!(tau > 0.0)) continue;
            const double den = tau * (b23 + tau) + 1.0;
            if (!(den > 0.0)) continue;
            const double l2 = sqrt(a23 / den), l3 = tau * l2, l1 = w0 * l2 + w1 * l3;
            if (!(l1 >= 0.0) || nl >= 4) continue;
            Ls[3 * nl] = l1; Ls[3 * nl + 1] = l2; Ls[3 * nl + 2] = l3;
            ++nl;
        }
    }
    // X^-1 of X = [d12, d13, nx] (columns): rows (d13 x nx, nx x d12, nx) / nn
    double xi0[3], xi1[3];
    pnp_cross(d13, nx, xi0);
    pnp_cross(nx, d12, xi1);
    int nr = 0;
    for (int k = 0; k < nl; ++k) {
        double l[3] = {Ls[3 * k], Ls[3 * k + 1], Ls[3 * k + 2]};
        for (int it = 0; it < PNP_P3P_POLISH; ++it) {
            const double r[3] = {l[0] * l[0] + l[1] * l[1] + b12 * l[0] * l[1] - a12,
                                 l[0] * l[0] + l[2] * l[2] + b13 * l[0] * l[2] - a13,
                                 l[1] * l[1] + l[2] * l[2] + b23 * l[1] * l[2] - a23};
            const double j0[3] = {2.0 * l[0] + b12 * l[1], 2.0 * l[1] + b12 * l[0], 0.0};
            const double j1[3] = {2.0 * l[0] + b13 * l[2], 0.0, 2.0 * l[2] + b13 * l[0]};
            const double j2[3] = {0.0, 2.0 * l[1] + b23 * l[2], 2.0 * l[2] + b23 * l[1]};
            double c12[3], c20[3], c01[3];
            pnp_cross(j1, j2, c12);
            pnp_cross(j2, j0, c20);
            pnp_cross(j0, j1, c01);
            const double det = pnp_dot(j0, c12);
            if (det == 0.0 || !pnp_finite(det)) break;
            double nl3[3];
            bool ok = true;
            for (int a = 0; a < 3; ++a) {                  // J^-1 = [c12, c20, c01] (columns) / det
                nl3[a] = l[a] - (c12[a] * r[0] + c20[a] * r[1] + c01[a] * r[2]) / det;
                ok = ok && pnp_finite(nl3[a]);
            }
            if (!ok) break;
            for (int a = 0; a < 3; ++a) l[a] = nl3[a];
        }
        double yd1[3], yd2[3], ny[3];
        for (int a = 0; a < 3; ++a) { yd1[a] = l[0] * y[a] - l[1] * y[3 + a]; yd2[a] = l[0] * y[a] - l[2] * y[6 + a]; }
        pnp_cross(yd1, yd2, ny);
        double *R = Rs + 9 * nr, *t = ts + 3 * nr;
        bool ok = true;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                R[3 * r + c] = (yd1[r] * xi0[c] + yd2[r] * xi1[c] + ny[r] * nx[c]) / nn;
                ok = ok && pnp_finite(R[3 * r + c]);
            }
        for (int r = 0; r < 3; ++r) {
            t[r] = l[0] * y[r] - (R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2]);
            ok = ok && pnp_finite(t[r]);
        }
        if (ok) ++nr;
    }
    return nr;
}

// p = R x + t; the squared pixel error against (u, v); false (and *e2 = +inf) where the depth is not positive
PNP_HD bool pnp_reproject(const double *R, const double *t, const double *cam, const double *x, double u, double v, double *e2) {
    const double px = R[0] * x[0] + R[1] * x[1] + R[2] * x[2] + t[0];
    const double py = R[3] * x[0] + R[4] * x[1] + R[5] * x[2] + t[1];
    const double pz = R[6] * x[0] + R[7] * x[1] + R[8] * x[2] + t[2];
    if (!(pz > 0.0)) { *e2 = INFINITY; return false; }
    const double du = cam[0] * px / pz + cam[2] - u, dv = cam[1] * py / pz + cam[3] - v;
    *e2 = du * du + dv * dv;
    return true;
}
PNP_HD bool pnp_inlier(const double *R, const double *t, const double *cam, const double *x, double u, double v, double thr2) {
    double e2;
    return pnp_reproject(R, t, cam, x, u, v, &e2) && e2 <= thr2;
}

// sigma2 of level l in [0, PNP_MAX_LEVEL]: 36^l and 25^l are integers below 2^53
PNP_HD double pnp_level_sigma2(int l) {
    int64_t num = 1, den = 1;
    for (int i = 0; i < l; ++i) { num *= 36; den *= 25; }
    return (double)num / (double)den;
}
PNP_HD bool pnp_inlier_level(const double *R, const double *t, const double *cam, const double *x, double u, double v, double thr2,
                             double sigma2) {
    double e2;
    return pnp_reproject(R, t, cam, x, u, v, &e2) && e2 <= thr2 * sigma2;
}

// the root a fourth correspondence picks; -1 for n == 0
PNP_HD int pnp_select(int n, const double *Rs, const double *ts, const double *cam, const double *x4, double u4, double v4) {
    int best = -1;
    double be = INFINITY;
    for (int k = 0; k < n; ++k) {
        double e2;
        pnp_reproject(Rs + 9 * k, ts + 3 * k, cam, x4, u4, v4, &e2);
        if (best < 0 || e2 < be) { best = k; be = e2; }
    }
    return best;
}

// One hypothesis from four correspondences (X4 [12], pixels uv4 [8]): false when the minimal solver has no root.
PNP_HD bool pnp_hypothesis(const double *X4, const double *uv4, const double *cam, double *R, double *t) {
    double Yb[9], Rs[36], ts[12];
    for (int i = 0; i < 3; ++i) {
        Yb[3 * i] = (uv4[2 * i] - cam[2]) / cam[0];
        Yb[3 * i + 1] = (uv4[2 * i + 1] - cam[3]) / cam[1];
        Yb[3 * i + 2] = 1.0;
    }
    const int n = pnp_p3p(X4, Yb, Rs, ts);
    const int k = pnp_select(n, Rs, ts, cam, X4 + 9, uv4[6], uv4[7]);
    if (k < 0) return false;
    for (int e = 0; e < 9; ++e) R[e] = Rs[9 * k + e];
    for (int e = 0; e < 3; ++e) t[e] = ts[3 * k + e];
    return true;
}

// the rows Ju, Jv of J and the residual (ru, rv) of one correspondence; false where its depth under (R, t) is not positive
PNP_HD bool pnp_gn_rows(const double *R, const double *t, const double *cam, const double *x, double u, double v, double *Ju, double *Jv,
                        double *ru, double *rv) {
    const double px = R[0] * x[0] + R[1] * x[1] + R[2] * x[2] + t[0];
    const double py = R[3] * x[0] + R[4] * x[1] + R[5] * x[2] + t[1];
    const double pz = R[6] * x[0] + R[7] * x[1] + R[8] * x[2] + t[2];
    if (!(pz > 0.0)) return false;
    const double iz = 1.0 / pz, a = cam[0] * iz, b = cam[1] * iz, xz = px * iz, yz = py * iz;
    // Jpi = [[a, 0, -a xz], [0, b, -b yz]],  dp / d delta = [-[p]x, I]
    Ju[0] = -a * xz * py; Ju[1] = a * (pz + xz * px); Ju[2] = -a * py; Ju[3] = a; Ju[4] = 0.0; Ju[5] = -a * xz;
    Jv[0] = -b * (pz + yz * py); Jv[1] = b * yz * px; Jv[2] = b * px; Jv[3] = 0.0; Jv[4] = b; Jv[5] = -b * yz;
    *ru = cam[0] * xz + cam[2] - u;
    *rv = cam[1] * yz + cam[3] - v;
    return true;
}

// adds one correspondence's 27 terms to s; a point whose depth under (R, t) is not positive adds nothing
PNP_HD void pnp_gn_accumulate(const double *R, const double *t, const double *cam, const double *x, double u, double v, double *s) {
    double Ju[6], Jv[6], ru, rv;
    if (!pnp_gn_rows(R, t, cam, x, u, v, Ju, Jv, &ru, &rv)) return;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) s[k++] += Ju[i] * Ju[j] + Jv[i] * Jv[j];
    for (int i = 0; i < 6; ++i) s[21 + i] += Ju[i] * ru + Jv[i] * rv;
}

// the level-aware form: every term times w = 1 / sigma2 of the correspondence's level
PNP_HD void pnp_gn_accumulate_level(const double *R, const double *t, const double *cam, const double *x, double u, double v, double w,
                                    double *s) {
    double Ju[6], Jv[6], ru, rv;
    if (!pnp_gn_rows(R, t, cam, x, u, v, Ju, Jv, &ru, &rv)) return;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) s[k++] += (Ju[i] * Ju[j] + Jv[i] * Jv[j]) * w;
    for (int i = 0; i < 6; ++i) s[21 + i] += (Ju[i] * ru + Jv[i] * rv) * w;
}

// delta = -A^-1 b of the 27 sums; false (singular) and delta = 0 by the rule above
PNP_HD bool pnp_gn_solve(const double *s, double *x) {
    double A[6][6], L[6][6], D[6];
    for (int i = 0; i < 6; ++i) x[i] = 0.0;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = s[k++];
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int m = 0; m < j; ++m) d -= L[j][m] * L[j][m] * D[m];
        if (!pnp_finite(d) || !(d > PNP_PIVOT_REL * A[j][j])) return false;
        D[j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double a = A[i][j];
            for (int m = 0; m < j; ++m) a -= L[i][m] * L[j][m] * D[m];
            L[i][j] = a / d;
        }
    }
    double y[6], z[6];
    for (int i = 0; i < 6; ++i) {                          // L y = -b
        double a = -s[21 + i];
        for (int m = 0; m < i; ++m) a -= L[i][m] * y[m];
        y[i] = a;
    }
    for (int i = 0; i < 6; ++i) y[i] /= D[i];
    bool ok = true;
    for (int i = 5; i >= 0; --i) {                         // L^T z = y
        double a = y[i];
        for (int m = i + 1; m < 6; ++m) a -= L[m][i] * z[m];
        z[i] = a;
        ok = ok && pnp_finite(a);
    }
    if (!ok) return false;
    for (int i = 0; i < 6; ++i) x[i] = z[i];
    return true;
}

// (R, t) <- Exp(delta) (R, t); returns |delta|
PNP_HD double pnp_gn_apply(const double *delta, double *R, double *t) {
    double Re[9], te[3], Rn[9], tn[3];
    se3_exp(delta, Re, te);
    se3_mul(Re, te, R, t, Rn, tn);
    for (int e = 0; e < 9; ++e) R[e] = Rn[e];
    for (int e = 0; e < 3; ++e) t[e] = tn[e];
    double n = 0.0;
    for (int e = 0; e < 6; ++e) n += delta[e] * delta[e];
    return sqrt(n);
}
