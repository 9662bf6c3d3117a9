// ba.h -- two-view bundle adjustment of a verified keyframe pair in float64, shared by the kernel of vis_ba.hip and the host
// tests (compiled for the host with __host__ / __device__ defined away, as pnp.h is).  It follows the PnP fit of pnp.h the way
// rtabmap's computeTransformation follows its PnP with a local bundle adjustment at its defaults; rtabmap and g2o are third
// party and were not available to compare against: parity with them is unpinned.  tests/vis_ba_reference.py restates this file.
//
// Convention: T = (R, t) maps points of the "from" camera frame into the "to" camera frame (pnp.h).  View a = "from", view b = "to".
//
//   unknowns    T, started at the PnP result, and one point Y_k per correspondence of the adjusted set, in the "from" camera
//               frame, started at the "from" keyframe's 3D point.
//   residuals   view a: (fx_a Yx / Yz + cx_a - u_a, fy_a Yy / Yz + cy_a - v_a, w_a (1 / Yz - 1 / Z_a)), each square times
//               1 / sigma2[level in a]; view b: the same of Q = R Y + t against the "to" keypoint, w_b and 1 / sigma2[level in b],
//               its third component only where the "to" point has a depth (Z_b finite and positive, 1 / Z_b finite).
//               w = fx * baseline is the weight of a stereo disparity; sigma2 is pnp_level_sigma2.
//   depth       Yz <= 0 or Qz <= 0 at the linearisation point: the correspondence adds nothing to the step and its point does
//               not move; at a cost evaluation it adds nothing; at a recount it is dropped.
//   step        Gauss-Newton with the points eliminated (Schur complement), no damping.  Per point H_pp = sum J_p^T J_p (3 x 3),
//               g_p = sum J_p^T r, H_cp = J_c^T J_p (6 x 3) with J_c = J_b [-[Q]x, I] of the left perturbation T <- Exp(delta) T.
//               H_pp^-1 = adjugate / determinant (pnp_sym_adj).  Pivot rule: the point is free iff det is finite and
//               det > BA_PIVOT_REL * H_pp[0][0] H_pp[1][1] H_pp[2][2] (Hadamard: det <= that product); otherwise it is held
//               fixed for the step and only the 27 plain PnP terms of its "to" pixel (pnp_gn_accumulate_level) are added.
//               A free point adds H_cc - H_cp H_pp^-1 H_cp^T (upper triangle, row by row: s[0 .. 20]) and
//               g_c - H_cp H_pp^-1 g_p (s[21 .. 26]).  delta = pnp_gn_solve(s); T <- pnp_gn_apply(delta);
//               Y_k <- Y_k - H_pp^-1 (g_p + H_cp^T delta) with the blocks of the SAME linearisation point.
//   cost        sum over the set of |r_a|^2 / sigma2[level in a] + |r_b|^2 / sigma2[level in b] (no robust kernel).
//   keep        Yz > 0, Qz > 0, u-v error^2 in a <= thr2 sigma2[level in a] and in b <= thr2 sigma2[level in b].
// The rounds, the guard on the cost, the stopping rule and the status rules are the kernel's: include/cslam_hip.h states them.
#pragma once
#include "pnp.h"

#ifndef BA_HD
#define BA_HD __host__ __device__ static inline
#endif

#define BA_PIVOT_REL 1e-11         // det H_pp at or below this share of the product of its diagonal: the point is held fixed
#define BA_GN_TOL 1e-10            // a step of |delta| below it is taken and ends the round (VIS_GN_TOL of vis.hip)
#define BA_MAX_CORR 2048           // most correspondences of an adjusted set (VIS_MAX_CORR)
#define BA_COST_SLACK 1e-9         // a round is discarded when its cost ends above (1 + this) times the cost it started with
#define BA_FREE 1
#define BA_HELD 2

struct BaView { double fx, fy, cx, cy, w; };               // intrinsics and the depth weight fx * baseline
// one correspondence: keypoint and 1 / Z of both views (ib == 0: the "to" point has no depth), 1 / sigma2 of both levels
struct BaObs { double ua, va, ia, ub, vb, ib, sa, sb; };
struct BaBlocks { double Hpp[6], gp[3], Hcp[18], Hcc[21], gc[6]; };

// 1 / Z of an observed point, or 0 where it has no usable depth
BA_HD double ba_inv_depth(double z) {
    if (!(z > 0.0) || !pnp_finite(z)) return 0.0;
    const double iz = 1.0 / z;
    return pnp_finite(iz) ? iz : 0.0;
}

// residual r [3] of point P (in the view's frame, Pz > 0) and the Jacobian with respect to P,
//   [[a, 0, jx], [0, b, jy], [0, 0, jz]] as j = (a, b, jx, jy, jz); io = the observed 1 / Z, 0: no depth term
BA_HD void ba_view(const BaView &c, const double *P, double u, double v, double io, double *r, double *j) {
    const double iz = 1.0 / P[2], xz = P[0] * iz, yz = P[1] * iz;
    const bool depth = io != 0.0;
    j[0] = c.fx * iz; j[1] = c.fy * iz; j[2] = -j[0] * xz; j[3] = -j[1] * yz; j[4] = depth ? -c.w * iz * iz : 0.0;
    r[0] = c.fx * xz + c.cx - u; r[1] = c.fy * yz + c.cy - v; r[2] = depth ? c.w * (iz - io) : 0.0;
}

BA_HD void ba_transform(const double *R, const double *t, const double *Y, double *Q) {
    Q[0] = R[0] * Y[0] + R[1] * Y[1] + R[2] * Y[2] + t[0];
    Q[1] = R[3] * Y[0] + R[4] * Y[1] + R[5] * Y[2] + t[1];
    Q[2] = R[6] * Y[0] + R[7] * Y[1] + R[8] * Y[2] + t[2];
}

// the blocks of one correspondence at (R, t, Y); false where a depth is not positive
BA_HD bool ba_blocks(const double *R, const double *t, const BaView &ca, const BaView &cb, const BaObs &o, const double *Y, BaBlocks *B) {
    double Q[3];
    ba_transform(R, t, Y, Q);
    if (!(Y[2] > 0.0) || !(Q[2] > 0.0)) return false;
    double ra[3], ja[5], rb[3], jb[5];
    ba_view(ca, Y, o.ua, o.va, o.ia, ra, ja);
    ba_view(cb, Q, o.ub, o.vb, o.ib, rb, jb);
    // A = J_b R (3 x 3), C = J_b [-[Q]x, I] (3 x 6)
    double A[3][3], C[3][6];
    const double G0[6] = {0.0, Q[2], -Q[1], 1.0, 0.0, 0.0}, G1[6] = {-Q[2], 0.0, Q[0], 0.0, 1.0, 0.0}, G2[6] = {Q[1], -Q[0], 0.0, 0.0, 0.0, 1.0};
    for (int c = 0; c < 3; ++c) {
        A[0][c] = jb[0] * R[c] + jb[2] * R[6 + c];
        A[1][c] = jb[1] * R[3 + c] + jb[3] * R[6 + c];
        A[2][c] = jb[4] * R[6 + c];
    }
    for (int i = 0; i < 6; ++i) {
        C[0][i] = jb[0] * G0[i] + jb[2] * G2[i];
        C[1][i] = jb[1] * G1[i] + jb[3] * G2[i];
        C[2][i] = jb[4] * G2[i];
    }
    // view a: J_a^T J_a and J_a^T r_a of the triangular J_a
    B->Hpp[0] = o.sa * (ja[0] * ja[0]); B->Hpp[1] = 0.0; B->Hpp[2] = o.sa * (ja[0] * ja[2]);
    B->Hpp[3] = o.sa * (ja[1] * ja[1]); B->Hpp[4] = o.sa * (ja[1] * ja[3]);
    B->Hpp[5] = o.sa * (ja[2] * ja[2] + ja[3] * ja[3] + ja[4] * ja[4]);
    B->gp[0] = o.sa * (ja[0] * ra[0]); B->gp[1] = o.sa * (ja[1] * ra[1]); B->gp[2] = o.sa * (ja[2] * ra[0] + ja[3] * ra[1] + ja[4] * ra[2]);
    int k = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++k) B->Hpp[k] += o.sb * (A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j]);
    for (int i = 0; i < 3; ++i) B->gp[i] += o.sb * (A[0][i] * rb[0] + A[1][i] * rb[1] + A[2][i] * rb[2]);
    k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) B->Hcc[k] = o.sb * (C[0][i] * C[0][j] + C[1][i] * C[1][j] + C[2][i] * C[2][j]);
    for (int i = 0; i < 6; ++i) {
        B->gc[i] = o.sb * (C[0][i] * rb[0] + C[1][i] * rb[1] + C[2][i] * rb[2]);
        for (int c = 0; c < 3; ++c) B->Hcp[3 * i + c] = o.sb * (C[0][i] * A[0][c] + C[1][i] * A[1][c] + C[2][i] * A[2][c]);
    }
    return true;
}

// H_pp^-1 as (i00, i01, i02, i11, i12, i22); false by the pivot rule
BA_HD bool ba_point_inverse(const double *Hpp, double *inv) {
    double adj[6];
    pnp_sym_adj(Hpp, adj);
    const double det = Hpp[0] * adj[0] + Hpp[1] * adj[1] + Hpp[2] * adj[2];
    if (!pnp_finite(det) || !(det > BA_PIVOT_REL * (Hpp[0] * Hpp[3] * Hpp[5]))) return false;
    for (int e = 0; e < 6; ++e) inv[e] = adj[e] / det;
    return true;
}
BA_HD void ba_sym_vec(const double *m, const double *x, double *y) {
    y[0] = m[0] * x[0] + m[1] * x[1] + m[2] * x[2];
    y[1] = m[1] * x[0] + m[3] * x[1] + m[4] * x[2];
    y[2] = m[2] * x[0] + m[4] * x[1] + m[5] * x[2];
}

// adds one correspondence's 27 reduced terms to s; returns 0 (nothing added), BA_FREE or BA_HELD
BA_HD int ba_accumulate(const double *R, const double *t, const BaView &ca, const BaView &cb, const BaObs &o, const double *Y, double *s) {
    BaBlocks B;
    if (!ba_blocks(R, t, ca, cb, o, Y, &B)) return 0;
    double inv[6];
    if (!ba_point_inverse(B.Hpp, inv)) {
        const double cam[4] = {cb.fx, cb.fy, cb.cx, cb.cy};
        pnp_gn_accumulate_level(R, t, cam, Y, o.ub, o.vb, o.sb, s);
        return BA_HELD;
    }
    double M[6][3], w[3];
    for (int i = 0; i < 6; ++i) ba_sym_vec(inv, B.Hcp + 3 * i, M[i]);       // row i of H_cp H_pp^-1 (H_pp^-1 is symmetric)
    ba_sym_vec(inv, B.gp, w);
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k)
            s[k] += B.Hcc[k] - (M[i][0] * B.Hcp[3 * j] + M[i][1] * B.Hcp[3 * j + 1] + M[i][2] * B.Hcp[3 * j + 2]);
    for (int i = 0; i < 6; ++i) s[21 + i] += B.gc[i] - (B.Hcp[3 * i] * w[0] + B.Hcp[3 * i + 1] * w[1] + B.Hcp[3 * i + 2] * w[2]);
    return BA_FREE;
}

// the point's own update for the step delta, at the linearisation point (R, t, Y) of the accumulate pass
BA_HD int ba_back_substitute(const double *R, const double *t, const BaView &ca, const BaView &cb, const BaObs &o, const double *delta,
                             double *Y) {
    BaBlocks B;
    if (!ba_blocks(R, t, ca, cb, o, Y, &B)) return 0;
    double inv[6], v[3], d[3];
    if (!ba_point_inverse(B.Hpp, inv)) return BA_HELD;
    for (int c = 0; c < 3; ++c) {
        double a = B.gp[c];
        for (int i = 0; i < 6; ++i) a += B.Hcp[3 * i + c] * delta[i];
        v[c] = a;
    }
    ba_sym_vec(inv, v, d);
    for (int c = 0; c < 3; ++c) Y[c] -= d[c];
    return BA_FREE;
}

BA_HD double ba_cost(const double *R, const double *t, const BaView &ca, const BaView &cb, const BaObs &o, const double *Y) {
    double Q[3], ra[3], ja[5], rb[3], jb[5];
    ba_transform(R, t, Y, Q);
    if (!(Y[2] > 0.0) || !(Q[2] > 0.0)) return 0.0;
    ba_view(ca, Y, o.ua, o.va, o.ia, ra, ja);
    ba_view(cb, Q, o.ub, o.vb, o.ib, rb, jb);
    return o.sa * (ra[0] * ra[0] + ra[1] * ra[1] + ra[2] * ra[2]) + o.sb * (rb[0] * rb[0] + rb[1] * rb[1] + rb[2] * rb[2]);
}

// the recount: thr2 = reproj_error^2, s2a / s2b = sigma2 of the levels
BA_HD bool ba_keep(const double *R, const double *t, const BaView &ca, const BaView &cb, const BaObs &o, const double *Y, double thr2,
                   double s2a, double s2b) {
    double Q[3], ra[3], ja[5], rb[3], jb[5];
    ba_transform(R, t, Y, Q);
    if (!(Y[2] > 0.0) || !(Q[2] > 0.0)) return false;
    ba_view(ca, Y, o.ua, o.va, o.ia, ra, ja);
    ba_view(cb, Q, o.ub, o.vb, o.ib, rb, jb);
    return ra[0] * ra[0] + ra[1] * ra[1] <= thr2 * s2a && rb[0] * rb[0] + rb[1] * rb[1] <= thr2 * s2b;
}

// The guard of a round on the cost before (c0) and after (c1).  At a converged start both are the same sum up to the rounding
// of 2048 terms (relative 5e-13 at most): the slack keeps that noise from deciding, and a rise of a billionth is no worsening.
BA_HD bool ba_round_rejected(double c0, double c1) { return !pnp_finite(c1) || c1 > c0 * (1.0 + BA_COST_SLACK); }

// thread 0's part of a step: the solve, the pose update and its checks.  Returns 1: no step (singular or not finite),
// 0: step taken, 2: step taken and |delta| < BA_GN_TOL; Rn, tn = the new pose where a step is taken
BA_HD int ba_pose_step(const double *tot, const double *R, const double *t, double *delta, double *Rn, double *tn) {
    if (!pnp_gn_solve(tot, delta)) return 1;
    for (int e = 0; e < 9; ++e) Rn[e] = R[e];
    for (int e = 0; e < 3; ++e) tn[e] = t[e];
    const double nd = pnp_gn_apply(delta, Rn, tn);
    bool fin = pnp_finite(nd);
    for (int e = 0; e < 9; ++e) fin = fin && pnp_finite(Rn[e]);
    for (int e = 0; e < 3; ++e) fin = fin && pnp_finite(tn[e]);
    if (!fin) return 1;
    return nd < BA_GN_TOL ? 2 : 0;
}
