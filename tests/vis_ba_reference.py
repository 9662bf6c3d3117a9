"""A numpy restatement of the two-view bundle adjustment after PnP (include/cslam_hip.h, "Two-view bundle adjustment after
PnP"; csrc/ba.h), on top of vis_reference.py and vis_levels_reference.py, which stay as they are.  Written from that
statement, for the tests.  float64 by default; `dtype=np.longdouble` runs the same rule in extended precision.

Conventions as there: T maps "from" camera points into the "to" camera frame; view a = "from", view b = "to"; cam =
(fx, fy, cx, cy); the depth weight of a view is fx * baseline."""
import numpy as np

import vis_levels_reference as lv
import vis_reference as vr

PIVOT_REL = 1e-11
GN_TOL = 1e-10
COST_SLACK = 1e-9
MAX_CORR = 2048
STEP_GUARD = 10.0              # steps are compared exactly only where no |delta| lies within this factor of GN_TOL
RECOUNT_GUARD = 1e-6           # recount decisions only where the pixel error is this far (px) from its threshold
COST_GUARD = 1e-10             # rounds discarded only where cost after / cost before is this far from 1 + COST_SLACK


def sigma2(dtype=np.float64):
    return np.array([dtype(36 ** l) / dtype(25 ** l) for l in range(lv.MAX_LEVEL + 1)], dtype=dtype)


def inv_depth(z):
    """1 / Z, or 0 where the point has no usable depth."""
    z = np.asarray(z)
    with np.errstate(all="ignore"):
        iz = 1.0 / z
    ok = np.isfinite(z) & (z > 0.0) & np.isfinite(iz)
    return np.where(ok, iz, 0.0).astype(z.dtype)


def se3_exp(xi):
    """vis_reference.se3_exp in the dtype of xi."""
    w, v = xi[:3], xi[3:]
    th = np.sqrt((w * w).sum())
    W = np.array([[0 * th, -w[2], w[1]], [w[2], 0 * th, -w[0]], [-w[1], w[0], 0 * th]], dtype=xi.dtype)
    I = np.identity(3).astype(xi.dtype)
    if th < 1e-8:
        return I + W + W @ W / 2, v + W @ v / 2
    a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return I + a * W + b * W @ W, (I + b * W + c * W @ W) @ v


def ldl_solve(A, b):
    """vis_reference.gn_solve in the dtype of A: delta = -A^-1 b by an unpivoted LDL^T, None where a pivot fails."""
    n = len(b)
    L, D = np.identity(n).astype(A.dtype), np.zeros(n, dtype=A.dtype)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
            if not np.isfinite(d) or not d > 1e-11 * A[j, j]:
                return None
            D[j] = d
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / d
        y = np.zeros(n, dtype=A.dtype)
        for i in range(n):
            y[i] = -b[i] - (L[i, :i] * y[:i]).sum()
        y = y / D
        x = np.zeros(n, dtype=A.dtype)
        for i in range(n - 1, -1, -1):
            x[i] = y[i] - (L[i + 1:, i] * x[i + 1:]).sum()
    return x if np.all(np.isfinite(x)) else None


def view(cam, w, P, u, v, io):
    """Residuals r [n, 3] and Jacobians J [n, 3, 3] with respect to P of a view."""
    iz = 1.0 / P[:, 2]
    xz, yz = P[:, 0] * iz, P[:, 1] * iz
    depth = io != 0.0
    J = np.zeros((len(P), 3, 3), dtype=P.dtype)
    J[:, 0, 0], J[:, 1, 1] = cam[0] * iz, cam[1] * iz
    J[:, 0, 2], J[:, 1, 2] = -cam[0] * iz * xz, -cam[1] * iz * yz
    J[:, 2, 2] = np.where(depth, -w * iz * iz, 0.0)
    r = np.stack([cam[0] * xz + cam[2] - u, cam[1] * yz + cam[3] - v, np.where(depth, w * (iz - io), 0.0)], axis=1)
    return r, J


class Problem:
    """The adjusted set of one pair: observations [M] per view, weights, cameras."""

    def __init__(self, ua, va, ia, ub, vb, ib, la, lb, cam_a, cam_b, base_a, base_b, dtype):
        c = lambda x: np.asarray(x, dtype=np.float64).astype(dtype)
        self.ua, self.va, self.ia, self.ub, self.vb, self.ib = c(ua), c(va), c(ia), c(ub), c(vb), c(ib)
        self.cam_a, self.cam_b = c(cam_a), c(cam_b)
        self.wa, self.wb = self.cam_a[0] * dtype(base_a), self.cam_b[0] * dtype(base_b)
        s2 = sigma2(dtype)
        self.s2a, self.s2b = s2[la], s2[lb]
        self.dtype = dtype

    def residuals(self, R, t, Y, idx):
        """(ra, Ja, rb, Jb, Q) of the rows idx, all of positive depth in both views."""
        Q = Y[idx] @ R.T + t
        ra, Ja = view(self.cam_a, self.wa, Y[idx], self.ua[idx], self.va[idx], self.ia[idx])
        rb, Jb = view(self.cam_b, self.wb, Q, self.ub[idx], self.vb[idx], self.ib[idx])
        return ra, Ja, rb, Jb, Q

    def live(self, R, t, Y, member):
        Q = Y @ R.T + t
        return member & (Y[:, 2] > 0.0) & (Q[:, 2] > 0.0)

    def cost(self, R, t, Y, member):
        idx = np.nonzero(self.live(R, t, Y, member))[0]
        ra, _, rb, _, _ = self.residuals(R, t, Y, idx)
        return ((ra * ra).sum(axis=1) / self.s2a[idx] + (rb * rb).sum(axis=1) / self.s2b[idx]).sum()

    def blocks(self, R, t, Y, member):
        """Per live member: Hpp [n, 3, 3], gp [n, 3], Hcp [n, 6, 3], Hcc [n, 6, 6], gc [n, 6], and the plain PnP terms."""
        idx = np.nonzero(self.live(R, t, Y, member))[0]
        ra, Ja, rb, Jb, Q = self.residuals(R, t, Y, idx)
        sa, sb = 1.0 / self.s2a[idx], 1.0 / self.s2b[idx]
        G = np.zeros((len(idx), 3, 6), dtype=self.dtype)
        G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = Q[:, 2], -Q[:, 1], -Q[:, 2], Q[:, 0], Q[:, 1], -Q[:, 0]
        G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
        A = Jb @ R
        C = Jb @ G
        e = np.einsum
        Hpp = sa[:, None, None] * e("kri,krj->kij", Ja, Ja) + sb[:, None, None] * e("kri,krj->kij", A, A)
        gp = sa[:, None] * e("kri,kr->ki", Ja, ra) + sb[:, None] * e("kri,kr->ki", A, rb)
        Hcp = sb[:, None, None] * e("kri,krj->kij", C, A)
        Hcc = sb[:, None, None] * e("kri,krj->kij", C, C)
        gc = sb[:, None] * e("kri,kr->ki", C, rb)
        Hcc2 = sb[:, None, None] * e("kri,krj->kij", C[:, :2], C[:, :2])
        gc2 = sb[:, None] * e("kri,kr->ki", C[:, :2], rb[:, :2])
        return idx, Hpp, gp, Hcp, Hcc, gc, Hcc2, gc2

    @staticmethod
    def point_inverse(Hpp):
        """(inv [n, 3, 3], free [n]) by adjugate over determinant and the pivot rule."""
        m = [Hpp[:, 0, 0], Hpp[:, 0, 1], Hpp[:, 0, 2], Hpp[:, 1, 1], Hpp[:, 1, 2], Hpp[:, 2, 2]]
        a = [m[3] * m[5] - m[4] * m[4], m[2] * m[4] - m[1] * m[5], m[1] * m[4] - m[2] * m[3], m[0] * m[5] - m[2] * m[2],
             m[1] * m[2] - m[0] * m[4], m[0] * m[3] - m[1] * m[1]]
        det = m[0] * a[0] + m[1] * a[1] + m[2] * a[2]
        with np.errstate(all="ignore"):
            free = np.isfinite(det) & (det > PIVOT_REL * (m[0] * m[3] * m[5]))
            inv = np.stack([np.stack([a[0], a[1], a[2]], 1), np.stack([a[1], a[3], a[4]], 1), np.stack([a[2], a[4], a[5]], 1)], 1) / det[:, None, None]
        return inv, free

    def step(self, R, t, Y, member):
        """One Gauss-Newton step: (R, t, Y, |delta| or None where no step is taken, points held fixed)."""
        idx, Hpp, gp, Hcp, Hcc, gc, Hcc2, gc2 = self.blocks(R, t, Y, member)
        inv, free = self.point_inverse(Hpp)
        f, h = free, ~free
        M = Hcp[f] @ inv[f]
        S = (Hcc[f] - M @ np.transpose(Hcp[f], (0, 2, 1))).sum(axis=0) + Hcc2[h].sum(axis=0)
        g = (gc[f] - np.einsum("kij,kj->ki", M, gp[f])).sum(axis=0) + gc2[h].sum(axis=0)
        held = int(h.sum())
        delta = ldl_solve(S, g)
        if delta is None:
            return R, t, Y, None, held
        Re, te = se3_exp(delta)
        Rn, tn = Re @ R, Re @ t + te
        nd = np.sqrt((delta * delta).sum())
        if not (np.isfinite(nd) and np.all(np.isfinite(Rn)) and np.all(np.isfinite(tn))):
            return R, t, Y, None, held
        Yn = Y.copy()
        v = gp[f] + np.einsum("kij,ki->kj", Hcp[f], np.broadcast_to(delta, (int(f.sum()), 6)))
        Yn[idx[f]] = Y[idx[f]] - np.einsum("kij,kj->ki", inv[f], v)
        return Rn, tn, Yn, nd, held

    def keep(self, R, t, Y, member, thr2):
        """(the members that stay, the smallest | pixel error / sigma - threshold | over the live members of both views)."""
        live = self.live(R, t, Y, member)
        idx = np.nonzero(live)[0]
        ra, _, rb, _, _ = self.residuals(R, t, Y, idx)
        ea, eb = ra[:, 0] ** 2 + ra[:, 1] ** 2, rb[:, 0] ** 2 + rb[:, 1] ** 2
        out = np.zeros(len(Y), dtype=bool)
        out[idx] = (ea <= thr2 * self.s2a[idx]) & (eb <= thr2 * self.s2b[idx])
        thr = np.sqrt(thr2)
        guard = min([np.inf] + [float(np.abs(np.sqrt(x / s) - thr).min()) for x, s in ((ea, self.s2a[idx]), (eb, self.s2b[idx])) if len(x)])
        return out, guard

    def dense_normal(self, R, t, Y, member):
        """The full (6 + 3 n)-square Gauss-Newton normal matrix over the live members (float64), pose first."""
        idx, Hpp, gp, Hcp, Hcc, gc, _, _ = self.blocks(R, t, Y, member)
        n = len(idx)
        H = np.zeros((6 + 3 * n, 6 + 3 * n))
        H[:6, :6] = Hcc.sum(axis=0)
        for k in range(n):
            H[:6, 6 + 3 * k:9 + 3 * k] = Hcp[k]
            H[6 + 3 * k:9 + 3 * k, :6] = Hcp[k].T
            H[6 + 3 * k:9 + 3 * k, 6 + 3 * k:9 + 3 * k] = Hpp[k]
        return H


def adjust(kp_a, pts_a, kp_b, pts_b, rows, T0, flags0, cam_a, cam_b, base_a=0.1, base_b=0.1, lv_a=None, lv_b=None, reproj_error=2.0,
           min_inliers=20, ba_iterations=10, ba_rounds=2, pnp_status=0, dtype=np.float64):
    """The adjustment of one pair.  rows [K, 2] (row of "from", row of "to"), flags0 [K] what PnP flagged, T0 its transform.
    Returns dict(T, status, flags [K] bool, points [K, 3], cost (before, after), set_in, set_out, steps, discarded, held,
    deltas: every |delta| taken, guard_recount, guard_cost, problem, member_in, Y: the final points of the set, final: members)."""
    kp_a, pts_a, kp_b, pts_b = (np.asarray(x, dtype=np.float64) for x in (kp_a, pts_a, kp_b, pts_b))
    rows, flags0 = np.asarray(rows, dtype=np.int64).reshape(-1, 2), np.asarray(flags0).astype(bool)
    K = len(rows)
    T0 = np.asarray(T0, dtype=np.float64)
    out = dict(T=T0.copy(), status=int(pnp_status), flags=flags0.copy(), points=np.full((K, 3), np.nan), cost=(np.nan, np.nan),
               set_in=int(flags0.sum()), set_out=int(flags0.sum()), steps=0, discarded=0, held=0, deltas=[], guard_recount=np.inf,
               guard_cost=np.inf)
    if pnp_status != 0 or ba_rounds == 0 or ba_iterations == 0:
        return out
    i, j = rows[:, 0], rows[:, 1]
    inside = (i >= 0) & (i < len(kp_a)) & (j >= 0) & (j < len(kp_b))
    ic, jc = np.where(inside, i, 0), np.where(inside, j, 0)
    if len(kp_a) == 0 or len(kp_b) == 0:
        inside[:] = False
        ic, jc = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        kp_a, pts_a, kp_b, pts_b = (np.concatenate([x, np.zeros((1, x.shape[1]))]) for x in (kp_a, pts_a, kp_b, pts_b))
    ia, ib = inv_depth(pts_a[ic, 2]), inv_depth(pts_b[jc, 2])
    usable = (flags0 & inside & np.isfinite(kp_a[ic]).all(axis=1) & np.isfinite(kp_b[jc]).all(axis=1) & np.isfinite(pts_a[ic, :2]).all(axis=1)
              & (ia != 0.0))
    src = np.nonzero(usable)[0]
    M = len(src)
    if M > MAX_CORR:
        return dict(out, status=3, set_in=M, set_out=M)
    la = np.zeros(M, dtype=np.int64) if lv_a is None else np.asarray(lv_a)[ic[src]].astype(np.int64)
    lb = np.zeros(M, dtype=np.int64) if lv_b is None else np.asarray(lv_b)[jc[src]].astype(np.int64)
    pr = Problem(kp_a[ic[src], 0], kp_a[ic[src], 1], ia[src], kp_b[jc[src], 0], kp_b[jc[src], 1], ib[src], la, lb, cam_a, cam_b, base_a, base_b, dtype)
    R, t = T0[:3, :3].astype(dtype), T0[:3, 3].astype(dtype)
    Y = pts_a[ic[src]].astype(dtype)
    member = np.ones(M, dtype=bool)
    thr2 = dtype(reproj_error) * dtype(reproj_error)
    steps = discarded = held = 0
    deltas, g_rec, g_cost = [], np.inf, np.inf
    cost_first = cost_last = dtype(0)
    with np.errstate(all="ignore"):
        for rnd in range(ba_rounds):
            R0, t0, Y0 = R, t, Y
            c0 = pr.cost(R, t, Y, member)
            if rnd == 0:
                cost_first = c0
            for _ in range(ba_iterations):
                R, t, Y, nd, h = pr.step(R, t, Y, member)
                held += h
                if nd is None:
                    break
                steps += 1
                deltas.append(float(nd))
                if nd < GN_TOL:
                    break
            c1 = pr.cost(R, t, Y, member)
            if np.isfinite(c1) and c0 > 0:
                g_cost = min(g_cost, abs(float(c1 / c0) - (1.0 + COST_SLACK)))
            if not np.isfinite(c1) or c1 > c0 * (1.0 + COST_SLACK):
                R, t, Y, c1 = R0, t0, Y0, c0
                discarded += 1
            cost_last = c1
            member, g = pr.keep(R, t, Y, member, thr2)
            g_rec = min(g_rec, g)
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = R.astype(np.float64), t.astype(np.float64)
    flags = np.zeros(K, dtype=bool)
    flags[src] = member
    points = np.full((K, 3), np.nan)
    points[src[member]] = Y[member].astype(np.float64)
    return dict(T=T, status=0 if member.sum() >= min_inliers else 1, flags=flags, points=points, cost=(float(cost_first), float(cost_last)),
                set_in=M, set_out=int(member.sum()), steps=steps, discarded=discarded, held=held, deltas=deltas, guard_recount=g_rec,
                guard_cost=g_cost, problem=pr, Y=Y, final=member, R=R, t=t, src=src)


def steps_decided(rec):
    """True where no |delta| lies within STEP_GUARD of GN_TOL: the number of steps is then compared exactly."""
    return all(not (GN_TOL / STEP_GUARD <= d <= GN_TOL * STEP_GUARD) for d in rec["deltas"])


def result_cond(rec):
    """cond of the full normal matrix of the restatement at its result (for sets small enough to hold it)."""
    H = rec["problem"].dense_normal(rec["R"], rec["t"], rec["Y"], rec["final"])
    return float(np.linalg.cond(H))


def register_ba(kf_from, kf_to, cam_from, cam_to=None, baselines=0.1, nndr=0.8, ba_iterations=10, ba_rounds=2, **kwargs):
    """(matches, the PnP record, the adjustment's record) of two keyframes (keypoints, points, descriptors[, levels]): the
    level-aware PnP and level weights where both carry levels."""
    cam_to = cam_from if cam_to is None else cam_to
    ba, bb = (baselines, baselines) if np.ndim(baselines) == 0 else baselines
    levels = len(kf_from) > 3 and len(kf_to) > 3
    if levels:
        rows, pnp = lv.register(kf_from, kf_to, cam_to, nndr, **kwargs)
    else:
        rows, pnp = vr.register(kf_from, kf_to, cam_to, nndr, **kwargs)
    rec = adjust(kf_from[0], kf_from[1], kf_to[0], kf_to[1], rows, pnp["T"], pnp["inliers"], cam_from, cam_to, ba, bb,
                 kf_from[3] if levels else None, kf_to[3] if levels else None, kwargs.get("reproj_error", 2.0), kwargs.get("min_inliers", 20),
                 ba_iterations, ba_rounds, pnp["status"])
    return rows, pnp, rec


# ---- scenes of the tests -------------------------------------------------------------------------------------------
def project(cam, P):
    return np.stack([cam[0] * P[:, 0] / P[:, 2] + cam[2], cam[1] * P[:, 1] / P[:, 2] + cam[3]], axis=1)


def back_project(cam, uv, z):
    return np.stack([(uv[:, 0] - cam[2]) / cam[0] * z, (uv[:, 1] - cam[3]) / cam[1] * z, z], axis=1)


def stereo_scene(seed, M, cam, baseline, depth, size, noise=0.5, levels=1, max_deg=10.0, max_t=0.3):
    """M landmarks seen by two stereo cameras of a planted T: pixels of "from" uniform over `size` = (W, H), depths uniform in
    `depth`; in each view the keypoint gets +-noise 1.2^level px uniform, the disparity fx baseline / Z +-noise px uniform, and
    the view's 3D point is the back-projection of the noisy keypoint at the noisy depth, as a stereo keyframe has it.
    Returns dict(kp_a, pts_a, kp_b, pts_b, lv_a, lv_b, T, P: the true points in "from")."""
    rng = np.random.default_rng(seed)
    cam = np.asarray(cam, dtype=np.float64)
    R = vr.random_rotation(rng, max_deg)
    t = rng.uniform(-max_t, max_t, 3)
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = R, t
    px = np.stack([rng.uniform(0.0, size[0], M), rng.uniform(0.0, size[1], M)], axis=1)
    P = back_project(cam, px, rng.uniform(depth[0], depth[1], M))
    Q = P @ R.T + t
    out = dict(T=T, P=P)
    for name, X in (("a", P), ("b", Q)):
        lvl = rng.integers(0, levels, M)
        kp = project(cam, X) + rng.uniform(-noise, noise, (M, 2)) * (1.2 ** lvl)[:, None]
        disp = cam[0] * baseline / X[:, 2] + rng.uniform(-noise, noise, M)
        z = np.where(disp > 0.0, cam[0] * baseline / np.where(disp > 0.0, disp, 1.0), np.nan)
        out["kp_" + name], out["pts_" + name], out["lv_" + name] = kp, back_project(cam, kp, z), lvl.astype(np.int32)
    return out


FAR_CAM = np.array([100.0, 100.0, 80.0, 60.0])             # the far scene: a 160 x 120 image, fx = fy = 100, baseline 0.2 m
FAR_BASELINE = 0.2


def far_scene(seed, M=150, depth=(3.0, 8.0)):
    """The scene of the accuracy condition: M correspondences, depths 3 - 8 m, +-0.5 px on u, v and the disparity of both
    views, no outliers, level 0.  Returns (scene, T0: the Gauss-Newton PnP fit on all correspondences, started at the plant)."""
    s = stereo_scene(seed, M, FAR_CAM, FAR_BASELINE, depth, (160.0, 120.0))
    ok = np.isfinite(s["pts_a"]).all(axis=1)
    R, t, _, _ = vr.refine(s["T"][:3, :3], s["T"][:3, 3], FAR_CAM, s["pts_a"], s["kp_b"], ok, 1e9, 10, 1)
    T0 = np.identity(4)
    T0[:3, :3], T0[:3, 3] = R, t
    return s, T0, ok


def pose_errors(T, plant):
    """(largest translation component error, rotation error in degrees)."""
    dR = T[:3, :3] @ plant[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.abs(T[:3, 3] - plant[:3, 3]).max()), float(ang)


CAM = vr.CAM                                                 # the planted scenes of the kernel tests: 640 x 480, fx = 525
BASELINE = 0.1
SET_SIZES = (20, 63, 64, 65, 255, 256, 257, 2048)


def planted_case(size, seed=None, extra=7, nan_to=0.1, levels=4, depth=(1.5, 6.0)):
    """A pair whose adjusted set has exactly `size` members: `size` noisy landmarks (levels 0 .. levels - 1 in both views, a
    share `nan_to` of the "to" points without depth) flagged 1, and `extra` rows of unrelated pixels flagged 0, rows shuffled.
    T0 is the level-aware Gauss-Newton PnP fit on the flagged rows, started at the plant: what PnP ends with.
    Returns dict(kp_a, pts_a, kp_b, pts_b, lv_a, lv_b, rows, flags, T0, T)."""
    seed = 500 + size if seed is None else seed
    s = stereo_scene(seed, size + extra, CAM, BASELINE, depth, (640.0, 480.0), levels=levels)
    rng = np.random.default_rng(seed + 9000)
    n = size + extra
    flags = np.zeros(n, dtype=bool)
    flags[rng.permutation(n)[:size]] = True
    s["kp_b"][~flags] = np.stack([rng.uniform(0, 640, extra), rng.uniform(0, 480, extra)], axis=1)
    s["pts_b"][rng.permutation(np.nonzero(flags)[0])[:int(np.ceil(nan_to * size))]] = np.nan
    perm = rng.permutation(n)                               # the "to" keyframe in another order
    inv = np.argsort(perm)
    s["kp_b"], s["pts_b"], s["lv_b"] = s["kp_b"][perm], s["pts_b"][perm], s["lv_b"][perm]
    rows = np.stack([np.arange(n), inv], axis=1).astype(np.int64)
    s2 = lv.SIGMA2[s["lv_b"][rows[:, 1]]]
    R, t, _, _, _ = lv.refine(s["T"][:3, :3], s["T"][:3, 3], CAM, s["pts_a"], s["kp_b"][rows[:, 1]], s2, flags, 2.0, 10, 1)
    T0 = np.identity(4)
    T0[:3, :3], T0[:3, 3] = R, t
    return dict(s, rows=rows, flags=flags, T0=T0)


def run_case(c, **kw):
    """The restatement on a `planted_case` (or any dict of its keys)."""
    return adjust(c["kp_a"], c["pts_a"], c["kp_b"], c["pts_b"], c["rows"], c["T0"], c["flags"], c.get("cam_a", CAM), c.get("cam_b", CAM),
                  c.get("base_a", BASELINE), c.get("base_b", BASELINE), c.get("lv_a"), c.get("lv_b"), **kw)


def _named(name, c, **kw):
    return dict(c, name=name, **kw)


def all_cases():
    """Every staged case of the kernel tests, each a dict of `planted_case`'s keys, a name and optional settings."""
    cases = [_named("size %d" % n, planted_case(n)) for n in SET_SIZES]
    # a correspondence PnP cannot see: "to" pixel and "from" point are consistent, the "from" keypoint is 5 px off
    c = planted_case(100, seed=611, levels=1)
    k = int(np.nonzero(c["flags"])[0][17])
    c["kp_a"][k, 0] += 5.0
    cases.append(_named("displaced from keypoint", c, displaced=k))
    c = planted_case(80, seed=612)
    c["pts_b"][:] = np.nan                                  # scale is fixed by "from" alone
    cases.append(_named("no to depth", c))
    seed = 700
    while planted_case(60, seed=seed)["T0"][2, 3] > -0.15:  # a plant that moves the camera forward
        seed += 1
    c = planted_case(60, seed=seed)
    k = int(np.nonzero(c["flags"])[0][5])
    c["pts_a"][k], c["kp_a"][k] = (0.0, 0.0, 0.05), CAM[2:]  # in front of "from", behind "to" at T0
    cases.append(_named("behind at T0", c, behind=k))
    # no parallax between the views (T0 a pure rotation) and next to no depth weight: H_pp has no third pivot at T0 and every
    # point is held fixed for the first step, which is then the plain PnP step
    s = stereo_scene(613, 70, CAM, BASELINE, (1.5, 6.0), (640.0, 480.0), levels=1, max_t=0.0)
    rows = np.repeat(np.arange(70)[:, None], 2, axis=1)
    cases.append(_named("held by the pivot rule", dict(s, rows=rows, flags=np.ones(70, dtype=bool), T0=s["T"].copy()), base_a=1e-9, base_b=1e-9))
    # nothing adjusted: what PnP wrote passes through
    c = planted_case(64)
    cases.append(_named("pnp status 1", c, pnp_status=1))
    z = planted_case(10, seed=614)
    cases.append(_named("pnp status 2", dict(z, flags=np.zeros_like(z["flags"]), T0=np.identity(4)), pnp_status=2))
    big = planted_case(2049, seed=615, extra=0)
    cases.append(_named("pnp status 3", dict(big, flags=np.zeros_like(big["flags"]), T0=np.identity(4)), pnp_status=3))
    cases.append(_named("no rounds", c, ba_rounds=0))
    cases.append(_named("no iterations", c, ba_iterations=0))
    cases.append(_named("above the cap", big))
    cases.append(_named("too few remain", planted_case(20), min_inliers=21))
    return cases


_LONG = {}


def tolerance(c, rec):
    """The allowance of T and the refined points against the float64 restatement `rec` of case `c`: 8 eps cond(H) with H the
    restatement's full normal matrix at its result for sets of at most 257; above, 4 x the restatement's own distance from
    its np.longdouble run (the margin covers a different but fixed summation order)."""
    if rec["set_in"] <= 257:
        return 8.0 * np.finfo(np.float64).eps * result_cond(rec)
    if c["name"] not in _LONG:
        _LONG[c["name"]] = run_case(c, dtype=np.longdouble, **settings(c))
    ext = _LONG[c["name"]]
    assert np.array_equal(ext["flags"], rec["flags"])
    m = rec["flags"]
    return 4.0 * max(np.abs(ext["T"] - rec["T"]).max(), np.abs(ext["points"][m] - rec["points"][m]).max())


def settings(c):
    return {k: c[k] for k in ("reproj_error", "min_inliers", "ba_iterations", "ba_rounds", "pnp_status") if k in c}


def compare(c, got, want, name):
    """A result (of the kernel, or of csrc/ba.h on the host) against the restatement's record `want` of case `c`: dict(T, cost,
    info [8], flags, points).  Exactly: status, PnP status, set size in, rounds discarded, points held fixed; the steps where
    `steps_decided`; set size out and the flags where every recount decision is RECOUNT_GUARD px from its threshold; T and the
    refined points within `tolerance`.  Prints every measured distance beside its allowance and returns them."""
    info = got["info"]
    assert info[0] == want["status"] and info[6] == c.get("pnp_status", 0), name
    assert info[1] == want["set_in"] and info[4] == want["discarded"] and info[5] == want["held"], (name, info, want["discarded"], want["held"])
    assert want["guard_cost"] >= COST_GUARD, name
    if steps_decided(want):
        assert info[3] == want["steps"], name
    if want["guard_recount"] >= RECOUNT_GUARD:
        assert info[2] == want["set_out"] and np.array_equal(got["flags"], want["flags"]), name
    if "problem" not in want:                               # nothing adjusted: PnP's bytes
        assert got["T"].tobytes() == np.asarray(c["T0"], dtype=np.float64).tobytes() and np.array_equal(got["flags"], np.asarray(c["flags"], bool))
        assert np.isnan(got["points"]).all() and np.isnan(got["cost"]).all()
        return 0.0, 0.0
    tol = tolerance(c, want)
    d_T = np.abs(got["T"] - want["T"]).max()
    both = got["flags"] & want["flags"]
    d_P = np.abs(got["points"][both] - want["points"][both]).max() if both.any() else 0.0
    assert np.isnan(got["points"][~got["flags"]]).all() and np.isfinite(got["points"][got["flags"]]).all()
    print("%s: T %.3g, points %.3g, allowed %.3g; cost %.6g -> %.6g (restatement %.6g -> %.6g)" % (
        name, d_T, d_P, tol, got["cost"][0], got["cost"][1], want["cost"][0], want["cost"][1]))
    assert d_T <= tol and d_P <= tol, name
    assert abs(got["cost"][0] - want["cost"][0]) <= 1e-9 * want["cost"][0] and abs(got["cost"][1] - want["cost"][1]) <= 1e-6 * want["cost"][1]
    return d_T, d_P
