"""A float64 numpy restatement of the visual verification (include/cslam_hip.h, "Visual loop closures"): the matcher, the
sampler, P3P, the selection by the fourth point, the scoring and the refinement.  Written from that statement, for the tests.

Conventions as there: T maps "from" camera points into the "to" camera frame; cam = (fx, fy, cx, cy)."""
import numpy as np

MASK = (1 << 64) - 1
POPC = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


# ---- matcher -------------------------------------------------------------------------------------------------------
def hamming(a, b):
    """[n, m] Hamming distances of uint8 rows."""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), dtype=np.int64)
    return POPC[a[:, None, :] ^ b[None, :, :]].sum(axis=2)


def match(a, b, nndr=0.8):
    """rows [K, 2] (from row, to row), ascending in the from row."""
    D = hamming(a, b)
    n, m = D.shape
    if m < 2 or n == 0:
        return np.zeros((0, 2), dtype=np.int64)
    i1 = np.argmin(D, axis=1)                              # the first of equals
    d1 = D[np.arange(n), i1]
    D2 = D.copy()
    D2[np.arange(n), i1] = 1 << 20
    d2 = D2.min(axis=1)
    ok = d1.astype(np.float64) <= nndr * d2.astype(np.float64)
    owner = {}
    for i in np.nonzero(ok)[0]:
        key = (int(d1[i]), int(i))
        j = int(i1[i])
        if j not in owner or key < owner[j]:
            owner[j] = key
    rows = sorted((i, j) for j, (_, i) in owner.items())
    return np.array(rows, dtype=np.int64).reshape(-1, 2)


# ---- sampler -------------------------------------------------------------------------------------------------------
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, h, M):
    s = mix64(seed & MASK)
    idx = []
    for j in range(4):
        pick = None
        for a in range(16):
            c = mix64((s + ((h << 6) | (j << 4) | a)) & MASK) % M
            if c not in idx:
                pick = c
                break
        if pick is None:
            pick = min(c for c in range(M) if c not in idx)
        idx.append(int(pick))
    return idx


# ---- P3P (Lambda Twist) --------------------------------------------------------------------------------------------
def _sym(m):
    return np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])


def _adj(Mx):
    return np.array([[Mx[1, 1] * Mx[2, 2] - Mx[1, 2] * Mx[2, 1], Mx[0, 2] * Mx[2, 1] - Mx[0, 1] * Mx[2, 2], Mx[0, 1] * Mx[1, 2] - Mx[0, 2] * Mx[1, 1]],
                     [Mx[1, 2] * Mx[2, 0] - Mx[1, 0] * Mx[2, 2], Mx[0, 0] * Mx[2, 2] - Mx[0, 2] * Mx[2, 0], Mx[0, 2] * Mx[1, 0] - Mx[0, 0] * Mx[1, 2]],
                     [Mx[1, 0] * Mx[2, 1] - Mx[1, 1] * Mx[2, 0], Mx[0, 1] * Mx[2, 0] - Mx[0, 0] * Mx[2, 1], Mx[0, 0] * Mx[1, 1] - Mx[0, 1] * Mx[1, 0]]])


def cubic_root(b, c, d):
    disc = b * b - 3.0 * c
    if disc >= 0.0:
        v = np.sqrt(disc)
        t1 = (-b - v) / 3.0
        k = ((t1 + b) * t1 + c) * t1 + d
        if k > 0.0:
            r = t1 - np.sqrt(-k / (3.0 * t1 + b))
        else:
            t2 = (-b + v) / 3.0
            k = ((t2 + b) * t2 + c) * t2 + d
            r = t2 + np.sqrt(-k / (3.0 * t2 + b)) if k < 0.0 else -b / 3.0
        if not np.isfinite(r):
            r = -b / 3.0
    else:
        r = -b / 3.0
        if abs((3.0 * r + 2.0 * b) * r + c) < 1e-4:
            r += 1.0
    for _ in range(50):
        fx, fpx = ((r + b) * r + c) * r + d, (3.0 * r + 2.0 * b) * r + c
        if fx == 0.0 or fpx == 0.0:
            break
        step = fx / fpx
        if not np.isfinite(step):
            break
        r -= step
        if abs(step) <= 1e-15 * abs(r):
            break
    return r


def _eigvec(Mx, lam):
    B = Mx - lam * np.identity(3)
    cs = [np.cross(B[0], B[1]), np.cross(B[0], B[2]), np.cross(B[1], B[2])]
    ns = [float(c @ c) for c in cs]
    k = int(np.argmax(ns))                                 # the first of equals
    if not (ns[k] > 0.0 and np.isfinite(ns[k])):
        return None
    return cs[k] / np.sqrt(ns[k])


def p3p(X, Yb):
    """X [3, 3] points, Yb [3, 3] bearings.  Returns (list of (R, t), guard): guard = the smallest relative separation of a
    quantity from the value at which the number of roots changes (collinearity, discriminants, tau > 0, l1 >= 0)."""
    with np.errstate(all="ignore"):
        return _p3p(np.asarray(X, dtype=np.float64), np.asarray(Yb, dtype=np.float64))


def _p3p(X, Yb):
    guard = np.inf
    nrm = np.sqrt((Yb * Yb).sum(axis=1))
    if not (np.all(nrm > 0.0) and np.all(np.isfinite(nrm))):
        return [], 0.0
    y = Yb / nrm[:, None]
    d12, d13, d23 = X[0] - X[1], X[0] - X[2], X[1] - X[2]
    nx = np.cross(d12, d13)
    a12, a13, a23, nn = d12 @ d12, d13 @ d13, d23 @ d23, nx @ nx
    if not np.all(np.isfinite([a12, a13, a23, nn])):
        return [], 0.0
    if not (nn > 1e-20 * a12 * a13) or not (a23 > 0.0):
        return [], 0.0
    guard = min(guard, nn / (a12 * a13))                   # how far from collinear
    b12, b13, b23 = -2.0 * (y[0] @ y[1]), -2.0 * (y[0] @ y[2]), -2.0 * (y[1] @ y[2])
    D1 = _sym([a23, 0.5 * a23 * b12, 0.0, a23 - a12, -0.5 * a12 * b23, -a12])
    D2 = _sym([a23, 0.0, 0.5 * a23 * b13, -a13, -0.5 * a13 * b23, a23 - a13])
    J1, J2 = _adj(D1), _adj(D2)
    k0, k3 = D1[0] @ J1[:, 0], -(D2[0] @ J2[:, 0])
    k1, k2 = -np.trace(J1 @ D2), np.trace(D1 @ J2)
    if k3 == 0.0:
        return [], 0.0
    g = cubic_root(k2 / k3, k1 / k3, k0 / k3)
    if not np.isfinite(g):
        return [], 0.0
    A = D1 - g * D2
    tr = np.trace(A)
    mn = (A[0, 0] * A[1, 1] - A[0, 1] ** 2) + (A[0, 0] * A[2, 2] - A[0, 2] ** 2) + (A[1, 1] * A[2, 2] - A[1, 2] ** 2)
    dq = tr * tr - 4.0 * mn
    if not dq >= 0.0:
        return [], 0.0
    sq = np.sqrt(dq)
    big = 0.5 * (tr + sq) if tr >= 0.0 else 0.5 * (tr - sq)
    if big == 0.0:
        return [], 0.0
    small = mn / big
    L0, L1 = max(big, small), min(big, small)
    if not L0 > 0.0:
        return [], 0.0
    v0, v1 = _eigvec(A, L0), _eigvec(A, L1)
    if v0 is None or v1 is None:
        return [], 0.0
    ratio = -L1 / L0
    guard = min(guard, abs(ratio))
    sv = np.sqrt(ratio) if ratio > 0.0 else 0.0
    Ls = []
    for s in (sv, -sv):
        w2 = 1.0 / (s * v1[0] - v0[0])
        w0, w1 = (v0[1] - s * v1[1]) * w2, (v0[2] - s * v1[2]) * w2
        a = 1.0 / ((a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12)
        b = (a13 * b12 * w1 - a12 * b13 * w0 - 2.0 * w0 * w1 * (a12 - a13)) * a
        c = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * a
        disc = b * b - 4.0 * c
        if not np.isfinite(disc):
            guard = 0.0
            continue
        guard = min(guard, abs(disc) / (b * b + 4.0 * abs(c) + 1e-300))
        if not disc >= 0.0:
            continue
        q = np.sqrt(disc)
        r1 = 0.5 * (-b - q) if b >= 0.0 else 0.5 * (-b + q)
        for tau in (r1, c / r1 if r1 != 0.0 else 0.0):
            guard = min(guard, abs(tau) / (1.0 + abs(tau)))
            if not tau > 0.0:
                continue
            den = tau * (b23 + tau) + 1.0
            if not den > 0.0:
                continue
            l2 = np.sqrt(a23 / den)
            l3 = tau * l2
            l1 = w0 * l2 + w1 * l3
            guard = min(guard, abs(l1) / (l2 + l3))
            if not l1 >= 0.0 or len(Ls) >= 4:
                continue
            Ls.append(np.array([l1, l2, l3]))
    Xi = np.stack([np.cross(d13, nx), np.cross(nx, d12), nx]) / nn
    out = []
    for l in Ls:
        for _ in range(3):
            r = np.array([l[0] ** 2 + l[1] ** 2 + b12 * l[0] * l[1] - a12, l[0] ** 2 + l[2] ** 2 + b13 * l[0] * l[2] - a13,
                          l[1] ** 2 + l[2] ** 2 + b23 * l[1] * l[2] - a23])
            J = np.array([[2.0 * l[0] + b12 * l[1], 2.0 * l[1] + b12 * l[0], 0.0], [2.0 * l[0] + b13 * l[2], 0.0, 2.0 * l[2] + b13 * l[0]],
                          [0.0, 2.0 * l[1] + b23 * l[2], 2.0 * l[2] + b23 * l[1]]])
            det = J[0] @ np.cross(J[1], J[2])
            if det == 0.0 or not np.isfinite(det):
                break
            Ji = np.stack([np.cross(J[1], J[2]), np.cross(J[2], J[0]), np.cross(J[0], J[1])], axis=1) / det
            nl = l - Ji @ r
            if not np.all(np.isfinite(nl)):
                break
            l = nl
        yd1, yd2 = l[0] * y[0] - l[1] * y[1], l[0] * y[0] - l[2] * y[2]
        Y = np.stack([yd1, yd2, np.cross(yd1, yd2)], axis=1)
        R = Y @ Xi
        t = l[0] * y[0] - R @ X[0]
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            out.append((R, t))
    return out, float(guard)


# ---- projection, selection, scoring --------------------------------------------------------------------------------
def reproj_e2(R, t, cam, X, uv):
    """Squared pixel errors [M]; +inf where the depth is not positive."""
    X, uv = np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    P = X @ R.T + t
    with np.errstate(all="ignore"):
        du = cam[0] * P[:, 0] / P[:, 2] + cam[2] - uv[:, 0]
        dv = cam[1] * P[:, 1] / P[:, 2] + cam[3] - uv[:, 1]
        e2 = du * du + dv * dv
    return np.where(P[:, 2] > 0.0, e2, np.inf)


def hypothesis(X4, uv4, cam):
    """(R, t, guard) or (None, None, guard) of four correspondences."""
    Yb = np.stack([(uv4[:3, 0] - cam[2]) / cam[0], (uv4[:3, 1] - cam[3]) / cam[1], np.ones(3)], axis=1)
    roots, guard = p3p(X4[:3], Yb)
    if not roots:
        return None, None, guard
    errs = [float(reproj_e2(R, t, cam, X4[3], uv4[3])[0]) for R, t in roots]
    k = int(np.argmin(errs))                               # the first of equals
    if len(errs) > 1:
        o = sorted(errs)
        guard = min(guard, (o[1] - o[0]) / (o[1] + 1e-300) if np.isfinite(o[1]) else 1.0)
    return roots[k][0], roots[k][1], guard


def hypotheses(X, uv, cam, iterations, reproj_error, seed):
    """Per hypothesis: R, t, valid, inlier count, guard_roots, guard_threshold (smallest | error - threshold | in pixels
    over all correspondences), and the [iterations, M] inlier masks."""
    X, uv, cam = np.asarray(X, dtype=np.float64), np.asarray(uv, dtype=np.float64), np.asarray(cam, dtype=np.float64)
    M = len(X)
    Rs, ts = np.zeros((iterations, 3, 3)), np.zeros((iterations, 3))
    valid, cnt = np.zeros(iterations, dtype=bool), np.zeros(iterations, dtype=np.int64)
    g_roots, g_thr = np.zeros(iterations), np.full(iterations, np.inf)
    masks = np.zeros((iterations, M), dtype=bool)
    for h in range(iterations):
        idx = sample(seed, h, M)
        R, t, g = hypothesis(X[idx], uv[idx], cam)
        g_roots[h] = g
        if R is None:
            continue
        e2 = reproj_e2(R, t, cam, X, uv)
        masks[h] = e2 <= reproj_error * reproj_error
        Rs[h], ts[h], valid[h], cnt[h] = R, t, True, masks[h].sum()
        fin = np.isfinite(e2)
        if fin.any():
            g_thr[h] = np.abs(np.sqrt(e2[fin]) - reproj_error).min()
    return dict(R=Rs, t=ts, valid=valid, count=cnt, guard_roots=g_roots, guard_threshold=g_thr, masks=masks)


def best_hypothesis(count):
    return int(np.argmax(count))                           # the most inliers, then the lowest h


# ---- refinement ----------------------------------------------------------------------------------------------------
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    W = skew(w)
    if th < 1e-8:
        return np.identity(3) + W + 0.5 * W @ W, v + 0.5 * W @ v
    a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.identity(3) + a * W + b * W @ W, (np.identity(3) + b * W + c * W @ W) @ v


def gn_jacobian(R, t, cam, X, uv):
    """J [M, 2, 6], r [M, 2], in_front [M] of the left perturbation Exp(delta) T, delta = [omega, v]."""
    P = X @ R.T + t
    z = P[:, 2]
    J = np.zeros((len(X), 2, 6))
    with np.errstate(all="ignore"):
        Jpi = np.zeros((len(X), 2, 3))
        Jpi[:, 0, 0], Jpi[:, 0, 2] = cam[0] / z, -cam[0] * P[:, 0] / z ** 2
        Jpi[:, 1, 1], Jpi[:, 1, 2] = cam[1] / z, -cam[1] * P[:, 1] / z ** 2
        for k in range(len(X)):
            J[k] = Jpi[k] @ np.hstack([-skew(P[k]), np.identity(3)])
        r = np.stack([cam[0] * P[:, 0] / z + cam[2] - uv[:, 0], cam[1] * P[:, 1] / z + cam[3] - uv[:, 1]], axis=1)
    return J, r, z > 0.0


def gn_sums(R, t, cam, X, uv):
    """(A [6, 6], b [6]) over the correspondences with positive depth."""
    J, r, ok = gn_jacobian(R, t, cam, np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2))
    J, r = J[ok], r[ok]
    return np.einsum("kai,kaj->ij", J, J), np.einsum("kai,ka->i", J, r)


def gn_solve(A, b, pivot_rel=1e-11):
    """delta = -A^-1 b by an unpivoted LDL^T, or None (singular) where a pivot is not above pivot_rel times its diagonal."""
    L, D = np.identity(6), np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
            if not np.isfinite(d) or not d > pivot_rel * A[j, j]:
                return None
            D[j] = d
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / d
        y = np.linalg.solve(L, -b) / D
        x = np.linalg.solve(L.T, y)
    return x if np.all(np.isfinite(x)) else None


def refine(R, t, cam, X, uv, mask, reproj_error, refine_iterations, refine_rounds):
    """Rounds of { Gauss-Newton on the inlier set, recount }: (R, t, mask, steps)."""
    steps = 0
    for _ in range(refine_rounds):
        for _ in range(refine_iterations):
            A, b = gn_sums(R, t, cam, X[mask], uv[mask])
            d = gn_solve(A, b)
            if d is None:
                break
            Re, te = se3_exp(d)
            R, t = Re @ R, Re @ t + te
            steps += 1
            if np.linalg.norm(d) < 1e-10:
                break
        mask = reproj_e2(R, t, cam, X, uv) <= reproj_error * reproj_error
    return R, t, mask, steps


def pnp_ransac(X, uv, cam, iterations=300, reproj_error=2.0, min_inliers=20, refine_iterations=10, refine_rounds=2, seed=0, cap=2048):
    """dict(T, status, inliers [given] bool, dropped, best_hypothesis, hyp: the hypotheses' record or None)."""
    X, uv, cam = np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2), np.asarray(cam, dtype=np.float64)
    use = np.isfinite(X).all(axis=1) & np.isfinite(uv).all(axis=1)
    Xu, uvu = X[use], uv[use]
    M = len(Xu)
    out = dict(T=np.identity(4), inliers=np.zeros(len(X), dtype=bool), dropped=int(len(X) - M), best_hypothesis=-1, hyp=None)
    if M > cap:
        return dict(out, status=3)
    if M < max(4, min_inliers):
        return dict(out, status=2)
    hyp = hypotheses(Xu, uvu, cam, iterations, reproj_error, seed)
    h = best_hypothesis(hyp["count"])
    T = np.identity(4)
    mask = np.zeros(M, dtype=bool)
    if hyp["valid"][h]:
        R, t, mask, _ = refine(hyp["R"][h], hyp["t"][h], cam, Xu, uvu, hyp["masks"][h], reproj_error, refine_iterations, refine_rounds)
        T[:3, :3], T[:3, 3] = R, t
    inl = np.zeros(len(X), dtype=bool)
    inl[np.nonzero(use)[0]] = mask
    return dict(out, T=T, status=0 if mask.sum() >= min_inliers else 1, inliers=inl, best_hypothesis=h, hyp=hyp)


def register(kf_from, kf_to, cam, nndr=0.8, **kwargs):
    """(matches, pnp_ransac record) of two keyframes (keypoints, points, descriptors)."""
    rows = match(kf_from[2], kf_to[2], nndr)
    X = np.asarray(kf_from[1], dtype=np.float64)[rows[:, 0]]
    uv = np.asarray(kf_to[0], dtype=np.float64)[rows[:, 1]]
    return rows, pnp_ransac(X, uv, cam, **kwargs)


# ---- scenes of the tests -------------------------------------------------------------------------------------------
CAM = np.array([525.0, 525.0, 319.5, 239.5])               # 640 x 480


def random_rotation(rng, max_deg):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    return se3_exp(np.concatenate([axis * np.deg2rad(rng.uniform(0.0, max_deg)), np.zeros(3)]))[0]


def planted_scene(seed, M=200, outliers=0.5, noise=0.5, max_deg=30.0, cam=CAM, shape=None):
    """M correspondences of a planted T ("from" camera -> "to" camera): "to" pixels uniform over 640 x 480 at depths 1-10 m,
    +-noise px uniform, the first round(outliers M) rows (after a shuffle) replaced by random pixels.  `shape`: None,
    "plane" (all points on one plane of the "from" frame) or "line".  Returns (X, uv, T, is_outlier)."""
    rng = np.random.default_rng(seed)
    R = random_rotation(rng, max_deg)
    t = rng.uniform(-0.5, 0.5, 3)
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = R, t
    px = np.stack([rng.uniform(0.0, 640.0, M), rng.uniform(0.0, 480.0, M)], axis=1)
    depth = rng.uniform(1.0, 10.0, M)
    P = np.stack([(px[:, 0] - cam[2]) / cam[0] * depth, (px[:, 1] - cam[3]) / cam[1] * depth, depth], axis=1)     # "to" frame
    if shape == "plane":                                    # z = 4 + 0.3 x - 0.2 y in the "to" frame
        depth = 4.0 / (1.0 - 0.3 * (px[:, 0] - cam[2]) / cam[0] + 0.2 * (px[:, 1] - cam[3]) / cam[1])
        P = np.stack([(px[:, 0] - cam[2]) / cam[0] * depth, (px[:, 1] - cam[3]) / cam[1] * depth, depth], axis=1)
    elif shape == "line":
        s = rng.uniform(-1.0, 1.0, M)
        P = np.array([0.2, -0.1, 4.0]) + s[:, None] * np.array([1.0, 0.5, 0.8])
        px = np.stack([cam[0] * P[:, 0] / P[:, 2] + cam[2], cam[1] * P[:, 1] / P[:, 2] + cam[3]], axis=1)
    X = (P - t) @ R                                          # R^T (P - t)
    uv = px + rng.uniform(-noise, noise, (M, 2)) if noise > 0.0 else px.copy()
    out = np.zeros(M, dtype=bool)
    out[rng.permutation(M)[:int(round(outliers * M))]] = True
    uv[out] = np.stack([rng.uniform(0.0, 640.0, out.sum()), rng.uniform(0.0, 480.0, out.sum())], axis=1)
    return X, uv, T, out


def keyframe_pair(seed, landmarks=600, distractors=200, flips=10, no_depth=0.1, cam=CAM):
    """Two synthetic keyframes (keypoints, points, descriptors) of `landmarks` common landmarks, each with `distractors`
    keypoints of its own, descriptors with at most `flips` flipped bits between the views, a share of keypoints without depth
    (NaN points), rows shuffled per view.  Returns (kf_from, kf_to, T, landmark id per row of each: -1 = distractor)."""
    rng = np.random.default_rng(seed)
    X, uv_to, T, _ = planted_scene(seed + 1000, M=landmarks, outliers=0.0, noise=0.5, max_deg=20.0, cam=cam)
    uv_from = np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], axis=1)
    desc = rng.integers(0, 256, (landmarks, 32), dtype=np.uint8)

    def view(uv, pts, d):
        n = landmarks + distractors
        bits = np.unpackbits(d, axis=1)
        for k in range(landmarks):
            bits[k, rng.choice(256, rng.integers(0, flips + 1), replace=False)] ^= 1
        dd = np.concatenate([np.packbits(bits, axis=1), rng.integers(0, 256, (distractors, 32), dtype=np.uint8)])
        kp = np.concatenate([uv, np.stack([rng.uniform(0, 640, distractors), rng.uniform(0, 480, distractors)], axis=1)])
        depth = rng.uniform(1.0, 10.0, distractors)
        far = np.stack([(kp[landmarks:, 0] - cam[2]) / cam[0] * depth, (kp[landmarks:, 1] - cam[3]) / cam[1] * depth, depth], axis=1)
        p3 = np.concatenate([pts, far])
        p3[rng.random(n) < no_depth] = np.nan
        ids = np.concatenate([np.arange(landmarks), -np.ones(distractors, dtype=np.int64)])
        o = rng.permutation(n)
        return (kp[o].astype(np.float32), p3[o].astype(np.float32), dd[o]), ids[o]

    P_to = X @ T[:3, :3].T + T[:3, 3]
    kf_a, ids_a = view(uv_from, X, desc)
    kf_b, ids_b = view(uv_to, P_to, desc)
    return kf_a, kf_b, T, ids_a, ids_b


HYP_GUARD = 1e-5               # hypotheses whose guard is below it are left out of the per-hypothesis comparison (test_vis_gpu.py)
HYP_SIZES = (4, 5, 63, 64, 65, 257)


def hyp_scene(M):
    """The scene of M correspondences of the per-hypothesis tests; its sampler seed is M."""
    return planted_scene(40 + M, M=M, outliers=0.3)
