"""The level-aware PnP RANSAC of include/cslam_hip.h and csrc/pnp.h restated in float64 numpy, on top of vis_reference.py
(which stays as it is): sigma2[l] = 36^l / 25^l scales the inlier threshold of a correspondence whose "to" keypoint has
level l and divides its Gauss-Newton terms.  Sampler, P3P, selection, best key, stopping and status rules are
vis_reference's."""
import numpy as np

import vis_reference as vr

MAX_LEVEL = 7
SIGMA2 = np.array([np.float64(36 ** l) / np.float64(25 ** l) for l in range(MAX_LEVEL + 1)])


def inliers(e2, s2, reproj_error):
    """The weighted inlier rule on squared errors e2 (inf: depth not positive)."""
    return e2 <= (reproj_error * reproj_error) * s2


def guard(e2, s2, reproj_error):
    """The smallest | sqrt(e2 / sigma2) - threshold | in pixels over the correspondences with a finite error."""
    fin = np.isfinite(e2)
    return float(np.abs(np.sqrt(e2[fin] / s2[fin]) - reproj_error).min()) if fin.any() else np.inf


def hypotheses(X, uv, s2, cam, iterations, reproj_error, seed):
    """vis_reference.hypotheses (poses and validity are its own) with the masks, counts and threshold guards of the weighted rule."""
    hyp = vr.hypotheses(X, uv, cam, iterations, reproj_error, seed)
    for h in range(iterations):
        hyp["guard_threshold"][h] = np.inf
        if hyp["valid"][h]:
            e2 = vr.reproj_e2(hyp["R"][h], hyp["t"][h], cam, X, uv)
            hyp["masks"][h] = inliers(e2, s2, reproj_error)
            hyp["count"][h] = hyp["masks"][h].sum()
            hyp["guard_threshold"][h] = guard(e2, s2, reproj_error)
    return hyp


def gn_terms(R, t, cam, X, uv, w):
    """The weighted terms [k, 27] of the correspondences with positive depth: the upper triangle of J^T J row by row, then J^T r,
    each times w."""
    J, r, ok = vr.gn_jacobian(R, t, cam, np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2))
    J, r, w = J[ok], r[ok], np.asarray(w, dtype=np.float64)[ok]
    iu = np.triu_indices(6)
    JtJ = np.einsum("kai,kaj->kij", J, J)[:, iu[0], iu[1]]
    Jtr = np.einsum("kai,ka->ki", J, r)
    return np.concatenate([JtJ, Jtr], axis=1) * w[:, None]


def gn_sums(R, t, cam, X, uv, w):
    """(A [6, 6], b [6]) of the weighted terms."""
    s = gn_terms(R, t, cam, X, uv, w).sum(axis=0)
    A = np.zeros((6, 6))
    iu = np.triu_indices(6)
    A[iu] = s[:21]
    A = A + A.T - np.diag(np.diag(A))
    return A, s[21:]


def refine(R, t, cam, X, uv, s2, mask, reproj_error, refine_iterations, refine_rounds):
    """vis_reference.refine with the weights 1 / sigma2 and the weighted recount: (R, t, mask, steps, guard of the recounts)."""
    steps, g = 0, np.inf
    w = 1.0 / s2
    for _ in range(refine_rounds):
        for _ in range(refine_iterations):
            A, b = gn_sums(R, t, cam, X[mask], uv[mask], w[mask])
            d = vr.gn_solve(A, b)
            if d is None:
                break
            Re, te = vr.se3_exp(d)
            R, t = Re @ R, Re @ t + te
            steps += 1
            if np.linalg.norm(d) < 1e-10:
                break
        e2 = vr.reproj_e2(R, t, cam, X, uv)
        mask = inliers(e2, s2, reproj_error)
        g = min(g, guard(e2, s2, reproj_error))
    return R, t, mask, steps, g


def pnp_ransac(X, uv, levels, cam, iterations=300, reproj_error=2.0, min_inliers=20, refine_iterations=10, refine_rounds=2, seed=0, cap=2048):
    """vis_reference.pnp_ransac with `levels` [given], the level of the "to" keypoint of every correspondence.  The record
    also holds guard: the smallest | sqrt(e2 / sigma2) - threshold | over the best hypothesis' inlier set and every recount."""
    X, uv, cam = np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2), np.asarray(cam, dtype=np.float64)
    levels = np.asarray(levels)
    assert levels.shape == (len(X),) and (len(levels) == 0 or (levels.min() >= 0 and levels.max() <= MAX_LEVEL))
    use = np.isfinite(X).all(axis=1) & np.isfinite(uv).all(axis=1)
    Xu, uvu, s2 = X[use], uv[use], SIGMA2[levels[use]]
    M = len(Xu)
    out = dict(T=np.identity(4), inliers=np.zeros(len(X), dtype=bool), dropped=int(len(X) - M), best_hypothesis=-1, hyp=None, guard=np.inf)
    if M > cap:
        return dict(out, status=3)
    if M < max(4, min_inliers):
        return dict(out, status=2)
    hyp = hypotheses(Xu, uvu, s2, cam, iterations, reproj_error, seed)
    h = vr.best_hypothesis(hyp["count"])
    T, g = np.identity(4), np.inf
    mask = np.zeros(M, dtype=bool)
    if hyp["valid"][h]:
        R, t, mask, _, g = refine(hyp["R"][h], hyp["t"][h], cam, Xu, uvu, s2, hyp["masks"][h], reproj_error, refine_iterations, refine_rounds)
        g = min(g, hyp["guard_threshold"][h])
        T[:3, :3], T[:3, 3] = R, t
    inl = np.zeros(len(X), dtype=bool)
    inl[np.nonzero(use)[0]] = mask
    return dict(out, T=T, status=0 if mask.sum() >= min_inliers else 1, inliers=inl, best_hypothesis=h, hyp=hyp, guard=g)


def register(kf_from, kf_to, cam, nndr=0.8, **kwargs):
    """(matches, pnp_ransac record) of two level keyframes (keypoints, points, descriptors, levels)."""
    rows = vr.match(kf_from[2], kf_to[2], nndr)
    X = np.asarray(kf_from[1], dtype=np.float64)[rows[:, 0]]
    uv = np.asarray(kf_to[0], dtype=np.float64)[rows[:, 1]]
    return rows, pnp_ransac(X, uv, np.asarray(kf_to[3])[rows[:, 1]], cam, **kwargs)


def planted_level_scene(seed, M=200, levels=4, outliers=0.5, base_noise=0.5):
    """vis_reference.planted_scene without noise, then per correspondence a level drawn from 0 .. levels - 1 and pixel noise
    +- base_noise 1.2^l uniform; the gross outliers are the scene's.  Returns (X, uv, levels [M], T, is_outlier)."""
    X, uv, T, out = vr.planted_scene(seed, M=M, outliers=outliers, noise=0.0)
    rng = np.random.default_rng(seed + 7000)
    lv = rng.integers(0, levels, M)
    uv = uv + rng.uniform(-1.0, 1.0, (M, 2)) * (base_noise * 1.2 ** lv)[:, None]
    return X, uv, lv.astype(np.int64), T, out
