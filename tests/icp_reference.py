"""Float64 restatement of open3d's point-to-point `registration_icp` (a helper for the ICP tests, not a test).

open3d's documented loop (pipelines/registration/Registration.cpp, RegistrationICP): evaluate the source at `init`;
then up to `max_iteration` times: fit the rigid transform without scale (Eigen::umeyama: SVD of the 3 x 3 covariance
with the det = -1 reflection fix) to the current correspondences, move the source, re-evaluate, and stop when
|delta fitness| < relative_fitness and |delta inlier_rmse| < relative_rmse (absolute differences).  An evaluation takes
each moved source point's nearest target point, keeps it when the distance is within the radius, and reports
fitness = kept / |source| and inlier_rmse = sqrt(mean d^2 over the kept), both 0 when nothing is kept.

No open3d is available where these tests run, so parity with open3d itself is not pinned; this file follows its
documented algorithm.  Also here: open3d's voxel down-sampling rule and the synthetic street scene of the tests.
"""
import numpy as np
from scipy.spatial import cKDTree

DEFAULT_STAGES = ((4.0, 30), (2.0, 30), (1.0, 100))
SECTOR_DEG = 6.0                      # ScanContext: 360 / 60 sectors


def Rt2T(R, t):
    T = np.identity(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def rot_z(deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def yaw_init(deg):
    """4 x 4 seed: rotation about z by `deg`, no translation."""
    return Rt2T(rot_z(deg), np.zeros(3))


def apply_T(T, pts):
    return pts @ T[:3, :3].T + T[:3, 3]


def apply_T_fma(T, pts):
    """T . p with the rounding of the kernels (csrc/icp.hip icp_apply): per row fma(T0, x, fma(T1, y, fma(T2, z, T3))),
    each fma rounded once.  Exact rational arithmetic, rounded by float(); for the small clouds of the
    correspondence tests, whose 1e-14 bound on d^2 is about the contraction inside d^2, not the rounding of T . p."""
    from fractions import Fraction as F

    def fma(a, b, c):
        return float(F(a) * F(b) + F(c))

    out = np.empty((len(pts), 3))
    for i, (x, y, z) in enumerate(np.asarray(pts, dtype=np.float64).tolist()):
        for r in range(3):
            t0, t1, t2, t3 = (float(v) for v in T[r])
            out[i, r] = fma(t0, x, fma(t1, y, fma(t2, z, t3)))
    return out


def sqdist(p, q):
    d = p - q
    return (d * d).sum(axis=-1)


def nn_brute(p, q):
    """argmin over all of q for each row of p (ties -> lower index); for the small cases."""
    d2 = ((p[:, None, :] - q[None, :, :]) ** 2).sum(axis=-1)
    idx = d2.argmin(axis=1)
    return idx, d2[np.arange(len(p)), idx]


def nn_kdtree(p, tree):
    _, idx = tree.query(p, k=1)
    return idx, sqdist(p, tree.data[idx])


def umeyama_rigid(p, q):
    """R, t minimising sum |q - (R p + t)|^2, no scale (Eigen::umeyama(p, q, false))."""
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    sigma = (q - mq).T @ (p - mp) / len(p)
    U, _, Vt = np.linalg.svd(sigma)
    s = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        s[2] = -1.0
    R = U @ np.diag(s) @ Vt
    return R, mq - R @ mp


class Result:
    def __init__(self, T, fitness, rmse, corr, iterations, history):
        self.transformation = T
        self.fitness = fitness
        self.inlier_rmse = rmse
        self.correspondence_set = corr
        self.iterations = iterations
        self.history = history            # (fitness, inlier_rmse) of every evaluation, history[0] at init


def registration_icp(src, dst, max_correspondence_distance, init=None, max_iteration=100, relative_fitness=1e-6,
                     relative_rmse=1e-6, brute=False):
    src = np.asarray(src, dtype=np.float64)
    dst = np.asarray(dst, dtype=np.float64)
    T = np.identity(4) if init is None else np.array(init, dtype=np.float64)
    tree = None if brute else cKDTree(dst)
    r2 = max_correspondence_distance ** 2

    def evaluate(cur):
        idx, d2 = nn_brute(cur, dst) if brute else nn_kdtree(cur, tree)
        keep = d2 <= r2
        n = int(keep.sum())
        corr = np.stack([np.nonzero(keep)[0], idx[keep]], axis=1)
        if n == 0:
            return 0.0, 0.0, corr
        return n / len(src), float(np.sqrt(d2[keep].sum() / n)), corr

    cur = apply_T(T, src)
    fit, rmse, corr = evaluate(cur)
    history = [(fit, rmse)]
    iterations = 0
    for i in range(max_iteration):
        if len(corr):
            R, t = umeyama_rigid(cur[corr[:, 0]], dst[corr[:, 1]])
            U = Rt2T(R, t)
            T = U @ T
            cur = apply_T(U, cur)
        prev = (fit, rmse)
        fit, rmse, corr = evaluate(cur)
        history.append((fit, rmse))
        iterations = i + 1
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    return Result(T, fit, rmse, corr, iterations, history)


def register_staged(src, dst, voxel_size, init=None, stages=DEFAULT_STAGES, brute=False):
    """The stages back to back, each from the previous stage's transform.  Returns the list of per-stage results."""
    out = []
    T = init
    for mult, iters in stages:
        out.append(registration_icp(src, dst, mult * voxel_size, T, iters, brute=brute))
        T = out[-1].transformation
    return out


def stop_margin(history, tol=1e-6):
    """Smallest distance of a fitness / rmse delta from `tol` over the last two rounds of a stage: the stopping round
    (or the cap) and the round before it.  A GPU run whose sums differ in the last bits takes the same decisions as
    long as this is far above that difference."""
    m = np.inf
    for k in (len(history) - 1, len(history) - 2):
        if k >= 1:
            for a, b in zip(history[k], history[k - 1]):
                m = min(m, abs(abs(a - b) - tol))
    return m


def rotation_error_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def voxel_average(points, voxel):
    """open3d's voxel_down_sample: origin = min - voxel / 2, voxel index = floor((p - origin) / voxel), one output point
    per occupied voxel = the mean of its points.  open3d's output order is that of a hash map; here voxels come in
    lexicographic index order."""
    pts = np.asarray(points, dtype=np.float64)
    pts = pts[np.isfinite(pts).all(axis=1)]
    origin = pts.min(axis=0) - voxel / 2.0
    key = np.floor((pts - origin) / voxel).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    out = np.zeros((len(cnt), 3))
    np.add.at(out, inv, pts)
    return out / cnt[:, None]


def street_scene(seed, n_raw=9000, voxel=0.5):
    """Two scans of one synthetic street from two poses.  Returns (src, dst, T_true, yaw_deg) with dst ~ T_true . src.

    A 60 x 60 m ground patch with 2 cm z noise (half the raw points) and 14 box outlines (walls only) 2-8 m wide and
    2-6 m high; two independent 60 % subsamples; the second gets 2 cm noise and is moved by a yaw in U(20, 160) degrees
    and t in (+-1.5, +-1.5, +-0.2) m; both are voxel-averaged."""
    rng = np.random.default_rng(seed)
    n_ground = n_raw // 2
    ground = np.stack([rng.uniform(-30, 30, n_ground), rng.uniform(-30, 30, n_ground),
                       0.02 * rng.standard_normal(n_ground)], axis=1)
    parts = [ground]
    n_box = 14
    per_box = (n_raw - n_ground) // n_box
    for _ in range(n_box):
        cx, cy = rng.uniform(-25, 25, 2)
        wx, wy = rng.uniform(2, 8, 2)
        h = rng.uniform(2, 6)
        s = rng.uniform(0, 2 * (wx + wy), per_box)           # position along the outline
        x = np.where(s < wx, s, np.where(s < wx + wy, wx, np.where(s < 2 * wx + wy, 2 * wx + wy - s, 0.0)))
        y = np.where(s < wx, 0.0, np.where(s < wx + wy, s - wx, np.where(s < 2 * wx + wy, wy, 2 * (wx + wy) - s)))
        parts.append(np.stack([cx - wx / 2 + x, cy - wy / 2 + y, rng.uniform(0, h, per_box)], axis=1))
    raw = np.concatenate(parts)
    a = raw[rng.random(len(raw)) < 0.6]
    b = raw[rng.random(len(raw)) < 0.6]
    b = b + 0.02 * rng.standard_normal(b.shape)
    yaw = float(rng.uniform(20, 160))
    t = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-0.2, 0.2)])
    T_true = Rt2T(rot_z(yaw), t)
    return voxel_average(a, voxel), voxel_average(apply_T(T_true, b), voxel), T_true, yaw


def seed_yaw(yaw_deg):
    """The true yaw as ScanContext would report it: rounded to its 6 degree sector."""
    return SECTOR_DEG * np.round(yaw_deg / SECTOR_DEG)
