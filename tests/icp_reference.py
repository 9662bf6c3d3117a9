"""Float64 restatement of open3d's point-to-point `registration_icp` (a helper for the ICP tests, not a test).

open3d's documented loop (pipelines/registration/Registration.cpp, RegistrationICP): evaluate the source at `init`;
then up to `max_iteration` times: fit the rigid transform without scale (Eigen::umeyama: SVD of the 3 x 3 covariance
with the det = -1 reflection fix) to the current correspondences, move the source, re-evaluate, and stop when
|delta fitness| < relative_fitness and |delta inlier_rmse| < relative_rmse (absolute differences).  An evaluation takes
each moved source point's nearest target point, keeps it when the distance is within the radius, and reports
fitness = kept / |source| and inlier_rmse = sqrt(mean d^2 over the kept), both 0 when nothing is kept.

No open3d is available where these tests run, so parity with open3d itself is not pinned; this file follows its
documented algorithm.  Also here: open3d's voxel down-sampling rule, the synthetic street scene of the tests, and (at the
end) the extended-precision rigid fit, the generators and the kernel-order sums of tests/test_rigid_fit_*.py.
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


# ---- the rigid fit itself: an extended-precision reference and the generators of tests/test_rigid_fit_*.py ----------
LD = np.longdouble
ULP_BOUND = 256.0                     # moved points: at most this many ulp of the largest coordinate from the reference


class RigidFit:
    """R [3, 3] and t [3] (float64), the singular values of the covariance (descending), the means (longdouble)."""

    def __init__(self, R, t, sv, mp, mq):
        self.R, self.t, self.sv, self.mp, self.mq = R, t, sv, mp, mq

    def moved(self, pts):
        """R (p - mean p) + mean q in extended precision: no cancellation against a large translation."""
        return (np.asarray(pts, dtype=LD) - self.mp) @ self.R.astype(LD).T + self.mq

    def rmse(self, p, q, w=None):
        r = np.asarray(q, dtype=LD) - self.moved(p)
        w = np.ones(len(r), dtype=LD) if w is None else np.asarray(w, dtype=LD)
        return float(np.sqrt((w * (r * r).sum(axis=1)).sum() / w.sum()))


def rigid_fit_ld(p, q, w=None, centre=True):
    """The proper rotation R and t minimising sum w |q - (R p + t)|^2, no scale.  Means and centred products in
    numpy.longdouble (64-bit mantissa where these tests run), the SVD of the 3 x 3 covariance in float64 with the
    det = -1 correction.  `centre=False`: no centring and t = 0, the chain rotation of csrc/robust.hip."""
    p, q = np.asarray(p, dtype=LD).reshape(-1, 3), np.asarray(q, dtype=LD).reshape(-1, 3)
    w = np.ones(len(p), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    zero = np.zeros(3, dtype=LD)
    mp = (w[:, None] * p).sum(axis=0) / w.sum() if centre else zero
    mq = (w[:, None] * q).sum(axis=0) / w.sum() if centre else zero
    sigma = ((q - mq) * w[:, None]).T @ (p - mp) / w.sum()
    U, sv, Vt = np.linalg.svd(sigma.astype(np.float64))
    s = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        s[2] = -1.0
    R = U @ np.diag(s) @ Vt
    t = (mq - mp @ R.astype(LD).T).astype(np.float64)
    return RigidFit(R, t, sv, mp, mq)


def moved_ld(T, pts):
    """T . p in extended precision for a float64 4 x 4 (or 3 x 3: no translation)."""
    T = np.asarray(T, dtype=LD)
    out = np.asarray(pts, dtype=LD) @ T[:3, :3].T
    return out + T[:3, 3] if T.shape[1] == 4 else out


def coord_ulp(*sets):
    """One ulp of the largest |coordinate| over the given point sets."""
    return float(np.spacing(max(float(np.abs(np.asarray(s, dtype=np.float64)).max()) for s in sets if len(s))))


def moved_error_ulps(T, fit, pts, *coords):
    """max |T . p - T_ref . p| over `pts` in ulp of the largest coordinate of `coords` (default: pts)."""
    err = float(np.abs(moved_ld(T, pts) - fit.moved(pts)).max())
    return err / coord_ulp(*(coords or (pts,)))


def rotation_defects(R):
    return float(np.abs(R @ R.T - np.identity(3)).max()), abs(float(np.linalg.det(R)) - 1.0)


ANGLES_DEG = (0.0, 1e-12, 1e-8, 1.0, 90.0, 179.0, 180.0 - 1e-6, 180.0)
AXES = {"z": (0.0, 0.0, 1.0), "x": (1.0, 0.0, 0.0), "diagonal": (1.0, 1.0, 1.0), "generic": (0.3, -0.8, 0.52)}


def axis_angle(axis, deg):
    """Rodrigues' formula in extended precision, rounded once: exact at 0, 90 and 180 degrees."""
    k = np.asarray(axis, dtype=LD)
    k = k / np.sqrt((k * k).sum())
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=LD)
    a = LD(deg) * LD("3.14159265358979323846264338327950288") / LD(180)
    s, c = np.sin(a), np.cos(a)
    if deg == 0.0:
        s, c = LD(0), LD(1)
    elif deg == 90.0:
        s, c = LD(1), LD(0)
    elif deg == 180.0:
        s, c = LD(0), LD(-1)
    return (np.identity(3, dtype=LD) + s * K + (LD(1) - c) * (K @ K)).astype(np.float64)


def angle_cases():
    """[(name, R)] for every angle about every axis."""
    return [("%s-%g" % (name, deg), axis_angle(axis, deg)) for name, axis in AXES.items() for deg in ANGLES_DEG]


def rotated(R, pts):
    """R . p rounded once from extended precision: noise-free matches."""
    return (np.asarray(pts, dtype=LD) @ np.asarray(R, dtype=LD).T).astype(np.float64)


def chain_all(ms, md):
    """The chain differences csrc/robust.hip fits when every row is a member, in float64 as rb_tim takes them."""
    return ms[1:] - ms[:-1], md[1:] - md[:-1]


def generic_cloud(n, seed, extents=(20.0, 14.0, 9.0)):
    rng = np.random.default_rng(4000 + seed)
    return rng.standard_normal((n, 3)) * np.asarray(extents)


def deficient_clouds():
    """{name: source points} of the rank-deficient and ambiguous sets; `unique` says whether the rotation is defined."""
    rng = np.random.default_rng(4100)
    plane = np.concatenate([rng.uniform(-20, 20, (100, 2)), np.zeros((100, 1))], axis=1)
    line = np.outer(rng.uniform(-20, 20, 40), np.array([0.6, -0.3, 0.74]))
    return {"plane-z0": (plane, True), "plane-z5": (plane + np.array([0.0, 0.0, 5.0]), True), "collinear": (line, False),
            "two-points": (rng.uniform(-20, 20, (2, 3)), False), "one-point": (rng.uniform(-20, 20, (1, 3)), False),
            "coincident": (np.repeat(rng.uniform(-20, 20, (1, 3)), 5, axis=0), False)}


DEFICIENT_R = (0.3, -0.8, 0.52), 37.0          # the motion of the rank-deficient cases: axis, degrees


def reflection_cases():
    """[(name, ms, md)]: the best orthogonal map is a reflection."""
    mirror = np.diag([1.0, 1.0, -1.0])
    a = generic_cloud(200, 1)
    b = generic_cloud(200, 2, (20.0, 10.0, 2.0))
    return [("mirrored", a, a @ mirror), ("anisotropic-mirrored-rotated", b, rotated(axis_angle((0.3, -0.8, 0.52), 63.0), b @ mirror))]


SUM_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513)
LATTICE_RADIUS = 1.0
FAR_OFFSETS = tuple(2.0 ** e for e in (10, 14, 17, 20))
FAR_DIRECTION = np.array([1.0, 0.7, 0.01])


def lattice_pair(kept, seed, R=None, t=None, noise=0.0, scale=1.0, dims=3, lift=0.0):
    """A pair whose correspondences are known: (src, dst, partner).  The source is a jittered lattice (4 m cells, +-0.75 m
    jitter: at least 2.5 m between points) of `kept` + kept // 3 points around the origin; the target is the `kept` of
    them moved by (R, t) (default 0.5 degrees about a generic axis and 0.2 m) with `noise` of Gaussian noise, rows
    permuted.  partner[i] is the target row of source row i, -1 for the third that has none (beyond any radius below
    1.5 m).  `scale` multiplies everything (the radius too is then LATTICE_RADIUS * scale).  `dims` = 2: a lattice in the
    plane z = `lift`; 1: on the x axis."""
    rng = np.random.default_rng(5000 + 7 * kept + seed)
    n = kept + kept // 3
    side = int(np.ceil(n ** (1.0 / dims) - 1e-9))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * dims, indexing="ij"), axis=-1).reshape(-1, dims)
    cells = cells[rng.permutation(len(cells))[:n]]
    src = np.zeros((n, 3))
    src[:, :dims] = (cells - (side - 1) / 2.0) * 4.0 + rng.uniform(-0.75, 0.75, (n, dims))
    src[:, 2] += lift
    has = np.zeros(n, dtype=bool)
    has[rng.permutation(n)[:kept]] = True
    R = axis_angle((0.3, -0.8, 0.52), 0.5) if R is None else R
    t = np.array([0.12, -0.1, 0.11]) if t is None else np.asarray(t, dtype=np.float64)
    moved = rotated(R, src[has]) + t + noise * rng.standard_normal((kept, 3))
    perm = rng.permutation(kept)
    dst = np.empty_like(moved)
    dst[perm] = moved
    partner = np.full(n, -1, dtype=np.int64)
    partner[np.nonzero(has)[0]] = perm
    return src * scale, dst * scale, partner


def nearest_margin(moved_src, dst, partner):
    """(largest distance to a partner, smallest (second-nearest - nearest) over the kept, smallest nearest distance of
    the rows without a partner): the input condition of handle 2."""
    d = np.sqrt(((moved_src[:, None, :] - dst[None, :, :]) ** 2).sum(axis=-1))
    kept = partner >= 0
    order = np.argsort(d, axis=1)
    assert np.array_equal(order[kept, 0], partner[kept])
    first = d[np.arange(len(d)), order[:, 0]]
    second = d[np.arange(len(d)), order[:, 1]] if dst.shape[0] > 1 else np.full(len(d), np.inf)
    return float(first[kept].max()), float((second - first)[kept].min()), float(first[~kept].min()) if (~kept).any() else np.inf


def known_fit(src, dst, partner, init=None):
    """The reference of handle 2: the fit to the known correspondences of the source moved by `init` in extended precision
    (the rounding of the kernels' T . p is theirs, not the reference's).  Returns (RigidFit, the moved kept source points
    as longdouble, their partners)."""
    kept = partner >= 0
    p = moved_ld(np.identity(4) if init is None else init, src[kept])
    q = dst[partner[kept]]
    return rigid_fit_ld(p, q), p, q


# ---- the sums of csrc/icp.hip in numpy, in the kernels' order (for the host build of csrc/horn.h) -------------------
def wave_tree(v):
    """Lane 0 of icp_wave_sum over [64, k] values: v += shfl_down(v, off) for off = 32 .. 1."""
    v = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[:64 - off] = v[:64 - off] + v[off:64]
    return v[0]


def kernel_sums(p, q, keep, origin):
    """The 17 sums of icp_merge_kernel + icp_solve_kernel for source rows `p` (already moved), their nearest target rows
    `q`, the kept mask and the sums' origin: per row n, p - o, q - o, (q - o)(p - o)^T, d^2; zeros for a dead row; a
    shuffle tree per wave, waves in order, blocks in order."""
    n = len(p)
    v = np.zeros((-(-n // 256) * 256, 17))
    ps, qs = p - origin, q - origin
    v[:n, 0] = 1.0
    v[:n, 1:4], v[:n, 4:7] = ps, qs
    for b in range(3):
        for a in range(3):
            v[:n, 7 + 3 * b + a] = qs[:, b] * ps[:, a]
    d = p - q
    v[:n, 16] = d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0])
    v[:n][~keep] = 0.0
    total = np.zeros(17)
    for blk in range(len(v) // 256):
        waves = [wave_tree(v[256 * blk + 64 * w:256 * blk + 64 * (w + 1)]) for w in range(4)]
        acc = waves[0]
        for w in waves[1:]:
            acc = acc + w
        total = total + acc
    return total


def chain_sums(a, b, w=None):
    """The 9 weighted sums of rb_rotation_kernel as the 17 of horn.h: n = 1, zero means, M[3 y + x] = sum w (b_y a_x);
    per thread in ascending k (stride 256), then the tree."""
    w = np.ones(len(a)) if w is None else w
    v = np.zeros((256, 9))
    for k in range(len(a)):
        for y in range(3):
            for x in range(3):
                v[k % 256, 3 * y + x] += w[k] * (b[k, y] * a[k, x])
    waves = [wave_tree(v[64 * i:64 * (i + 1)]) for i in range(4)]
    acc = waves[0]
    for x in waves[1:]:
        acc = acc + x
    s = np.zeros(17)
    s[0] = 1.0
    s[7:16] = acc
    return s


def compose(U, T):
    """T <- U . T as icp_solve_kernel writes it (plain float64, left to right)."""
    out = np.identity(4)
    for a in range(3):
        for b in range(4):
            out[a, b] = U[a, 0] * T[0, b] + U[a, 1] * T[1, b] + U[a, 2] * T[2, b] + (U[a, 3] if b == 3 else 0.0)
    return out


# ---- section C: a scene on a dyadic grid and its copy far from the origin --------------------------------------------
DYADIC = 2.0 ** -10
FAR_C = np.array([2.0 ** 17, 2.0 ** 16, 2.0 ** 10])


def dyadic(pts):
    return np.round(np.asarray(pts, dtype=np.float64) / DYADIC) * DYADIC


def dyadic_scene(seed=5, n=1500):
    """About `n` points of a ground patch and three walls within 12 m, on the 2^-10 m grid, no two equal; and the
    viewpoint (outside the scene, above the ground)."""
    rng = np.random.default_rng(6000 + seed)
    g = n // 2
    parts = [np.stack([rng.uniform(-12, 12, g), rng.uniform(-12, 12, g), 0.02 * rng.standard_normal(g)], axis=1)]
    for x0, y0, dx, dy in ((-8.0, 3.0, 9.0, 0.0), (4.0, -9.0, 0.0, 11.0), (-6.0, -7.0, 6.0, 5.0)):
        m = (n - g) // 3
        s = rng.uniform(0, 1, m)
        parts.append(np.stack([x0 + dx * s, y0 + dy * s, rng.uniform(0, 4, m)], axis=1) + 0.01 * rng.standard_normal((m, 3)))
    pts = np.unique(dyadic(np.concatenate(parts)), axis=0)
    return pts[rng.permutation(len(pts))], np.array([-15.0, -14.0, 1.75])


def registration_icp_ld(src, dst, radius, init=None, max_iteration=100, relative_fitness=1e-6, relative_rmse=1e-6):
    """`registration_icp` with the transform kept in extended precision and the centred fit of `rigid_fit_ld`: every
    round moves the ORIGINAL source by the accumulated transform, as the kernels do, and rounds the moved points to
    float64 for the search only.  Returns a Result whose `transformation` is a longdouble 4 x 4."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    T = np.identity(4, dtype=LD) if init is None else np.asarray(init, dtype=LD).copy()
    tree = cKDTree(dst)
    r2 = radius ** 2

    def evaluate():
        cur = moved_ld(T, src)
        idx, d2 = nn_kdtree(cur.astype(np.float64), tree)
        keep = d2 <= r2
        n = int(keep.sum())
        corr = np.stack([np.nonzero(keep)[0], idx[keep]], axis=1)
        return cur, ((0.0, 0.0) if n == 0 else (n / len(src), float(np.sqrt(d2[keep].sum() / n)))), corr

    cur, (fit, rmse), corr = evaluate()
    history, iterations = [(fit, rmse)], 0
    for i in range(max_iteration):
        if len(corr):
            f = rigid_fit_ld(cur[corr[:, 0]], dst[corr[:, 1]])
            U = np.identity(4, dtype=LD)
            U[:3, :3] = f.R
            U[:3, 3] = f.mq - f.mp @ f.R.astype(LD).T
            T = U @ T
        prev = (fit, rmse)
        cur, (fit, rmse), corr = evaluate()
        history.append((fit, rmse))
        iterations = i + 1
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    return Result(T, fit, rmse, corr, iterations, history)


def street_crop(n=600):
    """The `n` points of each scan of street_scene(103) nearest to one spot of the street (the same spot in both
    frames), the source already turned by the ScanContext seed: (src, dst), a pair that the identity registers."""
    src, dst, T_true, yaw = street_scene(103)
    spot = np.array([4.0, -3.0, 0.0])
    a = src[np.argsort(((src - spot) ** 2).sum(axis=1), kind="stable")[:n]]
    b = dst[np.argsort(((dst - apply_T(T_true, spot[None])[0]) ** 2).sum(axis=1), kind="stable")[:n]]
    return apply_T(yaw_init(seed_yaw(yaw)), a), b
