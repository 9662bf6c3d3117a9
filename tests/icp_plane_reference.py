"""Float64 restatement of the point-to-plane update of csrc/plane.h (a helper for the point-to-plane tests, not a test).

The rule, as include/cslam_hip.h states it: for the kept correspondences (p = T . src_i, q its nearest target point, n the
target's normal at q)  r = (p - q) . n,  J = [(p - o) x n, n],  A = sum J J^T,  b = sum J r,  o = the pair's sum origin
(the first target point rounded to a 1024 m grid);  x = -A^-1 b by an unpivoted LDL^T, det A = the product of D;  the
update is the identity with fewer than six correspondences, a zero pivot, a NaN / infinite / |.| < 1e-6 determinant or a
non-finite solution;  U' = (Rz(x2) Ry(x1) Rx(x0), (x3, x4, x5)) about o, t = t' + o - R o in the frame.  The loop around
it -- correspondences, fitness, inlier_rmse, the stopping rule, the stages -- is that of tests/icp_reference.py.

No open3d is available where these tests run: the determinant rule restates open3d's SolveLinearSystemPSD from memory and
parity with open3d itself is not pinned.
"""
import numpy as np
from scipy.spatial import cKDTree

import fpfh_reference as fref
import icp_reference as ref

LD = np.longdouble
MIN_DET = 1e-6
ORIGIN_GRID = 1024.0
NSUM = 29


def sum_origin(q0):
    return ORIGIN_GRID * np.rint(np.asarray(q0, dtype=np.float64) / ORIGIN_GRID)


def reference_normals(dst, voxel):
    """The targets' normals at the reference's `extract_fpfh` parameters (2 voxels, 30 neighbours, viewpoint at the origin)."""
    return fref.estimate_normals(dst, *fref.radius_neighbors(dst, 2.0 * voxel, 30), 2.0 * voxel, 30)


def system(p, q, n, o):
    """(A [6, 6], b [6]) of the correspondences, in the dtype of p."""
    J = np.concatenate([np.cross(p - o, n), n], axis=1)
    r = ((p - q) * n).sum(axis=1)
    return J.T @ J, J.T @ r


def ldlt_solve(A, b):
    """(x = -A^-1 b, det A) by an unpivoted LDL^T in the dtype of A; (None, 0.0) at a pivot that is exactly zero."""
    L = np.identity(6, dtype=A.dtype)
    D = np.zeros(6, dtype=A.dtype)
    for j in range(6):
        d = A[j, j] - sum(L[j, m] * L[j, m] * D[m] for m in range(j))
        if d == 0.0:
            return None, 0.0
        D[j] = d
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - sum(L[i, m] * L[j, m] * D[m] for m in range(j))) / d
    y = np.zeros(6, dtype=A.dtype)
    for i in range(6):
        y[i] = -b[i] - sum(L[i, m] * y[m] for m in range(i))
    y = y / D
    x = np.zeros(6, dtype=A.dtype)
    for i in range(5, -1, -1):
        x[i] = y[i] - sum(L[m, i] * x[m] for m in range(i + 1, 6))
    return x, D.prod()


def solve(A, b, count):
    """(x or None where the update is the identity, det A as the rule computes it)."""
    if count < 6:
        return None, 0.0
    with np.errstate(all="ignore"):
        x, det = ldlt_solve(A, b)
    if x is None or not np.isfinite(det) or abs(det) < MIN_DET or not np.all(np.isfinite(x)):
        return None, float(det)
    return x, float(det)


def rotation(x):
    """Rz(x2) . Ry(x1) . Rx(x0), in the dtype of x."""
    sx, cx, sy, cy, sz, cz = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]], dtype=x.dtype)


def update(p, q, n, o=None):
    """(U [4, 4] in frame coordinates, det A) of one update from the moved source points p, their target points q and the
    normals n at q; U is the identity where the rule says so."""
    o = np.zeros(3) if o is None else np.asarray(o, dtype=np.float64)
    U = np.identity(4)
    if len(p) == 0:
        return U, 0.0
    A, b = system(p, q, n, o)
    x, det = solve(A, b, len(p))
    if x is not None:
        U[:3, :3] = rotation(x)
        U[:3, 3] = x[3:] + o - U[:3, :3] @ o
    return U, det


class UpdateLD:
    """One update in numpy.longdouble: `moved(pts)` = R (pts - o) + t' + o without rounding to float64 on the way."""

    def __init__(self, p, q, n, o):
        self.o = np.asarray(o, dtype=LD)
        A, b = system(np.asarray(p, dtype=LD), np.asarray(q, dtype=LD), np.asarray(n, dtype=LD), self.o)
        self.x, self.det = ldlt_solve(A, b)
        assert self.x is not None and len(p) >= 6
        self.R = rotation(self.x)

    def moved(self, pts):
        return (np.asarray(pts, dtype=LD) - self.o) @ self.R.T + self.x[3:] + self.o


def registration_icp(src, dst, normals, max_correspondence_distance, init=None, max_iteration=100, relative_fitness=1e-6,
                     relative_rmse=1e-6, brute=False):
    """icp_reference.registration_icp with the point-to-plane update.  Every round moves the ORIGINAL source by the
    accumulated transform, as the kernels do.  Returns an icp_reference.Result with `dets`: det A of every update."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    T = np.identity(4) if init is None else np.array(init, dtype=np.float64)
    tree = None if brute else cKDTree(dst)
    r2 = max_correspondence_distance ** 2
    o = sum_origin(dst[0])

    def evaluate(cur):
        idx, d2 = ref.nn_brute(cur, dst) if brute else ref.nn_kdtree(cur, tree)
        keep = d2 <= r2
        k = int(keep.sum())
        corr = np.stack([np.nonzero(keep)[0], idx[keep]], axis=1)
        if k == 0:
            return 0.0, 0.0, corr
        return k / len(src), float(np.sqrt(d2[keep].sum() / k)), corr

    cur = ref.apply_T(T, src)
    fit, rmse, corr = evaluate(cur)
    history, dets, iterations = [(fit, rmse)], [], 0
    for i in range(max_iteration):
        if len(corr):
            U, det = update(cur[corr[:, 0]], dst[corr[:, 1]], normals[corr[:, 1]], o)
            dets.append(det)
            T = U @ T
            cur = ref.apply_T(T, src)
        prev = (fit, rmse)
        fit, rmse, corr = evaluate(cur)
        history.append((fit, rmse))
        iterations = i + 1
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    out = ref.Result(T, fit, rmse, corr, iterations, history)
    out.dets = dets
    return out


def register_staged(src, dst, normals, voxel_size, init=None, stages=ref.DEFAULT_STAGES, brute=False):
    out, T = [], init
    for mult, iters in stages:
        out.append(registration_icp(src, dst, normals, mult * voxel_size, T, iters, brute=brute))
        T = out[-1].transformation
    return out


def nn_margin(moved, dst, radius):
    """How far the correspondences are from turning: (smallest (second-nearest - nearest) distance over the source points
    whose nearest target is within 2 radii, smallest | nearest - radius |)."""
    d, _ = cKDTree(dst).query(moved, k=2)
    near = d[:, 0] <= 2.0 * radius
    return float((d[near, 1] - d[near, 0]).min()), float(np.abs(d[:, 0] - radius).min())


# ---- the sums of icp_merge_kernel<PLANE> + icp_solve_kernel<PLANE> in numpy, in the kernels' order ---------------------
def kernel_sums(p, q, n, keep, origin):
    """The 29 sums for source rows `p` (already moved), their nearest target rows `q`, the normals `n` at those, the kept
    mask and the sums' origin: n, d^2, the upper triangle of J J^T row by row, J r; zeros for a dead row; a shuffle tree per
    wave, waves in order, blocks in order."""
    m = len(p)
    v = np.zeros((-(-m // 256) * 256, NSUM))
    J = np.concatenate([np.cross(p - origin, n), n], axis=1)
    d = p - q
    v[:m, 0] = 1.0
    v[:m, 1] = d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0])
    k = 2
    for i in range(6):
        for j in range(i, 6):
            v[:m, k] = J[:, i] * J[:, j]
            k += 1
    v[:m, 23:29] = J * (d * n).sum(axis=1)[:, None]
    v[:m][~keep] = 0.0
    total = np.zeros(NSUM)
    for blk in range(len(v) // 256):
        waves = [ref.wave_tree(v[256 * blk + 64 * w:256 * blk + 64 * (w + 1)]) for w in range(4)]
        acc = waves[0]
        for w in waves[1:]:
            acc = acc + w
        total = total + acc
    return total


def planted_normals(count, seed):
    """`count` unit normals spread over the sphere (no two families: every direction is constrained)."""
    rng = np.random.default_rng(7000 + seed)
    v = rng.standard_normal((count, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)
