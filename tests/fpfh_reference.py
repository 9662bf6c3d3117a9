"""Float64 restatement of the rules of csrc/fpfh.hip (a helper for the FPFH tests, not a test): neighbour lists, normals,
SPFH / FPFH and nearest neighbours in feature space, as include/cslam_hip.h states them.

The rules follow open3d's EstimateNormals.cpp and Feature.cpp in structure; no open3d is available where these tests
run, so parity with open3d itself is not pinned.  Normals come from `numpy.linalg.eigh`, matching is stated twice: by
`argmin` and by `scipy.spatial.cKDTree` exactly as the reference's `find_knn_cpu` does it (icp_utils.py:40-46).
Also here: the scene of the tests, and the measures of how close a scene comes to the decisions that rounding could turn.
"""
import numpy as np
from scipy.spatial import cKDTree

from icp_reference import voxel_average

BINS = 33
EDGE = 1e-9                   # a pair feature closer than this to a decision is "edge-close"


# ---- rule 1: neighbour lists ------------------------------------------------------------------------------------------
def sq_distances(pts, i):
    d = pts - pts[i]
    return d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0])


def radius_neighbors(pts, radius, max_nn):
    """(idx [n, max_nn] int32 padded with -1, d2 [n, max_nn] padded with inf, count [n]): point i first, then the others
    with d2 <= radius^2 in ascending (d2, index), max_nn entries in all."""
    pts = np.asarray(pts, dtype=np.float64)
    n = len(pts)
    idx = np.full((n, max_nn), -1, dtype=np.int32)
    d2 = np.full((n, max_nn), np.inf)
    count = np.zeros(n, dtype=np.int32)
    r2 = radius * radius
    for i in range(n):
        d = sq_distances(pts, i)
        others = np.nonzero(d <= r2)[0]
        others = others[others != i]
        others = others[np.lexsort((others, d[others]))][:max_nn - 1]
        k = 1 + len(others)
        idx[i, 0], d2[i, 0] = i, 0.0
        idx[i, 1:k], d2[i, 1:k] = others, d[others]
        count[i] = k
    return idx, d2, count


def prefix_counts(d2, count, radius, max_nn):
    """Entries of each list that a search at (radius, max_nn) returns: the first min(max_nn, entries with d2 <= r^2)."""
    within = (d2 <= radius * radius).sum(axis=1)
    return np.minimum(np.minimum(count, max_nn), within).astype(np.int32)


# ---- rule 2: normals --------------------------------------------------------------------------------------------------
def covariances(pts, idx, k):
    """[n, 3, 3] covariance of the first k[i] list entries relative to point i (zeros where k < 3)."""
    n = len(pts)
    cov = np.zeros((n, 3, 3))
    for i in range(n):
        if k[i] >= 3:
            q = pts[idx[i, :k[i]]] - pts[i]
            c = q - q.sum(axis=0) / k[i]
            cov[i] = c.T @ c / k[i]
    return cov


def orient(normals, pts, viewpoint):
    """n . (viewpoint - p) >= 0; where it is exactly 0 the component of largest magnitude is positive."""
    out = normals.copy()
    dot = (out * (np.asarray(viewpoint, dtype=np.float64) - pts)).sum(axis=1)
    big = np.abs(out).argmax(axis=1)
    flip = (dot < 0) | ((dot == 0) & (out[np.arange(len(out)), big] < 0))
    out[flip] = -out[flip]
    return out


def estimate_normals(pts, idx, d2, count, radius, max_nn, viewpoint=(0.0, 0.0, 0.0), return_eigenvalues=False):
    pts = np.asarray(pts, dtype=np.float64)
    k = prefix_counts(d2, count, radius, max_nn)
    w, v = np.linalg.eigh(covariances(pts, idx, k))
    normals = v[:, :, 0].copy()
    normals[k < 3] = (0.0, 0.0, 1.0)
    normals = orient(normals, pts, viewpoint)
    return (normals, w, k) if return_eigenvalues else normals


def angles(a, b):
    """Angle between the rows of a and b, accurate near 0."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1))


# ---- rule 3: SPFH and FPFH ----------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def pair_features(p1, n1, p2, n2):
    """open3d's ComputePairFeatures for rows of pairs: f [m, 3] and |a1| - |a2|, the quantity its swap decides on."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = p2 - p1
        length = np.sqrt(_dot(d, d))
        a1, a2 = _dot(n1, d) / length, _dot(n2, d) / length
        swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
        m1 = np.where(swap[:, None], n2, n1)
        m2 = np.where(swap[:, None], n1, n2)
        d = np.where(swap[:, None], -d, d)
        f2 = np.where(swap, -a2, a1)
        v = np.cross(d, m1)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = np.cross(m1, v)
        f = np.stack([np.arctan2(_dot(w, m2), _dot(m1, m2)), _dot(v, m2), f2], axis=1)
    zero = (length == 0.0) | (vn == 0.0)
    f[zero] = 0.0
    return f, np.where(zero, np.inf, np.abs(a1) - np.abs(a2))


def bin_coordinates(f):
    """Before floor and clamp: 11 (f0 + pi) / (2 pi), 11 (f1 + 1) / 2, 11 (f2 + 1) / 2."""
    return np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) / 2.0, 11.0 * (f[:, 2] + 1.0) / 2.0], axis=1)


def compute_spfh(pts, normals, idx, count, return_edge=False):
    """[n, 33] SPFH: integer counts times 100 / (k - 1).  With `return_edge` also the number of edge-close pairs of every
    point: pairs with a feature within EDGE of an inner bin edge, or with ||a1| - |a2|| < EDGE at the swap."""
    pts = np.asarray(pts, dtype=np.float64)
    n, width = idx.shape
    k = np.minimum(count, width)
    e = np.arange(width)[None, :]
    rows, cols = np.nonzero((e >= 1) & (e < k[:, None]))
    j = idx[rows, cols]
    f, swap_margin = pair_features(pts[rows], normals[rows], pts[j], normals[j])
    x = bin_coordinates(f)
    with np.errstate(invalid="ignore"):
        b = np.where(x >= 0, np.clip(np.floor(x), 0, 10), 0).astype(np.int64)
    counts = np.zeros((n, BINS), dtype=np.int64)
    for g in range(3):
        np.add.at(counts, (rows, 11 * g + b[:, g]), 1)
    scale = np.where(k > 1, 100.0 / np.maximum(k - 1, 1), 0.0)
    spfh = counts * scale[:, None]
    if not return_edge:
        return spfh
    nearest = np.clip(np.round(x), 1, 10)                          # inner edges only: 0 and 11 are clamped away
    to_edge = np.abs(x - nearest) * np.array([2.0 * np.pi / 11.0, 2.0 / 11.0, 2.0 / 11.0])
    close = (to_edge < EDGE).any(axis=1) | (np.abs(swap_margin) < EDGE)
    n_edge = np.zeros(n, dtype=np.int64)
    np.add.at(n_edge, rows[close], 1)
    return spfh, n_edge


def compute_fpfh(spfh, idx, d2, count):
    n, width = idx.shape
    out = np.zeros((n, BINS))
    for i in range(n):
        acc = np.zeros(BINS)
        for e in range(1, min(int(count[i]), width)):
            if d2[i, e] != 0.0:
                acc = acc + spfh[idx[i, e]] / d2[i, e]
        for g in range(3):
            s = np.cumsum(acc[11 * g:11 * g + 11])[-1]              # ascending bin order
            if s != 0.0:
                acc[11 * g:11 * g + 11] = acc[11 * g:11 * g + 11] * (100.0 / s)
        out[i] = acc + spfh[i]
    return out


def extract_fpfh(pts, voxel_size, viewpoint=(0.0, 0.0, 0.0)):
    """The reference's `extract_fpfh` (icp_utils.py:26-37) by the rules above, with two separate searches."""
    pts = np.asarray(pts, dtype=np.float64)
    normals = estimate_normals(pts, *radius_neighbors(pts, 2.0 * voxel_size, 30), 2.0 * voxel_size, 30, viewpoint)
    idx, d2, count = radius_neighbors(pts, 5.0 * voxel_size, 100)
    return compute_fpfh(compute_spfh(pts, normals, idx, count), idx, d2, count)


# ---- rule 4: matching ---------------------------------------------------------------------------------------------------
def match_argmin(a, b, return_distance=False):
    """argmin_j sum_d (a_d - b_d)^2, the sum accumulated in ascending d, ties -> the lower j."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nn = np.empty(len(a), dtype=np.int64)
    dist = np.empty(len(a))
    for i0 in range(0, len(a), 512):
        blk = a[i0:i0 + 512]
        acc = np.zeros((len(blk), len(b)))
        for d in range(a.shape[1]):
            df = blk[:, d, None] - b[None, :, d]
            acc = acc + df * df
        nn[i0:i0 + 512] = acc.argmin(axis=1)
        dist[i0:i0 + 512] = acc.min(axis=1)
    return (nn, dist) if return_distance else nn


def match_kdtree(a, b):
    """The reference's find_knn_cpu (icp_utils.py:40-46) with knn = 1."""
    _, nn = cKDTree(b).query(a, k=1)
    return np.asarray(nn, dtype=np.int64)


def mutual(nn01, nn10):
    """The reference's find_correspondences from the two nearest-neighbour arrays (icp_utils.py:49-65)."""
    idx0 = np.arange(len(nn01))
    keep = nn10[nn01] == idx0
    return idx0[keep], nn01[keep]


def find_correspondences(a, b):
    return mutual(match_argmin(a, b), match_argmin(b, a))


# ---- the scene of the tests -----------------------------------------------------------------------------------------------
VOXEL = 0.5
SCENE_SHIFT = np.array([13.0, 9.5, -1.9])       # the sensor (the origin) is outside the scene and 1.9 m above its ground
SCENE_SEEDS = (1, 2, 3)


def feature_scene(seed, n_raw=8000, voxel=VOXEL):
    """A scene dense enough for the features to mean something: a 16 x 16 m undulating ground z = 0.4 sin(0.5 x) cos(0.4 y)
    with 2 cm noise (5/8 of the raw points) and three noisy wall patches, shifted off the origin and voxel-averaged:
    about 1.4k points at 0.5 m."""
    rng = np.random.default_rng(seed)
    n_ground = n_raw * 5 // 8
    x, y = rng.uniform(-8, 8, n_ground), rng.uniform(-8, 8, n_ground)
    parts = [np.stack([x, y, 0.4 * np.sin(0.5 * x) * np.cos(0.4 * y) + 0.02 * rng.standard_normal(n_ground)], axis=1)]
    per_wall = (n_raw - n_ground) // 3
    walls = (((-5.0, -6.0), (1.0, 0.15), 7.0, 3.5), ((2.0, 1.0), (-0.2, 1.0), 6.0, 4.0), ((-4.0, 5.0), (0.8, -0.6), 8.0, 3.0))
    for (cx, cy), (ux, uy), length, height in walls:
        u = np.array([ux, uy]) / np.hypot(ux, uy)
        s = rng.uniform(-length / 2, length / 2, per_wall)
        h = rng.uniform(0.0, height, per_wall)
        off = 0.02 * rng.standard_normal(per_wall)                   # across the wall
        parts.append(np.stack([cx + s * u[0] - off * u[1], cy + s * u[1] + off * u[0], h], axis=1))
    return voxel_average(np.concatenate(parts) + SCENE_SHIFT, voxel)


def moved_copy(pts, seed):
    """A rigidly moved, row-permuted copy: (copy, T, perm) with copy[k] = T . pts[perm[k]]; the viewpoint of the copy
    is T . origin = T[:3, 3]."""
    rng = np.random.default_rng(1000 + seed)
    a, b, c = np.deg2rad(rng.uniform(20, 160)), np.deg2rad(rng.uniform(-8, 8)), np.deg2rad(rng.uniform(-8, 8))
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(c), -np.sin(c)], [0.0, np.sin(c), np.cos(c)]])
    T = np.identity(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = rng.uniform(-3, 3, 3)
    perm = rng.permutation(len(pts))
    return pts[perm] @ T[:3, :3].T + T[:3, 3], T, perm


def true_partner_share(idx0, idx1, perm, n):
    """Share of the n points of the scene whose mutual match in the moved copy is their own image: feats0 = the scene,
    feats1 = the copy, whose row k is the image of scene row perm[k]."""
    return float((perm[idx1] == idx0).sum()) / n


# ---- how close a scene comes to a decision ------------------------------------------------------------------------------
def list_margins(d2, count, radius):
    """Smallest relative distance between two consecutive d2 of a list (the caller passes uncut lists, so that the
    entries on both sides of a cut are compared too)."""
    gap = np.inf
    for i in range(len(d2)):
        row = d2[i, 1:count[i]]
        if len(row) >= 2:
            gap = min(gap, float((np.diff(row) / row[1:]).min()))
    return gap


def radius_margin(pts, radius):
    """Smallest relative distance between a d2 of the cloud and radius^2."""
    r2 = radius * radius
    m = np.inf
    for i in range(len(pts)):
        d = sq_distances(pts, i)
        m = min(m, float(np.abs(d - r2).min() / r2))
    return m
