"""The three rules of csrc/cloud.h restated in numpy: back-projection (float32), the keyframe voxel filter (float32, PCL
VoxelGrid's index rule with the sum order fixed, then the clip on z), and the map assembly (float64).  Ordered sums are
loops.  Parity with PCL itself is unpinned (PCL is not available, and its std::sort is not stable); the kernels are
compared with THIS file bit for bit."""
import numpy as np

F = np.float32
AXIS_LIMIT = 2 ** 21
CELL_LIMIT = 2.0 ** 31

SCENE_CAMERA = (60.0, 61.0, 31.5, 23.5)


class RangeError(ValueError):
    """The cloud's status: a non-finite cell, a cell of magnitude 2^31 or more, or an index of 2^21 or more."""


# ---- back-projection -------------------------------------------------------------------------------------------------
def constants(camera, depth_dtype):
    fx, fy, cx, cy = (float(c) for c in camera)
    unit = float(F(1) * F(0.001)) if depth_dtype == np.uint16 else 1.0
    return F(cx), F(cy), F(unit / fx), F(unit / fy)


def back_project(image, depth, camera):
    """(points float32 [H * W, 3], colors uint8 [H * W, 3]) in row-major pixel order; NaN rows for invalid depths."""
    depth = np.asarray(depth)
    H, W = depth.shape
    cxf, cyf, kx, ky = constants(camera, depth.dtype)
    u = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    with np.errstate(all="ignore"):
        d = depth.astype(F)
        x = ((u - cxf) * d) * kx
        y = ((v - cyf) * d) * ky
        z = d * F(0.001) if depth.dtype == np.uint16 else d
        valid = depth != 0 if depth.dtype == np.uint16 else np.isfinite(depth)
    pts = np.stack([x, y, z], axis=-1).astype(F)
    pts[~valid] = np.nan
    image = np.asarray(image)
    rgb = image[:, :, ::-1] if image.ndim == 3 else np.repeat(image[:, :, None], 3, axis=2)
    return pts.reshape(H * W, 3), np.ascontiguousarray(rgb).reshape(H * W, 3)


def back_project_metres_first(depth, camera):
    """The other formula (metres first, then divide by fx), for the fact that the two differ."""
    fx, fy, cx, cy = (F(c) for c in camera)
    H, W = depth.shape
    z = depth.astype(F) * F(0.001)
    u = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    pts = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=-1).astype(F)
    pts[depth == 0] = np.nan
    return pts.reshape(H * W, 3)


# ---- the shared grid machinery ---------------------------------------------------------------------------------------
def _cells(p, scale):
    """Keyframe rule for float32 (floor(p * inv)), map rule for float64 (floor(p / voxel))."""
    with np.errstate(all="ignore"):
        return np.floor(p * scale) if p.dtype == F else np.floor(p / scale)


def grid_indices(pts, scale):
    """Integer indices [n, 3] of finite rows `pts` (float32 with scale = inv, float64 with scale = voxel): the cell minus
    the cell of the minimum, per axis.  Raises RangeError by the status rule."""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    c0, c1 = _cells(lo, scale), _cells(hi, scale)
    if not (np.all(np.isfinite(c0)) and np.all(np.isfinite(c1)) and np.all(np.abs(c0.astype(np.float64)) < CELL_LIMIT)):
        raise RangeError("cell out of range")
    with np.errstate(all="ignore"):
        q = c1 - c0
    if not np.all((q >= 0) & (q < AXIS_LIMIT)):
        raise RangeError("index of 2^21 or more")
    return (_cells(pts, scale) - c0).astype(np.int64)


def segment_means(pts, colors, ijk):
    """One row per occupied voxel in ascending (iz, iy, ix): xyz summed one point at a time in input order from zero in the
    dtype of `pts`, divided once by the count; colours as integer sums, truncating division."""
    key = (ijk[:, 2] << 42) | (ijk[:, 1] << 21) | ijk[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    starts = np.flatnonzero(np.r_[True, skey[1:] != skey[:-1]]) if len(skey) else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], len(skey)]
    m, T = len(starts), pts.dtype.type
    out = np.zeros((m, 3), dtype=pts.dtype)
    rgb = np.zeros((m, 3), dtype=np.uint8) if colors is not None else None
    counts = (ends - starts).astype(np.int64)
    for r in range(m):
        rows = order[starts[r]:ends[r]]
        ax, ay, az = T(0), T(0), T(0)
        for i in rows:
            ax, ay, az = ax + pts[i, 0], ay + pts[i, 1], az + pts[i, 2]
        cnt = T(len(rows))
        out[r] = (ax / cnt, ay / cnt, az / cnt)
        if colors is not None:
            rgb[r] = colors[rows].astype(np.int64).sum(axis=0) // len(rows)
    return out, rgb, counts


# ---- keyframe filter -------------------------------------------------------------------------------------------------
def voxel_filter(points, colors, leaf, max_range=None):
    """(points float32, colors or None, counts) of the keyframe filter; with `max_range` the clip 0 <= z <= max_range."""
    pts = np.asarray(points, dtype=F)
    keep = np.isfinite(pts).all(axis=1)
    pts = pts[keep]
    colors = None if colors is None else np.asarray(colors)[keep]
    if len(pts) == 0:
        return np.zeros((0, 3), dtype=F), None if colors is None else np.zeros((0, 3), dtype=np.uint8), np.zeros(0, dtype=np.int64)
    inv = F(1) / F(leaf)
    out, rgb, counts = segment_means(pts, colors, grid_indices(pts, inv))
    if max_range is not None:
        sel = (out[:, 2] >= F(0)) & (out[:, 2] <= F(max_range))
        out, counts = out[sel], counts[sel]
        rgb = None if rgb is None else rgb[sel]
    return out, rgb, counts


def keyframe_cloud(image, depth, camera, leaf=0.05, max_range=2.0):
    pts, rgb = back_project(image, depth, camera)
    return voxel_filter(pts, rgb, leaf, max_range)


# ---- map assembly ----------------------------------------------------------------------------------------------------
def transform(points, T):
    p = np.asarray(points).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def assemble_map(clouds, poses, voxel, sensor_to_body=None):
    """clouds: a list of (points, colors or None) in keyframe order; poses: a list of 4 x 4.  Returns (points float64,
    colors or None, counts)."""
    pw, cols = [], []
    for (p, c), T in zip(clouds, poses):
        T = np.asarray(T, dtype=np.float64)
        T = T if sensor_to_body is None else T @ np.asarray(sensor_to_body, dtype=np.float64)
        p = np.asarray(p)
        keep = np.isfinite(p).all(axis=1)
        pw.append(transform(p[keep], T))
        cols.append(None if c is None else np.asarray(c)[keep])
    pw = np.concatenate(pw, axis=0) if pw else np.zeros((0, 3))
    colors = np.concatenate(cols, axis=0) if cols and all(c is not None for c in cols) else None
    if len(pw) == 0:
        return np.zeros((0, 3)), colors, np.zeros(0, dtype=np.int64)
    return segment_means(pw, colors, grid_indices(pw, np.float64(voxel)))


# ---- the scene the facts and the GPU tests share ---------------------------------------------------------------------
def scene_depth(H=48, W=64, seed=3):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    d = (1500 + 8 * u + 5 * v + rng.integers(0, 40, (H, W))).astype(np.uint16)
    d[rng.random((H, W)) < 0.1] = 0
    return d


def scene_image(H=48, W=64, seed=3, channels=3):
    rng = np.random.default_rng(seed + 1000)
    return rng.integers(0, 256, (H, W, 3) if channels == 3 else (H, W), dtype=np.uint8)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.identity(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def scene_poses():
    T1 = np.identity(4)
    T1[:3, 3] = (1000.0, 0.0, 0.0)
    T2 = np.identity(4)
    T2[:3, :3] = rotation((0.2, 1.0, 0.1), 0.3)
    T2[:3, 3] = (1000.25, -0.1, 0.05)
    return T1, T2


_SCENE = {}


def scene_keyframes():
    """The two keyframes of the map facts, filtered at leaf 0.05 (unclipped): computed once and shared, never changed."""
    if "kf" not in _SCENE:
        d, img = scene_depth(), scene_image()
        out = []
        for depth in (d, np.roll(d, 3, axis=1)):
            p, c = back_project(img, depth, SCENE_CAMERA)
            out.append(voxel_filter(p, c, 0.05))
        _SCENE["kf"] = out
    return _SCENE["kf"]
