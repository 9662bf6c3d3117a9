"""The scale pyramid of the keyframe features of include/cslam_hip.h restated in numpy, on top of feat_reference.py and
stereo_reference.py: integers up to the final coordinates (one float64 division and one subtraction): the yardstick that
feat_pyr_level_kernel / feat_pyr_merge_kernel (csrc/feat.hip) and csrc/feat_pyr.h equal bit for bit.  Written from the
statement in the header, not from feat_pyr.h.  Images are [H, W] uint8, keypoints (x, y)."""
import functools

import numpy as np

import feat_reference as fr
import stereo_reference as sr

MAX_LEVELS = 8


def level_size(n, l):
    return (n * 5 ** l + 6 ** l // 2) // 6 ** l


def level_sizes(shape, levels):
    return [(level_size(int(shape[0]), l), level_size(int(shape[1]), l)) for l in range(levels)]


def taps(n_l, n_prev):
    """(i0, i1, a) int64 [n_l] of every output index of an axis."""
    x = np.arange(n_l, dtype=np.int64)
    u = ((2 * x + 1) * n_prev * 1024) // (2 * n_l) - 512
    u = np.clip(u, 0, (n_prev - 1) * 1024)
    i0 = u >> 10
    return i0, np.minimum(i0 + 1, n_prev - 1), u & 1023


def resample(g, shape):
    """The image of `shape` from the image g of the level below."""
    j0, j1, b = taps(shape[0], g.shape[0])
    i0, i1, a = taps(shape[1], g.shape[1])
    g = g.astype(np.int64)
    a, b = a[None, :], b[:, None]
    top = g[j0][:, i0] * (1024 - a) + g[j0][:, i1] * a
    bottom = g[j1][:, i0] * (1024 - a) + g[j1][:, i1] * a
    v = (top * (1024 - b) + bottom * b + (1 << 19)) >> 20
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def pyramid(g, levels):
    """The level images: level 0 is g itself, level l comes from level l - 1."""
    out = [np.asarray(g).copy()]
    for h, w in level_sizes(g.shape, levels)[1:]:
        out.append(resample(out[-1], (h, w)))
    return out


def base_pixel(x, n_0, n_l):
    return ((2 * np.asarray(x, dtype=np.int64) + 1) * n_0) // (2 * n_l)


def base_coord(x, n_0, n_l):
    return ((2 * np.asarray(x, dtype=np.int64) + 1) * n_0).astype(np.float64) / np.float64(2 * n_l) - np.float64(0.5)


def valid_maps(depth, levels):
    """uint8 maps per level: 1 where the depth at the level-0 pixel under the level pixel is valid."""
    H, W = depth.shape
    ok = fr.depth_valid(depth)
    return [ok[base_pixel(np.arange(h), H, h)][:, base_pixel(np.arange(w), W, w)].astype(np.uint8) for h, w in level_sizes(depth.shape, levels)]


def budgets(max_features, levels):
    w = [5 ** l * 6 ** (levels - 1 - l) for l in range(levels)]
    b = [max_features * x // sum(w) for x in w]
    b[0] += max_features - sum(b)
    return b


def points(kp, Z, camera):
    """The point rule on level-0 coordinates kp float64 [k, 2] and Z float64 [k]; an invalid Z gives a NaN row."""
    fx, fy, cx, cy = (np.float64(v) for v in camera[:4])
    ok = np.isfinite(Z) & (Z > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        pts = np.stack([((kp[:, 0] - cx) * Z) / fx, ((kp[:, 1] - cy) * Z) / fy, Z], axis=1)
    pts[~ok] = np.nan
    return pts


def level_features(levels_g, maps, max_features, quality_level, min_distance, border):
    """Per level (keypoints, responses, bins, descriptors) with the level's budget, each level an image of its own."""
    out = []
    for l, (g, n) in enumerate(zip(levels_g, budgets(max_features, len(levels_g)))):
        R, rmax = fr.response(g)
        if n > 0:
            kp, resp = fr.select(R, None if maps is None else maps[l], n, quality_level, min_distance, border, rmax)
        else:
            kp, resp = np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int32)
        bins, desc, _ = fr.describe(g, kp)
        out.append((kp, resp, bins, desc))
    return out


def merge(shape, feats):
    """Rows of a frame from the per-level features: level 0 first; keypoints in level-0 coordinates and pixels."""
    H, W = shape
    sizes = level_sizes(shape, len(feats))
    lkp = np.concatenate([f[0] for f in feats]).astype(np.int32).reshape(-1, 2)
    lev = np.concatenate([np.full(len(f[0]), l, dtype=np.int32) for l, f in enumerate(feats)])
    kx = np.concatenate([base_coord(f[0][:, 0], W, sizes[l][1]) for l, f in enumerate(feats)])
    ky = np.concatenate([base_coord(f[0][:, 1], H, sizes[l][0]) for l, f in enumerate(feats)])
    px = np.concatenate([base_pixel(f[0][:, 0], W, sizes[l][1]) for l, f in enumerate(feats)])
    py = np.concatenate([base_pixel(f[0][:, 1], H, sizes[l][0]) for l, f in enumerate(feats)])
    rows = dict(keypoints=np.stack([kx, ky], axis=1).astype(np.float64).reshape(-1, 2), level_keypoints=lkp, levels=lev,
                responses=np.concatenate([f[1] for f in feats]).astype(np.int32), bins=np.concatenate([f[2] for f in feats]).astype(np.int32),
                descriptors=np.concatenate([f[3] for f in feats]).astype(np.uint8).reshape(-1, 32))
    return rows, np.stack([px, py], axis=1).astype(np.int64).reshape(-1, 2)


def extract(image, depth, camera, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19, depth_as_mask=True):
    g = fr.gray(image)
    feats = level_features(pyramid(g, levels), valid_maps(depth, levels) if depth_as_mask else None, max_features, quality_level,
                           min_distance, border)
    rows, base = merge(g.shape, feats)
    d = depth[base[:, 1], base[:, 0]].astype(np.float32)
    Z = np.where(fr.depth_valid(d), d.astype(np.float64), np.nan)
    rows["points"] = points(rows["keypoints"], Z, camera)
    return rows


def extract_stereo(left, right, camera, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19, min_disparity=1,
                   max_disparity=128, uniqueness=15, lr_tolerance=1):
    gl, gr = fr.gray(left), fr.gray(right)
    feats = level_features(pyramid(gl, levels), None, max_features, quality_level, min_distance, border)
    rows, base = merge(gl.shape, feats)
    m = sr.match(gl, gr, base, camera, min_disparity, max_disparity, uniqueness, lr_tolerance)
    rows["points"] = points(rows["keypoints"], m["points"][:, 2], camera)
    rows["disparity"], rows["status"] = m["disparity"], m["status"]
    return rows


# ---- the two-distance scene --------------------------------------------------------------------------------------------
SCENE_SHAPE = (144, 192)
SCENE_CAMERA = (200.0, 200.0, 95.5, 71.5)
SCENE_Z = (2.88, 2.0)                                      # the same plane from 2.88 m (view A) and from 2.0 m (view B)
SCENE_SCALE = 1.44


def render(cells, sub, shape=SCENE_SHAPE, mean=5):
    """Blocks of `sub` sub-pixels, `mean` x `mean` sub-pixels averaged per pixel (rounded to nearest): blocks of sub / mean
    pixels, pixel u covering sub-pixels [mean u, mean u + mean)."""
    H, W = shape
    idx = lambda n: np.arange(n * mean) // sub
    big = cells[idx(H)][:, idx(W)].astype(np.int64)
    s = big.reshape(H, mean, W, mean).sum(axis=(1, 3))
    return ((2 * s + mean * mean) // (2 * mean * mean)).astype(np.uint8)


def scene():
    """(image A, image B, depth A, depth B): the plane of random cells from Z = 2.88 m (blocks of 10 pixels) and from 2.0 m
    (14.4 pixels); a point at pixel u_A of A lies at u_B + 1/2 = 1.44 (u_A + 1/2) of B."""
    cells = np.random.default_rng(7).integers(0, 256, (40, 40))
    A, B = render(cells, 50), render(cells, 72)
    return A, B, np.full(SCENE_SHAPE, SCENE_Z[0], dtype=np.float32), np.full(SCENE_SHAPE, SCENE_Z[1], dtype=np.float32)


def scene_transform():
    """T with x_A = R x_B + t, from view B to view A: no rotation, t = (-0.44 (cx + 1/2) Z_B / fx, -0.44 (cy + 1/2) Z_B / fy,
    Z_A - Z_B = 0.88 m forward)."""
    fx, fy, cx, cy = SCENE_CAMERA
    T = np.identity(4)
    T[:3, 3] = [-(SCENE_SCALE - 1) * (cx + 0.5) * SCENE_Z[1] / fx, -(SCENE_SCALE - 1) * (cy + 0.5) * SCENE_Z[1] / fy, SCENE_Z[0] - SCENE_Z[1]]
    return T


def scene_map(kp_a):
    """Where keypoints of A lie in B."""
    return SCENE_SCALE * (np.asarray(kp_a, dtype=np.float64) + 0.5) - 0.5


@functools.lru_cache(maxsize=None)
def scene_features(levels):
    """The restatement's features of the two views, computed once: `levels` = 0 is the single-scale chain of feat_reference."""
    A, B, dA, dB = scene()
    if levels == 0:
        return fr.extract(A, dA, SCENE_CAMERA), fr.extract(B, dB, SCENE_CAMERA)
    return extract(A, dA, SCENE_CAMERA, levels=levels), extract(B, dB, SCENE_CAMERA, levels=levels)


def scene_bounds():
    """(translation, rotation) bounds of the registration: the 2 px reprojection threshold at the coarsest of 4 levels'
    pixel size, in metres at Z_B / fx per pixel and in radians at half the image width."""
    px = 2.0 * (6.0 / 5.0) ** 3
    return px * SCENE_Z[1] / SCENE_CAMERA[0], px / (SCENE_SHAPE[1] / 2)
