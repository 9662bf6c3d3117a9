"""The sub-pixel keypoints of include/cslam_hip.h restated in numpy, on top of feat_pyramid_reference.py (which stays as it
is): the offset rule on the int32 response maps and the level-0 coordinate rule: the yardstick that feat_pyr_subpix_kernel /
feat_pyr_merge_kernel (csrc/feat.hip) and csrc/feat_pyr.h equal bit for bit.  Written from the statement in the header, not
from feat_pyr.h.  Response maps are [H, W] int32, keypoints (x, y)."""
import functools

import numpy as np

import feat_pyramid_reference as fp
import feat_reference as fr
import stereo_reference as sr


def offset(m, c, p):
    """The offset of a maximum along one axis from the responses before (m), at (c) and after (p) it: Python integers up
    to one float64 division."""
    m, c, p = int(m), int(c), int(p)
    den, num = m - 2 * c + p, m - p
    if den >= 0:                                           # a plateau, or not a maximum along the axis
        return np.float64(0.0)
    off = np.float64(num) / np.float64(2 * den)
    return np.float64(min(max(off, np.float64(-0.5)), np.float64(0.5)))


def offsets(R, kp):
    """float64 [k, 2] = (off x, off y) of the keypoints kp [k, 2] on the map R; a neighbour outside the image (and a keypoint
    outside it) gives 0 along that axis."""
    R = np.asarray(R)
    H, W = R.shape
    out = np.zeros((len(kp), 2), dtype=np.float64)
    for i, (x, y) in enumerate(np.asarray(kp, dtype=np.int64).reshape(-1, 2)):
        if not (0 <= x < W and 0 <= y < H):
            continue
        if 1 <= x <= W - 2:
            out[i, 0] = offset(R[y, x - 1], R[y, x], R[y, x + 1])
        if 1 <= y <= H - 2:
            out[i, 1] = offset(R[y - 1, x], R[y, x], R[y + 1, x])
    return out


def coord(x, off, n_0, n_l):
    """The level-0 coordinate of level pixel x moved by off, in float64 in the order of the statement."""
    x = np.asarray(x, dtype=np.int64)
    return ((2 * x + 1).astype(np.float64) + np.float64(2.0) * np.asarray(off, dtype=np.float64)) * np.float64(n_0) / np.float64(2 * n_l) \
        - np.float64(0.5)


def refine(shape, levels_g, feats, rows):
    """`rows` of feat_pyramid_reference.merge with the keypoints refined on the level maps, and the key offsets added."""
    H, W = shape
    sizes = fp.level_sizes(shape, len(feats))
    offs = [offsets(fr.response(g)[0], f[0]) for g, f in zip(levels_g, feats)]
    kx = np.concatenate([coord(f[0][:, 0], o[:, 0], W, sizes[l][1]) for l, (f, o) in enumerate(zip(feats, offs))])
    ky = np.concatenate([coord(f[0][:, 1], o[:, 1], H, sizes[l][0]) for l, (f, o) in enumerate(zip(feats, offs))])
    return dict(rows, keypoints=np.stack([kx, ky], axis=1).astype(np.float64).reshape(-1, 2),
                offsets=np.concatenate(offs).reshape(-1, 2))


def extract(image, depth, camera, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19, depth_as_mask=True):
    """feat_pyramid_reference.extract with sub-pixel keypoints: depth is still read at the integer level-0 pixel."""
    g = fr.gray(image)
    levels_g = fp.pyramid(g, levels)
    feats = fp.level_features(levels_g, fp.valid_maps(depth, levels) if depth_as_mask else None, max_features, quality_level, min_distance,
                              border)
    rows, base = fp.merge(g.shape, feats)
    rows = refine(g.shape, levels_g, feats, rows)
    d = depth[base[:, 1], base[:, 0]].astype(np.float32)
    Z = np.where(fr.depth_valid(d), d.astype(np.float64), np.nan)
    rows["points"] = fp.points(rows["keypoints"], Z, camera)
    return rows


def extract_stereo(left, right, camera, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19, min_disparity=1,
                   max_disparity=128, uniqueness=15, lr_tolerance=1):
    """feat_pyramid_reference.extract_stereo with sub-pixel keypoints: the stereo rule still runs at the integer pixel."""
    gl, gr = fr.gray(left), fr.gray(right)
    levels_g = fp.pyramid(gl, levels)
    feats = fp.level_features(levels_g, None, max_features, quality_level, min_distance, border)
    rows, base = fp.merge(gl.shape, feats)
    rows = refine(gl.shape, levels_g, feats, rows)
    m = sr.match(gl, gr, base, camera, min_disparity, max_disparity, uniqueness, lr_tolerance)
    rows["points"] = fp.points(rows["keypoints"], m["points"][:, 2], camera)
    rows["disparity"], rows["status"] = m["disparity"], m["status"]
    return rows


@functools.lru_cache(maxsize=None)
def scene_features(levels=4):
    """The restatement's sub-pixel features of the two views of feat_pyramid_reference.scene, computed once."""
    A, B, dA, dB = fp.scene()
    return extract(A, dA, fp.SCENE_CAMERA, levels=levels), extract(B, dB, fp.SCENE_CAMERA, levels=levels)
