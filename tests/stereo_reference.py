"""The stereo rule of include/cslam_hip.h restated in numpy, integers up to the one float64 division of the parabola and the
triangulation: the yardstick that feat_stereo_kernel (csrc/feat.hip) and csrc/stereo.h equal bit for bit.  Written from the
statement in the header, not from stereo.h.  Images are [H, W] uint8, keypoints (u, v)."""
import numpy as np

import feat_reference

HALF_W, HALF_H = 7, 1
COST_MAX = 45 * 255 * 255
ACCEPTED, OUTSIDE, NO_RANGE, EDGE, NOT_UNIQUE, LEFT_RIGHT = range(6)


def key(cost, d):
    return (cost << 9) | d


def search_range(u, min_disparity, max_disparity):
    """(D_lo, D_hi, whether there is something to search)."""
    lo, hi = min_disparity - 1, min(max_disparity + 1, u - HALF_W)
    return lo, hi, hi - lo >= 2


def not_unique(second, best, uniqueness):
    return second * 100 <= best * (100 + uniqueness)       # Python integers: exact


def parabola(d, a, b, c):
    return np.float64(d) + np.float64(a - c) / np.float64(2 * (a - 2 * b + c))


def triangulate(u, v, disparity, camera):
    fx, fy, cx, cy, baseline = (np.float64(x) for x in camera)
    Z = (baseline * fx) / np.float64(disparity)
    return np.array([((np.float64(u) - cx) * Z) / fx, ((np.float64(v) - cy) * Z) / fy, Z], dtype=np.float64)


def costs(A, B, v, ua, first, last):
    """[last - first + 1] Python ints: the window of A at column ua against the windows of B at columns first .. last."""
    a = A[v - HALF_H:v + HALF_H + 1, ua - HALF_W:ua + HALF_W + 1].astype(np.int64)
    strip = B[v - HALF_H:v + HALF_H + 1, first - HALF_W:last + HALF_W + 1].astype(np.int64)
    w = np.lib.stride_tricks.sliding_window_view(strip, 2 * HALF_W + 1, axis=1)         # [3, count, 15]
    return [int(x) for x in ((w - a[:, None, :]) ** 2).sum(axis=(0, 2))]


def match_one(L, R, u, v, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1):
    """(status, disparity float64 or NaN, (d*, a, b, c))."""
    H, W = L.shape
    nan = np.float64(np.nan)
    if not (HALF_W <= u <= W - 1 - HALF_W and HALF_H <= v <= H - 1 - HALF_H):
        return OUTSIDE, nan, (-1, -1, -1, -1)
    lo, hi, ok = search_range(u, min_disparity, max_disparity)
    if not ok:
        return NO_RANGE, nan, (-1, -1, -1, -1)
    C = costs(L, R, v, u, u - hi, u - lo)[::-1]            # C[d - lo]
    ds = lo + min(range(len(C)), key=lambda i: key(C[i], lo + i))
    at = lambda d: C[d - lo] if lo <= d <= hi else -1
    best = (ds, at(ds - 1), at(ds), at(ds + 1))
    if ds in (lo, hi):
        return EDGE, nan, best
    others = [C[d - lo] for d in range(lo, hi + 1) if abs(d - ds) >= 2]
    if others and not_unique(min(others), C[ds - lo], uniqueness):
        return NOT_UNIQUE, nan, best
    if lr_tolerance >= 0:
        ur = u - ds
        hi2 = min(max_disparity + 1, W - 1 - HALF_W - ur)
        C2 = costs(R, L, v, ur, ur + lo, ur + hi2)         # C2[e - lo]
        es = lo + min(range(len(C2)), key=lambda i: key(C2[i], lo + i))
        if abs(es - ds) > lr_tolerance:
            return LEFT_RIGHT, nan, best
    a, b, c = best[1:]
    assert a - 2 * b + c > 0 and a > b and c >= b
    return ACCEPTED, parabola(ds, a, b, c), best


def match(L, R, keypoints, camera, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1):
    """What `stereo_match` returns: disparity float64 [k], status int32 [k], best int32 [k, 4], points float64 [k, 3]."""
    kp = np.asarray(keypoints, dtype=np.int64).reshape(-1, 2)
    disp, status = np.full(len(kp), np.nan, dtype=np.float64), np.zeros(len(kp), dtype=np.int32)
    best, pts = np.zeros((len(kp), 4), dtype=np.int32), np.full((len(kp), 3), np.nan, dtype=np.float64)
    for k, (u, v) in enumerate(kp.tolist()):
        status[k], disp[k], best[k] = match_one(L, R, u, v, min_disparity, max_disparity, uniqueness, lr_tolerance)
        if status[k] == ACCEPTED:
            pts[k] = triangulate(u, v, disp[k], camera)
    return dict(disparity=disp, status=status, best=best, points=pts)


def extract_stereo(left, right, camera, max_features=1000, quality_level=0.001, min_distance=7, border=19, min_disparity=1,
                   max_disparity=128, uniqueness=15, lr_tolerance=1):
    """The whole stereo frame: the features of feat_reference on the left image without a mask, then the rule."""
    gl, gr = feat_reference.gray(left), feat_reference.gray(right)
    R, rmax = feat_reference.response(gl)
    kp, resp = feat_reference.select(R, None, max_features, quality_level, min_distance, border, rmax)
    bins, desc, _ = feat_reference.describe(gl, kp)
    m = match(gl, gr, kp, camera, min_disparity, max_disparity, uniqueness, lr_tolerance)
    return dict(keypoints=kp, responses=resp, bins=bins, descriptors=desc, points=m["points"], disparity=m["disparity"], status=m["status"])


# ---- planted scenes ------------------------------------------------------------------------------------------------
def blocks(H, W, seed, block=4):
    """Random grey blocks (the prototype's texture: one cell more than needed in each direction)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (H // block + 1, W // block + 1)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((block, block), np.uint8))[:H, :W])


def shifted_pair(H, W, shift, seed=1):
    """(L, R) with R[x] = L[x + shift]: every point has disparity `shift`."""
    bg = blocks(H, W + 64, seed)
    return np.ascontiguousarray(bg[:, shift:shift + W]), np.ascontiguousarray(bg[:, 2 * shift:2 * shift + W])


def foreground_pair(H=48, W=200):
    """A background at disparity 5 and a foreground block, rows 10 .. 39 and left columns 90 .. 129, at disparity 20."""
    L, R = shifted_pair(H, W, 5)
    fg = blocks(H, W + 64, 2)
    L, R = L.copy(), R.copy()
    L[10:40, 90:130] = fg[10:40, 90:130]
    R[10:40, 70:110] = fg[10:40, 90:130]
    return L, R


def stripes(H, W, shift=0):
    x = np.arange(W) + shift
    return np.ascontiguousarray(np.tile(((x // 4) % 2 * 255).astype(np.uint8), (H, 1)))


def smooth_pair(H, W, shift):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f = lambda x, y: 127 + 60 * np.sin(0.21 * x + 0.1 * y) + 50 * np.sin(0.047 * x * 1.7 - 0.3 * y) + 15 * np.sin(0.9 * x)
    return np.rint(f(xx, yy)).astype(np.uint8), np.rint(f(xx + shift, yy)).astype(np.uint8)
