"""The dense form of the stereo rule of include/cslam_hip.h restated in numpy: what stereo_dense_kernel
(csrc/stereo_dense.hip) equals bit for bit at every pixel.  Written from the statement in the header; of stereo_reference.py
only the small rules (key, not_unique, parabola) and the scene makers are used.

  slab    per image row, C(u, d) for every column and every d of D_lo .. max_disparity + 1 at once: the 3-high column costs,
          their prefix sums along the columns, C = the difference of two prefix sums 15 columns apart.  Uniform in u: a left
          pixel without a range of its own still owns costs that the back search of right pixels needs.
  left    the minimum key along d over D_lo .. min(max_disparity + 1, u - 7); the rival of the uniqueness rule is looked for
          among the FOUR smallest keys only (d* is one, d* - 1 and d* + 1 are the only others left out).
  right   once per right pixel ur: the minimum key along the diagonal C(ur + e, e), e = D_lo .. min(max_disparity + 1,
          W - 8 - ur), whichever left pixel asks.
Images are [H, W] uint8.
"""
import numpy as np

import stereo_reference as sr

HALF_W, HALF_H = sr.HALF_W, sr.HALF_H
TILE = (256, 32, 32)                 # csrc/stereo_dense.h: columns per tile, disparities per tile, columns per segment


def slab(L, R, v, d_lo, d_max):
    """int64 [W, d_max - d_lo + 1]: C(u, d) of row v; -1 where a window leaves the image."""
    W = L.shape[1]
    Lr, Rr = L[v - HALF_H:v + HALF_H + 1].astype(np.int64), R[v - HALF_H:v + HALF_H + 1].astype(np.int64)
    C = np.full((W, d_max - d_lo + 1), -1, dtype=np.int64)
    for i, d in enumerate(range(d_lo, d_max + 1)):
        if W - d < 2 * HALF_W + 1:
            continue
        col = ((Lr[:, d:] - Rr[:, :W - d]) ** 2).sum(axis=0)           # the column cost of x = d .. W - 1
        P = np.concatenate([[0], np.cumsum(col)])                      # P[k] = the sum over x = d .. d + k - 1
        u = np.arange(d + HALF_W, W - HALF_W)                          # right window and left window inside the image
        C[u, i] = P[u + HALF_W + 1 - d] - P[u - HALF_W - d]
    return C


def dense(L, R, camera, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1):
    """status uint8 [H, W], disparity float64 [H, W] (NaN unless accepted), disparity32 and depth float32 [H, W], best int32
    [H, W, 4]."""
    H, W = L.shape
    fx, baseline = np.float64(camera[0]), np.float64(camera[4])
    d_lo, d_max = min_disparity - 1, max_disparity + 1
    status = np.full((H, W), sr.OUTSIDE, dtype=np.uint8)
    disp = np.full((H, W), np.nan, dtype=np.float64)
    best = np.full((H, W, 4), -1, dtype=np.int32)
    for v in range(HALF_H, H - HALF_H):
        if W < 2 * HALF_W + 1:
            break
        C = slab(L, R, v, d_lo, d_max)
        es = np.full(W, -1, dtype=np.int64)                            # the right search, once per right pixel
        for ur in range(HALF_W, W - HALF_W):
            e = np.arange(d_lo, min(d_max, W - 1 - HALF_W - ur) + 1)
            if len(e):
                es[ur] = e[np.argmin(sr.key(C[ur + e, e - d_lo], e))]
        for u in range(HALF_W, W - HALF_W):
            d_hi = min(d_max, u - HALF_W)
            if d_hi - d_lo < 2:
                status[v, u] = sr.NO_RANGE
                continue
            c = C[u, :d_hi - d_lo + 1]
            keys = sr.key(c, np.arange(d_lo, d_hi + 1))
            four = np.sort(keys)[:4]
            ds = int(four[0] & 511)
            at = lambda d: int(c[d - d_lo]) if d_lo <= d <= d_hi else -1
            best[v, u] = (ds, at(ds - 1), at(ds), at(ds + 1))
            if ds in (d_lo, d_hi):
                status[v, u] = sr.EDGE
                continue
            rivals = [int(k >> 9) for k in four[1:] if abs(int(k & 511) - ds) >= 2]
            if rivals and sr.not_unique(rivals[0], at(ds), uniqueness):
                status[v, u] = sr.NOT_UNIQUE
                continue
            if lr_tolerance >= 0 and abs(int(es[u - ds]) - ds) > lr_tolerance:
                status[v, u] = sr.LEFT_RIGHT
                continue
            status[v, u] = sr.ACCEPTED
            disp[v, u] = sr.parabola(ds, *best[v, u, 1:].tolist())
    with np.errstate(invalid="ignore"):
        depth = ((baseline * fx) / disp).astype(np.float32)
    return dict(status=status, disparity=disp, disparity32=disp.astype(np.float32), depth=depth, best=best)


def sparse_everywhere(L, R, camera, **params):
    """stereo_reference.match with every pixel as a keypoint, in the shapes of `dense`."""
    H, W = L.shape
    m = sr.match(L, R, all_pixels(H, W), camera, **params)
    return dict(status=m["status"].astype(np.uint8).reshape(H, W), disparity=m["disparity"].reshape(H, W),
                best=m["best"].reshape(H, W, 4), z=m["points"][:, 2].reshape(H, W))


def all_pixels(H, W):
    vv, uu = np.mgrid[0:H, 0:W]
    return np.stack([uu.reshape(-1), vv.reshape(-1)], axis=1).astype(np.int32)


def counts(status):
    return tuple(int((status == s).sum()) for s in range(6))


# ---- the twelve scenes: (name, maker of (L, R), parameters, pixels per status 0 .. 5) --------------------------------
CAMERA = (100.0, 110.0, 31.5, 2.25, 0.2)


def _noise():
    rng = np.random.default_rng(0)
    return tuple((rng.integers(0, 2, (4, 80)) * 255).astype(np.uint8) for _ in range(2))


SCENES = [
    ("foreground", lambda: tuple(x[6:16] for x in sr.foreground_pair()), dict(max_disparity=32), (1304, 512, 16, 32, 47, 89)),
    ("foreground_lr0", lambda: tuple(x[8:13] for x in sr.foreground_pair()), dict(max_disparity=32, lr_tolerance=0),
     (480, 442, 6, 12, 26, 34)),
    ("shifted", lambda: sr.shifted_pair(5, 65, 10), dict(max_disparity=16), (120, 172, 6, 27, 0, 0)),
    ("one_column", lambda: sr.shifted_pair(3, 15, 3), dict(max_disparity=4), (0, 44, 1, 0, 0, 0)),
    ("four_columns", lambda: sr.shifted_pair(3, 18, 3), dict(max_disparity=4), (0, 50, 2, 2, 0, 0)),
    ("min5", lambda: sr.shifted_pair(4, 129, 20, seed=3), dict(min_disparity=5, max_disparity=40), (188, 286, 12, 30, 0, 0)),
    ("full_range", lambda: sr.shifted_pair(3, 300, 30, seed=4), dict(max_disparity=255), (255, 614, 2, 14, 4, 11)),
    ("stripes", lambda: (sr.stripes(3, 70), sr.stripes(3, 70, 3)), dict(max_disparity=20), (7, 154, 2, 2, 45, 0)),
    ("constant", lambda: (np.full((3, 40), 90, np.uint8), np.full((3, 40), 90, np.uint8)), dict(max_disparity=8), (0, 94, 2, 24, 0, 0)),
    ("noise", _noise, dict(max_disparity=30, uniqueness=0), (69, 188, 4, 3, 20, 36)),
    ("smooth", lambda: sr.smooth_pair(4, 90, 10.5), dict(max_disparity=24, uniqueness=100, lr_tolerance=-1), (130, 208, 4, 18, 0, 0)),
    ("min_is_max", lambda: sr.shifted_pair(3, 40, 1), dict(min_disparity=1, max_disparity=1), (24, 94, 2, 0, 0, 0)),
]


def scene(k):
    name, make, params, want = SCENES[k]
    L, R = make()
    return np.ascontiguousarray(L), np.ascontiguousarray(R), params, want
