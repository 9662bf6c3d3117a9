"""The keyframe features of include/cslam_hip.h restated in numpy, integers throughout (float64 only in the 3D points):
the yardstick that csrc/feat.hip and csrc/feat.h equal bit for bit.  Written from the statement in the header, not from
feat.h.  Images are [H, W] uint8, keypoints (x, y)."""
import numpy as np

MASK = (1 << 64) - 1
SEED = 0x0BADC0FFEE0DDF00
CS8 = [(16384, 0), (16069, 3196), (15137, 6270), (13623, 9102), (11585, 11585), (9102, 13623), (6270, 15137), (3196, 16069)]
BLUR = np.array([1, 6, 15, 20, 15, 6, 1], dtype=np.int64)
PATCH_RADIUS, PATTERN_RADIUS, MIN_BORDER = 15, 13, 18


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(n):
    """Draw n of the generator: ((x, y), kept)."""
    v = mix64((SEED + n) & MASK)
    x, y = (v & 0xFFFFFFFF) % 27 - 13, (v >> 32) % 27 - 13
    return (x, y), x * x + y * y <= PATTERN_RADIUS ** 2


def base_pattern():
    """[256, 4] (px, py, qx, qy)."""
    out, n = [], 0
    while len(out) < 256:
        pts = []
        while len(pts) < 2:
            p, keep = draw(n)
            n += 1
            if keep:
                pts.append(p)
        if pts[0] != pts[1]:
            out.append(pts[0] + pts[1])
    return np.array(out, dtype=np.int64)


def direction(k):
    c, s = CS8[k % 8]
    for _ in range(k // 8 % 4):
        c, s = -s, c
    return c, s


def round14(v):
    return (v + 8192) >> 14 if v >= 0 else -((-v + 8192) >> 14)


def rotate(x, y, k):
    c, s = CS8[k % 8]
    u, v = round14(x * c - y * s), round14(x * s + y * c)
    for _ in range(k // 8 % 4):
        u, v = -v, u
    return u, v


_PATTERNS = {}


def pattern(k):
    if k not in _PATTERNS:
        base = base_pattern() if "base" not in _PATTERNS else _PATTERNS["base"]
        _PATTERNS["base"] = base
        _PATTERNS[k] = np.array([rotate(int(r[0]), int(r[1]), k) + rotate(int(r[2]), int(r[3]), k) for r in base], dtype=np.int64)
    return _PATTERNS[k]


def gray(img):
    img = np.asarray(img)
    if img.ndim == 2:
        return img.copy()
    b, g, r = (img[:, :, c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def isqrt(D):
    s = np.floor(np.sqrt(D.astype(np.float64))).astype(np.int64)
    s = s - (s * s > D)
    s = s + ((s + 1) * (s + 1) <= D)
    assert np.all(s * s <= D) and np.all((s + 1) * (s + 1) > D)
    return s


def box3(m):
    p = np.pad(m, 1, mode="reflect")
    H, W = m.shape
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


def response(g, parts=False):
    """(R int32 [H, W], Rmax)."""
    p = np.pad(g.astype(np.int64), 1, mode="reflect")
    H, W = g.shape
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ix = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    iy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    a, b, c = box3(ix * ix), box3(ix * iy), box3(iy * iy)
    D = (a - c) ** 2 + 4 * b * b
    R = (a + c) - isqrt(D)
    assert R.min() >= 0 and R.max() <= 18727200
    if parts:
        return a, b, c, D
    return R.astype(np.int32), int(R.max())


def depth_valid(depth):
    return np.isfinite(depth) & (depth > 0)


def candidates(R, rmax, valid, quality_level, border):
    """Pixel indices of the candidates in order: response descending, then pixel index ascending."""
    H, W = R.shape
    R = R.astype(np.int64)
    ok = R.astype(np.float64) > np.float64(quality_level) * np.float64(rmax)
    p = np.pad(R, 1, mode="constant", constant_values=-1)
    for dy in range(3):
        for dx in range(3):
            ok &= R >= p[dy:dy + H, dx:dx + W]
    inside = np.zeros((H, W), dtype=bool)
    if H > 2 * border and W > 2 * border:
        inside[border:H - border, border:W - border] = True
    ok &= inside
    if valid is not None:
        ok &= np.asarray(valid).astype(bool)
    idx = np.flatnonzero(ok)
    key = ((rmax - R.reshape(-1)[idx]) << 32) | idx
    return idx[np.argsort(key, kind="stable")]


def select(R, valid=None, max_features=1000, quality_level=0.001, min_distance=7, border=19, rmax=None):
    """The sequential greedy rule: (keypoints int32 [k, 2] = (x, y), responses int32 [k])."""
    H, W = R.shape
    rmax = int(R.max()) if rmax is None else rmax
    kept = []
    for i in candidates(R, rmax, valid, quality_level, border):
        if len(kept) == max_features:
            break
        y, x = divmod(int(i), W)
        if all((x - u) ** 2 + (y - v) ** 2 >= min_distance ** 2 for u, v in kept):
            kept.append((x, y))
    kp = np.array(kept, dtype=np.int32).reshape(-1, 2)
    return kp, R[kp[:, 1], kp[:, 0]].astype(np.int32)


_DISC = [(dx, dy) for dy in range(-PATCH_RADIUS, PATCH_RADIUS + 1) for dx in range(-PATCH_RADIUS, PATCH_RADIUS + 1)
         if dx * dx + dy * dy <= PATCH_RADIUS ** 2]


def moments(g, x, y):
    m10 = sum(dx * int(g[y + dy, x + dx]) for dx, dy in _DISC)
    m01 = sum(dy * int(g[y + dy, x + dx]) for dx, dy in _DISC)
    return m10, m01


def bin_scores(m10, m01):
    return [m10 * direction(k)[0] + m01 * direction(k)[1] for k in range(32)]


def blurred_patch(g, x, y):
    """[31, 31] unnormalised sums around (x, y): entry [dy + 15, dx + 15]."""
    p = g[y - MIN_BORDER:y + MIN_BORDER + 1, x - MIN_BORDER:x + MIN_BORDER + 1].astype(np.int64)
    h = sum(BLUR[k] * p[:, k:k + 31] for k in range(7))
    return sum(BLUR[k] * h[k:k + 31, :] for k in range(7))


def describe(g, keypoints):
    """(bins int32 [k], descriptors uint8 [k, 32], unique [k] bool: the best bin has no tie)."""
    bins, desc, unique = [], [], []
    for x, y in np.asarray(keypoints, dtype=np.int64).reshape(-1, 2):
        x, y = int(x), int(y)
        sc = bin_scores(*moments(g, x, y))
        k = sc.index(max(sc))                              # exact Python integers, the lowest k on ties
        b = blurred_patch(g, x, y)
        pat = pattern(k)
        bits = b[pat[:, 1] + 15, pat[:, 0] + 15] < b[pat[:, 3] + 15, pat[:, 2] + 15]
        desc.append(np.packbits(bits.astype(np.uint8), bitorder="little"))
        bins.append(k)
        unique.append(sc.count(max(sc)) == 1)
    return (np.array(bins, dtype=np.int32), np.array(desc, dtype=np.uint8).reshape(-1, 32), np.array(unique, dtype=bool))


def back_project(depth, keypoints, camera):
    fx, fy, cx, cy = (np.float64(v) for v in camera)
    kp = np.asarray(keypoints, dtype=np.int64).reshape(-1, 2)
    d = depth[kp[:, 1], kp[:, 0]].astype(np.float32)
    ok = depth_valid(d)
    Z = d.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        X = ((kp[:, 0].astype(np.float64) - cx) * Z) / fx
        Y = ((kp[:, 1].astype(np.float64) - cy) * Z) / fy
    pts = np.stack([X, Y, Z], axis=1)
    pts[~ok] = np.nan
    return pts


def extract(image, depth, camera, max_features=1000, quality_level=0.001, min_distance=7, border=19, depth_as_mask=True):
    g = gray(image)
    R, rmax = response(g)
    kp, resp = select(R, depth_valid(depth) if depth_as_mask else None, max_features, quality_level, min_distance, border, rmax)
    bins, desc, _ = describe(g, kp)
    return dict(keypoints=kp, responses=resp, bins=bins, descriptors=desc, points=back_project(depth, kp, camera))


def block_texture(H, W, seed, block=8):
    """Random grey blocks of `block` pixels: corners where four blocks meet."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 256, size=((H + block - 1) // block, (W + block - 1) // block), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(cells, np.ones((block, block), dtype=np.uint8))[:H, :W])
