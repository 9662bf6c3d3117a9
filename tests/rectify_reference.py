"""float64 numpy restatement of csrc/rectify.h, operation for operation (numpy rounds every product and sum on its own, as
the header does under -ffp-contract=off), and a test-only renderer of the raw views a distorted, rotated camera would see.

A raw camera is 26 float64: K = (fx, fy, cx, cy), D = (k1, k2, p1, p2, k3, k4, k5, k6), R row-major, P = (fx', fy', cx',
cy') and Tx fx'.  A map is int32 [H, W, 2] = (qx, qy) in 1/32 pixel, both NONE where there is no source position."""
import numpy as np

import feat_reference

NONE = -2 ** 31
Q_LIMIT = 2.0 ** 26


def camera(K, D, R, P, tx=0.0):
    D = list(D) + [0.0] * (8 - len(D))
    return np.array(list(K) + D + list(np.asarray(R, dtype=np.float64).reshape(9)) + list(P) + [tx], dtype=np.float64)


def identity_camera(P):
    return camera(P, [0.0] * 8, np.identity(3), P)


def rotation(w):
    """exp of the rotation vector w (Rodrigues)."""
    w = np.asarray(w, dtype=np.float64)
    t = float(np.linalg.norm(w))
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t < 1e-12:
        return np.identity(3) + Kx
    return np.identity(3) + (np.sin(t) / t) * Kx + ((1.0 - np.cos(t)) / (t * t)) * (Kx @ Kx)


# ---- the rule --------------------------------------------------------------------------------------------------------
def distort(cam, xn, yn):
    """(mx, my) of normalised (xn, yn): the second half of the map, in the header's order."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in cam[:12])
    r2 = xn * xn + yn * yn
    r4 = r2 * r2
    r6 = r4 * r2
    rad = (1.0 + k1 * r2 + k2 * r4 + k3 * r6) / (1.0 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = xn * rad + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
    yd = yn * rad + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
    return fx * xd + cx, fy * yd + cy


def rect_map(cam, H, W):
    cam = np.asarray(cam, dtype=np.float64)
    R = cam[12:21]
    pfx, pfy, pcx, pcy = cam[21:25]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        x = (u - pcx) / pfx
        y = (v - pcy) / pfy
        X = R[0] * x + R[3] * y + R[6]
        Y = R[1] * x + R[4] * y + R[7]
        Wd = R[2] * x + R[5] * y + R[8]
        xn = X / Wd
        yn = Y / Wd
        mx, my = distort(cam, xn, yn)
        fqx = np.floor(mx * 32.0 + 0.5)
        fqy = np.floor(my * 32.0 + 0.5)
        ok = (Wd > 0.0) & (np.abs(fqx) < Q_LIMIT) & (np.abs(fqy) < Q_LIMIT)
    q = np.full((H, W, 2), NONE, dtype=np.int32)
    q[..., 0][ok] = fqx[ok].astype(np.int32)
    q[..., 1][ok] = fqy[ok].astype(np.int32)
    return q


def bilinear(src, q):
    """(image uint8 [H, W] or [H, W, 3], valid uint8 [H, W]) of a uint8 source through the map q."""
    src = np.asarray(src)
    s3 = src.reshape(src.shape[0], src.shape[1], -1).astype(np.int64)
    Hs, Ws, C = s3.shape
    qx, qy = q[..., 0].astype(np.int64), q[..., 1].astype(np.int64)
    none = (qx == NONE) | (qy == NONE)
    x0, y0, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    total = np.zeros(qx.shape + (C,), dtype=np.int64)
    ok = np.ones(qx.shape, dtype=bool)
    for dx, dy, w in ((0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)):
        x, y = x0 + dx, y0 + dy
        inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        p = s3[np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)]
        total += np.where((inside & (w != 0))[..., None], w[..., None] * p, 0)
        ok &= inside | (w == 0)
    out = ((total + 512) >> 10).astype(np.uint8)
    out[none] = 0
    return (out[..., 0] if src.ndim == 2 else out), (ok & ~none).astype(np.uint8)


def nearest(src, q, mask=None):
    """The source element (its bits) at ((qx + 16) >> 5, (qy + 16) >> 5), 0 outside, 0 where `mask` is 0."""
    src = np.ascontiguousarray(src)
    bits = src.view({2: np.uint16, 4: np.uint32}[src.dtype.itemsize])
    Hs, Ws = bits.shape
    qx, qy = q[..., 0].astype(np.int64), q[..., 1].astype(np.int64)
    xs, ys = (qx + 16) >> 5, (qy + 16) >> 5
    ok = (qx != NONE) & (qy != NONE) & (xs >= 0) & (xs < Ws) & (ys >= 0) & (ys < Hs)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    out = np.where(ok, bits[np.clip(ys, 0, Hs - 1), np.clip(xs, 0, Ws - 1)], 0).astype(bits.dtype)
    return out.view(src.dtype)


def rectify(cam, H, W, image):
    return bilinear(image, rect_map(cam, H, W))


# ---- the test's renderer: what a raw camera sees of a texture that the rectified camera sees undistorted ------------------
def render_raw(texture, x_offset, cam, Hr, Wr):
    """The raw view uint8 [Hr, Wr]: for each raw pixel the distortion is inverted by 30 rounds of fixed-point iteration, the ray
    is rotated by R and projected by P, and the texture (whose column x_offset is the rectified column 0) is sampled
    bilinearly in float64, edge replicated, and rounded."""
    cam = np.asarray(cam, dtype=np.float64)
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = cam[:12]
    R = cam[12:21].reshape(3, 3)
    pfx, pfy, pcx, pcy = cam[21:25]
    v, u = np.meshgrid(np.arange(Hr, dtype=np.float64), np.arange(Wr, dtype=np.float64), indexing="ij")
    xd, yd = (u - cx) / fx, (v - cy) / fy
    xn, yn = xd.copy(), yd.copy()
    for _ in range(30):
        r2 = xn * xn + yn * yn
        rad = (1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2) / (1.0 + k4 * r2 + k5 * r2 * r2 + k6 * r2 * r2 * r2)
        dx = 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
        dy = p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
        xn, yn = (xd - dx) / rad, (yd - dy) / rad
    X = R[0, 0] * xn + R[0, 1] * yn + R[0, 2]
    Y = R[1, 0] * xn + R[1, 1] * yn + R[1, 2]
    Z = R[2, 0] * xn + R[2, 1] * yn + R[2, 2]
    tu, tv = pfx * X / Z + pcx + x_offset, pfy * Y / Z + pcy
    T = np.asarray(texture, dtype=np.float64)
    Ht, Wt = T.shape
    tu, tv = np.clip(tu, 0.0, Wt - 1.0), np.clip(tv, 0.0, Ht - 1.0)
    x0, y0 = np.minimum(np.floor(tu).astype(np.int64), Wt - 2), np.minimum(np.floor(tv).astype(np.int64), Ht - 2)
    a, b = tu - x0, tv - y0
    val = (1.0 - b) * ((1.0 - a) * T[y0, x0] + a * T[y0, x0 + 1]) + b * ((1.0 - a) * T[y0 + 1, x0] + a * T[y0 + 1, x0 + 1])
    return np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)


# ---- the end-to-end scene: the stereo scene of test_stereo_gpu.py behind mildly distorted, slightly rotated raw cameras --------
SCENE_P = (100.0, 100.0, 80.0, 60.0)
SCENE_BASELINE = 0.2
SCENE_K = (98.0, 99.0, 81.5, 58.75)
SCENE_SIZE = (120, 160)
SCENE_PLANT = (-0.32, 0.0, 0.0)
# what the restatement chain gave (test_rectify_cpu.py asserts it); test_rectify_gpu.py expects the MI355X to give the same
SCENE_RECTIFIED = dict(keypoints=[110, 115], accepted=[110, 114], matches=77, inliers=76)
SCENE_RAW = dict(keypoints=[109, 107], accepted=[76, 68], matches=59, inliers=39)


def scene_cameras():
    left = camera(SCENE_K, (-0.08, 0.02, 0.001, -0.0015), rotation([0.004, -0.006, 0.008]), SCENE_P)
    right = camera(SCENE_K, (-0.07, 0.015, -0.0008, 0.001), rotation([-0.003, 0.005, -0.007]), SCENE_P, tx=-SCENE_BASELINE * SCENE_P[0])
    return left, right


def scene():
    """(raw lefts, raw rights, left camera, right camera): two stereo frames 16 columns apart, true disparity 10 = 2 m."""
    tex = feat_reference.block_texture(120, 200, seed=7)
    left, right = scene_cameras()
    H, W = SCENE_SIZE
    lefts = [render_raw(tex, a, left, H, W) for a in (0, 16)]
    rights = [render_raw(tex, a + 10, right, H, W) for a in (0, 16)]
    return lefts, rights, left, right


# ---- the cases of test_rectify_cpu.py (host build, sanitizer program) and test_rectify_gpu.py -----------------------------
BLOCK, RUN = 256, 4                        # csrc/rectify.h: threads per workgroup, destination pixels per thread of the remap
BASE_K, BASE_P = (31.0, 29.5, 20.25, 17.5), (33.0, 32.0, 24.5, 19.75)
BASE_D = (-0.21, 0.07, 0.004, -0.003, -0.01, 0.02, -0.005, 0.001)
BASE_R = (0.03, -0.05, 0.08)


def map_cases():
    """(name, camera float64 [26], H, W): every term of the rule alone and together, the sizes around a workgroup's 256 pixels,
    and the three ways to have no source position."""
    out = [("identity", identity_camera(BASE_P), 40, 49),
           ("intrinsics", camera(BASE_K, [], np.identity(3), BASE_P), 40, 49),
           ("rotation", camera(BASE_P, [], rotation(BASE_R), BASE_P), 40, 49),
           ("all", camera(BASE_K, BASE_D, rotation(BASE_R), BASE_P), 40, 49)]
    for k, name in enumerate(("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")):
        D = [0.0] * 8
        D[k] = BASE_D[k] * 3.0
        out.append((name, camera(BASE_K, D, np.identity(3), BASE_P), 13, 17))
    full = camera(BASE_K, BASE_D, rotation(BASE_R), BASE_P)
    out += [("size %d x %d" % s, full, s[0], s[1]) for s in ((2, 2), (2, 3), (3, 2), (5, 7), (2, 127), (2, 128), (2, 129), (3, 85), (3, 86),
                                                           (255, 2), (257, 3), (16, 16), (17, 31))]
    # a rotation of 80 degrees about y: Wd = sin(80) x + cos(80) <= 0 on the left of the image
    out.append(("behind", camera(BASE_K, BASE_D, rotation([0.0, np.deg2rad(80.0), 0.0]), (20.0, 20.0, 24.0, 10.0)), 21, 49))
    # xn = yn = 1 at pixel (6, 5): r2 = 2, 1 + k4 r2 = 0 exactly; the numerator is 0 there too (NaN) or 2 (infinity)
    out.append(("0 / 0", camera(BASE_K, (-0.5, 0, 0, 0, 0, -0.5, 0, 0), np.identity(3), (4.0, 4.0, 2.0, 1.0)), 9, 11))
    out.append(("2 / 0", camera(BASE_K, (0.5, 0, 0, 0, 0, -0.5, 0, 0), np.identity(3), (4.0, 4.0, 2.0, 1.0)), 9, 11))
    # |m| beyond 2^26 / 32 = 2^21 pixels away from the image centre, on both sides, in x and in y
    out.append(("far x", camera((3.0e7, 30.0, 20.0, 17.0), [], np.identity(3), BASE_P), 12, 49))
    out.append(("far y", camera((30.0, 2.5e8, 20.0, 17.0), [], np.identity(3), BASE_P), 40, 9))
    return out


def remainder_source(target):
    """A 2 x 2 source (a, b; c, d) whose sum at q = (1, 1), 961 a + 31 b + 31 c + d, leaves `target` modulo 1024."""
    for a in range(255, -1, -1):
        for b in range(256):
            d = (target - 961 * a - 31 * b) % 1024
            if d < 256:
                return np.array([[a, b], [0, d]], dtype=np.uint8)
    raise AssertionError(target)


def coordinates(n_src):
    """Quantised coordinates that meet every rule of a sampler along one axis of a source of n_src pixels."""
    q = [32 * x0 + a for x0 in (-2, -1, 0, 1, n_src - 2, n_src - 1, n_src) for a in (0, 1, 16, 31)]
    q += list(range(-33, 0)) + [15, 17, 47, 48, 49, 32 * (n_src - 1) + 15, 32 * (n_src - 1) + 17, NONE, NONE + 1, 2 ** 31 - 1, 2 ** 26, -2 ** 26]
    return np.array(q, dtype=np.int64)


def grid_map(Hs, Ws):
    """int32 [len(qy), len(qx), 2]: every coordinate of `coordinates` in x with every one in y."""
    qx, qy = coordinates(Ws), coordinates(Hs)
    return np.stack(np.broadcast_arrays(qx[None, :], qy[:, None]), axis=2).astype(np.int32)


def random_map(rng, H, W, Hs, Ws, none=0.05):
    q = np.stack([rng.integers(-48, 32 * Ws + 48, (H, W)), rng.integers(-48, 32 * Hs + 48, (H, W))], axis=2).astype(np.int32)
    q[rng.random((H, W)) < none] = NONE
    return q


def remap_cases():
    """(name, source uint8 [Hs, Ws] or [Hs, Ws, 3], map int32 [H, W, 2])."""
    rng = np.random.default_rng(11)
    out = []
    for C in (1, 3):
        src = rng.integers(0, 256, (5, 7, C), dtype=np.uint8)
        out.append(("grid, %d channels" % C, src[..., 0] if C == 1 else src, grid_map(5, 7)))
        for value in (0, 255):
            out.append(("all %d, %d channels" % (value, C), np.full((6, 4, C), value, np.uint8)[..., 0] if C == 1 else np.full((6, 4, C), value, np.uint8),
                        random_map(rng, 9, 13, 6, 4)))
    one = np.zeros((2, 3, 2), dtype=np.int32)
    one[0, 0] = (1, 1)                                                       # the other entries: the source's own corner
    for target in (511, 512, 513):
        src = remainder_source(target)
        assert (961 * int(src[0, 0]) + 31 * int(src[0, 1]) + 31 * int(src[1, 0]) + int(src[1, 1])) % 1024 == target
        out.append(("remainder %d" % target, src, one))
        out.append(("remainder %d, 3 channels" % target, np.stack([src, src[::-1], src.T], axis=2), one))
    # widths around a thread's run, a wave's 64 runs and a workgroup's 256 (an image is at least 2 x 2: no width of 1)
    sizes = [(2, w) for w in range(2, 10)] + [(3, 81), (3, 84), (2, 125), (2, 128), (2, 129), (5, 52), (5, 53), (3, 340), (3, 341), (2, 509), (2, 512),
                                               (2, 513), (257, 3), (65, 4), (65, 5)]
    for k, (H, W) in enumerate(sizes):
        C = 1 + 2 * (k % 2)
        src = rng.integers(0, 256, (4 + k % 5, 3 + k % 7, C), dtype=np.uint8)
        out.append(("%d x %d, %d channels" % (H, W, C), src[..., 0] if C == 1 else src, random_map(rng, H, W, src.shape[0], src.shape[1])))
    return out


def nearest_cases():
    """(name, source uint16 or float32 [Hs, Ws], map): the extremes by bits, the ties of (q + 16) >> 5 on both sides of zero, a
    depth image half the size of its destination."""
    rng = np.random.default_rng(12)
    u16 = rng.integers(1, 65535, (5, 7)).astype(np.uint16)
    u16[0, :4] = (0, 65535, 1, 32768)
    f32 = rng.standard_normal((5, 7)).astype(np.float32)
    f32.view(np.uint32)[0, :7] = (0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001)
    out = [("uint16 grid", u16, grid_map(5, 7)), ("float32 grid", f32, grid_map(5, 7))]
    # the camera of a half-size depth image: K halved about the pixel centres
    K = (BASE_K[0] / 2, BASE_K[1] / 2, (BASE_K[2] + 0.5) / 2 - 0.5, (BASE_K[3] + 0.5) / 2 - 0.5)
    half = rect_map(camera(K, BASE_D, rotation(BASE_R), BASE_P), 40, 49)
    out.append(("uint16 half size", rng.integers(0, 65536, (20, 25)).astype(np.uint16), half))
    out.append(("float32 half size", rng.standard_normal((20, 25)).astype(np.float32), half))
    for H, W in ((2, 127), (2, 128), (2, 129), (3, 2)):
        out.append(("uint16 %d x %d" % (H, W), rng.integers(0, 65536, (6, 5)).astype(np.uint16), random_map(rng, H, W, 6, 5)))
    return out


def batch_case():
    """A ragged batch: (sources, maps, map_index) with mixed sizes and channels, a map shared by several frames and frames of
    different maps."""
    rng = np.random.default_rng(13)
    maps = [random_map(rng, 9, 13, 6, 8), rect_map(camera(BASE_K, BASE_D, rotation(BASE_R), BASE_P), 40, 49), random_map(rng, 2, 5, 3, 3),
            random_map(rng, 17, 4, 6, 8)]
    index = np.array([1, 0, 1, 2, 3, 1, 0, 2], dtype=np.int32)
    shapes = [(40, 41, 3), (6, 8), (33, 50), (3, 3, 3), (6, 8, 3), (35, 42, 3), (7, 5), (2, 2)]
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes], maps, index
