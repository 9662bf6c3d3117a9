"""References and case tables of tests/test_heads_paths_gpu.py and tests/test_heads_reference_cpu.py (numpy only, no device).

VLAD (NetVLADLayer.forward, netvlad.py:94-130, K = 64 clusters):
  vlad_f64      the layer in float64, the 1e-12 floors of its three normalisations included -- the reference of every assertion
  vlad_seq32    the layer in float32 with every sum one chain in index order and one rounding per operation -- the yardstick:
                tol = 4 err(vlad_seq32, vlad_f64), per case and kind (why 4: two float32 orderings of the same sums differ by up to
                about 2 in their largest error; the second factor of two is spare).  Where that error is exactly zero (C = 1)
                the yardstick is the same restatement with the kernels' reciprocal-and-multiply normalisations
  vlad_defect   vlad_f64 with one of three defects planted at the last index (where tails go wrong)
  err           the largest |y - ref| / max_c |ref[n, k, :]| over (n, k, c)
  vlad_path     the dispatch rule of heads.hip's vlad_aggregate and of heads.vlad_aggregate
The float32 projection and the row normalisation have their operands, references and bounds at the end.
"""
import functools

import numpy as np

f32 = np.float32
K = 64
U = 2.0 ** -24                      # unit roundoff of float32
DEFECTS = ("aggregation_last_pixel", "asum_last_pixel", "logits_last_channel")


# ---------------------------------------------------------------------------------------------------------------- the layer ----
def _vlad64(x, w, b, cent, defect=None):
    B, C = x.shape[:2]
    xf = x.astype(np.float64).reshape(B, C, -1)
    xf = xf / np.maximum(np.linalg.norm(xf, axis=1, keepdims=True), 1e-12)
    w, cent = w.astype(np.float64), cent.astype(np.float64)
    if defect == "logits_last_channel":
        sa = np.einsum("kc,ncp->nkp", w[:, :-1], xf[:, :-1])
    else:
        sa = np.einsum("kc,ncp->nkp", w, xf)
    if b is not None:
        sa = sa + b.astype(np.float64)[None, :, None]
    a = np.exp(sa - sa.max(axis=1, keepdims=True))
    a /= a.sum(axis=1, keepdims=True)
    a_agg = a[:, :, :-1] if defect == "aggregation_last_pixel" else a
    a_sum = a[:, :, :-1] if defect in ("aggregation_last_pixel", "asum_last_pixel") else a
    v = np.einsum("nkp,ncp->nkc", a_agg, xf[:, :, :a_agg.shape[2]]) - a_sum.sum(axis=2)[:, :, None] * cent[None]
    v = v / np.maximum(np.linalg.norm(v, axis=2, keepdims=True), 1e-12)
    v = v.reshape(B, -1)
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12), a


def vlad_f64(x, w, b, cent):
    """x [B,C,H,W] (or [B,C,P]) float32, w [64,C], b [64] or None, cent [64,C] -> [B, 64 C] float64"""
    return _vlad64(x, w, b, cent)[0]


def vlad_assignment_f64(x, w, b, cent):
    """the soft assignment a [B,64,P] of vlad_f64"""
    return _vlad64(x, w, b, cent)[1]


def vlad_defect(x, w, b, cent, which):
    """vlad_f64 with a planted defect: `aggregation_last_pixel` -- the sum over the pixels (a x and a cent alike) stops one pixel
    early; `asum_last_pixel` -- only the sum of the assignments (the factor of the centroid) does; `logits_last_channel` -- the
    logits stop one channel early (the pixel norms do not)."""
    assert which in DEFECTS
    return _vlad64(x, w, b, cent, which)[0]


def _seq32_image(x, w, b, cent, recip=False):
    """one image [C,P] -> [64 C] float32; loops are the chains, numpy rounds every elementwise operation to float32"""
    C, P = x.shape
    ss = np.zeros(P, f32)
    for c in range(C):
        ss = ss + x[c] * x[c]
    xn = x * (f32(1.0) / np.maximum(np.sqrt(ss), f32(1e-12))) if recip else x / np.maximum(np.sqrt(ss), f32(1e-12))
    lg = np.zeros((K, P), f32)
    for c in range(C):
        lg = lg + w[:, c, None] * xn[c][None, :]
    if b is not None:
        lg = lg + b[:, None]
    e = np.exp(lg - lg.max(axis=0, keepdims=True))
    se = np.zeros(P, f32)
    for k in range(K):
        se = se + e[k]
    a = e / se
    asum, agg = np.zeros(K, f32), np.zeros((K, C), f32)
    for p in range(P):
        asum = asum + a[:, p]
        agg = agg + a[:, p, None] * xn[None, :, p]
    v = agg - asum[:, None] * cent
    s = np.zeros(K, f32)
    for c in range(C):
        s = s + v[:, c] * v[:, c]
    if recip:                                                # heads.hip: sc = 1 / max(nk, floor), gsum = sum_k (nk sc)^2, v sc gs
        nk = np.sqrt(s)
        sc = f32(1.0) / np.maximum(nk, f32(1e-12))
        nn = nk * sc
        gs = f32(1.0) / np.maximum(np.sqrt(np.cumsum(nn * nn, dtype=f32)[-1]), f32(1e-12))
        out = ((v * sc[:, None]) * gs).reshape(-1)
    else:
        v = (v / np.maximum(np.sqrt(s), f32(1e-12))[:, None]).reshape(-1)
        g = np.cumsum(v * v, dtype=f32)[-1]                  # an accumulation: sequential by construction
        out = v / np.maximum(np.sqrt(g), f32(1e-12))
    assert out.dtype == f32 and a.dtype == f32 and agg.dtype == f32
    return out


def vlad_seq32(x, w, b, cent, recip=False):
    """the layer in float32, every sum a single chain in index order, image by image -> [B, 64 C] float32.
    recip: the three normalisations as every kernel of heads.hip writes them -- a product with the rounded reciprocal of the
    floored norm in place of the layer's division, and the global norm from the clusters' rounded norms (nk sc)^2 -- the same
    chains otherwise.  One rounding more per normalisation: it is the yardstick only where the layer's own arithmetic has no
    error at all (`vlad_case`)."""
    B, C = x.shape[:2]
    xs = np.ascontiguousarray(x, dtype=f32).reshape(B, C, -1)
    w, cent = w.astype(f32), cent.astype(f32)
    b = None if b is None else b.astype(f32)
    return np.stack([_seq32_image(xs[n], w, b, cent, recip) for n in range(B)])


def err(y, ref):
    """largest |y - ref| / max_c |ref[n, k, :]| over (n, k, c); a cluster row that is all zero in the reference must be exactly zero
    in y (inf otherwise)"""
    B = ref.shape[0]
    y3 = np.asarray(y, dtype=np.float64).reshape(B, K, -1)
    r3 = np.asarray(ref, dtype=np.float64).reshape(B, K, -1)
    top = np.abs(r3).max(axis=2, keepdims=True)
    d = np.abs(y3 - r3)
    if np.any((top == 0) & (d > 0)):
        return float("inf")
    return float(np.max(d / np.where(top == 0, 1.0, top)))


def vlad_path(B, C, P, channels_last):
    """heads.hip's vlad_aggregate behind heads.vlad_aggregate: a channels-last map is used in place by the batch kernels (B > 8,
    P <= 256), the matrix form where it fits; any other map is NCHW (the wrapper converts)."""
    if channels_last and B > 8 and P <= 256:
        return "matrix" if C % 128 == 0 and C <= 512 and 32 <= P <= 200 else "fast_nhwc"
    if P > 256:
        return "generic"
    return "split" if B <= 8 else "fast"


# ---------------------------------------------------------------------------------------------------------------- the cases ----
# (B, C, P) by the path of the NCHW call / of the channels-last call where that differs; the smallest shapes at which each path can
# still go wrong.  `NO_BIAS`: the gaussian kind of these cases has no bias (one per path at least).
VLAD_CASES = {
    # 512 channels = the 512-thread configuration; 500, 33, 31, 1: no multiple of the 32-channel weight chunk; 257 = two pixel
    # chunks of 128 and one pixel; 385 = three and one; more than one image
    "generic": [(2, 512, 257), (1, 500, 385), (9, 33, 384), (2, 1, 257), (2, 31, 300)],
    # 256 = 16 full pixel tiles, 255 / 17 / 15 = a ragged one; 500, 33, 31, 1 = a ragged channel slab; P = 1: the assignment cancels
    # in the intra-normalisation, so that case checks the residual and the norms only
    "split": [(1, 512, 256), (8, 500, 255), (3, 33, 17), (1, 1, 16), (2, 31, 15), (8, 64, 1)],
    # both layouts.  (9, 31, 1): P = 1 as above
    "fast": [(9, 512, 256), (9, 500, 255), (9, 33, 17), (9, 31, 1), (9, 1, 9), (10, 96, 129)],
    # channels-last only: just outside the matrix form (P = 31, P = 201, C no multiple of 128, P > 200)
    "fast_nhwc": [(9, 512, 31), (9, 512, 201), (9, 500, 196), (9, 384, 256)],
    # channels-last only: one wave tile, one pixel more, the tile and eight-pixel-group tails 63..65, 193, 199, the full 200
    "matrix": [(9, 128, 32), (9, 256, 33), (9, 384, 63), (9, 512, 64), (9, 512, 65), (9, 128, 193), (9, 512, 199), (9, 256, 200)],
}
PAIR_CASES = [(1, 128, 33), (3, 384, 200)]        # cslam_vlad_aggregate_nhwc_pairs_dev takes any B >= 1: the matrix form's kernel
NO_BIAS = {(9, 33, 384), (3, 33, 17), (10, 96, 129), (9, 500, 196), (9, 384, 63)}
KINDS = ("gauss", "trunk")


def vlad_layouts(path, case):
    """the layouts a case of the table is given to the kernels in: (channels_last, path that runs)"""
    B, C, P = case
    if path in ("fast_nhwc", "matrix"):
        return [(True, path)]
    out = [(False, vlad_path(B, C, P, False))]
    if B > 8 and P <= 256:
        out.append((True, vlad_path(B, C, P, True)))
    return out


def all_vlad_cases():
    return [(path, case) for path, cases in VLAD_CASES.items() for case in cases]


def vlad_inputs(B, C, P, kind, seed=None):
    """-> x [B,C,P] float32, w [64,C], b [64] or None, cent [64,C].
    gauss: standard normal map, weights and bias, centroids uniform in [0, 1).
    trunk: what the trunk and a trained layer give -- a non-negative map (half of its entries zero, like a ReLU's) on a per-channel
    scale up to 30, every 37th channel dead (36, 73, ..: channel 0 lives, so that C = 1 has a map); centroids of unit norm, weights
    200 centroid and bias -100 |centroid|^2 (the layer's initialisation with alpha = 100: a steep softmax).  Pixel P // 2 of every
    frame is all zeros (P > 1); frame 0 is all zeros (B > 1); in the last frame (B > 2) every other pixel lies along centroid 5."""
    rng = np.random.default_rng(1000003 * B + 1009 * C + P + (0 if kind == "gauss" else 7) if seed is None else seed)
    if kind == "gauss":
        x = rng.standard_normal((B, C, P)).astype(f32)
        w = rng.standard_normal((K, C)).astype(f32)
        b = None if (B, C, P) in NO_BIAS else rng.standard_normal(K).astype(f32)
        cent = rng.random((K, C)).astype(f32)
        return x, w, b, cent
    assert kind == "trunk"
    scale = (30.0 * (1.0 - rng.random(C))).astype(f32)                                        # (0, 30]
    scale[-1] = f32(15.0) + scale[-1] / 2      # the last channel is where a tail goes wrong: never a faint one (a scale of 0.07 there
    scale[36::37] = 0                          # hid a lost last channel at (9, 512, 31): 3.8 tol)
    x = np.maximum(rng.standard_normal((B, C, P)), 0).astype(f32) * scale[None, :, None]
    # The centroids lie in a cone about the direction of a non-negative descriptor, (1 .. 1), of a width that gives the logits of
    # a pixel the same spread at every C (200 x 0.15 / sqrt(32): a standard deviation of about 5, assignments from 1e-13 to
    # 0.99).  With independent directions the spread would grow as 200 / sqrt(C) and, from C = 100 down, the smallest
    # assignments would underflow in float32 while float64 keeps them: `err` would compare a zero with 1e-60.
    t = 0.15 * np.sqrt(C / 32.0)
    cent = 1.0 + t * rng.standard_normal((K, C))
    cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(f32)
    w = (f32(200.0) * cent).astype(f32)
    b = (f32(-100.0) * np.sum(cent * cent, axis=1, dtype=f32)).astype(f32)
    if B > 2:
        # along centroid 5: the common direction plus s times what sets centroid 5 apart from it (s keeps the other clusters'
        # assignments above 1e-25), every pixel at a length of its own, a little noise, clipped like the rest of the map
        mid = cent.astype(np.float64).mean(axis=0)
        s = 3.0 / np.sqrt(max(C, 32) / 32.0)
        ray = mid + s * (cent[5].astype(np.float64) - mid)
        x[-1] = np.maximum(ray[:, None] * (1.0 + rng.random(P))[None, :] + (0.05 / np.sqrt(C)) * rng.random((C, P)), 0).astype(f32)
    x[:, 36::37] = 0
    if P > 1:
        x[:, :, P // 2] = 0
    if B > 1:
        x[0] = 0
    return x, w, b, cent


@functools.lru_cache(maxsize=6)
def vlad_case(B, C, P, kind):
    """-> dict: the inputs, ref = vlad_f64, yard = err(vlad_seq32, ref), tol = 4 yard; computed once per case and kind, read-only"""
    x, w, b, cent = vlad_inputs(B, C, P, kind)
    ref = vlad_f64(x, w, b, cent)
    yard = err(vlad_seq32(x, w, b, cent), ref)
    if yard == 0.0:
        # C = 1: every quotient of the layer is exact (x / sqrt(x x) = +- 1, v / sqrt(v v) = +- 1, 1 / sqrt(64) = 1 / 8), so
        # the float32 layer has no error to measure the kernels by, while their reciprocal-and-multiply normalisations round
        # once (measured on an MI355X: 5.96e-8 = 2^-24 in all four NCHW / NHWC paths on the gaussian kind, 0 on the trunk
        # kind).  That arithmetic is legitimate float32; the yardstick is then the restatement that normalises as they do.
        yard = err(vlad_seq32(x, w, b, cent, recip=True), ref)
    for a in (x, w, cent, ref) + (() if b is None else (b,)):
        a.setflags(write=False)
    return dict(x=x, w=w, b=b, cent=cent, ref=ref, yard=yard, tol=4.0 * yard)


# ------------------------------------------------------------------------------------------- the float32 projection, exactly ----
# Operands on which every product and every partial sum is an integer below 2^24 in any order: x in {-2, -1, 1, 2}, components in
# {-3 .. -1, 1 .. 3}, integer mean_proj, inv_scale powers of two.  The only rounding left is the epilogue's: the float32 sum of Dout
# squares (within Dout u in any order, so the norm within Dout u / 2), one square root and one division (one ulp = 2 u each):
#     |out - ref| <= (Dout / 2 + 4) u |ref|
# A wrong K slice, split boundary, clamped row or ragged store moves the raw sum by at least one unit.
PCA_GEMV = dict(B=(1, 2, 3, 4),
                # 32: one tail trip of lane 0..7; 288: tail only; 1792: seven tail trips, the 2048-float loop just not entered;
                # 2016: lanes 0..55 take the 2048-float trip, lanes 56..63 do not; 2048: the loop covers Din; 2336: both loops
                Din=(32, 288, 1792, 2016, 2048, 2336),
                # an odd Dout runs the j1 == j0 row; 129 = more than one workgroup of four waves x two rows ... x 16
                Dout=(1, 2, 7, 50, 129))
PCA_TILE = dict(B=(5, 128, 129),
                # K steps of 32 (split counts for 256 compute units, Dout <= 128, B <= 128: S = min(512, steps / 8)): 32 = one
                # step; 224 = seven steps, one split; 832 = 26 steps in splits of 9, 9, 8; 4096 = 128 steps in 16 equal splits;
                # 4128 = 129 steps: splits of 9 and a last one of three (the kt1 clamp)
                Din=(32, 224, 832, 4096, 4128),
                Dout=(1, 50, 127, 128, 129, 130))
PCA_ZERO_ROW = 2                    # row 2 of x is all zeros (B >= 3)


@functools.lru_cache(maxsize=1)
def pca_operands():
    """x [129, 4128], comp [130, 4128], mean_proj [130], inv_scale [130]: every case takes the leading rows and columns"""
    rng = np.random.default_rng(424242)
    x = rng.choice(np.array([-2, -1, 1, 2], f32), size=(129, 4128))
    x[PCA_ZERO_ROW] = 0
    comp = rng.choice(np.array([-3, -2, -1, 1, 2, 3], f32), size=(130, 4128))
    mp = rng.integers(-40, 41, size=130).astype(f32)
    inv = (2.0 ** rng.integers(-3, 4, size=130)).astype(f32)
    for a in (x, comp, mp, inv):
        a.setflags(write=False)
    return x, comp, mp, inv


def pca_ref(B, Din, Dout, mean, scale, drop_last=False):
    """-> (ref [B, Dout] float64, raw: the integer sums before the normalisation, float64).  drop_last: the last K term missing."""
    x, comp, mp, inv = pca_operands()
    kk = Din - 1 if drop_last else Din
    v = x[:B, :kk].astype(np.float64) @ comp[:Dout, :kk].astype(np.float64).T
    if mean:
        v = v - mp[:Dout].astype(np.float64)
    if scale:
        v = v * inv[:Dout].astype(np.float64)
    n = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
    n[n == 0] = 1
    return v / n, v


def pca_bound(Dout, ref):
    return (Dout / 2.0 + 4.0) * U * np.abs(ref)


def pca_epilogues(i):
    """(mean_proj given, inv_scale given) of the i-th call of a sweep: the four combinations in turn"""
    return bool(i & 1), bool(i & 2)


# ----------------------------------------------------------------------------------------------------- the row normalisation ----
# l2_normalize_kernel: 256 threads, ceil(d / 256) squares per thread in one chain, six shuffle steps, four wave partials added in
# turn: the sum of squares within (ceil(d / 256) + 10) u, the norm within half of that and one ulp (2 u) for the square root, the
# quotient one ulp more:
#     |out - ref| <= ((ceil(d / 256) + 10) / 2 + 4) u |ref|
L2_D = (1, 63, 255, 256, 257, 1000)
L2_N = (1, 37)


def l2_bound(d, ref):
    return ((-(-d // 256) + 10) / 2.0 + 4.0) * U * np.abs(ref)


def l2_rows(n, d, seed):
    """-> rows [n, d] float32 and the indices of the special rows: row 0 gaussian; with n = 37 also: `square` -- entries in
    {-3, 0, 3}, q^2 of them non-zero, so the sum of squares is the exact perfect square (3 q)^2; `zero` -- all zeros; `tiny` -- a norm
    below 1e-12 (entries 1e-14 or so: the squares are normal float32 numbers)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(f32)
    special = {}
    if n >= 4:
        q = int(np.sqrt(d))
        row = np.zeros(d, f32)
        row[rng.permutation(d)[:q * q]] = 3.0 * rng.choice(np.array([-1.0, 1.0], f32), size=q * q)
        x[1] = row
        x[2] = 0
        x[3] = (1e-14 * rng.standard_normal(d)).astype(f32) if d > 1 else f32(3e-13)
        special = dict(square=1, zero=2, tiny=3)
    return x, special


def l2_ref(x, eps, zero_norm_to_one):
    nrm = np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=1, keepdims=True))
    den = np.where(nrm == 0, 1.0, nrm) if zero_norm_to_one else np.maximum(nrm, np.float64(f32(eps)))
    return x.astype(np.float64) / den
