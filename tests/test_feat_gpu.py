"""GPU: the keyframe features (csrc/feat.hip through cslam_amd.front_end.visual_features) against their integer
restatement (tests/feat_reference.py).  Everything is compared bit for bit; only the end-to-end registration has bounds,
and they follow from the 2 px inlier threshold."""
import functools

import numpy as np
import pytest

import feat_reference as ref
from cslam_amd.front_end import visual_features as vf
from cslam_amd.front_end import visual_registration as vr

pytestmark = pytest.mark.gpu

T = vf.FEAT_TILE
# 2 x 2 and 3 x 3 (every pixel reflects), each side one below, at and one above the tile, and a map of several tiles
RESPONSE_SIZES = [(2, 2), (3, 3)] + [(h, w) for h in (T - 1, T, T + 1) for w in (T - 1, T, T + 1)] + [(2 * T + 8, 3 * T + 1), (2, 3 * T)]
TEXTURES = {(64, 80): 12, (96, 128): 69, (120, 160): 127}   # keypoints the restatement keeps there (computed on the CPU)


def content(kind, H, W, seed):
    if kind == "blocks":
        return ref.block_texture(H, W, seed, block=4)
    if kind == "noise":
        return (np.random.default_rng(seed).integers(0, 2, (H, W)) * 255).astype(np.uint8)
    q = np.zeros((H, W), dtype=np.uint8)                   # quadrants: the largest a, c and D at the crossing
    q[:H // 2, :W // 2] = 255
    q[H // 2:, W // 2:] = 255
    return q


@functools.lru_cache(maxsize=None)
def texture(H, W):
    g = ref.block_texture(H, W, seed=H)
    R, rmax = ref.response(g)
    kp, resp = ref.select(R, rmax=rmax)
    bins, desc, unique = ref.describe(g, kp)
    for a in (g, R, kp, resp, bins, desc, unique):
        a.setflags(write=False)
    return dict(gray=g, R=R, rmax=rmax, keypoints=kp, responses=resp, bins=bins, descriptors=desc, unique=unique)


# ---- response and grey ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blocks", "noise", "quadrants"])
def test_response_equals_the_restatement(kind):
    imgs = [content(kind, h, w, 10 * h + w) for h, w in RESPONSE_SIZES]
    got = vf.corner_response_batch(imgs)
    for g, (R, rmax) in zip(imgs, got):
        want_R, want_max = ref.response(g)
        assert R.dtype == np.int32 and R.shape == g.shape
        assert np.array_equal(R, want_R), g.shape
        assert rmax == want_max, g.shape
    if kind != "blocks":                                   # these reach past what 32 bits hold in D
        assert max(ref.response(g, parts=True)[3].max() for g in imgs) > 2 ** 40
    R, rmax = vf.corner_response(imgs[-2])                 # alone: the same bytes
    assert np.array_equal(R, got[-2][0]) and rmax == got[-2][1]


def test_gray_equals_the_restatement():
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    bgr[0, 0] = 255
    bgr[0, 1] = 0
    bgr[1, 0] = (255, 0, 0)
    bgr[1, 1] = (0, 255, 0)
    bgr[1, 2] = (0, 0, 255)
    mono = rng.integers(0, 256, (20, 31), dtype=np.uint8)
    g3, g1, g31 = vf.to_gray_batch([bgr, mono, mono[:, :, None]])
    assert g3.dtype == np.uint8 and np.array_equal(g3, ref.gray(bgr)) and g3[0, 0] == 255 and g3[0, 1] == 0
    assert np.array_equal(g1, mono) and np.array_equal(g31, mono)
    assert np.array_equal(vf.to_gray(bgr), g3)


# ---- selection on constructed response maps ------------------------------------------------------------------------
def check_selection(R, **kw):
    kp, resp = vf.select_keypoints(R, **kw)
    want_kp, want_resp = ref.select(R, **kw)
    assert kp.dtype == np.int32 and resp.dtype == np.int32
    assert np.array_equal(kp, want_kp) and np.array_equal(resp, want_resp)
    return kp.tolist()


def test_selection_constant_maps():
    assert check_selection(np.zeros((64, 96), dtype=np.int32)) == []
    # a constant map above zero: every pixel inside the border ties, the pixel index alone orders them
    kp = check_selection(np.full((64, 96), 5, dtype=np.int32))
    assert kp[:3] == [[19, 19], [26, 19], [33, 19]]


def test_selection_index_tie_rule_on_a_periodic_map():
    R = np.zeros((96, 128), dtype=np.int32)
    R[::8, ::8] = 1000                                     # equal responses 8 px apart
    assert len(check_selection(R)) == len(range(24, 77, 8)) * len(range(24, 109, 8))        # min_distance 7: all of them
    kp = check_selection(R, min_distance=9)                # now neighbours exclude each other: the lower index wins
    assert kp[:2] == [[24, 24], [40, 24]]
    check_selection(R, min_distance=12)
    R[::8, ::8] += (np.arange(12)[:, None] * 16 + np.arange(16)[None, :]).astype(np.int32) % 3          # three levels, many ties
    check_selection(R, min_distance=9)


def test_selection_dependency_chain():
    R = np.zeros((64, 300), dtype=np.int32)
    xs = 20 + 4 * np.arange(60)
    R[30, xs] = 1000 - np.arange(60)                       # 4 px apart, strictly decreasing: every second one is accepted
    kp = check_selection(R)
    assert kp == [[int(x), 30] for x in xs[::2]]
    R[30, xs] = 1000 + np.arange(60)                       # increasing: the chain runs from the other end
    assert check_selection(R) == [[int(x), 30] for x in xs[::-1][::2]]


def test_selection_distance_is_compared_on_integer_squares():
    R = np.zeros((64, 200), dtype=np.int32)
    R[30, 30], R[30, 37] = 900, 800                        # exactly 7 apart: accepted
    R[30, 80], R[35, 85] = 700, 600                        # (5, 5): 50 >= 49, accepted
    R[30, 130], R[35, 134] = 500, 400                      # (4, 5): 41 < 49, rejected
    assert check_selection(R) == [[30, 30], [37, 30], [80, 30], [85, 35], [130, 30]]
    assert check_selection(R, min_distance=8) == [[30, 30], [80, 30], [130, 30]]
    assert len(check_selection(R, min_distance=1)) == 6


def test_selection_max_features_truncates_the_same_list():
    t = texture(96, 128)
    kp, resp = vf.select_keypoints(t["R"], max_features=5)
    assert np.array_equal(kp, t["keypoints"][:5]) and np.array_equal(resp, t["responses"][:5])
    check_selection(t["R"], max_features=1)


def test_selection_validity_mask_drops_a_stripe():
    t = texture(96, 128)
    valid = np.ones((96, 128), dtype=bool)
    valid[:, 50:70] = False
    kp = check_selection(t["R"], valid=valid, min_distance=12)        # the texture's corners lie 8 apart: they compete
    assert all(not 50 <= x < 70 for x, _ in kp)
    before = set(map(tuple, ref.select(t["R"], min_distance=12)[0].tolist()))
    assert any(50 <= x < 70 for x, _ in before)            # the stripe held keypoints
    assert set(map(tuple, kp)) - before                    # and neighbours they had excluded take their place
    kp8, _ = vf.select_keypoints(t["R"], valid=valid.astype(np.uint8), min_distance=12)
    assert kp8.tolist() == kp


def test_selection_border_rows():
    R = np.zeros((64, 96), dtype=np.int32)
    R[18, 30], R[19, 50], R[44, 40], R[45, 60], R[30, 18], R[38, 19], R[30, 76], R[38, 77] = 10, 9, 8, 7, 6, 5, 4, 3
    assert check_selection(R) == [[50, 19], [40, 44], [19, 38], [76, 30]]
    assert check_selection(R, border=18) == [[30, 18], [50, 19], [40, 44], [60, 45], [18, 30], [19, 38], [76, 30], [77, 38]]


# ---- detection, descriptors and bins on textures -------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(TEXTURES))
def test_detection_and_description_on_a_block_texture(shape):
    t = texture(*shape)
    assert len(t["keypoints"]) == TEXTURES[shape]
    R, rmax = vf.corner_response(t["gray"])
    assert np.array_equal(R, t["R"]) and rmax == t["rmax"]
    kp, resp = vf.select_keypoints(R)
    assert np.array_equal(kp, t["keypoints"]) and np.array_equal(resp, t["responses"])
    bins, desc = vf.describe(t["gray"], kp)
    assert bins.dtype == np.int32 and desc.dtype == np.uint8 and desc.shape == (len(kp), 32)
    assert np.array_equal(bins, t["bins"]) and np.array_equal(desc, t["descriptors"])


def test_description_18_px_from_each_edge():
    g = texture(64, 80)["gray"]
    H, W = g.shape
    kp = np.array([[18, 18], [W - 19, 18], [18, H - 19], [W - 19, H - 19], [40, 18], [40, H - 19], [18, 30], [W - 19, 30], [40, 32]])
    bins, desc = vf.describe(g, kp)
    want_bins, want_desc, _ = ref.describe(g, kp)
    assert np.array_equal(bins, want_bins) and np.array_equal(desc, want_desc)
    assert vf.describe(g, np.zeros((0, 2), dtype=np.int32))[1].shape == (0, 32)


def test_quarter_turn_shifts_the_bin_by_8_and_keeps_the_bytes():
    t = texture(96, 128)
    g, kp = t["gray"], t["keypoints"]
    H, W = g.shape
    turned = np.ascontiguousarray(np.rot90(g))             # turned[i, j] = g[j, W - 1 - i]
    kp_t = np.stack([kp[:, 1], W - 1 - kp[:, 0]], axis=1)
    bins, desc = vf.describe(g, kp)
    bins_t, desc_t = vf.describe(turned, kp_t)
    _, _, unique_t = ref.describe(turned, kp_t)
    ok = t["unique"] & unique_t
    assert ok.mean() >= 0.99
    assert set(((bins_t - bins) % 32)[ok].tolist()) == {24}          # 8 backwards
    assert np.array_equal(desc_t[ok], desc[ok])


def same_floats(a, b):
    """The same bits, any NaN counting as NaN."""
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


# ---- points --------------------------------------------------------------------------------------------------------
def test_points_equal_numpy_bit_for_bit():
    rng = np.random.default_rng(4)
    depth = (0.3 + 9.0 * rng.random((40, 56))).astype(np.float32)
    depth[5, 7], depth[6, 8], depth[7, 9], depth[8, 10], depth[9, 11] = 0.0, np.nan, np.inf, -1.5, -np.inf
    kp = np.array([[7, 5], [8, 6], [9, 7], [10, 8], [11, 9], [0, 0], [55, 39], [0, 39], [55, 0]] +
                  [[int(rng.integers(56)), int(rng.integers(40))] for _ in range(300)])
    cam = (523.7, 519.1, 27.37, 19.81)
    pts = vf.back_project(depth, kp, cam)
    want = ref.back_project(depth, kp, cam)
    assert pts.dtype == np.float64 and pts.shape == (len(kp), 3)
    same_floats(pts, want)
    assert np.all(np.isnan(pts[:5])) and np.all(np.isfinite(pts[5:9]))
    mm = np.round(np.where(ref.depth_valid(depth), depth, 0.0) * 1000).astype(np.uint16)
    pts16 = vf.back_project(mm, kp, cam)
    want16 = ref.back_project(mm.astype(np.float32) * np.float32(0.001), kp, cam)
    same_floats(pts16, want16)
    assert np.all(np.isnan(pts16[:5]))                     # 0, NaN, inf and negative all became 0 mm: no depth


# ---- batches -------------------------------------------------------------------------------------------------------
def mixed_batch(seed, shapes):
    rng = np.random.default_rng(seed)
    images, depths = [], []
    for k, (H, W) in enumerate(shapes):
        g = ref.block_texture(H, W, seed=seed + k, block=6 + k % 3)
        images.append(np.stack([g, np.roll(g, 3, axis=1), g[::-1]], axis=2).copy() if k % 2 else g)
        d = (1.0 + rng.random((H, W))).astype(np.float32)
        d[:, W // 2:W // 2 + 9] = 0.0                      # a stripe without depth
        depths.append(d if k % 3 else np.round(d * 1000).astype(np.uint16))
    cams = np.array([[100.0 + k, 101.0, W / 2 + 0.25, H / 2 - 0.5] for k, (H, W) in enumerate(shapes)])
    return images, depths, cams


def same_features(a, b):
    for key in ("keypoints", "responses", "bins", "descriptors"):
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    same_floats(a["points"], b["points"])


def test_a_mixed_batch_equals_one_by_one_the_staged_calls_and_the_restatement():
    first = mixed_batch(1, [(64, 80), (41, 97), (120, 63), (50, 50), (77, 130)])
    second = mixed_batch(2, [(90, 45), (48, 160), (66, 66)])            # other sizes right after: the scratch is carved afresh
    for images, depths, cams in (first, second):
        got = vf.extract_features(images, depths, cams, max_features=40)
        for k, (img, d) in enumerate(zip(images, depths)):
            same_features(got[k], vf.extract_features([img], [d], cams[k], max_features=40)[0])
            same_features(got[k], ref.extract(img, vf.depth_metres(d), cams[k], max_features=40))
            assert 0 < len(got[k]["keypoints"]) <= 40
            # the staged calls
            g = vf.to_gray(img)
            R, _ = vf.corner_response(g)
            kp, resp = vf.select_keypoints(R, valid=ref.depth_valid(vf.depth_metres(d)), max_features=40)
            bins, desc = vf.describe(g, kp)
            same_features(got[k], dict(keypoints=kp, responses=resp, bins=bins, descriptors=desc, points=vf.back_project(d, kp, cams[k])))
    # without the mask a keypoint may have no depth: a NaN row
    images, depths, cams = first
    free = vf.extract_features(images, depths, cams, depth_as_mask=False)
    for k, f in enumerate(free):
        same_features(f, ref.extract(images[k], vf.depth_metres(depths[k]), cams[k], depth_as_mask=False))
    assert any(np.isnan(f["points"]).any() for f in free)
    kfs = vf.extract_keyframes(images, depths, cams, max_features=40)
    got = vf.extract_features(images, depths, cams, max_features=40)
    for kf, f in zip(kfs, got):
        assert isinstance(kf, vr.Keyframe) and kf.keypoints.dtype == np.float64 and kf.points.dtype == np.float64
        assert np.array_equal(kf.keypoints, f["keypoints"]) and np.array_equal(kf.descriptors, f["descriptors"])
        assert not np.isnan(kf.points).any()               # the mask leaves only keypoints with depth


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_extracted_keyframes_register_and_decide_the_next_keyframe():
    """Two views of one block texture 16 columns apart at 2 m depth.  Measured on the MI355X: 122 and 124 keypoints, 105 common
    to both views, 105 inliers, translation 2.6e-15 m from the plant (bound 0.04 m), rotation 4.2e-8 rad (bound 0.025 rad)."""
    tex = ref.block_texture(120, 200, seed=7)
    img_from, img_to = np.ascontiguousarray(tex[:, :160]), np.ascontiguousarray(tex[:, 16:176])
    depth = np.full((120, 160), 2.0, dtype=np.float32)
    cam = (100.0, 100.0, 80.0, 60.0)
    kf_from, kf_to = vf.extract_keyframes([img_from, img_to], [depth, depth], cam)
    want = [ref.extract(i, depth, cam) for i in (img_from, img_to)]
    ref_kfs = [vr.Keyframe(w["keypoints"].astype(np.float64), w["points"], w["descriptors"]) for w in want]
    for kf, w in zip((kf_from, kf_to), ref_kfs):
        assert all(np.array_equal(a, b) for a, b in zip(kf, w))
    common = len(set(map(tuple, (want[0]["keypoints"] - [16, 0]).tolist())) & set(map(tuple, want[1]["keypoints"].tolist())))
    reg = vr.register_pairs([(kf_from, kf_to)], cam)[0]
    reg_ref = vr.register_pairs([tuple(ref_kfs)], cam)[0]
    n_in = int(np.count_nonzero(reg.inliers))
    # a point seen at column u of "from" is seen at column u - 16 of "to": x_to = x_from - 16 Z / fx
    t_err = np.abs(reg.transformation[:3, 3] - [-16 * 2.0 / 100.0, 0.0, 0.0]).max()
    Rm = reg.transformation[:3, :3]
    angle = float(np.arccos(np.clip((np.trace(Rm) - 1.0) / 2.0, -1.0, 1.0)))
    print("keypoints %d and %d, common %d, inliers %d, translation error %.3g m, rotation %.3g rad"
          % (len(kf_from.keypoints), len(kf_to.keypoints), common, n_in, t_err, angle))
    assert reg.status == 0 and reg.success
    assert n_in >= common
    assert np.array_equal(reg.transformation, reg_ref.transformation) and np.array_equal(reg.inliers, reg_ref.inliers)
    assert np.array_equal(reg.matches, reg_ref.matches)
    assert t_err <= 2 * 2.0 / 100.0                        # 2 px at Z / fx metres per pixel
    assert angle <= 2.0 / 80.0                             # 2 px at the image's half width
    edge = reg.to_edge((0, 0), (0, 1))
    assert np.abs(edge.measurement @ reg.transformation - np.identity(4)).max() < 1e-12
    assert vf.is_new_keyframe(reg, len(kf_to.keypoints), 0.3) is False
    assert vf.is_new_keyframe(reg, len(kf_to.keypoints), 0.999) is True
