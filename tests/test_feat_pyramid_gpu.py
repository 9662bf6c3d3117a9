"""GPU: the scale pyramid of the keyframe features (feat_pyr_level_kernel, feat_pyr_merge_kernel and the chains of csrc/feat.hip
through cslam_amd.front_end.visual_pyramid) against its numpy restatement (tests/feat_pyramid_reference.py).  Everything is
compared bit for bit: level images, validity maps, keypoints, levels, responses, bins, descriptors and the uint64 views of
the float64 keypoints and points, NaN pattern included.  Only the end-to-end registration has bounds."""
import functools

import numpy as np
import pytest

import feat_pyramid_reference as ref
import feat_reference
import stereo_reference
from cslam_amd.front_end import visual_features as vf
from cslam_amd.front_end import visual_pyramid as vp
from cslam_amd.front_end import visual_registration as vr
from cslam_amd.front_end import visual_stereo as vs

pytestmark = pytest.mark.gpu

ROW_KEYS = ("keypoints", "level_keypoints", "levels", "responses", "bins", "descriptors", "points")
RUN, GROUP = vp.LEVEL_RUN, vp.LEVEL_RUN * vp.LEVEL_BLOCK  # bytes per thread and per workgroup of the level kernel


def same_floats(a, b):
    """The same bits, any NaN counting as NaN."""
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def same_rows(a, b, keys=ROW_KEYS):
    for key in keys:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        if a[key].dtype == np.float64:
            same_floats(a[key], b[key])
        else:
            assert np.array_equal(a[key], b[key]), key


def admitted(shape):
    """The largest number of levels whose top level is still 2 x 2."""
    return max(L for L in range(1, 9) if min(ref.level_sizes(shape, L)[-1]) >= 2)


def smallest_side(levels, border=19):
    n = 2 * border + 1
    while ref.level_size(n, levels - 1) < 2 * border + 1:
        n += 1
    return n


def content(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "block":
        return feat_reference.block_texture(H, W, seed, block=5)
    if kind == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy + xx) % 2) * 255).astype(np.uint8)       # a checkerboard of single pixels: every blend is between 0 and 255


# ---- level images --------------------------------------------------------------------------------------------------
LEVEL_SHAPES = [(2, 2), (3, 7), (16, 16), (17, 15), (39, 39), (40, 49),
                (5, RUN - 1), (5, RUN), (5, RUN + 1), (3, GROUP - 1), (3, GROUP), (3, GROUP + 1), (2, 2 * GROUP + RUN + 1)]


@pytest.mark.parametrize("kind", ["block", "noise", "checkerboard"])
def test_level_images_equal_the_restatement(kind):
    """All levels each size admits: images of one level count go through as one ragged batch."""
    images = [content(kind, H, W, seed=k) for k, (H, W) in enumerate(LEVEL_SHAPES)]
    counts = sorted({admitted(g.shape) for g in images})
    assert counts[0] == 2 and counts[-1] == 8
    for L in counts:
        batch = [g for g in images if admitted(g.shape) == L]
        got = vp.build_pyramid(batch, L)
        for g, levels in zip(batch, got):
            want = ref.pyramid(g, L)
            assert len(levels) == L and np.array_equal(levels[0], g)
            for l in range(L):
                assert levels[l].dtype == np.uint8 and levels[l].shape == want[l].shape, (g.shape, l)
                assert np.array_equal(levels[l], want[l]), (g.shape, l)
    # fewer levels than a size admits are the first of them
    g = images[5]
    assert all(np.array_equal(a, b) for a, b in zip(vp.build_pyramid([g], 3)[0], ref.pyramid(g, 8)[:3]))


def test_validity_maps_with_stripes_of_invalid_depth():
    shapes = [(40, 49), (17, 15), (3, 7), (39, GROUP // 8 + 1)]
    rng = np.random.default_rng(3)
    grays, depths = [], []
    for H, W in shapes:
        d = (0.5 + rng.random((H, W))).astype(np.float32)
        for k, bad in enumerate((0.0, -1.5, np.nan, np.inf, -np.inf)):
            d[:, (2 + 3 * k) % W] = bad                    # columns
        d[H // 2, :] = 0.0                                 # and a row
        grays.append(content("noise", H, W, seed=H))
        depths.append(d)
    for L in (1, 4):
        got = vp.build_pyramid(grays, L, depths=depths)
        for g, d, (levels, maps) in zip(grays, depths, got):
            want_g, want_m = ref.pyramid(g, L), ref.valid_maps(d, L)
            for l in range(L):
                assert np.array_equal(levels[l], want_g[l])
                assert maps[l].dtype == np.uint8 and np.array_equal(maps[l], want_m[l]), (g.shape, l)
            assert np.array_equal(maps[0], feat_reference.depth_valid(d).astype(np.uint8))
            assert 0 < maps[L - 1].sum() < maps[L - 1].size
    same = vp.build_pyramid(grays, 4)
    assert all(np.array_equal(a, b) for (lv, _), alone in zip(got, same) for a, b in zip(lv, alone))


# ---- one level is the single-scale chain ---------------------------------------------------------------------------
def mixed_batch(seed, shapes):
    rng = np.random.default_rng(seed)
    images, depths = [], []
    for k, (H, W) in enumerate(shapes):
        g = feat_reference.block_texture(H, W, seed=seed + k, block=6 + k % 3)
        images.append(np.stack([g, np.roll(g, 3, axis=1), g[::-1]], axis=2).copy() if k % 2 else g)
        d = (1.0 + rng.random((H, W))).astype(np.float32)
        d[:, W // 2:W // 2 + 9] = 0.0                      # a stripe without depth
        depths.append(d if k % 3 else np.round(d * 1000).astype(np.uint16))
    cams = np.array([[100.0 + k, 101.0, W / 2 + 0.25, H / 2 - 0.5] for k, (H, W) in enumerate(shapes)])
    return images, depths, cams


def test_one_level_equals_the_single_scale_chain_byte_for_byte():
    images, depths, cams = mixed_batch(1, [(64, 80), (41, 97), (120, 63)])
    for mask in (True, False):
        got = vp.extract_features_pyramid(images, depths, cams, levels=1, max_features=40, depth_as_mask=mask)
        one = vf.extract_features(images, depths, cams, max_features=40, depth_as_mask=mask)
        for a, b in zip(got, one):
            assert a["keypoints"].dtype == np.float64 and np.array_equal(a["keypoints"], b["keypoints"].astype(np.float64))
            assert np.array_equal(a["level_keypoints"], b["keypoints"]) and not a["levels"].any() and a["levels"].dtype == np.int32
            for key in ("responses", "bins", "descriptors"):
                assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
            same_floats(a["points"], b["points"])
            assert len(a["keypoints"]) > 0


# ---- the whole chain -----------------------------------------------------------------------------------------------
def chain_case(name):
    """(image, depth, camera, keyword arguments)."""
    if name.startswith("smallest"):
        L = int(name[-1])
        n = smallest_side(L)
        H, W = n, n + 5
        g, kw = feat_reference.block_texture(H, W, seed=L, block=6), dict(levels=L)
    elif name == "larger":
        H, W = 120, 160
        g, kw = feat_reference.block_texture(H, W, seed=3, block=8), dict(levels=4)
    elif name == "truncated":                              # budgets 5, 3, 2, 2: every level has more to give
        H, W = 120, 160
        g, kw = feat_reference.block_texture(H, W, seed=3, block=8), dict(levels=4, max_features=12)
    else:                                                  # "half": the upper half constant; "most": the upper 5/8
        H, W = 76, 100
        g, kw = feat_reference.block_texture(H, W, seed=5, block=7).copy(), dict(levels=4)
        g[:H // 2 if name == "half" else 5 * H // 8] = 90
    rng = np.random.default_rng(H)
    d = (1.0 + rng.random((H, W))).astype(np.float32)
    d[:, W // 3:W // 3 + (1 if name.startswith("smallest") else 12)] = np.nan           # a band without depth
    bgr = np.stack([g, g, g], axis=2)                      # grey of equal channels is the channel
    return (bgr if name == "larger" else g), d, (100.5, 101.0, W / 2 + 0.25, H / 2 - 0.5), kw


@functools.lru_cache(maxsize=None)
def chain_want(name, mask=True):
    image, d, cam, kw = chain_case(name)
    return ref.extract(image, d, cam, depth_as_mask=mask, **kw)


@pytest.mark.parametrize("name", ["smallest2", "smallest4", "smallest8", "larger", "truncated", "half", "most"])
def test_the_chain_equals_the_restatement(name):
    image, d, cam, kw = chain_case(name)
    got = vp.extract_features_pyramid([image], [d], cam, **kw)[0]
    want = chain_want(name)
    same_rows(got, want)
    L = kw["levels"]
    per_level = np.bincount(got["levels"], minlength=L)
    print(name, image.shape[:2], "rows per level", per_level.tolist())
    assert np.all(np.diff(got["levels"]) >= 0) and len(got["keypoints"]) > 0
    assert not np.isnan(got["points"]).any()               # the maps keep keypoints over invalid depth out
    assert np.all(np.abs(got["keypoints"][got["levels"] == 0] - got["level_keypoints"][got["levels"] == 0]) == 0)
    if name.startswith("smallest"):                        # the top level is 39 high: its only candidates lie on the middle row
        top = ref.level_sizes(image.shape, L)[-1]
        assert top[0] == 39 and min(ref.level_sizes((image.shape[0] - 1, image.shape[1]), L)[-1]) < 39
        assert np.all(got["level_keypoints"][got["levels"] == L - 1][:, 1] == 19)
    if name == "truncated":
        assert per_level.tolist() == ref.budgets(12, 4) == [5, 3, 2, 2]
        full = chain_want("larger")
        for l in range(4):                                 # a level's rows are the first of its rows at a larger budget
            a, b = got["level_keypoints"][got["levels"] == l], full["level_keypoints"][full["levels"] == l]
            assert np.array_equal(a, b[:len(a)]) and len(b) > len(a)
    if name in ("smallest4", "most"):
        assert (per_level == 0).any() and per_level[0] > 0  # a level without rows leaves no gap and shifts nothing
    if name == "larger":                                   # without the mask a keypoint may lie over invalid depth: a NaN row
        free = vp.extract_features_pyramid([image], [d], cam, depth_as_mask=False, **kw)[0]
        same_rows(free, chain_want(name, False))
        assert np.isnan(free["points"]).any()


# ---- batches -------------------------------------------------------------------------------------------------------
def test_a_ragged_batch_equals_one_by_one_and_the_reversed_batch():
    first = mixed_batch(1, [(70, 90), (67, 97), (120, 72), (75, 75)])
    second = mixed_batch(2, [(90, 68), (68, 160)])         # other sizes right after: the scratch is carved afresh
    for images, depths, cams in (first, second):
        got = vp.extract_features_pyramid(images, depths, cams, levels=4, max_features=60)
        back = vp.extract_features_pyramid(images[::-1], depths[::-1], cams[::-1], levels=4, max_features=60)[::-1]
        for k, (img, d) in enumerate(zip(images, depths)):
            same_rows(got[k], vp.extract_features_pyramid([img], [d], cams[k], levels=4, max_features=60)[0])
            same_rows(got[k], back[k])
            same_rows(got[k], ref.extract(img, vf.depth_metres(d), cams[k], levels=4, max_features=60))
            assert 0 < len(got[k]["keypoints"]) <= 60 and got[k]["levels"].max() >= 1
    kfs = vp.extract_keyframes_pyramid(*first, levels=4, max_features=60)
    for kf, f in zip(kfs, vp.extract_features_pyramid(*first, levels=4, max_features=60)):
        assert isinstance(kf, vr.Keyframe) and kf.keypoints.dtype == np.float64 and kf.points.dtype == np.float64
        assert np.array_equal(kf.keypoints, f["keypoints"]) and np.array_equal(kf.descriptors, f["descriptors"])
        same_floats(kf.points, f["points"])


def test_the_staged_calls_equal_the_chain():
    """build_pyramid with the maps, the single-scale staged calls on every level image, the Z under each keypoint, the merge."""
    images, depths, cams = mixed_batch(4, [(70, 90), (96, 68)])
    L, mf = 3, 30
    chain = vp.extract_features_pyramid(images, depths, cams, levels=L, max_features=mf)
    grays = vf.to_gray_batch(images)
    metres = [vf.depth_metres(d) for d in depths]
    pyramids = vp.build_pyramid(grays, L, depths=metres)
    budgets = vp.level_budgets(mf, L)
    feats = []
    for g, d, (levels, maps) in zip(grays, metres, pyramids):
        H, W = g.shape
        responses = [r for r, _ in vf.corner_response_batch(levels)]
        frame = []
        for l in range(L):
            kp, resp = vf.select_keypoints(responses[l], valid=maps[l], max_features=budgets[l])
            bins, desc = vf.describe(levels[l], kp)
            px, py = ref.base_pixel(kp[:, 0], W, levels[l].shape[1]), ref.base_pixel(kp[:, 1], H, levels[l].shape[0])
            frame.append(dict(keypoints=kp, responses=resp, bins=bins, descriptors=desc, z=d[py, px].astype(np.float64)))
        feats.append(frame)
    staged = vp.merge_levels([g.shape for g in grays], feats, cams, max_features=mf)
    for a, b in zip(staged, chain):
        same_rows(a, b)
        assert len(a["keypoints"]) > 0
    # the merge cuts a level at its budget and turns a Z that is no depth into a NaN row
    for f in feats[0]:
        f["z"] = f["z"].copy()
        f["z"][:1] = [0.0]
    cut = vp.merge_levels([grays[0].shape], [feats[0]], cams[0], max_features=6)[0]
    assert np.bincount(cut["levels"], minlength=L).tolist() == vp.level_budgets(6, L)
    assert np.isnan(cut["points"][cut["levels"] == 0][0]).all() and not np.isnan(cut["points"][1]).any()


# ---- stereo --------------------------------------------------------------------------------------------------------
STEREO_KEYS = ROW_KEYS + ("disparity", "status")


def planted_stereo():
    """The scene of test_stereo_gpu.py's end-to-end test: one block texture, true disparity 10."""
    tex = feat_reference.block_texture(120, 200, seed=7)
    cut = lambda a: np.ascontiguousarray(tex[:, a:a + 160])
    return [cut(0), cut(16)], [cut(10), cut(26)], (100.0, 100.0, 80.0, 60.0, 0.2)


def test_stereo_with_one_level_equals_the_single_scale_stereo_chain():
    lefts, rights, cam = planted_stereo()
    bgr = np.stack([lefts[1], lefts[1], lefts[1]], axis=2)
    got = vp.extract_features_stereo_pyramid([lefts[0], bgr], rights, cam, levels=1, max_features=80)
    one = vs.extract_features_stereo([lefts[0], bgr], rights, cam, max_features=80)
    for a, b in zip(got, one):
        assert np.array_equal(a["keypoints"], b["keypoints"].astype(np.float64)) and not a["levels"].any()
        for key in ("responses", "bins", "descriptors", "status"):
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
        same_floats(a["points"], b["points"])
        same_floats(a["disparity"], b["disparity"])
    kfs, kfs_one = vp.extract_keyframes_stereo_pyramid(lefts, rights, cam, levels=1), vs.extract_keyframes_stereo(lefts, rights, cam)
    for a, b in zip(kfs, kfs_one):
        assert np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.descriptors, b.descriptors)
        same_floats(a.points, b.points)


def test_stereo_with_three_levels_equals_the_restatement():
    lefts, rights, cam = planted_stereo()
    got = vp.extract_features_stereo_pyramid(lefts, rights, cam, levels=3, max_features=150)
    for g, left, right in zip(got, lefts, rights):
        want = ref.extract_stereo(left, right, cam, levels=3, max_features=150)
        same_rows(g, want, STEREO_KEYS)
        ok = g["status"] == 0
        assert np.array_equal(np.isnan(g["points"]).all(axis=1), ~ok) and ok.sum() > 20 and g["levels"].max() == 2
        # Z is the stereo rule's at the pixel under the keypoint; X and Y are the keypoint's own
        base = np.stack([ref.base_pixel(g["level_keypoints"][:, 0], 160, np.array([160, 133, 111])[g["levels"]]),
                         ref.base_pixel(g["level_keypoints"][:, 1], 120, np.array([120, 100, 83])[g["levels"]])], axis=1)
        m = stereo_reference.match(left, right, base, cam)
        same_floats(g["points"][:, 2], m["points"][:, 2])
        assert np.abs(g["points"][ok, 2] - 2.0).max() < 0.15
    # a rejected keypoint keeps its NaN row: a right image that matches nowhere
    flat = vp.extract_features_stereo_pyramid(lefts[:1], [np.full_like(rights[0], 7)], cam, levels=3, max_features=150)[0]
    assert len(flat["keypoints"]) == len(got[0]["keypoints"]) and np.isnan(flat["points"]).all() and np.all(flat["status"] != 0)


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_keyframes_from_two_distances_register_with_the_pyramid_only():
    """The plane of random cells seen from 2.88 m (view A, blocks of 10 pixels) and from 2.0 m (view B, 14.4 pixels), 144 x 192,
    registered from B to A.  One scale: 173 and 74 keypoints, 5 matches, the registration fails.  4 levels: 397 and 244
    keypoints, 91 usable matches, 86 inliers, translation 0.0257 m from the plant (bound 2 * 1.2^3 * Z_B / fx = 0.0346 m),
    rotation 0.0124 rad (bound 2 * 1.2^3 / 96 = 0.036 rad).  Measured on the MI355X; the restatement's keyframes and its own
    PnP RANSAC (tests/test_feat_pyramid_cpu.py) give the same figures, and the GPU keyframes equal the restatement's bit for bit."""
    A, B, dA, dB = ref.scene()
    cam = ref.SCENE_CAMERA
    one_a, one_b = vf.extract_keyframes([A, B], [dA, dB], cam)
    one = vr.register_pairs([(one_b, one_a)], cam)[0]
    print("one scale: %d and %d keypoints, %d matches, status %d" % (len(one_a.keypoints), len(one_b.keypoints), len(one.matches), one.status))
    assert not one.success and one.status != 0
    kf_a, kf_b = vp.extract_keyframes_pyramid([A, B], [dA, dB], cam, levels=4)
    ref_kfs = [vr.Keyframe(w["keypoints"], w["points"], w["descriptors"]) for w in ref.scene_features(4)]
    for kf, w in zip((kf_a, kf_b), ref_kfs):
        assert kf.keypoints.dtype == np.float64 and np.array_equal(kf.descriptors, w.descriptors)
        same_floats(kf.keypoints, w.keypoints)
        same_floats(kf.points, w.points)
    reg = vr.register_pairs([(kf_b, kf_a)], cam)[0]
    reg_ref = vr.register_pairs([(ref_kfs[1], ref_kfs[0])], cam)[0]
    n_in = int(np.count_nonzero(reg.inliers))
    t_err = np.abs(reg.transformation[:3, 3] - ref.scene_transform()[:3, 3]).max()
    Rm = reg.transformation[:3, :3]
    angle = float(np.arccos(np.clip((np.trace(Rm) - 1.0) / 2.0, -1.0, 1.0)))
    t_bound, r_bound = ref.scene_bounds()
    print("4 levels: %d and %d keypoints, %d matches, %d inliers, translation error %.3g m (bound %.3g), rotation %.3g rad (bound %.3g)"
          % (len(kf_a.keypoints), len(kf_b.keypoints), len(reg.matches), n_in, t_err, t_bound, angle, r_bound))
    assert reg.status == 0 and reg.success and n_in >= 20
    assert np.array_equal(reg.transformation, reg_ref.transformation) and np.array_equal(reg.inliers, reg_ref.inliers)
    assert np.array_equal(reg.matches, reg_ref.matches)
    assert t_err <= t_bound and angle <= r_bound
