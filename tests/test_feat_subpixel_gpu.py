"""GPU: the sub-pixel keypoints (feat_pyr_subpix_kernel, the sub-pixel form of feat_pyr_merge_kernel and the *_subpix chains of
csrc/feat.hip through cslam_amd.front_end.visual_pyramid) against their numpy restatement (tests/feat_subpixel_reference.py).
Everything is compared bit for bit: the offsets, the uint64 views of the refined keypoints and points, and every output the
refinement must leave alone against the chain without it."""
import numpy as np
import pytest

import feat_pyramid_reference as pyr_ref
import feat_reference
import feat_subpixel_reference as ref
from cslam_amd.front_end import visual_features as vf
from cslam_amd.front_end import visual_pyramid as vp
from test_feat_pyramid_gpu import ROW_KEYS, STEREO_KEYS, chain_case, content, mixed_batch, planted_stereo, same_floats, same_rows

pytestmark = pytest.mark.gpu

SUB_KEYS = ROW_KEYS + ("offsets",)
KEPT_KEYS = ("level_keypoints", "levels", "responses", "bins", "descriptors")      # what the refinement must not touch
SHAPES = [(2, 2), (3, 7), (16, 16), (17, 15), (40, 49)]   # around the 16-pixel tile of the response kernel
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def same_bits(a, b):
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def every_pixel(shape):
    H, W = shape
    return np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)


def check_offsets(maps, kps):
    got = vp.subpixel_offsets(maps, kps)
    assert len(got) == len(maps)
    for R, kp, g in zip(maps, kps, got):
        same_bits(g, ref.offsets(R, kp))
        assert np.abs(g).max(initial=0.0) <= 0.5
    return got


# ---- the staged call -----------------------------------------------------------------------------------------------
def test_staged_offsets_of_every_pixel_of_response_maps_equal_the_restatement():
    """Block, noise and checkerboard images of the five shapes as one ragged batch of 15 response maps; the keypoints are all
    pixels of each map, so every edge and corner, where a neighbour is missing, is among them."""
    maps = [feat_reference.response(content(kind, H, W, seed=H + W))[0].astype(np.int32)
            for kind in ("block", "noise", "checkerboard") for H, W in SHAPES]
    kps = [every_pixel(R.shape) for R in maps]
    got = check_offsets(maps, kps)
    moved = sum(int(np.count_nonzero(g)) for g in got)
    print("%d maps, %d keypoints, %d offsets that are not zero" % (len(maps), sum(map(len, kps)), moved))
    assert moved > 1000
    for R, kp, g in zip(maps, kps, got):                   # no offset along an axis whose neighbour is missing
        H, W = R.shape
        assert not g[(kp[:, 0] == 0) | (kp[:, 0] == W - 1), 0].any() and not g[(kp[:, 1] == 0) | (kp[:, 1] == H - 1), 1].any()


def test_staged_offsets_on_constructed_maps_with_extremes_and_plateaus():
    rng = np.random.default_rng(11)
    extremes = rng.choice(np.array([I32_MIN, -1, 0, 1, 7, I32_MAX], dtype=np.int64), (17, 15)).astype(np.int32)
    plateau = np.full((16, 16), 1000, dtype=np.int32)      # flat: den = 0 everywhere
    ridge = np.tile(np.array([1, 5, 5, 1, 9, 9, 9, 2], dtype=np.int32), (7, 2))      # one-sided plateaus along x, flat along y
    peak = np.zeros((3, 7), dtype=np.int32)
    peak[1, 3], peak[1, 2], peak[1, 4], peak[0, 3], peak[2, 3] = 90, 30, 60, 89, 10
    low = np.full((5, 5), I32_MAX, dtype=np.int32)
    low[2, 2] = I32_MIN                                    # a minimum: den = 2^33 - 2 >= 0
    top = np.full((5, 5), I32_MIN, dtype=np.int32)
    top[2, 2] = I32_MAX                                    # den = -(2^33 - 2), num = 0
    top[2, 3] = I32_MAX                                    # and a one-sided plateau of extremes: +-0.5
    maps = [extremes, plateau, ridge, peak, low, top]
    got = check_offsets(maps, [every_pixel(R.shape) for R in maps])
    at = lambda k, x, y: got[k][y * maps[k].shape[1] + x]
    assert not got[1].any() and not at(4, 2, 2).any() and at(4, 1, 2)[0] == -0.5 and at(4, 3, 2)[0] == 0.5
    assert at(2, 1, 3)[0] == 0.5 and at(2, 2, 3)[0] == -0.5 and at(2, 5, 3)[0] == 0.0 and not got[2][:, 1].any()
    assert at(3, 3, 1)[0] == np.float64(30 - 60) / np.float64(2 * (30 - 180 + 60)) and at(3, 3, 1)[1] == np.float64(89 - 10) / np.float64(2 * (89 - 180 + 10))
    assert at(5, 2, 2)[0] == 0.5 and at(5, 3, 2)[0] == -0.5 and at(5, 2, 2)[1] == 0.0
    assert len(np.unique(got[0])) > 10 and np.abs(got[0]).max() == 0.5


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_staged_offsets_around_the_workgroup_size(count):
    R = feat_reference.response(content("noise", 40, 49, seed=3))[0].astype(np.int32)
    kp = every_pixel(R.shape)[np.random.default_rng(count).permutation(R.size)[:count]]
    check_offsets([R], [kp])


def test_a_ragged_batch_of_maps_equals_one_by_one_and_the_reversed_batch():
    rng = np.random.default_rng(2)
    maps = [feat_reference.response(content("noise" if k % 2 else "block", H, W, seed=k))[0].astype(np.int32)
            for k, (H, W) in enumerate(SHAPES + [(49, 40), (2, 300)])]
    kps = [every_pixel(R.shape)[rng.permutation(R.size)[:n]] for R, n in zip(maps, (4, 0, 256, 255, 700, 1, 257))]
    batch = check_offsets(maps, kps)
    back = vp.subpixel_offsets(maps[::-1], kps[::-1])[::-1]
    for R, kp, g, b in zip(maps, kps, batch, back):
        same_bits(g, vp.subpixel_offsets([R], [kp])[0])
        same_bits(g, b)
    assert vp.subpixel_offsets([], []) == []


# ---- the chains ----------------------------------------------------------------------------------------------------
def sub_case(name):
    """chain_case of test_feat_pyramid_gpu, and "smallest1": the smallest frame of one level, 39 high, whose only candidates
    lie on the middle row (seed and block chosen so that there is one)."""
    if name != "smallest1":
        return chain_case(name)
    H, W = 39, 44
    d = (1.0 + np.random.default_rng(H).random((H, W))).astype(np.float32)
    return feat_reference.block_texture(H, W, seed=5, block=4), d, (100.5, 101.0, W / 2 + 0.25, H / 2 - 0.5), dict(levels=1)


def sub_want(name, mask=True):
    image, d, cam, kw = sub_case(name)
    return ref.extract(image, d, cam, depth_as_mask=mask, **kw)


@pytest.mark.parametrize("name", ["smallest1", "smallest2", "smallest4", "truncated"])
def test_the_sub_pixel_chain_equals_the_restatement_and_keeps_the_integer_outputs(name):
    """The smallest legal frames of 1, 2 and 4 levels and budgets that truncate every level (5, 3, 2, 2)."""
    image, d, cam, kw = sub_case(name)
    got = vp.extract_features_pyramid([image], [d], cam, subpixel=True, **kw)[0]
    same_rows(got, sub_want(name), SUB_KEYS)
    plain = vp.extract_features_pyramid([image], [d], cam, subpixel=False, **kw)[0]
    assert "offsets" not in plain and len(got["keypoints"]) > 0
    # the flag path without the flag gives the bytes of the pyramid's restatement
    same_rows(plain, pyr_ref.extract(image, d, cam, **kw))
    for key in KEPT_KEYS:
        assert got[key].dtype == plain[key].dtype and got[key].tobytes() == plain[key].tobytes(), key
    assert got["points"][:, 2].tobytes() == plain["points"][:, 2].tobytes()
    moved = got["offsets"].any(axis=1)
    print(name, image.shape[:2], "%d rows, %d moved" % (len(moved), moved.sum()))
    assert moved.any() and got["keypoints"][~moved].tobytes() == plain["keypoints"][~moved].tobytes()
    scale = 1.2 ** got["levels"][:, None]
    assert np.all(np.abs(got["keypoints"] - plain["keypoints"]) <= 0.5 * scale * 1.01)
    if name == "truncated":
        assert np.bincount(got["levels"], minlength=4).tolist() == [5, 3, 2, 2]
    if name == "smallest1":                                # one level: the single-scale chain with sub-pixel keypoints
        one = vf.extract_features([image], [d], cam)[0]
        assert np.array_equal(got["level_keypoints"], one["keypoints"]) and np.array_equal(got["descriptors"], one["descriptors"])
        moved_to = one["keypoints"].astype(np.float64) + got["offsets"]     # n_l = n_0: the rule is x + off up to its three roundings
        assert np.all(np.abs(got["keypoints"] - moved_to) <= 4 * np.finfo(np.float64).eps * (moved_to + 1.0))


def test_the_sub_pixel_chain_without_the_mask_keeps_nan_rows():
    image, d, cam, kw = sub_case("larger")
    got = vp.extract_features_pyramid([image], [d], cam, depth_as_mask=False, subpixel=True, **kw)[0]
    same_rows(got, sub_want("larger", False), SUB_KEYS)
    assert np.isnan(got["points"]).any() and not np.isnan(got["keypoints"]).any()


def test_a_ragged_sub_pixel_batch_equals_one_by_one_and_the_reversed_batch():
    images, depths, cams = mixed_batch(1, [(70, 90), (67, 97), (120, 72)])
    got = vp.extract_features_pyramid(images, depths, cams, levels=4, max_features=60, subpixel=True)
    back = vp.extract_features_pyramid(images[::-1], depths[::-1], cams[::-1], levels=4, max_features=60, subpixel=True)[::-1]
    for k, (img, d) in enumerate(zip(images, depths)):
        same_rows(got[k], vp.extract_features_pyramid([img], [d], cams[k], levels=4, max_features=60, subpixel=True)[0], SUB_KEYS)
        same_rows(got[k], back[k], SUB_KEYS)
        same_rows(got[k], ref.extract(img, vf.depth_metres(d), cams[k], levels=4, max_features=60), SUB_KEYS)
    kfs = vp.extract_level_keyframes(images, depths, cams, levels=4, max_features=60)
    for kf, f in zip(kfs, got):
        assert kf.levels.dtype == np.uint8 and np.array_equal(kf.levels, f["levels"]) and np.array_equal(kf.descriptors, f["descriptors"])
        same_floats(kf.keypoints, f["keypoints"])
        same_floats(kf.points, f["points"])
    plain = vp.extract_level_keyframes(images, depths, cams, levels=4, subpixel=False, max_features=60)
    for kf, f in zip(plain, vp.extract_features_pyramid(images, depths, cams, levels=4, max_features=60)):
        same_floats(kf.keypoints, f["keypoints"])


def test_the_sub_pixel_chain_equals_the_staged_calls():
    """The level images, their response maps and the staged offsets at the chain's own level keypoints; then the coordinate
    rule of the restatement on them."""
    images, depths, cams = mixed_batch(4, [(70, 90), (96, 68)])
    L = 3
    chain = vp.extract_features_pyramid(images, depths, cams, levels=L, max_features=30, subpixel=True)
    grays = vf.to_gray_batch(images)
    for g, f in zip(grays, chain):
        levels = vp.build_pyramid([g], L)[0]
        responses = [r for r, _ in vf.corner_response_batch(levels)]
        kps = [f["level_keypoints"][f["levels"] == l] for l in range(L)]
        staged = np.concatenate(vp.subpixel_offsets(responses, kps))
        same_bits(f["offsets"], staged)
        sizes = pyr_ref.level_sizes(g.shape, L)
        Wl, Hl = np.array([s[1] for s in sizes])[f["levels"]], np.array([s[0] for s in sizes])[f["levels"]]
        kx = np.array([ref.coord(x, o, g.shape[1], w) for x, o, w in zip(f["level_keypoints"][:, 0], staged[:, 0], Wl)])
        ky = np.array([ref.coord(y, o, g.shape[0], h) for y, o, h in zip(f["level_keypoints"][:, 1], staged[:, 1], Hl)])
        same_bits(f["keypoints"], np.stack([kx, ky], axis=1))
        assert len(staged) > 0 and staged.any()


# ---- stereo --------------------------------------------------------------------------------------------------------
def test_sub_pixel_stereo_with_three_levels_equals_the_restatement():
    lefts, rights, cam = planted_stereo()
    got = vp.extract_features_stereo_pyramid(lefts, rights, cam, levels=3, max_features=150, subpixel=True)
    plain = vp.extract_features_stereo_pyramid(lefts, rights, cam, levels=3, max_features=150)
    for g, p, left, right in zip(got, plain, lefts, rights):
        same_rows(g, ref.extract_stereo(left, right, cam, levels=3, max_features=150), STEREO_KEYS + ("offsets",))
        # the stereo rule ran at the same integer pixels: disparity, status and Z are the plain chain's
        for key in KEPT_KEYS + ("status",):
            assert g[key].tobytes() == p[key].tobytes(), key
        same_floats(g["disparity"], p["disparity"])
        same_floats(g["points"][:, 2], p["points"][:, 2])
        assert (g["status"] == 0).sum() > 20 and g["levels"].max() == 2 and g["offsets"].any()
    kfs = vp.extract_level_keyframes_stereo(lefts, rights, cam, levels=3, max_features=150)
    for kf, g in zip(kfs, got):
        same_floats(kf.keypoints, g["keypoints"])
        same_floats(kf.points, g["points"])
        assert np.array_equal(kf.levels, g["levels"]) and kf.levels.dtype == np.uint8
