"""GPU: the kernels of csrc/rectify.hip through cslam_amd.front_end.rectify against the numpy restatement
(tests/rectify_reference.py).  Everything is compared bit for bit: maps, images, validity, depth (NaN payloads included),
keyframes and registrations.  Only the end-to-end registration has bounds, those of the stereo end-to-end test."""
import functools

import numpy as np
import pytest

import feat_reference
import rectify_reference as ref
import stereo_reference
from cslam_amd.front_end import rectify as rc
from cslam_amd.front_end import stereo_depth as sd
from cslam_amd.front_end import visual_features as vf
from cslam_amd.front_end import visual_registration as vr
from cslam_amd.front_end import visual_stereo as vs

pytestmark = pytest.mark.gpu


def raw_camera(values, H, W):
    return rc.RawCamera(values[:4], values[4:12], values[12:21], values[21:26], (H, W))


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


def same_floats(a, b):
    """The same bits, any NaN counting as NaN."""
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def same_keyframes(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g.keypoints, w.keypoints) and np.array_equal(g.descriptors, w.descriptors)
        same_floats(g.points, w.points)


# ---- maps ------------------------------------------------------------------------------------------------------------
def test_maps_equal_the_restatement_one_by_one_and_as_a_ragged_batch():
    cases = ref.map_cases()
    want = [ref.rect_map(cam, H, W) for _, cam, H, W in cases]
    cams = [raw_camera(cam, H, W) for _, cam, H, W in cases]
    batch = rc.rectify_maps(cams).numpy()
    for (name, _, _, _), c, w, b in zip(cases, cams, want, batch):
        assert np.array_equal(b, w), name
        assert np.array_equal(rc.rectify_maps([c]).numpy()[0], w), name
    for g, w in zip(rc.rectify_maps(cams[::-1]).numpy(), want[::-1]):
        same(g, w)
    assert sum(int((w[..., 0] == ref.NONE).sum()) for w in want) == 441 + 1 + 1 + 540 + 351      # behind, 0 / 0, 2 / 0, far x, far y


# ---- remap -----------------------------------------------------------------------------------------------------------
def check_images(sources, maps, index=None):
    m = rc.RectifyMaps.from_numpy(maps)
    got = rc.rectify_images(sources, m, index)
    idx = range(len(sources)) if index is None else index
    assert len(got) == len(sources)
    for (img, valid), s, k in zip(got, sources, idx):
        w_img, w_valid = ref.bilinear(s, maps[k])
        same(img, w_img)
        same(valid, w_valid)
    return got


def test_remap_every_rule_of_the_sampler():
    """Constructed maps: exact multiples of 32, fractions 0, 1, 16 and 31, coordinates -33 .. -1, taps one pixel outside on
    every side, sentinels, the remainders 511, 512 and 513, all-0 and all-255 sources, the widths around a thread's run, a
    wave's 64 runs and a workgroup's 256, 1 and 3 channels; the source and the destination never have the same size."""
    cases = ref.remap_cases()
    for name, src, q in cases:
        assert src.shape[:2] != q.shape[:2], name
    check_images([c[1] for c in cases], [c[2] for c in cases])                 # one call: a ragged batch of every case
    for name, src, q in cases[:14]:                                            # and the constructed ones alone
        check_images([src], [q])


def test_nearest_bits_ties_and_sizes():
    for dtype in (np.uint16, np.float32):
        cases = [c for c in ref.nearest_cases() if c[1].dtype == dtype]
        m = rc.RectifyMaps.from_numpy([c[2] for c in cases])
        for got, (name, src, q) in zip(rc.rectify_depths([c[1] for c in cases], m), cases):
            same(got, ref.nearest(src, q))
        name, src, q = cases[0]
        same(rc.rectify_depths([src], rc.RectifyMaps.from_numpy([q]))[0], ref.nearest(src, q))
    f32 = dict((n, s) for n, s, _ in ref.nearest_cases())["float32 grid"]
    line = np.array([[(32 * x, 0) for x in range(7)]] * 2, dtype=np.int32)
    got = rc.rectify_depths([f32], rc.RectifyMaps.from_numpy([line]))[0]
    assert got[0].view(np.uint32).tolist() == [0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001]


def test_batches_equal_one_by_one_and_reversed():
    sources, maps, index = ref.batch_case()
    got = check_images(sources, maps, index)
    m = rc.RectifyMaps.from_numpy(maps)
    for k, s in enumerate(sources):
        img, valid = rc.rectify_images([s], m, index[k:k + 1])[0]
        same(img, got[k][0])
        same(valid, got[k][1])
    back = rc.rectify_images(sources[::-1], rc.RectifyMaps.from_numpy(maps[::-1]), len(maps) - 1 - index[::-1])
    for (img, valid), (w_img, w_valid) in zip(back, got[::-1]):
        same(img, w_img)
        same(valid, w_valid)
    grey = [k for k, s in enumerate(sources) if s.ndim == 2]
    depth = [sources[k].astype(np.uint16) * 257 for k in grey]
    for d, k, g in zip(depth, grey, rc.rectify_depths(depth, m, index[grey])):
        same(g, ref.nearest(d, maps[index[k]]))


# ---- the identity camera -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stereo_scene():
    tex = feat_reference.block_texture(120, 200, seed=7)
    cut = lambda a: np.ascontiguousarray(tex[:, a:a + 160])
    return [cut(0), cut(16)], [cut(10), cut(26)]


def identity_pair():
    left = rc.RawCamera(ref.SCENE_P, [], np.identity(3), ref.SCENE_P, ref.SCENE_SIZE)
    right = rc.RawCamera(ref.SCENE_P, [], np.identity(3), ref.SCENE_P + (-ref.SCENE_BASELINE * ref.SCENE_P[0],), ref.SCENE_SIZE)
    return left, right


def test_identity_camera_returns_the_input_bytes():
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (120, 160), dtype=np.uint8), rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)]
    maps = rc.rectify_maps([identity_pair()[0]])
    for (out, valid), img in zip(rc.rectify_images(imgs, maps, [0, 0]), imgs):
        same(out, img)
        assert valid.all()
    depth = rng.standard_normal((120, 160)).astype(np.float32)
    same(rc.rectify_depths([depth], maps)[0], depth)


def test_identity_camera_chain_equals_the_rectified_entry_points():
    lefts, rights = stereo_scene()
    left, right = identity_pair()
    cam = rc.stereo_camera(left, right)
    assert cam == ref.SCENE_P + (ref.SCENE_BASELINE,)
    kfs, valid = rc.extract_keyframes_stereo_raw(lefts, rights, left, right)
    same_keyframes(kfs, vs.extract_keyframes_stereo(lefts, rights, cam))
    assert np.array_equal(valid, np.ones((2, 2)))
    clouds, valid = rc.keyframe_clouds_stereo_raw(lefts, rights, left, right, max_disparity=32)
    for g, w in zip(clouds, sd.keyframe_clouds_stereo(lefts, rights, cam, max_disparity=32)):
        assert len(g.points) > 0
        same(g.points, w.points)
        same(g.colors, w.colors)


# ---- chains ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raw_scene():
    lefts, rights, lc, rcam = ref.scene()
    return lefts, rights, raw_camera(lc, *ref.SCENE_SIZE), raw_camera(rcam, *ref.SCENE_SIZE)


def test_stereo_chains_equal_the_staged_calls():
    lefts, rights, left, right = raw_scene()
    lefts = [lefts[0], np.stack([lefts[1], lefts[1][::-1], lefts[1]], axis=2)]          # a 3-channel left image in the batch
    maps = rc.rectify_maps([left, right])
    rl = rc.rectify_images(lefts, maps, [0, 0])
    rr = rc.rectify_images(rights, maps, [1, 1])
    cam = rc.stereo_camera(left, right)
    kfs, valid = rc.extract_keyframes_stereo_raw(lefts, rights, left, right)
    same_keyframes(kfs, vs.extract_keyframes_stereo([x for x, _ in rl], [x for x, _ in rr], cam))
    want_valid = np.array([[float(v.mean()) for _, v in side] for side in (rl, rr)]).T
    assert np.array_equal(valid, want_valid)
    kfs2, _ = rc.extract_keyframes_stereo_raw(lefts, rights, (maps, [0, 0]), (maps, [1, 1]))          # maps made before
    same_keyframes(kfs2, kfs)
    for voxel in (0.05, 0.0):
        clouds, valid = rc.keyframe_clouds_stereo_raw(lefts, rights, left, right, voxel_size=voxel, max_disparity=32)
        staged = sd.keyframe_clouds_stereo([x for x, _ in rl], [x for x, _ in rr], cam, voxel_size=voxel, max_disparity=32)
        for g, w in zip(clouds, staged):
            assert len(g.points) > 0
            same(g.points, w.points)
            same(g.colors, w.colors)
        assert np.array_equal(valid, want_valid)


def test_rgbd_chain_equals_the_staged_calls_and_masks_invalid_pixels():
    """A raw image smaller than the rectified one leaves a band of invalid pixels: their depth is 0 after the chain, so no
    keypoint lies there although the depth image itself has no hole."""
    lefts, _, left, _ = raw_scene()
    rng = np.random.default_rng(6)
    cut = [np.ascontiguousarray(x[:, :130]) for x in lefts]                                 # the raw camera saw 130 of 160 columns
    depths = [(1.5 + rng.random(cut[0].shape)).astype(np.float32),(1500 + rng.integers(0, 1000, cut[1].shape)).astype(np.uint16)]
    maps = rc.rectify_maps([left])
    q = maps.numpy()[0]
    kfs = rc.extract_keyframes_raw(cut, depths, left)
    staged_img = rc.rectify_images(cut, maps, [0, 0])
    staged_depth = rc.rectify_depths([vf.depth_metres(d) for d in depths], maps, [0, 0])
    masked = []
    for (img, valid), d, raw_d in zip(staged_img, staged_depth, depths):
        same(d, ref.nearest(vf.depth_metres(raw_d), q))
        assert 0.5 < valid.mean() < 0.9 and np.count_nonzero(d[valid == 0]) > 0             # invalid image pixels with a depth of their own
        masked.append(np.where(valid == 1, d, np.float32(0.0)))
    same_keyframes(kfs, vf.extract_keyframes([x for x, _ in staged_img], masked, left.projection))
    for kf, (_, valid) in zip(kfs, staged_img):
        k = kf.keypoints.astype(np.int64)
        assert len(k) > 20 and np.all(valid[k[:, 1], k[:, 0]] == 1)
    unmasked = vf.extract_keyframes([x for x, _ in staged_img], staged_depth, left.projection)
    assert any(np.any(v[kf.keypoints.astype(np.int64)[:, 1], kf.keypoints.astype(np.int64)[:, 0]] == 0) for kf, (_, v) in zip(unmasked, staged_img))


# ---- end to end --------------------------------------------------------------------------------------------------------
def registration(kf_from, kf_to):
    reg = vr.register_pairs([(kf_from, kf_to)], ref.SCENE_P)[0]
    t_err = float(np.abs(reg.transformation[:3, 3] - ref.SCENE_PLANT).max())
    Rm = reg.transformation[:3, :3]
    return reg, t_err, float(np.arccos(np.clip((np.trace(Rm) - 1.0) / 2.0, -1.0, 1.0)))


def test_raw_stereo_frames_register_once_rectified_and_not_before():
    """The scene of test_stereo_keyframes_register_and_decide_the_next_keyframe behind raw cameras with K = (98, 99, 81.5,
    58.75), mild distortion and rotations of about 0.01 rad.  The restatement chain gave, and the MI355X equals it bit
    for bit: 110 and 115 keypoints, 110 and 114 accepted, largest |d - 10| 0.493, 77 matches, 76 inliers, translation
    0.0088 m from the plant (-0.32, 0, 0) (bound 0.04 m), rotation 0.0041 rad (bound 0.025 rad).  The same raw frames
    without rectification: 76 of 109 and 68 of 107 accepted, 39 inliers, 0.060 m, outside the bound."""
    lefts, rights, left, right = raw_scene()
    cam = rc.stereo_camera(left, right)
    (kf_from, kf_to), valid = rc.extract_keyframes_stereo_raw(lefts, rights, left, right)
    H, W = ref.SCENE_SIZE
    want = [stereo_reference.extract_stereo(ref.rectify(left.values, H, W, l)[0], ref.rectify(right.values, H, W, r)[0], cam)
            for l, r in zip(lefts, rights)]
    ref_kfs = [vr.Keyframe(w["keypoints"].astype(np.float64), w["points"], w["descriptors"]) for w in want]
    same_keyframes([kf_from, kf_to], ref_kfs)
    reg, t_err, angle = registration(kf_from, kf_to)
    reg_ref = vr.register_pairs([tuple(ref_kfs)], cam[:4])[0]
    counts = dict(keypoints=[len(w["keypoints"]) for w in want], accepted=[int((w["status"] == 0).sum()) for w in want], matches=len(reg.matches),
                  inliers=int(np.count_nonzero(reg.inliers)))
    d_err = max(float(np.nanmax(np.abs(w["disparity"] - 10.0))) for w in want)
    print("rectified: %s, valid %s, largest |d - 10| %.3f, translation error %.3g m, rotation %.3g rad" % (counts, valid.tolist(), d_err, t_err, angle))
    assert reg.status == 0 and reg.success
    assert np.array_equal(reg.transformation, reg_ref.transformation) and np.array_equal(reg.inliers, reg_ref.inliers)
    assert np.array_equal(reg.matches, reg_ref.matches)
    assert counts == ref.SCENE_RECTIFIED
    assert t_err <= 0.04 and angle <= 0.025
    # the same frames as the camera driver gives them: why the feature exists
    raw_from, raw_to = vs.extract_keyframes_stereo(lefts, rights, cam)
    reg_raw, t_raw, angle_raw = registration(raw_from, raw_to)
    print("raw: %d inliers, translation error %.3g m, rotation %.3g rad" % (int(np.count_nonzero(reg_raw.inliers)), t_raw, angle_raw))
    assert not t_raw <= 0.04
