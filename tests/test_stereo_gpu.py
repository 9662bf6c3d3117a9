"""GPU: the stereo rule (feat_stereo_kernel of csrc/feat.hip through cslam_amd.front_end.visual_stereo) against its numpy
restatement (tests/stereo_reference.py).  Everything is compared bit for bit: status, best, and the uint64 views of the
disparity and the points, NaN pattern included.  Only the end-to-end registration has bounds, those of the RGB-D test."""
import functools

import numpy as np
import pytest

import feat_reference
import stereo_reference as ref
from cslam_amd.front_end import visual_features as vf
from cslam_amd.front_end import visual_registration as vr
from cslam_amd.front_end import visual_stereo as vs

pytestmark = pytest.mark.gpu

CAM = (100.0, 101.0, 80.25, 23.5, 0.2)


def same_floats(a, b):
    """The same bits, any NaN counting as NaN."""
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def same_match(got, want):
    for key in ("status", "best"):
        assert got[key].dtype == want[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
    same_floats(got["disparity"], want["disparity"])
    same_floats(got["points"], want["points"])
    assert np.array_equal(np.isnan(got["disparity"]), got["status"] != 0)
    assert np.array_equal(np.isnan(got["points"]).all(axis=1), got["status"] != 0)


def check(L, R, kp, cam=CAM, **kw):
    got = vs.stereo_match(L, R, kp, cam, **kw)
    same_match(got, ref.match(L, R, kp, cam, **kw))
    return got


@functools.lru_cache(maxsize=None)
def pair(H, W, shift):
    L, R = ref.shifted_pair(H, W, shift)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def foreground():
    L, R = ref.foreground_pair()
    kp = np.array([[u, v] for v in range(1, 47, 3) for u in range(7, 193, 3)], dtype=np.int32)
    want = ref.match(L, R, kp, CAM, 1, 64)
    for a in (L, R, kp) + tuple(want.values()):
        a.setflags(write=False)
    return L, R, kp, want


# ---- range lengths around the wave ---------------------------------------------------------------------------------
RANGE_K = (0, 1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 130, 131, 255, 256, 257, 258)


@pytest.mark.parametrize("max_disparity", [128, 255])
def test_range_lengths_around_the_wave(max_disparity):
    """u = 7 + k leaves D_hi = min(max_disparity + 1, k): ranges of 3, 4, 63 .. 67, 128 .. 130 and, with 255, 256 and 257
    disparities, 1 to 5 per lane; k = 0, 1 leave nothing to search."""
    L, R = pair(9, 300, 5)
    kp = np.array([[7 + k, 4] for k in RANGE_K], dtype=np.int32)
    lengths = set()
    for dmin in (1, 5, 6, 7):
        got = check(L, R, kp, min_disparity=dmin, max_disparity=max_disparity)
        for k, st in zip(RANGE_K, got["status"]):
            lo, hi, ok = ref.search_range(7 + k, dmin, max_disparity)
            assert (st == 2) == (not ok)
            lengths.add(hi - lo + 1)
        if dmin <= 5:
            assert (got["status"] == 0).sum() >= 10 and np.all(got["best"][got["status"] == 0, 0] == 5)
    assert {3, 4, 64, 65, 128, 129, 130} <= lengths
    assert ({256, 257} <= lengths) == (max_disparity == 255)


# ---- the smallest image --------------------------------------------------------------------------------------------
def test_the_smallest_images():
    rng = np.random.default_rng(5)
    L, R = (rng.integers(0, 256, (3, 15), dtype=np.uint8) for _ in range(2))
    got = check(L, R, [[7, 1], [6, 1], [8, 1], [7, 0], [7, 2], [0, 0]])
    assert got["status"].tolist() == [2, 1, 1, 1, 1, 1] and np.all(got["best"] == -1)
    L, R = (rng.integers(0, 256, (3, 18), dtype=np.uint8) for _ in range(2))
    got = check(L, R, [[7, 1], [8, 1], [9, 1], [10, 1], [6, 1], [11, 1], [9, 0], [9, 2], [0, 0], [-1, 1], [9, -1], [18, 1], [9, 3]])
    assert got["status"][:2].tolist() == [2, 2] and np.all(got["status"][2:4] >= 3) and np.all(got["status"][4:] == 1)
    L, R = pair(9, 40, 2)
    H, W = L.shape
    kp = [[u, v] for v in (1, H - 2) for u in (7, 12, W - 8)] + [[7, 4], [W - 8, 4], [6, 4], [W - 7, 4], [12, 0], [12, H - 1], [0, 0]]
    got = check(L, R, kp, max_disparity=8)
    assert got["status"][-5:].tolist() == [1] * 5 and not (got["status"][:8] == 1).any() and (got["status"] == 0).sum() >= 4
    assert vs.stereo_match(L, R, np.zeros((0, 2), dtype=np.int32), CAM)["points"].shape == (0, 3)


# ---- each status ---------------------------------------------------------------------------------------------------
def test_each_status_on_the_planted_scenes():
    L, R = pair(48, 200, 5)
    at = lambda u: np.array([[u, 5]], dtype=np.int32)
    assert [int(check(L, R, at(100), min_disparity=1, max_disparity=m)["status"][0]) for m in (4, 5, 6)] == [3, 0, 0]
    assert [int(check(L, R, at(100), min_disparity=m, max_disparity=64)["status"][0]) for m in (5, 6, 7)] == [0, 3, 3]
    got = check(L, R, [[7, 5], [8, 5], [9, 5], [10, 5], [100, 5]], max_disparity=64)
    assert got["status"].tolist() == [2, 2, 3, 3, 0] and got["disparity"][4] == 5.0
    assert got["points"][4].tolist() == ref.triangulate(100, 5, 5.0, CAM).tolist()
    P0, P3 = ref.stripes(48, 200), ref.stripes(48, 200, 3)
    kp = np.array([[u, 10] for u in range(80, 120)], dtype=np.int32)
    assert np.all(check(P0, P3, kp, max_disparity=64)["status"] == 4)
    assert np.all(check(P0, P0, kp, max_disparity=64)["status"] == 3)
    Z = np.full((48, 200), 77, dtype=np.uint8)
    got = check(Z, Z, [[100, 10]], max_disparity=64)
    assert got["status"].tolist() == [3] and got["best"].tolist() == [[0, -1, 0, 0]]


def test_foreground_over_background_and_the_left_right_check():
    L, R, kp, want = foreground()
    got = vs.stereo_match(L, R, kp, CAM, 1, 64)
    same_match(got, want)
    assert (got["status"] == 0).sum() == 857 and (got["status"] == 5).sum() == 61
    free = check(L, R, kp, max_disparity=64, lr_tolerance=-1)
    changed = free["status"] != got["status"]
    assert np.array_equal(changed, got["status"] == 5) and np.all(free["status"][changed] == 0)
    assert np.array_equal(free["best"], got["best"])
    wide = check(L, R, kp, max_disparity=64, lr_tolerance=255)
    assert np.array_equal(wide["status"], free["status"])
    strict = check(L, R, kp, max_disparity=64, lr_tolerance=0)
    assert (strict["status"] == 5).sum() >= 61


@pytest.mark.parametrize("uniqueness", [0, 100])
def test_uniqueness_at_its_ends(uniqueness):
    L, R, kp, want = foreground()
    got = check(L, R, kp, max_disparity=64, uniqueness=uniqueness)
    n4, n4_default = int((got["status"] == 4).sum()), int((want["status"] == 4).sum())
    assert n4 <= n4_default if uniqueness == 0 else n4 >= n4_default
    P0, P3 = ref.stripes(48, 200), ref.stripes(48, 200, 3)                    # equal minima: not unique even at 0 percent
    assert np.all(check(P0, P3, [[u, 10] for u in range(80, 120)], max_disparity=64, uniqueness=uniqueness)["status"] == 4)


# ---- noise ---------------------------------------------------------------------------------------------------------
def test_binary_noise_gives_the_largest_costs_and_ties():
    rng = np.random.default_rng(11)
    L, R = ((rng.integers(0, 2, (12, 330)) * 255).astype(np.uint8) for _ in range(2))
    kp = np.array([[u, v] for v in (1, 5, 10) for u in range(7, 323, 5)], dtype=np.int32)
    got = check(L, R, kp, max_disparity=255, lr_tolerance=-1)
    check(L, R, kp, max_disparity=255, uniqueness=0)
    assert got["best"][:, 1:].max() > 30 * 255 * 255
    # black against white: every cost is the largest there is, so every disparity ties and the lowest wins
    got = check(np.zeros_like(L), np.full_like(L, 255), kp, max_disparity=255)
    searched = got["status"] != 2
    assert np.all(got["status"][searched] == 3) and np.all(got["best"][searched, 0] == 0)
    assert np.all(got["best"][searched, 2] == ref.COST_MAX)
    # a few columns of texture in a flat image: most windows tie at cost 0
    F = np.zeros((12, 330), dtype=np.uint8)
    F[:, 100:104] = 255
    G = np.zeros((12, 330), dtype=np.uint8)
    G[:, 60:64] = 255
    check(F, G, kp, max_disparity=255)
    check(F, G, kp, max_disparity=255, uniqueness=0, lr_tolerance=0)


# ---- sub-pixel -----------------------------------------------------------------------------------------------------
def test_sub_pixel_disparity_on_a_smooth_texture():
    """A smooth texture sampled at shifts 10.0, 10.25, 10.5, 10.75.  Equality with the restatement is the gate; the largest
    |disparity - shift| over the accepted keypoints is printed: 0.091, 0.065, 0.042 and 0.096 (restatement and MI355X)."""
    kp = np.array([[u, v] for v in range(2, 46, 5) for u in range(90, 192, 7)], dtype=np.int32)
    worst = []
    for shift in (10.0, 10.25, 10.5, 10.75):
        L, R = ref.smooth_pair(48, 200, shift)
        got = check(L, R, kp, max_disparity=64)
        ok = got["status"] == 0
        assert ok.sum() == 135
        worst.append(float(np.abs(got["disparity"][ok] - shift).max()))
    print("largest |disparity - shift| at 10.0, 10.25, 10.5, 10.75: %.3f %.3f %.3f %.3f" % tuple(worst))


# ---- batches -------------------------------------------------------------------------------------------------------
def stereo_batch(seed, shapes, empty=None):
    """Frames of their own sizes at disparity 3 + k, 1- and 3-channel sides mixed; frame `empty` is flat: no keypoints."""
    lefts, rights, cams = [], [], []
    for k, (H, W) in enumerate(shapes):
        tex = feat_reference.block_texture(H, W + 32, seed=seed + k, block=6 + k % 3)
        if k == empty:
            tex = np.full((H, W + 32), 90, dtype=np.uint8)
        gl, gr = np.ascontiguousarray(tex[:, :W]), np.ascontiguousarray(tex[:, 3 + k:3 + k + W])
        bgr = lambda g: np.stack([g, np.roll(g, 3, axis=1), g[::-1]], axis=2).copy()
        lefts.append(bgr(gl) if k % 2 else gl)
        rights.append(bgr(gr) if k % 3 == 0 else gr)
        cams.append([100.0 + k, 101.0, W / 2 + 0.25, H / 2 - 0.5, 0.1 + 0.01 * k])
    return lefts, rights, np.array(cams)


def same_features(a, b):
    for key in ("keypoints", "responses", "bins", "descriptors", "status"):
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    same_floats(a["points"], b["points"])
    same_floats(a["disparity"], b["disparity"])


def test_a_ragged_batch_equals_one_by_one_the_staged_calls_and_the_restatement():
    first = stereo_batch(1, [(64, 80), (41, 97), (120, 63), (50, 50), (77, 130)], empty=3)
    second = stereo_batch(2, [(90, 45), (48, 160), (66, 66)])           # other sizes right after: the scratch is carved afresh
    nan_rows = 0
    for lefts, rights, cams in (first, second):
        got = vs.extract_features_stereo(lefts, rights, cams, max_features=40, max_disparity=20)
        staged = []
        for k, (left, right) in enumerate(zip(lefts, rights)):
            same_features(got[k], vs.extract_features_stereo([left], [right], cams[k], max_features=40, max_disparity=20)[0])
            same_features(got[k], ref.extract_stereo(left, right, cams[k], max_features=40, max_disparity=20))
            assert len(got[k]["keypoints"]) <= 40
            gl, gr = vf.to_gray(left), vf.to_gray(right)
            R, _ = vf.corner_response(gl)
            kp, resp = vf.select_keypoints(R, max_features=40)
            bins, desc = vf.describe(gl, kp)
            m = vs.stereo_match(gl, gr, kp, cams[k], max_disparity=20)
            same_features(got[k], dict(keypoints=kp, responses=resp, bins=bins, descriptors=desc, points=m["points"],
                                       disparity=m["disparity"], status=m["status"]))
            staged.append((gl, gr, kp))
            nan_rows += int(np.isnan(got[k]["points"]).any(axis=1).sum())
        # the staged stereo call on the whole batch, the frame without keypoints included
        many = vs.stereo_match_batch([s[0] for s in staged], [s[1] for s in staged], [s[2] for s in staged], cams, max_disparity=20)
        for k, m in enumerate(many):
            same_floats(m["points"], got[k]["points"])
            assert np.array_equal(m["status"], got[k]["status"])
    assert len(first[0]) == 5 and len(vs.extract_features_stereo(*first, max_features=40)[3]["keypoints"]) == 0
    assert nan_rows >= 1                                   # without a mask some keypoints have no correspondence
    kfs = vs.extract_keyframes_stereo(*first, max_features=40, max_disparity=20)
    got = vs.extract_features_stereo(*first, max_features=40, max_disparity=20)
    for kf, f in zip(kfs, got):
        assert isinstance(kf, vr.Keyframe) and kf.keypoints.dtype == np.float64 and kf.points.dtype == np.float64
        assert np.array_equal(kf.keypoints, f["keypoints"]) and np.array_equal(kf.descriptors, f["descriptors"])
        same_floats(kf.points, f["points"])


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_stereo_keyframes_register_and_decide_the_next_keyframe():
    """Two stereo views of one block texture 16 columns apart, true disparity 10 = 2 m at fx 100 and a baseline of 0.2 m.
    The restatement chain gave, and the MI355X equals it bit for bit: 122 and 124 keypoints, all status 0, largest
    |d - 10| 0.495, largest |Z - 2| 0.104 m, 105 matches, 105 inliers, translation 0.0047 m from the plant (-0.32, 0, 0)
    (bound 0.04 m), rotation 0.0027 rad (bound 0.025 rad)."""
    tex = feat_reference.block_texture(120, 200, seed=7)
    cut = lambda a: np.ascontiguousarray(tex[:, a:a + 160])
    lefts, rights = [cut(0), cut(16)], [cut(10), cut(26)]
    cam = (100.0, 100.0, 80.0, 60.0, 0.2)
    kf_from, kf_to = vs.extract_keyframes_stereo(lefts, rights, cam)
    want = [ref.extract_stereo(l, r, cam) for l, r in zip(lefts, rights)]
    ref_kfs = [vr.Keyframe(w["keypoints"].astype(np.float64), w["points"], w["descriptors"]) for w in want]
    for kf, w in zip((kf_from, kf_to), ref_kfs):
        assert np.array_equal(kf.keypoints, w.keypoints) and np.array_equal(kf.descriptors, w.descriptors)
        same_floats(kf.points, w.points)
    assert all(np.all(w["status"] == 0) for w in want)
    d_err = max(float(np.abs(w["disparity"] - 10.0).max()) for w in want)
    z_err = max(float(np.abs(w["points"][:, 2] - 2.0).max()) for w in want)
    reg = vr.register_pairs([(kf_from, kf_to)], cam[:4])[0]
    reg_ref = vr.register_pairs([tuple(ref_kfs)], cam[:4])[0]
    n_in = int(np.count_nonzero(reg.inliers))
    t_err = np.abs(reg.transformation[:3, 3] - [-16 * 2.0 / 100.0, 0.0, 0.0]).max()
    Rm = reg.transformation[:3, :3]
    angle = float(np.arccos(np.clip((np.trace(Rm) - 1.0) / 2.0, -1.0, 1.0)))
    print("keypoints %d and %d, largest |d - 10| %.3f, largest |Z - 2| %.3f m, matches %d, inliers %d, translation error %.3g m, "
          "rotation %.3g rad" % (len(kf_from.keypoints), len(kf_to.keypoints), d_err, z_err, len(reg.matches), n_in, t_err, angle))
    assert reg.status == 0 and reg.success
    assert np.array_equal(reg.transformation, reg_ref.transformation) and np.array_equal(reg.inliers, reg_ref.inliers)
    assert np.array_equal(reg.matches, reg_ref.matches)
    assert t_err <= 0.04 and angle <= 0.025
    assert vf.is_new_keyframe(reg, len(kf_to.keypoints), 0.3) is False
    assert vf.is_new_keyframe(reg, len(kf_to.keypoints), 0.999) is True
