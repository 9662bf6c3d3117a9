"""GPU: the level-aware PnP (vis_pnp_kernel<true> of csrc/vis.hip through cslam_amd.front_end.visual_registration) against its
float64 restatement (tests/vis_levels_reference.py), and the whole new path, sub-pixel level keyframes into the level-aware
registration, on the two-distance scene.  Decisions (flags, best hypothesis, counts, status) are compared exactly, each
guarded by the restatement's own distance from the threshold; T within 8 cond(A) eps of the restatement's, A being the
restatement's weighted normal matrix at its result: the rule of test_vis_gpu.py::scene_tol."""
import functools

import numpy as np
import pytest

import feat_pyramid_reference as pyr_ref
import feat_subpixel_reference as sub_ref
import vis_levels_reference as ref
import vis_reference as uni
from cslam_amd.front_end import visual_pyramid as vp
from cslam_amd.front_end import visual_registration as vr
from test_feat_pyramid_gpu import same_floats
from test_vis_gpu import same, scene_tol
from test_vis_levels_cpu import SCENE_GAIN, SCENE_GUARD, scene_directions, scene_errors

pytestmark = pytest.mark.gpu

CAM = uni.CAM
EPS = np.finfo(np.float64).eps


def level_tol(X, uv, lv, want):
    """8 cond(A) eps with the restatement's weighted A over its final inliers at its result."""
    m = want["inliers"]
    A, _ = ref.gn_sums(want["T"][:3, :3], want["T"][:3, 3], CAM, X[m], uv[m], 1.0 / ref.SIGMA2[lv[m]])
    return 8.0 * EPS * np.linalg.cond(A)


@functools.lru_cache(maxsize=None)
def level_scene(seed):
    X, uv, lv, T, out = ref.planted_level_scene(seed)
    return X, uv, lv, T, out, ref.pnp_ransac(X, uv, lv, CAM, seed=seed)


# ---- every level 0 is the uniform rule -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_all_levels_0_equal_the_uniform_pnp(seed):
    X, uv, T, out = uni.planted_scene(seed)
    want = uni.pnp_ransac(X, uv, CAM, seed=seed)
    a = vr.pnp_ransac_pairs([(X, uv)], CAM, seed=seed)[0]
    b = vr.pnp_ransac_level_pairs([(X, uv)], [np.zeros(len(X), dtype=np.uint8)], CAM, seed=seed)[0]
    assert a.status == b.status == 0 and a.best_hypothesis == b.best_hypothesis and a.dropped_no_depth == b.dropped_no_depth
    assert np.array_equal(a.matches, b.matches) and np.array_equal(a.inliers, b.inliers) and a.inliers.sum() == b.inliers.sum() > 20
    d = np.abs(a.transformation - b.transformation).max()
    print("seed %d: level-aware form at level 0 against the uniform kernel %.3g" % (seed, d))
    assert d <= scene_tol(X, uv, want)
    # and the best hypothesis' own count: without refinement the final flags are its inlier set
    a0 = vr.pnp_ransac_pairs([(X, uv)], CAM, seed=seed, refine_rounds=0)[0]
    b0 = vr.pnp_ransac_level_pairs([(X, uv)], [np.zeros(len(X), dtype=np.int64)], CAM, seed=seed, refine_rounds=0)[0]
    assert np.array_equal(a0.inliers, b0.inliers) and a0.inliers.sum() == want["hyp"]["count"][want["best_hypothesis"]]
    assert a0.transformation.tobytes() == b0.transformation.tobytes()


# ---- planted scenes with levels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_scene_with_levels(seed):
    """M = 200, levels 0 .. 3 drawn per correspondence, pixel noise +-0.5 1.2^l, half gross outliers."""
    X, uv, lv, T, out, want = level_scene(seed)
    h = want["best_hypothesis"]
    assert want["status"] == 0 and want["guard"] >= 1e-6 and set(lv.tolist()) == {0, 1, 2, 3}
    got = vr.pnp_ransac_level_pairs([(X, uv)], [lv], CAM, seed=seed)[0]
    assert got.status == 0 and got.success and got.dropped_no_depth == 0
    assert got.best_hypothesis == h
    assert np.array_equal(got.inliers, want["inliers"]) and not np.any(got.inliers & out)
    raw = vr.pnp_ransac_level_pairs([(X, uv)], [lv], CAM, seed=seed, refine_rounds=0)[0]
    assert raw.best_hypothesis == h and np.array_equal(raw.inliers, want["hyp"]["masks"][h]) and raw.inliers.sum() == want["hyp"]["count"][h]
    d_ref, d_plant, own = np.abs(got.transformation - want["T"]).max(), np.abs(got.transformation - T).max(), np.abs(want["T"] - T).max()
    tol = level_tol(X, uv, lv, want)
    print("seed %d: against the restatement %.3g (allowed %.3g), against the plant %.3g (the restatement's own %.3g), %d inliers, "
          "guard %.3g px" % (seed, d_ref, tol, d_plant, own, got.inliers.sum(), want["guard"]))
    assert d_ref <= tol and d_plant <= 2.0 * own


def test_status_edges_with_levels():
    """M = 3 and min_inliers - 1 usable are not attempted (status 2), 2048 are, 2049 are not (status 3)."""
    big = uni.planted_scene(10, M=2049, outliers=0.0)
    X, uv, _, _ = uni.planted_scene(9, M=60, outliers=0.0)
    lvl = lambda n: (np.arange(n) * 7 % 4).astype(np.int32)
    nan19 = X[:25].copy()
    nan19[:6] = np.nan                                     # 19 usable of 25
    pairs = [(X[:3], uv[:3]), (X[:19], uv[:19]), (nan19, uv[:25]), (big[0][:2048], big[1][:2048]), (big[0], big[1])]
    levels = [lvl(len(a)) for a, _ in pairs]
    got = vr.pnp_ransac_level_pairs(pairs, levels, CAM)
    want = [ref.pnp_ransac(a, b, l, CAM) for (a, b), l in zip(pairs, levels)]
    assert [g.status for g in got] == [2, 2, 2, 0, 3] == [w["status"] for w in want]
    for g, w in zip(got, want):
        assert np.all(np.isfinite(g.transformation)) and g.success == (g.status == 0)
        assert np.array_equal(g.inliers, w["inliers"]) and g.dropped_no_depth == w["dropped"] and g.best_hypothesis == w["best_hypothesis"]
        if g.status >= 2:
            assert np.array_equal(g.transformation, np.identity(4)) and g.best_hypothesis == -1 and not g.inliers.any()
    assert got[2].dropped_no_depth == 6 and want[3]["guard"] >= 1e-6
    assert np.abs(got[3].transformation - want[3]["T"]).max() <= level_tol(pairs[3][0], pairs[3][1], levels[3], want[3])


def test_batch_of_17_mixed_pairs_is_bit_identical_to_one_by_one_and_reversed():
    pairs, levels = [], []
    for k, M in enumerate((0, 3, 4, 64, 65, 257, 2048, 2049, 20, 19, 200, 1, 63, 256, 255, 100, 5)):
        X, uv, lv, _, _ = ref.planted_level_scene(70 + k, M=max(M, 1), levels=1 + k % 8, outliers=0.4 if M >= 20 else 0.0)
        X, uv, lv = X[:M].copy(), uv[:M].copy(), lv[:M].copy()
        if k % 3 == 0 and M:
            X[::7] = np.nan                                 # keypoints without depth
        pairs.append((X, uv))
        levels.append(lv)
    cams = np.tile(CAM, (17, 1))
    batch = vr.pnp_ransac_level_pairs(pairs, levels, cams)
    back = vr.pnp_ransac_level_pairs(pairs[::-1], levels[::-1], cams)[::-1]
    assert {0, 2, 3} <= set(g.status for g in batch) and max(l.max(initial=0) for l in levels) == 7
    for p, l, g, b in zip(pairs, levels, batch, back):
        assert same(g, vr.pnp_ransac_level_pairs([p], [l], CAM)[0]) and same(g, b)
    assert vr.pnp_ransac_level_pairs([], [], CAM) == [] and vr.register_level_pairs([], CAM) == []


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_level_keyframes_from_two_distances_register_in_both_directions():
    """The two-distance scene (144 x 192, the plane at 2.88 m and 2.0 m), 4 levels, 300 hypotheses, 2 px, seed 0: sub-pixel
    level keyframes and the level-aware registration beside the parent path (integer keyframes, uniform PnP) in the same run.
    The GPU keyframes equal the restatement's bit for bit, so matches, flags and best hypothesis are the restatement's, and
    its figures (tests/test_vis_levels_cpu.py) are the GPU's: B->A 0.0257 m / 0.0124 rad -> 0.0133 m / 0.0066 rad, A->B
    0.0357 m / 0.0124 rad -> 0.0125 m / 0.0044 rad."""
    A, B, dA, dB = pyr_ref.scene()
    cam = np.array(pyr_ref.SCENE_CAMERA)
    fine = vp.extract_level_keyframes([A, B], [dA, dB], cam, levels=4)
    plain = vp.extract_keyframes_pyramid([A, B], [dA, dB], cam, levels=4)
    for kf, w, p in zip(fine, sub_ref.scene_features(4), plain):
        assert isinstance(kf, vr.LevelKeyframe) and kf.levels.dtype == np.uint8
        same_floats(kf.keypoints, w["keypoints"])
        same_floats(kf.points, w["points"])
        assert np.array_equal(kf.descriptors, w["descriptors"]) and np.array_equal(kf.levels, w["levels"])
        assert np.array_equal(kf.descriptors, p.descriptors)
    t_bound, r_bound = pyr_ref.scene_bounds()
    new = vr.register_level_pairs([(fine[1], fine[0]), (fine[0], fine[1])], cam)
    old = vr.register_pairs([(plain[1], plain[0]), (plain[0], plain[1])], cam)
    as_tuple = lambda kf: (kf.keypoints, kf.points, kf.descriptors, kf.levels)
    for (name, i_from, i_to, plant), got, par in zip(scene_directions(), new, old):
        rows, want = ref.register(as_tuple(fine[i_from]), as_tuple(fine[i_to]), cam)
        assert want["guard"] >= SCENE_GUARD
        assert np.array_equal(got.matches, rows) and np.array_equal(got.matches, par.matches)
        assert np.array_equal(got.inliers, want["inliers"]) and got.best_hypothesis == want["best_hypothesis"] and got.status == want["status"] == 0
        use = np.isfinite(fine[i_from].points[rows[:, 0]]).all(axis=1)
        X, uv, lv = fine[i_from].points[rows[:, 0]][use], fine[i_to].keypoints[rows[:, 1]][use], fine[i_to].levels[rows[:, 1]][use]
        tol = level_tol(X, uv, lv, dict(want, inliers=want["inliers"][use]))
        d = np.abs(got.transformation - want["T"]).max()
        (t1, r1), (t0, r0) = scene_errors(got.transformation, plant), scene_errors(par.transformation, plant)
        print("%s: %d and %d keypoints, %d matches; integer + uniform %d inliers, %.4f m / %.4f rad; sub-pixel + level-aware %d inliers, "
              "%.4f m / %.4f rad; share %.3f; T against the restatement %.3g (allowed %.3g)"
              % (name, len(fine[i_from].keypoints), len(fine[i_to].keypoints), len(rows), par.inliers.sum(), t0, r0, got.inliers.sum(), t1, r1,
                 t1 / t0, d, tol))
        assert d <= tol
        assert got.success and t1 <= t_bound and r1 <= r_bound and t1 <= SCENE_GAIN * t0
        assert same(got, vr.compute_level_transformation(fine[i_from], fine[i_to], cam))
        edge = got.to_edge((0, 0), (1, 0))
        assert np.abs(np.asarray(edge[2]) @ got.transformation - np.identity(4)).max() < 1e-12
    # a LevelKeyframe goes into the uniform registration as it is
    assert same(vr.register_pairs([(fine[1], fine[0])], cam)[0], vr.register_pairs([(vr.Keyframe(*fine[1][:3]), vr.Keyframe(*fine[0][:3]))], cam)[0])
