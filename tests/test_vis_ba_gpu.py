"""GPU: the two-view bundle adjustment after PnP (csrc/vis_ba.hip through cslam_amd.front_end.visual_registration) against
its numpy restatement (tests/vis_ba_reference.py).

The staged cases are those of tests/test_vis_ba_cpu.py, compared by `vis_ba_reference.compare`: status, set size in, rounds
discarded and points held fixed exactly; the steps only where no |delta| of the restatement lies within a factor 10 of 1e-10;
set size out and the flags only where every recount decision of the restatement is 1e-6 px from its threshold; T and the
refined points within 8 eps cond(H), H the restatement's full (6 + 3 M)-square normal matrix at its result, for M <= 257, and
at 2048 within 4 x the float64 restatement's own distance from its np.longdouble run.
Measured on the MI355X: see the README ("Two-view bundle adjustment").
"""
import ctypes
import functools

import numpy as np
import pytest

import feat_reference
import stereo_reference
import vis_ba_reference as ba
import vis_reference as ref
from cslam_amd import _lib
from cslam_amd.front_end import visual_registration as vr
from cslam_amd.front_end import visual_stereo as vs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cases():
    return {c["name"]: c for c in ba.all_cases()}


@functools.lru_cache(maxsize=None)
def record(name):
    c = cases()[name]
    return ba.run_case(c, **ba.settings(c))


def keyframes(c):
    """The case as (keyframe_from, keyframe_to, the registration PnP would have given)."""
    da, db = np.zeros((len(c["kp_a"]), 32), np.uint8), np.zeros((len(c["kp_b"]), 32), np.uint8)
    if c.get("lv_a") is not None:
        a, b = vr.LevelKeyframe(c["kp_a"], c["pts_a"], da, c["lv_a"]), vr.LevelKeyframe(c["kp_b"], c["pts_b"], db, c["lv_b"])
    else:
        a, b = vr.Keyframe(c["kp_a"], c["pts_a"], da), vr.Keyframe(c["kp_b"], c["pts_b"], db)
    st = c.get("pnp_status", 0)
    return a, b, vr.VisualRegistration(np.asarray(c["T0"], dtype=np.float64), st == 0, st, c["rows"], np.asarray(c["flags"], bool), 0, 0)


def kwargs(c):
    kw = {k: c[k] for k in ("reproj_error", "min_inliers", "ba_iterations", "ba_rounds") if k in c}
    return dict(kw, cameras_to=c.get("cam_b", ba.CAM), baselines=(c.get("base_a", ba.BASELINE), c.get("base_b", ba.BASELINE)))


def adjust(c):
    a, b, reg = keyframes(c)
    return vr.bundle_adjust_pairs([(a, b)], [reg], c.get("cam_a", ba.CAM), **kwargs(c))[0]


def as_result(g):
    info = np.array([g.status, g.set_in, int(np.count_nonzero(g.inliers)), g.ba_steps, g.rounds_discarded, g.points_held, g.pnp.status, 0])
    return dict(T=g.transformation, cost=np.array([g.cost_before, g.cost_after]), info=info, flags=g.inliers, points=g.points)


def check(name):
    c = cases()[name]
    got = adjust(c)
    ba.compare(c, as_result(got), record(name), name)
    return c, got, record(name)


# ---- planted sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ba.SET_SIZES)
def test_planted_set_equals_the_restatement(size):
    """Sets of 20 .. 2048 flagged correspondences with levels 0 .. 3 in both views and a tenth of the "to" points without
    depth, T0 the level-aware Gauss-Newton PnP fit."""
    c, got, want = check("size %d" % size)
    assert got.success and got.set_in == size and isinstance(got, vr.VisualRegistration)
    assert np.abs(got.transformation - c["T"]).max() <= 2.0 * np.abs(want["T"] - c["T"]).max() + 1e-9
    assert got.cost_after < got.cost_before


def test_a_displaced_from_keypoint_is_dropped_in_round_one():
    """Its "to" pixel and "from" point are consistent, so PnP flags it; its "from" keypoint is 5 px off, which only the
    adjustment sees."""
    c, got, want = check("displaced from keypoint")
    k = c["displaced"]
    assert got.pnp.inliers[k] and not got.inliers[k] and np.isnan(got.points[k]).all()
    assert np.count_nonzero(got.inliers) == got.set_in - 1
    first = vr.bundle_adjust_pairs([keyframes(c)[:2]], [keyframes(c)[2]], ba.CAM, ba_rounds=1, **kwargs(c))[0]
    assert not first.inliers[k]                             # round 1 already


def test_every_to_depth_missing():
    c, got, want = check("no to depth")
    assert got.success and np.count_nonzero(got.inliers) == got.set_in


def test_a_point_behind_the_to_camera_at_the_start():
    c, got, want = check("behind at T0")
    k = c["behind"]
    assert got.pnp.inliers[k] and not got.inliers[k] and np.count_nonzero(got.inliers) == got.set_in - 1
    # it contributed nothing: without it the fit is the same to rounding
    d = dict(c, flags=c["flags"].copy())
    d["flags"][k] = False
    other = adjust(d)
    assert np.abs(other.transformation - got.transformation).max() <= ba.tolerance(c, want)


def test_points_without_a_third_pivot_are_held_fixed():
    c, got, want = check("held by the pivot rule")
    assert got.points_held >= got.set_in and got.ba_steps >= 1


# ---- nothing adjusted ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pnp status 1", "pnp status 2", "pnp status 3", "no rounds", "no iterations", "above the cap"])
def test_passthrough(name):
    c, got, want = check(name)
    assert got.transformation.tobytes() == np.asarray(c["T0"], np.float64).tobytes() and np.array_equal(got.inliers, c["flags"])
    assert got.status == want["status"] and got.ba_steps == 0 and np.isnan(got.points).all() and np.isnan(got.cost_before)
    if name == "pnp status 3":
        assert len(c["rows"]) == 2049


def test_too_few_remain_is_status_1_with_the_fit():
    c, got, want = check("too few remain")
    assert got.status == 1 and not got.success and got.ba_steps > 0
    with pytest.raises(ValueError):
        got.to_edge((0, 0), (1, 0))


# ---- batches -----------------------------------------------------------------------------------------------------------
def same(a, b):
    return (a.transformation.tobytes() == b.transformation.tobytes() and a.status == b.status and np.array_equal(a.inliers, b.inliers)
            and a.points.tobytes() == b.points.tobytes() and np.array([a.cost_before, a.cost_after]).tobytes() == np.array([b.cost_before, b.cost_after]).tobytes()
            and (a.set_in, a.ba_steps, a.rounds_discarded, a.points_held) == (b.set_in, b.ba_steps, b.rounds_discarded, b.points_held)
            and a.pnp.transformation.tobytes() == b.pnp.transformation.tobytes() and np.array_equal(a.pnp.inliers, b.pnp.inliers)
            and a.pnp.status == b.pnp.status and np.array_equal(a.matches, b.matches))


@functools.lru_cache(maxsize=None)
def ragged_cases():
    out = []
    for k, M in enumerate((0, 3, 4, 64, 65, 257, 2048, 2049, 20, 19, 200, 1, 63, 256, 255, 100, 5)):
        c = ba.planted_case(max(M, 1), seed=800 + k, extra=0 if M >= 2048 else 5)
        if M == 0:
            c = dict(c, kp_a=c["kp_a"][:0], pts_a=c["pts_a"][:0], lv_a=c["lv_a"][:0], kp_b=c["kp_b"][:0], pts_b=c["pts_b"][:0], lv_b=c["lv_b"][:0],
                     rows=c["rows"][:0], flags=c["flags"][:0])
        if M in (64, 257, 200, 256):
            c["pts_a"][::7] = np.nan                         # flagged rows that cannot be adjusted
        if k % 2:
            c = dict(c, lv_a=None, lv_b=None)                # no levels
        if M == 19:
            c = dict(c, pnp_status=1)
        out.append(c)
    return out


def test_batch_of_17_ragged_pairs_equals_one_by_one_and_reversed():
    cs = ragged_cases()
    kfs = [keyframes(c) for c in cs]
    pairs, regs = [k[:2] for k in kfs], [k[2] for k in kfs]
    batch = vr.bundle_adjust_pairs(pairs, regs, ba.CAM, baselines=ba.BASELINE)
    assert {0, 1, 3} <= set(g.status for g in batch) and any(g.set_in == 2048 for g in batch)
    back = vr.bundle_adjust_pairs(pairs[::-1], regs[::-1], ba.CAM, baselines=ba.BASELINE)[::-1]
    for p, r, g, h in zip(pairs, regs, batch, back):
        assert same(g, vr.bundle_adjust_pairs([p], [r], ba.CAM, baselines=ba.BASELINE)[0]) and same(g, h)
    assert vr.bundle_adjust_pairs([], [], ba.CAM) == [] and vr.register_pairs_ba([], ba.CAM) == []


@functools.lru_cache(maxsize=None)
def chain_pairs():
    """Keyframe pairs with descriptors (vis_reference.keyframe_pair); every other pair carries levels."""
    out = []
    for s, (landmarks, distractors) in enumerate([(300, 100), (0, 0), (257, 43), (30, 8), (120, 30), (600, 200)]):
        if landmarks == 0:
            e = vr.Keyframe(np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 32), np.uint8))
            out.append((e, vr.Keyframe(*ref.keyframe_pair(95, landmarks=5, distractors=0)[1])))
            continue
        a, b = ref.keyframe_pair(60 + s, landmarks=landmarks, distractors=distractors)[:2]
        if s % 2:
            rng = np.random.default_rng(s)
            out.append((vr.LevelKeyframe(*a, rng.integers(0, 4, len(a[0])).astype(np.uint8)), vr.LevelKeyframe(*b, rng.integers(0, 4, len(b[0])).astype(np.uint8))))
        else:
            out.append((vr.Keyframe(*a), vr.Keyframe(*b)))
    return out


def test_chained_call_equals_the_staged_calls():
    pairs = chain_pairs()
    got = vr.register_pairs_ba(pairs, ref.CAM, min_inliers=8)
    assert [g.pnp.status for g in got] == [0, 2, 0, 0, 0, 0] and all(g.status == 0 for g in got if g.pnp.status == 0)
    for (a, b), g in zip(pairs, got):
        levels = hasattr(a, "levels")
        pnp = (vr.register_level_pairs if levels else vr.register_pairs)([(a, b)], ref.CAM, min_inliers=8)[0]
        assert pnp.transformation.tobytes() == g.pnp.transformation.tobytes() and np.array_equal(pnp.inliers, g.pnp.inliers)
        assert pnp.status == g.pnp.status and np.array_equal(pnp.matches, g.matches) and pnp.best_hypothesis == g.best_hypothesis
        assert same(g, vr.bundle_adjust_pairs([(a, b)], [pnp], ref.CAM, min_inliers=8)[0])
        assert same(g, vr.compute_transformation_ba(a, b, ref.CAM, min_inliers=8))
    back = vr.register_pairs_ba(pairs[::-1], ref.CAM, min_inliers=8)[::-1]
    assert all(same(g, h) for g, h in zip(got, back))


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_launch():
    c = cases()["size 20"]
    a, b, reg = keyframes(c)
    bad = vr.LevelKeyframe(a.keypoints, a.points, a.descriptors, np.full(len(a.keypoints), 8))
    for call in (lambda: vr.bundle_adjust_pairs([(bad, b)], [reg], ba.CAM), lambda: vr.register_pairs_ba([(bad, b)], ba.CAM),
                 lambda: vr.bundle_adjust_pairs([(a, b)], [reg], ba.CAM, baselines=0.0), lambda: vr.register_pairs_ba([(a, b)], ba.CAM, baselines=(0.1, -1.0)),
                 lambda: vr.bundle_adjust_pairs([(a, b)], [reg, reg], ba.CAM), lambda: vr.bundle_adjust_pairs([(a, b)], [reg], np.ones((2, 4))),
                 lambda: vr.register_pairs_ba([(a, b)], ba.CAM, ba_rounds=-1)):
        with pytest.raises(ValueError):
            call()
    # the C ABI refuses the same on its host copies: nothing is launched, so null device pointers are never touched
    lib = _lib.load()
    off = np.array([0, 4], dtype=np.int64)
    lv_bad, lv_ok = np.array([0, 1, 9, 0], dtype=np.int32), np.zeros(4, dtype=np.int32)
    host = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    one = ctypes.c_void_p(256)                               # a non-null address that is never dereferenced: the host checks come first

    def call(levels, base, rounds=2):
        base = np.array([base], dtype=np.float64)
        return lib.cslam_vis_ba_dev(one, one, one, one, one, one, one, one, one, one, one, one, one, None, one, one, one, 1, 2.0, 20, 10, rounds,
                                    one, one, one, one, one, host(off), host(off), host(off), host(levels), host(levels), host(base), None)

    assert call(lv_bad, (0.1, 0.1)) == -1 and b"levels" in lib.cslam_last_error()
    assert call(lv_ok, (0.1, 0.0)) == -1 and b"baselines" in lib.cslam_last_error()
    assert call(lv_ok, (0.1, 0.1), rounds=-1) == -1


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_stereo_keyframes_register_with_the_adjustment():
    """The 120 x 160 stereo block-texture pair of tests/test_stereo_gpu.py (disparity 10 = 2 m at fx 100, baseline 0.2 m, the
    views 16 columns = 0.32 m apart): the GPU's keyframes equal the restatement's bit for bit, so the chain on either gives the
    same bits; the result equals the restatement chain's by the rules above and stays within the scene's bounds of 0.04 m
    and 0.025 rad."""
    tex = feat_reference.block_texture(120, 200, seed=7)
    cut = lambda a: np.ascontiguousarray(tex[:, a:a + 160])
    lefts, rights = [cut(0), cut(16)], [cut(10), cut(26)]
    cam = (100.0, 100.0, 80.0, 60.0, 0.2)
    kf_from, kf_to = vs.extract_keyframes_stereo(lefts, rights, cam)
    want_kf = [stereo_reference.extract_stereo(l, r, cam) for l, r in zip(lefts, rights)]
    ref_kfs = [vr.Keyframe(w["keypoints"].astype(np.float64), w["points"], w["descriptors"]) for w in want_kf]
    got = vr.register_pairs_ba([(kf_from, kf_to)], cam[:4], baselines=cam[4])[0]
    assert same(got, vr.register_pairs_ba([tuple(ref_kfs)], cam[:4], baselines=cam[4])[0])
    rows, pnp, want = ba.register_ba(tuple(ref_kfs[0]), tuple(ref_kfs[1]), np.array(cam[:4]), baselines=cam[4])
    assert np.array_equal(got.matches, rows) and np.array_equal(got.pnp.inliers, pnp["inliers"]) and got.pnp.status == pnp["status"] == 0
    # the adjustment alone, from the GPU's own PnP result, against the restatement from the same start
    c = dict(name="stereo pair", kp_a=ref_kfs[0].keypoints, pts_a=ref_kfs[0].points, kp_b=ref_kfs[1].keypoints, pts_b=ref_kfs[1].points,
             rows=got.matches, flags=got.pnp.inliers, T0=got.pnp.transformation, cam_a=np.array(cam[:4]), cam_b=np.array(cam[:4]),
             base_a=cam[4], base_b=cam[4])
    ba.compare(c, as_result(got), ba.run_case(c), "stereo pair")
    plant = np.identity(4)
    plant[0, 3] = -16 * 2.0 / 100.0
    for name, T in (("PnP", got.pnp.transformation), ("adjusted", got.transformation)):
        t_err, angle = ba.pose_errors(T, plant)
        print("%s: translation error %.4f m, rotation %.4f rad" % (name, t_err, np.radians(angle)))
    t_err, angle = ba.pose_errors(got.transformation, plant)
    assert got.success and t_err <= 0.04 and np.radians(angle) <= 0.025
    assert want["status"] == 0 and np.array_equal(got.inliers, want["flags"])
