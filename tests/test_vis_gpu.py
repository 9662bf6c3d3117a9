"""GPU: the visual verification (csrc/vis.hip through cslam_amd.front_end.visual_registration) against its float64
restatement (tests/vis_reference.py).  The matcher is compared exactly; the hypotheses one by one except those the
restatement's own conditioning guard leaves out; the planted scenes against the restatement and against the plant."""
import functools

import numpy as np
import pytest

import vis_reference as ref
from cslam_amd.back_end import pose_graph as pg
from cslam_amd.front_end import visual_registration as vr

pytestmark = pytest.mark.gpu

CAM = ref.CAM
# Per-hypothesis comparison, the six scenes of `hyp_scene` with 300 hypotheses each.
# HYP_POSE_TOL: 8 x the restatement's own worst error against the plant on the noise-free twins of the scenes (all-inlier
# hypotheses above the guard): 0, 0, 1.64e-13, 4.63e-13, 5.83e-13, 8.45e-12 for M = 4 .. 257.  Measured on the MI355X, largest
# entry of (R, t) minus the restatement's over the hypotheses above the guard: 9.7e-15, 1.2e-14, 2.1e-13, 2.4e-12, 2.0e-12,
# 1.7e-12.
# HYP_GUARD: relative separation in the root decisions and pixels at the threshold; 1e-5 is more than 1e4 above the measured
# pose difference (2.4e-12).  It leaves out 0, 0, 1.0, 2.0, 2.7 and 2.7 % of the hypotheses (the restatement alone, on the CPU).
HYP_GUARD = ref.HYP_GUARD
HYP_POSE_TOL = 8 * 8.45e-12
HYP_MAX_LEFT_OUT = 0.05            # a condition on the scenes, not a tolerance: a scene that misses it gets another seed
# Planted scenes, T against the restatement's T.  The restatement sits on its own stationary point to 1e-16 (one more of its
# steps moves no entry by more than that), so its own error is that of the point itself: the solution of the 6 x 6 normal
# equations A delta = -b moves by up to cond(A) eps when the sums are rounded differently, which is all that differs between
# the kernel and numpy.  Allowed: 8 cond(A) eps with A the restatement's at its result (cond(A) = 120, 74, 86 for the three
# seeds and 1.5e3 on the plane: 2.1e-13, 1.3e-13, 1.5e-13, 2.6e-12).  Measured on the MI355X: 4.4e-16, 1.6e-15, 6.4e-16.
# Against the plant: twice the restatement's own error against the plant (7.6e-4, 5.9e-4, 2.8e-4).


def scene_tol(X, uv, want):
    m = want["inliers"]
    A, _ = ref.gn_sums(want["T"][:3, :3], want["T"][:3, 3], CAM, X[m], uv[m])
    return 8.0 * np.finfo(np.float64).eps * np.linalg.cond(A)


hyp_scene = ref.hyp_scene


@functools.lru_cache(maxsize=None)
def ref_hyp(M):
    X, uv, _, _ = hyp_scene(M)
    return ref.hypotheses(X, uv, CAM, 300, 2.0, M)


@functools.lru_cache(maxsize=None)
def ref_scene(seed, shape=None):
    X, uv, T, out = ref.planted_scene(seed, shape=shape)
    return X, uv, T, out, ref.pnp_ransac(X, uv, CAM, seed=seed)


# ---- matcher -------------------------------------------------------------------------------------------------------
def descs(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def near(rng, d, flips):
    bits = np.unpackbits(d, axis=1)
    for k in range(len(d)):
        bits[k, rng.choice(256, flips, replace=False)] ^= 1
    return np.packbits(bits, axis=1)


def matcher_pairs():
    rng = np.random.default_rng(0)
    pairs = []
    for na in (0, 1, 255, 256, 257):
        for nb in (0, 1, 2, 255, 256, 257, 513):
            b = descs(rng, nb)
            a = descs(rng, na)
            if nb:                                          # most "from" rows are a few bits from some "to" row
                src = rng.integers(0, nb, na)
                a = np.where((rng.random(na) < 0.7)[:, None], near(rng, b[src], 6), a) if na else a
            pairs.append((a, b))
    return pairs


def special_pairs():
    rng = np.random.default_rng(1)
    b = descs(rng, 300)
    dup = np.concatenate([b[:10], b[:10], descs(rng, 280)])                  # duplicate "to" rows: d1 == d2
    a_dup = np.concatenate([b[:5], near(rng, b[5:10], 3)])                   # 0 == 0 and 3 == 3 both pass <=
    comp = (descs(rng, 4), None)
    comp = (comp[0], np.concatenate([~comp[0], ~comp[0][:1]]))               # complements: distance 256
    zeros = (np.zeros((7, 32), np.uint8), np.zeros((9, 32), np.uint8))
    last = descs(rng, 513)
    a_last = near(rng, np.repeat(last[512:513], 3, axis=0), 2)               # nearest in the last row of the last partial chunk
    five_eq = np.repeat(b[17:18], 5, axis=0)                                 # five rows claim one "to" row, equal distances
    five_ne = np.concatenate([near(rng, b[33:34], k) for k in (4, 2, 3, 2, 5)])     # unequal: the first of the two at distance 2
    return [(a_dup, dup), comp, zeros, (a_last, last), (five_eq, b), (five_ne, b), (np.concatenate([five_eq, five_ne]), b)]


@pytest.mark.parametrize("nndr", [0.8, 1.0, 0.0])
def test_matcher_equals_the_restatement(nndr):
    pairs = matcher_pairs() + special_pairs()
    got = vr.match_descriptors_pairs(pairs, nndr)
    total = 0
    for (a, b), g in zip(pairs, got):
        want = ref.match(a, b, nndr)
        assert g.dtype == np.int64 and np.array_equal(g, want), (len(a), len(b), nndr)
        total += len(want)
    assert total > (1000 if nndr > 0.0 else 5)              # nndr 0: only d1 == 0 passes
    if nndr == 0.8:
        sp = special_pairs()
        got = [vr.match_descriptors(a, b) for a, b in sp]
        assert got[0].tolist() == [[k, k] for k in range(5)]                # 0 <= 0.8 * 0 passes, 3 <= 0.8 * 3 does not
        assert len(got[1]) == 0                             # complements: 256 <= 0.8 * 256 is false
        assert got[2].tolist() == [[0, 0]]                  # all rows at distance 0 of all: row 0 keeps "to" row 0
        assert set(got[3][:, 1].tolist()) == {512}
        assert got[4].tolist() == [[0, 17]] and got[5].tolist() == [[1, 33]]


def test_matcher_duplicate_rows_pass_only_at_equal_distance_zero():
    """d1 == d2 > 0 fails d1 <= 0.8 d2; d1 == d2 == 0 passes, and so does any d1 == d2 at nndr = 1."""
    a, b = special_pairs()[0]
    assert vr.match_descriptors(a, b, 0.8)[:, 0].tolist() == [0, 1, 2, 3, 4]
    assert vr.match_descriptors(a, b, 1.0)[:, 0].tolist() == list(range(10))


def test_matcher_batch_equals_one_by_one():
    pairs = (matcher_pairs()[::3] + special_pairs())[:17]
    assert len(pairs) == 17 and any(len(a) == 0 for a, _ in pairs) and any(len(b) == 0 for _, b in pairs)
    batch = vr.match_descriptors_pairs(pairs)
    for (a, b), g in zip(pairs, batch):
        assert np.array_equal(g, vr.match_descriptors(a, b))
    assert vr.match_descriptors_pairs([]) == []


# ---- hypotheses ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", ref.HYP_SIZES)
def test_hypotheses_equal_the_restatement(M):
    X, uv, _, _ = hyp_scene(M)
    want = ref_hyp(M)
    keep = (want["guard_roots"] >= HYP_GUARD) & (want["guard_threshold"] >= HYP_GUARD)
    share = 1.0 - keep.mean()
    print("M %d: %.1f %% of the hypotheses left out by the guard" % (M, 100 * share))
    assert share <= HYP_MAX_LEFT_OUT
    best = ref.best_hypothesis(want["count"])
    assert want["guard_threshold"][best] >= 1e-6 and np.all(want["guard_threshold"][want["valid"]] >= 1e-6)
    worst = 0.0
    for iterations in (1, 255, 256, 257, 300):
        got = vr.hypotheses((X, uv), CAM, iterations, 2.0, seed=M)
        k = keep[:iterations]
        assert np.array_equal(got.valid[k], want["valid"][:iterations][k])
        assert np.array_equal(got.inliers[k], want["count"][:iterations][k])
        v = k & want["valid"][:iterations]
        if v.any():
            worst = max(worst, np.abs(got.R[v] - want["R"][:iterations][v]).max(), np.abs(got.t[v] - want["t"][:iterations][v]).max())
        assert np.all(np.isfinite(got.R)) and np.all(np.isfinite(got.t))
        # the best hypothesis and its inlier set are never left out
        b = ref.best_hypothesis(want["count"][:iterations])
        assert got.best_hypothesis == b
        assert np.array_equal(got.best_inliers, want["masks"][b] if want["valid"][b] else np.zeros(M, dtype=bool))
    print("M %d: largest pose difference %.3g" % (M, worst))
    assert worst <= HYP_POSE_TOL


# ---- planted scenes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_scene(seed):
    X, uv, T, out, want = ref_scene(seed)
    assert want["status"] == 0 and want["hyp"]["guard_threshold"][want["best_hypothesis"]] >= 1e-6
    got = vr.pnp_ransac_pairs([(X, uv)], CAM, seed=seed)[0]
    assert got.status == 0 and got.success and got.dropped_no_depth == 0
    assert got.best_hypothesis == want["best_hypothesis"]
    assert np.array_equal(got.inliers, want["inliers"]) and not np.any(got.inliers & out)
    assert np.array_equal(got.matches, np.repeat(np.arange(200)[:, None], 2, axis=1))
    d_ref, d_plant, own = np.abs(got.transformation - want["T"]).max(), np.abs(got.transformation - T).max(), np.abs(want["T"] - T).max()
    print("seed %d: against the restatement %.3g, against the plant %.3g (the restatement's own %.3g), %d inliers"
          % (seed, d_ref, d_plant, own, got.inliers.sum()))
    assert d_ref <= scene_tol(X, uv, want) and d_plant <= 2.0 * own


# ---- edges ---------------------------------------------------------------------------------------------------------
def test_status_edges():
    rng = np.random.default_rng(5)
    X, uv, T, _ = ref.planted_scene(9, M=60, outliers=0.0)
    rand = lambda n: np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1)
    all_out = (X, rand(60))
    exact = (np.concatenate([X[:20], X[20:]]), np.concatenate([uv[:20], rand(40)]))           # exactly 20 inliers ...
    nan_pts = (np.full((30, 3), np.nan), uv[:30])
    big = ref.planted_scene(10, M=2049, outliers=0.0)
    pairs = [all_out, (X[:3], uv[:3]), (X[:19], uv[:19]), (big[0], big[1]), exact, nan_pts, (big[0][:2048], big[1][:2048])]
    got = vr.pnp_ransac_pairs(pairs, CAM)
    want = [ref.pnp_ransac(a, b, CAM) for a, b in pairs]
    assert [g.status for g in got] == [1, 2, 2, 3, 0, 2, 0] == [w["status"] for w in want]
    for g, w in zip(got, want):
        assert np.all(np.isfinite(g.transformation)) and g.success == (g.status == 0)
        assert np.array_equal(g.inliers, w["inliers"]) and g.dropped_no_depth == w["dropped"]
        if g.status >= 2:
            assert np.array_equal(g.transformation, np.identity(4)) and g.best_hypothesis == -1 and not g.inliers.any()
    assert got[4].inliers.sum() == 20 and got[4].inliers[:20].all()
    assert got[5].dropped_no_depth == 30
    assert not np.array_equal(got[0].transformation, np.identity(4))        # status 1 carries the best fit found
    with pytest.raises(ValueError):
        got[0].to_edge((0, 0), (0, 1))


def test_plane_is_solved_and_line_ends_without_nan():
    X, uv, T, out, want = ref_scene(4, "plane")
    got = vr.pnp_ransac_pairs([(X, uv)], CAM, seed=4)[0]
    assert got.status == 0 == want["status"] and np.array_equal(got.inliers, want["inliers"])
    assert np.abs(got.transformation - want["T"]).max() <= scene_tol(X, uv, want)
    assert np.abs(got.transformation - T).max() <= 2.0 * np.abs(want["T"] - T).max()
    X, uv, T, _ = ref.planted_scene(6, M=100, outliers=0.2, shape="line")
    got = vr.pnp_ransac_pairs([(X, uv)], CAM)[0]
    assert got.status in (1, 2) and np.all(np.isfinite(got.transformation))


# ---- determinism and batching --------------------------------------------------------------------------------------
def same(a, b):
    return (a.transformation.tobytes() == b.transformation.tobytes() and a.status == b.status and np.array_equal(a.inliers, b.inliers)
            and a.best_hypothesis == b.best_hypothesis and a.dropped_no_depth == b.dropped_no_depth and np.array_equal(a.matches, b.matches))


def test_runs_are_bit_identical_and_the_seed_only_moves_the_best_hypothesis():
    X, uv, T, out, _ = ref_scene(1)
    a, b = vr.pnp_ransac_pairs([(X, uv)], CAM, seed=1)[0], vr.pnp_ransac_pairs([(X, uv)], CAM, seed=1)[0]
    assert same(a, b)
    c = vr.pnp_ransac_pairs([(X, uv)], CAM, seed=12345)[0]
    assert c.best_hypothesis != a.best_hypothesis and np.array_equal(c.inliers, a.inliers)


def test_batch_of_17_mixed_pairs_is_bit_identical_to_one_by_one():
    pairs = []
    for k, M in enumerate((0, 3, 4, 64, 65, 257, 2048, 2049, 20, 19, 200, 1, 63, 256, 255, 100, 5)):
        X, uv, _, _ = ref.planted_scene(70 + k, M=max(M, 1), outliers=0.4 if M >= 20 else 0.0)
        X, uv = X[:M].copy(), uv[:M].copy()
        if k % 3 == 0 and M:
            X[::7] = np.nan                                 # keypoints without depth
        pairs.append((X, uv))
    cams = np.tile(CAM, (17, 1))
    batch = vr.pnp_ransac_pairs(pairs, cams)
    assert {0, 2, 3} <= set(g.status for g in batch)
    for p, g in zip(pairs, batch):
        assert same(g, vr.pnp_ransac_pairs([p], CAM)[0])
    assert vr.pnp_ransac_pairs([], CAM) == [] and vr.register_pairs([], CAM) == []


# ---- whole chain ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_pair(seed):
    kf_a, kf_b, T, ids_a, ids_b = ref.keyframe_pair(seed)
    return vr.Keyframe(*kf_a), vr.Keyframe(*kf_b), T, ids_a, ids_b


def test_compute_transformation_on_synthetic_keyframes():
    kf_a, kf_b, T, ids_a, ids_b = chain_pair(0)
    got = vr.compute_transformation(kf_a, kf_b, CAM)
    rows, want = ref.register(kf_a, kf_b, CAM)
    assert got.success and want["status"] == 0
    assert np.array_equal(got.matches, rows)                # no pair, of distractors or not, beyond what the restatement accepts
    wrong = (ids_a[got.matches[:, 0]] != ids_b[got.matches[:, 1]]) | (ids_a[got.matches[:, 0]] < 0)
    print("%d matches, %d of them not of one landmark, %d without depth, %d inliers" % (len(rows), wrong.sum(), got.dropped_no_depth,
                                                                                     got.inliers.sum()))
    assert got.dropped_no_depth == want["dropped"] > 0 and np.array_equal(got.inliers, want["inliers"])
    assert not np.any(got.inliers & wrong)
    assert np.abs(got.transformation - T).max() <= 2.0 * np.abs(want["T"] - T).max()


def test_register_pairs_equals_the_single_calls():
    pairs = [chain_pair(s)[:2] for s in range(8)]
    batch = vr.register_pairs(pairs, CAM)
    assert all(g.success for g in batch)
    for (a, b), g in zip(pairs, batch):
        assert same(g, vr.compute_transformation(a, b, CAM))


def test_to_edge_closes_a_two_chain_pose_graph():
    """Two chains of 20 poses; the second starts 0.8 m and 0.15 rad off.  One verified closure between pose 10 of each, as
    `to_edge` gives it, moves the second chain onto the plant to within the registration's own error carried along the chain.
    Measured on the MI355X: registration error 1.8e-4 (largest entry of T minus the plant), largest pose error after optimize
    4.0e-4."""
    kf_a, kf_b, T, _, _ = chain_pair(0)
    reg = vr.compute_transformation(kf_a, kf_b, CAM)
    reg_err = np.abs(reg.transformation - T).max()
    step = np.identity(4)
    step[:3, :3], step[:3, 3] = ref.se3_exp(np.array([0.0, 0.0, 0.05, 0, 0, 0]))[0], [0.5, 0.0, 0.0]
    truth = {}
    a10 = np.identity(4)
    for k in range(20):
        truth[(0, k)] = np.linalg.matrix_power(step, k)
    a10 = truth[(0, 10)]
    b10 = a10 @ np.linalg.inv(T)                            # T = pose(to)^-1 pose(from): "from" is (0, 10), "to" is (1, 10)
    for k in range(20):
        truth[(1, k)] = b10 @ np.linalg.matrix_power(step, k - 10) if k >= 10 else b10 @ np.linalg.inv(np.linalg.matrix_power(step, 10 - k))
    off = np.identity(4)
    off[:3, :3], off[:3, 3] = ref.se3_exp(np.array([0.0, 0.15, 0.0, 0, 0, 0]))[0], [0.8, -0.3, 0.2]
    values = {k: (v if k[0] == 0 else off @ v) for k, v in truth.items()}
    edges = [((r, k), (r, k + 1), step, pg.DEFAULT_NOISE_STD) for r in (0, 1) for k in range(19)]
    edges.append(reg.to_edge((0, 10), (1, 10)))
    res = pg.optimize(values, edges)
    err = max(np.abs(res.poses[k] - truth[k]).max() for k in truth)
    print("registration error %.3g, largest pose error after optimize %.3g" % (reg_err, err))
    # a pose of the second chain is b10' . step^(k - 10): an entry of the closure's rotation error e moves a point 5 m down the
    # chain (10 steps of 0.5 m) by up to 5 e in each of two other axes, on top of the closure's own translation error e;
    # 1e-6 for the optimiser's stopping rule (abs_tol 1e-5 on a cost weighted by 1 / sigma^2)
    assert err <= reg_err * (1.0 + 2 * 5.0) + 1e-6


def test_register_scratch_is_carved_afresh_for_every_batch():
    """One stream, so one scratch block: a pair of 38 keypoints, then three larger pairs with an empty keyframe among them,
    then the small pair again.  Both small results equal, bit for bit, the one computed before anything else here."""
    import torch

    def kf(seed, landmarks, distractors):
        a, b = ref.keyframe_pair(seed, landmarks=landmarks, distractors=distractors)[:2]
        return vr.Keyframe(*a), vr.Keyframe(*b)

    none = vr.Keyframe(np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 32), np.uint8))
    small, large = [kf(90, 30, 8)], [kf(91, 300, 100), (none, kf(92, 5, 0)[1]), kf(93, 257, 43)]
    first = vr.register_pairs(small, CAM, min_inliers=8)[0]
    with torch.cuda.stream(torch.cuda.Stream()):
        runs = [vr.register_pairs(p, CAM, min_inliers=8) for p in (small, large, small)]
    assert first.status == 0 and same(runs[0][0], first) and same(runs[2][0], first)
    assert [g.status for g in runs[1]] == [0, 2, 0]
    for g, w in zip(runs[1], vr.register_pairs(large, CAM, min_inliers=8)):
        assert same(g, w)
