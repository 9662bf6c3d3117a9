"""GPU: the batched point-to-point ICP (csrc/icp.hip through cslam_amd.lidar_pr.icp_utils) against the float64
restatement of open3d's loop in tests/icp_reference.py.  The shapes are the smallest at which the kernels can still go
wrong: one point, a partial block, several blocks, targets around the LDS chunk size C, several chunk lanes.
tests/test_icp_cpu.py checks that the iteration counts compared here do not hang on the last bits."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import icp_reference as ref

pytestmark = pytest.mark.gpu

VOXEL = 0.5


@pytest.fixture(scope="module")
def icp():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils


@pytest.fixture(scope="module")
def rigid():
    rng = np.random.default_rng(11)
    return ref.Rt2T(Rotation.from_rotvec([0.4, -0.9, 0.7]).as_matrix(), rng.uniform(-0.5, 0.5, 3))


@pytest.fixture(scope="module")
def clouds(icp, rigid):
    """Random normal clouds and their float64 brute-force answers, computed once: key (ns, nd, moved)."""
    rng = np.random.default_rng(7)
    ch = icp.ICP_CHUNK
    srcs = {ns: rng.standard_normal((ns, 3)) for ns in (1, 257, 1000)}
    dsts = {nd: rng.standard_normal((nd, 3)) for nd in (1, 63, ch - 1, ch, ch + 1, 2 * ch + 3)}
    moved = {ns: ref.apply_T_fma(rigid, s) for ns, s in srcs.items()}
    out = {}
    for ns, s in srcs.items():
        for nd, d in dsts.items():
            for mv in (False, True):
                idx, d2 = ref.nn_brute(moved[ns] if mv else s, d)
                out[(ns, nd, mv)] = (s, d, idx, d2)
    return out


def check_correspondences(got, want_idx, want_d2, radius):
    idx, d2 = got
    keep = want_d2 <= radius * radius
    assert idx.dtype == np.int32 and np.array_equal(idx, np.where(keep, want_idx, -1))
    rel = np.abs(d2 - want_d2) / want_d2
    assert rel.max() <= 1e-14, rel.max()


@pytest.mark.parametrize("moved", [False, True], ids=["identity", "rigid"])
def test_correspondences_equal_brute_force(icp, clouds, rigid, moved):
    cases = [(k, v) for k, v in clouds.items() if k[2] == moved]
    for (ns, nd, _), (s, d, idx, d2) in cases:                        # each pair alone, about half the points kept
        radius = float(np.sqrt(np.median(d2))) if ns > 1 else float(np.sqrt(d2[0])) * 1.5
        got = icp.nearest_correspondences([(s, d)], radius, [rigid] if moved else None)[0]
        check_correspondences(got, idx, d2, radius)
        if ns > 1:
            assert 0.3 < np.mean(got[0] >= 0) < 0.7
    radius = float(np.sqrt(np.median(np.concatenate([v[3] for _, v in cases]))))       # and all of them as one batch
    got = icp.nearest_correspondences([(v[0], v[1]) for _, v in cases], radius, [rigid] * len(cases) if moved else None)
    for g, (_, (s, d, idx, d2)) in zip(got, cases):
        check_correspondences(g, idx, d2, radius)


def test_ties_go_to_the_lower_index(icp):
    rng = np.random.default_rng(8)
    src = rng.standard_normal((300, 3))
    q = rng.standard_normal((icp.ICP_CHUNK + 5, 3))
    want, _ = ref.nn_brute(src, q)
    idx, _ = icp.nearest_correspondences([(src, np.repeat(q, 2, axis=0))], 100.0)[0]      # duplicates side by side
    assert np.array_equal(idx, 2 * want)
    idx, _ = icp.nearest_correspondences([(src, np.concatenate([q, q]))], 100.0)[0]      # duplicates in another chunk
    assert np.array_equal(idx, want)
    idx, _ = icp.nearest_correspondences([(src, np.concatenate([q, q, q[:9]]))], 100.0)[0]
    assert np.array_equal(idx, want)


def test_more_chunks_than_chunk_lanes(icp):
    """A target of more than ICP_MAX_LANES chunks: every lane walks several chunks, and the duplicate of each point sits
    in a later chunk of another (or the same) lane.  Alone and in a batch with a small pair."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(13)
    src = rng.standard_normal((70, 3))
    q = rng.standard_normal((icp.ICP_MAX_LANES * icp.ICP_CHUNK + 519, 3))
    want, want_d2 = ref.nn_kdtree(src, cKDTree(q))
    big = np.concatenate([q, q])
    radius = float(np.sqrt(np.median(want_d2)))
    small = (src[:5], q[:40])
    small_want = ref.nn_brute(*small)
    for pairs in ([(src, big)], [small, (src, big), small]):
        got = icp.nearest_correspondences(pairs, radius)
        check_correspondences(got[len(pairs) // 2], want, want_d2, radius)
        if len(pairs) > 1:
            check_correspondences(got[0], *small_want, radius)
            check_correspondences(got[2], *small_want, radius)


@pytest.fixture(scope="module")
def scene103():
    src, dst, T_true, yaw = ref.street_scene(103, 9000, VOXEL)
    init = ref.yaw_init(ref.seed_yaw(yaw))
    return src, dst, init, ref.registration_icp(src, dst, VOXEL, init, 100)


def test_one_stage_equals_the_restatement(icp, scene103):
    src, dst, init, want = scene103
    got = icp.registration_icp(src, dst, VOXEL, init, max_iteration=100)
    dT = np.abs(got.transformation - want.transformation).max()
    print("iterations %d (restatement %d), correspondences %d, max |T - T_ref| = %.3e, d fitness %.1e, d rmse %.1e"
          % (got.iterations, want.iterations, got.correspondences, dT, abs(got.fitness - want.fitness),
             abs(got.inlier_rmse - want.inlier_rmse)))
    assert 3 < want.iterations < 100
    assert got.iterations == want.iterations
    assert got.correspondences == len(want.correspondence_set) == len(got.correspondence_set)
    assert np.array_equal(got.correspondence_set, want.correspondence_set)
    assert dT <= 1e-9
    assert abs(got.fitness - want.fitness) <= 1e-12 and abs(got.inlier_rmse - want.inlier_rmse) <= 1e-12
    assert np.array_equal(got.transformation[3], [0.0, 0.0, 0.0, 1.0])


def test_iteration_cap(icp, scene103):
    src, dst, init, _ = scene103
    want = ref.registration_icp(src, dst, VOXEL, init, 3)
    got = icp.registration_icp(src, dst, VOXEL, init, max_iteration=3)
    assert want.iterations == 3 and got.iterations == 3
    assert np.array_equal(got.correspondence_set, want.correspondence_set)
    assert np.abs(got.transformation - want.transformation).max() <= 1e-9
    assert abs(got.fitness - want.fitness) <= 1e-12 and abs(got.inlier_rmse - want.inlier_rmse) <= 1e-12
    zero = icp.registration_icp(src, dst, VOXEL, init, max_iteration=0)                 # evaluation only
    assert zero.iterations == 0 and np.array_equal(zero.transformation, init)
    assert abs(zero.fitness - want.history[0][0]) <= 1e-12 and abs(zero.inlier_rmse - want.history[0][1]) <= 1e-12


def test_no_correspondences(icp):
    rng = np.random.default_rng(9)
    src = rng.uniform(-5, 5, (700, 3))
    dst = src + np.array([100.0, 0.0, 0.0])
    init = ref.yaw_init(30.0)
    r = icp.registration_icp(src, dst, VOXEL, init)
    assert np.array_equal(r.transformation, init)
    assert (r.fitness, r.inlier_rmse, r.correspondences, r.iterations) == (0.0, 0.0, 0, 1)
    assert r.correspondence_set.shape == (0, 2)
    transform, success = icp.compute_transform(src, dst, VOXEL, 0, init_yaw_deg=330.0)
    assert not success and success.fitness == 0.0 and success.inlier_rmse == 0.0 and success.iterations == 1
    assert np.abs(success.transformation - init).max() < 1e-15
    vals = [transform.translation.x, transform.translation.y, transform.translation.z, transform.rotation.x,
            transform.rotation.y, transform.rotation.z, transform.rotation.w]
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(success.transformation))
    valid, t, R = icp.solve_icp(src, dst, VOXEL, 0)
    assert valid is False and np.array_equal(t, np.zeros(3)) and np.array_equal(R, np.identity(3))


def test_batch_equals_singles_bit_for_bit(icp):
    rng = np.random.default_rng(10)
    a_src, a_dst, _, a_yaw = ref.street_scene(101, 9000, VOXEL)
    b_src, b_dst, _, b_yaw = ref.street_scene(102, 9000, VOXEL)
    same = a_src[:600]
    one_dst = rng.uniform(-1, 1, (50, 3))
    pairs = [(one_dst[7:8] + 0.05, one_dst),                         # a 1-point source
             (same, same),                                           # stops in round 1: nothing to improve
             (a_src, a_dst),                                         # runs to the cap of both stages
             (b_src[:1500], b_dst[:1300]),
             (a_src[:257] + 100.0, a_dst)]                           # no correspondences at all
    yaws = [None, 0.0, 360.0 - ref.seed_yaw(a_yaw), 360.0 - ref.seed_yaw(b_yaw), None]
    stages = ((4.0, 3), (1.0, 2))

    def raw(results):
        return b"".join(r.transformation.tobytes() + np.array([r.fitness, r.inlier_rmse]).tobytes()
                        + bytes([r.iterations]) + r.correspondences.to_bytes(4, "little") for r in results)

    batch = icp.register_pairs(pairs, VOXEL, yaws, stages)
    assert batch[0].correspondences == 1 and batch[0].fitness == 1.0
    assert batch[1].iterations == 1 and batch[1].fitness == 1.0 and batch[1].inlier_rmse < 1e-12
    assert batch[2].iterations == 2 and 0.1 < batch[2].fitness < 1.0
    assert batch[4].correspondences == 0 and batch[4].iterations == 1
    singles = [icp.register_pairs([p], VOXEL, [y], stages)[0] for p, y in zip(pairs, yaws)]
    for k, (b, s) in enumerate(zip(batch, singles)):
        assert raw([b]) == raw([s]), "pair %d differs between the batch and alone" % k
    assert raw(icp.register_pairs(pairs, VOXEL, yaws, stages)) == raw(batch)
    rev = icp.register_pairs(pairs[::-1], VOXEL, yaws[::-1], stages)
    assert raw(rev[::-1]) == raw(batch)


def test_end_to_end_with_scancontext_yaw(icp):
    """Seed 0 of the 60 000-point recipe.  The yaw sign is fixed here: descriptors of dst in the bank, searched with the
    descriptor of src, seed = Rz(-last_yaw_diff_deg)."""
    from cslam_amd.lidar_pr.scancontext import ScanContext
    from cslam_amd.lidar_pr.scancontext_matching import ScanContextMatching
    src, dst, T_true, yaw = ref.street_scene(0, 60000, VOXEL)
    desc_src, desc_dst = ScanContext({}, None).compute_embeddings([src, dst])
    matcher = ScanContextMatching()
    matcher.add_item(desc_dst, 0)
    items, sims = matcher.search(desc_src, 1)
    yaw_diff = matcher.last_yaw_diff_deg
    print("true yaw %.2f, ScanContext yaw shift %.0f (seed %.0f), similarity %.3f" % (yaw, yaw_diff, 360 - yaw_diff, sims[0]))
    assert items == [0]
    assert abs((360.0 - yaw_diff) - yaw) <= ref.SECTOR_DEG, "ScanContext's yaw is more than a sector off"
    transform, success = icp.compute_transform(src, dst, VOXEL, 1000, init_yaw_deg=yaw_diff, min_fitness=0.9)
    T = success.transformation
    rot = ref.rotation_error_deg(T[:3, :3], T_true[:3, :3])
    tr = float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
    want = ref.register_staged(src, dst, VOXEL, icp.yaw_seed(yaw_diff))[-1]
    dT = np.abs(T - want.transformation).max()
    print("rotation error %.4f deg, translation error %.4f m, fitness %.4f, iterations %d (restatement %d), "
          "max |T - T_ref| = %.3e" % (rot, tr, success.fitness, success.iterations, want.iterations, dT))
    assert success and rot <= 0.1 and tr <= 0.1
    assert dT <= 1e-9 and success.iterations == want.iterations
    assert success.correspondences == len(want.correspondence_set)
    assert abs(success.fitness - want.fitness) <= 1e-12 and abs(success.inlier_rmse - want.inlier_rmse) <= 1e-12
    q = Rotation.from_matrix(T[:3, :3]).as_quat()
    got_q = np.array([transform.rotation.x, transform.rotation.y, transform.rotation.z, transform.rotation.w])
    assert min(np.abs(got_q - q).max(), np.abs(got_q + q).max()) < 1e-12
    assert [transform.translation.x, transform.translation.y, transform.translation.z] == list(T[:3, 3])
    _, unseeded = icp.compute_transform(src, dst, VOXEL, 1000, init_yaw_deg=None, min_fitness=0.9)
    print("without the yaw seed: fitness %.4f, correspondences %d" % (unseeded.fitness, unseeded.correspondences))
    assert unseeded.fitness < 0.7 and not unseeded
    assert unseeded.correspondences > 1000                          # the count alone would have accepted it


def test_typed_errors(icp):
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(12)
    pts = rng.standard_normal((40, 3))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.CslamHipError, match="max_dist"):
            icp.registration_icp(pts, pts, bad)
        with pytest.raises(_lib.CslamHipError, match="max_dist"):
            icp.nearest_correspondences([(pts, pts)], bad)
    with pytest.raises(_lib.CslamHipError, match="invalid argument"):
        icp.registration_icp(np.zeros((0, 3)), pts, 1.0)
    with pytest.raises(_lib.CslamHipError, match="invalid argument"):
        icp.registration_icp(pts, np.full((5, 3), np.nan), 1.0)    # every row dropped
    with pytest.raises(_lib.CslamHipError, match="at least one point"):
        icp.register_pairs([(pts, pts), (pts[:0], pts)], 1.0)
    dev = torch.device("cuda", 0)
    t_pts = torch.from_numpy(pts).to(dev)
    good = torch.tensor([0, 20, 40], dtype=torch.int64, device=dev)
    idx = torch.full((40,), 77, dtype=torch.int32, device=dev)
    d2 = torch.full((40,), 77.0, dtype=torch.float64, device=dev)
    T = torch.empty((2, 16), dtype=torch.float64, device=dev)
    stats = torch.empty((2, 4), dtype=torch.float64, device=dev)
    dist = (C.c_double * 1)(1.0)
    iters = (C.c_int * 1)(5)
    for off in ([0, 30, 20], [0, 20, 20], [-1, 20, 40]):
        bad = torch.tensor(off, dtype=torch.int64, device=dev)
        for so, do in ((bad, good), (good, bad)):
            assert lib.cslam_icp_correspondences_dev(t_pts.data_ptr(), so.data_ptr(), t_pts.data_ptr(), do.data_ptr(), 2, None,
                                                     1.0, idx.data_ptr(), d2.data_ptr(), None) == -1
            assert lib.cslam_icp_register_dev(t_pts.data_ptr(), so.data_ptr(), t_pts.data_ptr(), do.data_ptr(), 2, None, dist,
                                              iters, 1, 1e-6, 1e-6, T.data_ptr(), stats.data_ptr(), None) == -1
    args = (t_pts.data_ptr(), good.data_ptr(), t_pts.data_ptr(), good.data_ptr())
    assert lib.cslam_icp_correspondences_dev(*args, 0, None, 1.0, idx.data_ptr(), d2.data_ptr(), None) == -1
    assert lib.cslam_icp_register_dev(*args, 2, None, dist, iters, 0, 1e-6, 1e-6, T.data_ptr(), stats.data_ptr(), None) == -1
    assert lib.cslam_icp_register_dev(*args, 2, None, dist, (C.c_int * 1)(-1), 1, 1e-6, 1e-6, T.data_ptr(), stats.data_ptr(),
                                      None) == -1
    assert lib.cslam_icp_register_dev(*args, 2, None, dist, iters, 1, 1e-6, 1e-6, None, stats.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert int((idx != 77).sum()) == 0 and int((d2 != 77.0).sum()) == 0          # nothing was launched
    assert lib.cslam_icp_correspondences_dev(*args, 2, None, 1.0, idx.data_ptr(), d2.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == list(range(20)) * 2                              # each pair: a cloud against itself


def test_scratch_is_carved_afresh_for_every_batch(icp):
    """One stream, so one scratch block: a pair of a few rows (every piece shorter than 256 bytes), then three larger pairs
    with a one-point member, then the small pair again.  The block keeps what the larger batch wrote and is cut differently
    each time; both small results equal, byte for byte, the one computed before anything else here."""
    import torch
    rng = np.random.default_rng(31)
    T = ref.Rt2T(Rotation.from_rotvec([0.02, -0.03, 0.05]).as_matrix(), np.array([0.1, -0.05, 0.02]))

    def pair(ns, nd):
        src = rng.uniform(-3.0, 3.0, (max(ns, nd), 3))
        return src[:ns], ref.apply_T_fma(T, src)[:nd]

    small, large = [pair(23, 37)], [pair(300, 411), pair(1, 1), pair(257, 500)]
    stages = ((4.0, 3), (1.0, 2))

    def raw(pairs):
        return b"".join(r.transformation.tobytes() + np.array([r.fitness, r.inlier_rmse]).tobytes() + bytes([r.iterations])
                        + r.correspondences.to_bytes(4, "little") for r in icp.register_pairs(pairs, VOXEL, None, stages))

    first = raw(small)
    with torch.cuda.stream(torch.cuda.Stream()):
        runs = [raw(small), raw(large), raw(small)]
    assert runs[0] == first and runs[2] == first
    assert runs[1] == raw(large) and len(runs[1]) == 3 * len(first)
