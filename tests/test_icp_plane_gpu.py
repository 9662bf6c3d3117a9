"""GPU: the point-to-plane estimator of the batched ICP (csrc/icp.hip + csrc/plane.h through cslam_amd.lidar_pr.icp_utils,
`estimation="point_to_plane"`) against the float64 restatement of tests/icp_plane_reference.py.  The shapes are the smallest
at which the kernels can still go wrong: fewer correspondences than unknowns, a partial wave, one block, three blocks, a
target of one LDS chunk and a point.  tests/test_icp_plane_cpu.py checks that the iteration counts and correspondence sets
compared here do not hang on the last bits."""
import ctypes as C

import numpy as np
import pytest

import icp_plane_reference as pref
import icp_reference as ref
from test_icp_plane_cpu import E2E_SEED, GPU_CASES, SIZES, VOXEL, whole_case

pytestmark = pytest.mark.gpu

PLANE = "point_to_plane"
FAR_C = np.array([2.0 ** 17, -2.0 ** 16, 1024.0])


@pytest.fixture(scope="module")
def u():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils


@pytest.fixture(scope="module")
def whole():
    """Per case of GPU_CASES: (src, dst, the restatement's normals, init, the restatement's stages), computed once."""
    return {name: whole_case(seed, n_raw, stages) for name, seed, n_raw, stages in GPU_CASES}


def staged(u, src, dst, normals, init, stages):
    """The stages back to back on given normals: `registration_icp` from the previous stage's transform."""
    out, T = None, init
    for mult, iters in stages:
        out = u.registration_icp(src, dst, mult * VOXEL, T, max_iteration=iters, estimation=PLANE, target_normals=normals)
        T = out.transformation
    return out


def check_against(got, want, what):
    dT = np.abs(got.transformation - want.transformation).max()
    print("%s: iterations %d (restatement %d), correspondences %d, max |T - T_ref| = %.3e, d fitness %.1e, d rmse %.1e"
          % (what, got.iterations, want.iterations, got.correspondences, dT, abs(got.fitness - want.fitness),
             abs(got.inlier_rmse - want.inlier_rmse)))
    assert got.iterations == want.iterations
    assert got.correspondences == len(want.correspondence_set) == len(got.correspondence_set)
    assert np.array_equal(got.correspondence_set, want.correspondence_set)
    assert dT <= 1e-9
    assert abs(got.fitness - want.fitness) <= 1e-12 and abs(got.inlier_rmse - want.inlier_rmse) <= 1e-12
    assert np.array_equal(got.transformation[3], [0.0, 0.0, 0.0, 1.0])


# ---- one update with known correspondences -------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", SIZES + (1025,))
def test_one_update_equals_the_restatement(u, kept):
    """A lattice pair with planted unit normals, max_iteration = 1; in one batched call the source of exactly `kept` rows
    (every row has a partner) and the one with a third more rows that have none.  1025 = a target of ICP_CHUNK + 1 points."""
    assert kept != 1025 or kept == u.ICP_CHUNK + 1
    src, dst, partner = ref.lattice_pair(kept, 0, noise=0.02)
    normals = pref.planted_normals(kept, kept)
    assert len(dst) == kept
    pairs = [(src[partner >= 0], dst), (src, dst)]
    got = u.registration_icp_pairs(pairs, ref.LATTICE_RADIUS, max_iteration=1, estimation=PLANE, target_normals=normals)
    for (s, d), g in zip(pairs, got):
        want = pref.registration_icp(s, d, normals, ref.LATTICE_RADIUS, None, 1, brute=True)
        assert len(want.dets) == 1 and (want.dets[0] == 0.0 if kept < 6 else abs(want.dets[0]) >= 1.0)
        check_against(g, want, "%d of %d source rows kept" % (kept, len(s)))
        assert g.iterations == 1 and g.correspondences == kept
        if kept < 6:
            assert np.array_equal(g.transformation, np.identity(4))                   # fewer correspondences than unknowns
        else:
            assert not np.array_equal(g.transformation, np.identity(4))
    alone = u.registration_icp(src, dst, ref.LATTICE_RADIUS, max_iteration=1, estimation=PLANE, target_normals=normals)
    assert alone.transformation.tobytes() == got[1].transformation.tobytes()


# ---- whole registrations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in GPU_CASES])
def test_registration_on_the_restatements_normals(u, whole, name):
    src, dst, normals, init, want = whole[name]
    stages = dict((n, s) for n, _, _, s in GPU_CASES)[name]
    check_against(staged(u, src, dst, normals, init, stages), want[-1], name + ", normals of fpfh_reference")


@pytest.mark.parametrize("name", [c[0] for c in GPU_CASES])
def test_registration_on_the_normals_of_the_gpu_chain(u, whole, name):
    """`register_pairs` estimates the targets' normals on the device (2 voxels, 30 neighbours); the restatement runs on
    fpfh_reference's.  A normal's sign does not enter the update."""
    src, dst, normals, init, want = whole[name]
    seed, n_raw, stages = [(s, r, st) for n, s, r, st in GPU_CASES if n == name][0]
    yaw = ref.street_scene(seed, n_raw, VOXEL)[3]
    assert np.abs(u.yaw_seed(360.0 - ref.seed_yaw(yaw)) - init).max() <= 1e-14
    gpu_normals = u.estimate_normals(dst, 2.0 * VOXEL, 30)
    print("normals of the GPU chain against fpfh_reference: max |n - n_ref| = %.2e" % np.abs(gpu_normals - normals).max())
    got = u.register_pairs([(src, dst)], VOXEL, 360.0 - ref.seed_yaw(yaw), stages, correspondence_sets=True, estimation=PLANE)[0]
    # the seed of register_pairs is Rz(-(360 - yaw)), equal to `init` to the last bit or two: the restatement starts from it
    again = pref.register_staged(src, dst, normals, VOXEL, u.yaw_seed(360.0 - ref.seed_yaw(yaw)), stages)
    assert [s.iterations for s in again] == [s.iterations for s in want]
    check_against(got, again[-1], name + ", normals of the GPU chain")


def test_iteration_cap_and_evaluation_only(u, whole):
    src, dst, normals, init, _ = whole["scene 103, one stage"]
    want = pref.registration_icp(src, dst, normals, VOXEL, init, 3)
    got = u.registration_icp(src, dst, VOXEL, init, max_iteration=3, estimation=PLANE, target_normals=normals)
    assert want.iterations == 3 and got.iterations == 3
    assert np.array_equal(got.correspondence_set, want.correspondence_set)
    assert np.abs(got.transformation - want.transformation).max() <= 1e-9
    assert abs(got.fitness - want.fitness) <= 1e-12 and abs(got.inlier_rmse - want.inlier_rmse) <= 1e-12
    zero = u.registration_icp(src, dst, VOXEL, init, max_iteration=0, estimation=PLANE, target_normals=normals)
    assert zero.iterations == 0 and np.array_equal(zero.transformation, init)
    assert abs(zero.fitness - want.history[0][0]) <= 1e-12 and abs(zero.inlier_rmse - want.history[0][1]) <= 1e-12


def raw(results):
    return b"".join(r.transformation.tobytes() + np.array([r.fitness, r.inlier_rmse]).tobytes()
                    + bytes([r.iterations]) + r.correspondences.to_bytes(4, "little") for r in results)


def test_batch_equals_singles_bit_for_bit(u, whole):
    """Four pairs of different sizes in one call; the identical pair stops after one update, the street pairs run on."""
    a_src, a_dst, _, a_init, _ = whole["scene 21, default stages"]
    b_src, b_dst, _, b_yaw = ref.street_scene(103, 2400, VOXEL)
    same = a_src[:600]
    l_src, l_dst, _ = ref.lattice_pair(65, 0, noise=0.02)              # no neighbours within 2 voxels: normals (0, 0, 1)
    pairs = [(same, same), (a_src, a_dst), (b_src[:700], b_dst), (l_src, l_dst)]
    a_yaw = ref.street_scene(21, 2400, VOXEL)[3]
    yaws = [0.0, 360.0 - ref.seed_yaw(a_yaw), 360.0 - ref.seed_yaw(b_yaw), None]
    stages = ((4.0, 30), (1.0, 30))
    batch = u.register_pairs(pairs, VOXEL, yaws, stages, estimation=PLANE)
    print("iterations of the last stage: %s, fitness %s" % ([r.iterations for r in batch], ["%.3f" % r.fitness for r in batch]))
    assert batch[0].iterations == 1 and batch[0].fitness == 1.0 and batch[0].inlier_rmse < 1e-12
    assert batch[1].iterations > 1 and 0.5 < batch[1].fitness < 1.0
    assert len({len(s) for s, _ in pairs}) == 4 and len({len(d) for _, d in pairs}) == 4
    singles = [u.register_pairs([p], VOXEL, [y], stages, estimation=PLANE)[0] for p, y in zip(pairs, yaws)]
    for k, (b, s) in enumerate(zip(batch, singles)):
        assert raw([b]) == raw([s]), "pair %d differs between the batch and alone" % k
    assert raw(u.register_pairs(pairs[::-1], VOXEL, yaws[::-1], stages, estimation=PLANE)[::-1]) == raw(batch)


# ---- degenerate pairs ------------------------------------------------------------------------------------------------
def test_ground_only_pair_is_left_where_it_is(u):
    """All normals exactly (0, 0, 1): A has a zero row, every update is the identity and the loop stops after one."""
    rng = np.random.default_rng(14)
    src = np.concatenate([rng.uniform(-10, 10, (700, 2)), np.zeros((700, 1))], axis=1)
    init = ref.yaw_init(30.0)
    dst = ref.apply_T(init, src)[rng.permutation(700)] + np.array([0.0, 0.0, 0.125])
    normals = np.tile([0.0, 0.0, 1.0], (700, 1))
    r = u.registration_icp(src, dst, VOXEL, init, estimation=PLANE, target_normals=normals)
    assert np.array_equal(r.transformation, init) and r.iterations == 1
    assert r.correspondences == 700 and r.fitness == 1.0 and abs(r.inlier_rmse - 0.125) <= 1e-12
    want = pref.registration_icp(src, dst, normals, VOXEL, init)
    assert want.iterations == 1 and want.dets == [0.0] and np.array_equal(want.transformation, init)
    point = u.registration_icp(src, dst, VOXEL, init)                   # point-to-point closes the gap
    assert point.inlier_rmse < 1e-9


def test_no_correspondences(u):
    rng = np.random.default_rng(9)
    src = rng.uniform(-5, 5, (700, 3))
    dst = src + np.array([100.0, 0.0, 0.0])
    init = ref.yaw_init(30.0)
    r = u.registration_icp(src, dst, VOXEL, init, estimation=PLANE, target_normals=pref.planted_normals(700, 3))
    assert np.array_equal(r.transformation, init)
    assert (r.fitness, r.inlier_rmse, r.correspondences, r.iterations) == (0.0, 0.0, 0, 1)
    assert r.correspondence_set.shape == (0, 2)
    transform, success = u.compute_transform(src, dst, VOXEL, 0, init_yaw_deg=330.0, estimation=PLANE)
    assert not success and success.fitness == 0.0 and success.inlier_rmse == 0.0 and success.iterations == 1
    assert np.abs(success.transformation - init).max() < 1e-15


def test_dropped_target_rows_take_their_normals_along(u, whole):
    src, dst, normals, init, _ = whole["scene 21, default stages"]
    want = u.registration_icp(src, dst, 4 * VOXEL, init, max_iteration=5, estimation=PLANE, target_normals=normals)
    real = np.ones(len(dst) + 3, dtype=bool)
    real[[3, 4, 502]] = False
    holes, padded = np.full((len(real), 3), np.nan), np.tile([1.0, 0.0, 0.0], (len(real), 1))
    holes[real], padded[real] = dst, normals
    holes[502, 1] = 0.0                                                 # one non-finite coordinate is enough
    got = u.registration_icp(src, holes, 4 * VOXEL, init, max_iteration=5, estimation=PLANE, target_normals=padded)
    assert raw([got]) == raw([want]) and np.array_equal(got.correspondence_set, want.correspondence_set)


# ---- far from the origin -----------------------------------------------------------------------------------------------
def test_far_frame(u, whole):
    """The scene-21 pair moved by (2^17, -2^16, 1024) m: the iteration count of the run at the origin, and the moved source
    points, shifted back, within 256 ulp of the largest coordinate of the origin run's."""
    src, dst, normals, init, _ = whole["scene 21, default stages"]
    near = staged(u, src, dst, normals, init, ref.DEFAULT_STAGES)
    far_init = ref.Rt2T(init[:3, :3], FAR_C - init[:3, :3] @ FAR_C)
    far = staged(u, src + FAR_C, dst + FAR_C, normals, far_init, ref.DEFAULT_STAGES)
    moved_near = ref.moved_ld(near.transformation, src)
    moved_far = ref.moved_ld(far.transformation, src + FAR_C) - FAR_C.astype(ref.LD)
    ulps = float(np.abs(moved_far - moved_near).max()) / ref.coord_ulp(src + FAR_C, dst + FAR_C)
    print("far frame: iterations %d (origin %d), moved points %.2f ulp of the largest coordinate from the origin run's"
          % (far.iterations, near.iterations, ulps))
    assert far.iterations == near.iterations and far.correspondences == near.correspondences
    assert ulps <= ref.ULP_BOUND


# ---- the default estimator is untouched ----------------------------------------------------------------------------------
def test_point_to_point_by_name_is_the_default(u, whole):
    src, dst, _, init, _ = whole["scene 21, default stages"]
    yaw = 360.0 - ref.seed_yaw(ref.street_scene(21, 2400, VOXEL)[3])
    pairs = [(src, dst), (src[:300], dst[:500])]
    a = u.registration_icp_pairs(pairs, VOXEL, [init, init], max_iteration=8)
    b = u.registration_icp_pairs(pairs, VOXEL, [init, init], max_iteration=8, estimation="point_to_point")
    assert raw(a) == raw(b) and all(np.array_equal(x.correspondence_set, y.correspondence_set) for x, y in zip(a, b))
    assert raw(u.register_pairs(pairs, VOXEL, yaw)) == raw(u.register_pairs(pairs, VOXEL, yaw, estimation="point_to_point"))
    c = u.registration_icp_pairs(pairs[:1], VOXEL, [init], max_iteration=8, estimation=PLANE,
                                 target_normals=whole["scene 21, default stages"][2])
    assert raw(c) != raw(a[:1])                                         # and the other estimator is another one


# ---- end to end ------------------------------------------------------------------------------------------------------
def pose_errors(T, T_true):
    return ref.rotation_error_deg(T[:3, :3], T_true[:3, :3]), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


def test_compute_transform_end_to_end(u):
    """street_scene(2) by both coarse alignments.  The planted pose is recovered to within twice the error the restatement
    makes from the same start on the same scene."""
    src, dst, T_true, yaw = ref.street_scene(E2E_SEED, 9000, VOXEL)
    normals = pref.reference_normals(dst, VOXEL)
    yaw_diff = 360.0 - ref.seed_yaw(yaw)
    # coarse="yaw"
    msg, ok = u.compute_transform(src, dst, VOXEL, 50, init_yaw_deg=yaw_diff, min_fitness=0.5, estimation=PLANE)
    pairs = u.register_pairs([(src, dst)], VOXEL, yaw_diff, estimation=PLANE)[0]
    assert ok and ok.transformation.tobytes() == pairs.transformation.tobytes()
    assert (ok.fitness, ok.inlier_rmse, ok.correspondences, ok.iterations) == (pairs.fitness, pairs.inlier_rmse,
                                                                               pairs.correspondences, pairs.iterations)
    assert (msg.translation.x, msg.translation.y, msg.translation.z) == tuple(float(v) for v in ok.transformation[:3, 3])
    valid, t, R = u.solve_icp(src, dst, VOXEL, 50, init_yaw_deg=yaw_diff, estimation=PLANE)
    assert valid and np.array_equal(ref.Rt2T(R, t), ok.transformation)
    want = pref.register_staged(src, dst, normals, VOXEL, u.yaw_seed(yaw_diff))[-1]
    got_err, want_err = pose_errors(ok.transformation, T_true), pose_errors(want.transformation, T_true)
    print("coarse=yaw: %.4f deg %.4f m (restatement %.4f deg %.4f m), last stage %d updates (restatement %d)"
          % (*got_err, *want_err, ok.iterations, want.iterations))
    assert got_err[0] <= 2.0 * want_err[0] and got_err[1] <= 2.0 * want_err[1]
    point = u.compute_transform(src, dst, VOXEL, 50, init_yaw_deg=yaw_diff, min_fitness=0.5)[1]
    assert point.transformation.tobytes() != ok.transformation.tobytes()
    # coarse="teaser"
    msg, ok = u.compute_transform(src, dst, VOXEL, 50, coarse="teaser", estimation=PLANE)
    valid, t, R = u.solve_teaser_pairs([(src, dst)], VOXEL, 50, estimation=PLANE)[0]
    assert ok and valid and ok.transformation.tobytes() == valid.transformation.tobytes()
    assert np.array_equal(ref.Rt2T(R, t), ok.transformation)
    assert (msg.translation.x, msg.translation.y, msg.translation.z) == tuple(float(v) for v in t)
    v2, t2, R2 = u.solve_teaser(src, dst, VOXEL, 50, estimation=PLANE)
    v3, t3, R3 = u.solve_icp(src, dst, VOXEL, 50, coarse="teaser", estimation=PLANE)
    assert np.array_equal(t2, t) and np.array_equal(R2, R) and np.array_equal(t3, t) and np.array_equal(R3, R)
    point = u.compute_transform(src, dst, VOXEL, 50, coarse="teaser")[1]             # the coarse fit is untouched
    assert point and np.array_equal(point.clique, ok.clique)
    assert (point.clique_size, point.certified, point.status, point.matches, point.nodes) == (
        ok.clique_size, ok.certified, ok.status, ok.matches, ok.nodes)
    assert point.coarse.tobytes() == ok.coarse.tobytes() and point.transformation.tobytes() != ok.transformation.tobytes()
    want = pref.registration_icp(src, dst, normals, VOXEL, ok.coarse, 100)
    assert 1 < want.iterations < 100 and ref.stop_margin(want.history) >= 1e-9 and min(abs(d) for d in want.dets) >= 1.0
    got_err, want_err = pose_errors(ok.transformation, T_true), pose_errors(want.transformation, T_true)
    print("coarse=teaser: %.4f deg %.4f m (restatement %.4f deg %.4f m), %d updates (restatement %d), max |T - T_ref| = %.2e"
          % (*got_err, *want_err, ok.iterations, want.iterations, np.abs(ok.transformation - want.transformation).max()))
    assert got_err[0] <= 2.0 * want_err[0] and got_err[1] <= 2.0 * want_err[1]
    assert ok.iterations == want.iterations


# ---- typed errors through the C ABI --------------------------------------------------------------------------------------
def test_typed_errors(u):
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(12)
    pts = rng.standard_normal((40, 3))
    dev = torch.device("cuda", 0)
    t_pts = torch.from_numpy(pts).to(dev)
    t_nrm = torch.from_numpy(pref.planted_normals(40, 2)).to(dev)
    good = torch.tensor([0, 20, 40], dtype=torch.int64, device=dev)
    T = torch.full((2, 16), 77.0, dtype=torch.float64, device=dev)
    stats = torch.full((2, 4), 77.0, dtype=torch.float64, device=dev)
    dist, iters = (C.c_double * 1)(1.0), (C.c_int * 1)(5)

    def call(so, do, nrm, n=2, n_stages=1, out=T.data_ptr()):
        return lib.cslam_icp_register_plane_dev(t_pts.data_ptr(), so.data_ptr(), t_pts.data_ptr(), do.data_ptr(), nrm, n, None,
                                                dist, iters, n_stages, 1e-6, 1e-6, out, stats.data_ptr(), None)

    assert call(good, good, None) == -1
    assert b"d_dst_normals" in lib.cslam_last_error()
    for off in ([0, 30, 20], [0, 20, 20], [-1, 20, 40]):
        bad = torch.tensor(off, dtype=torch.int64, device=dev)
        for so, do in ((bad, good), (good, bad)):
            assert call(so, do, t_nrm.data_ptr()) == -1
            assert b"offsets" in lib.cslam_last_error()
    assert call(good, good, t_nrm.data_ptr(), n=0) == -1 and b"n_pairs" in lib.cslam_last_error()
    assert call(good, good, t_nrm.data_ptr(), n_stages=0) == -1 and b"n_stages" in lib.cslam_last_error()
    assert call(good, good, t_nrm.data_ptr(), out=None) == -1
    torch.cuda.synchronize()
    assert int((T != 77.0).sum()) == 0 and int((stats != 77.0).sum()) == 0             # nothing was launched
    assert call(good, good, t_nrm.data_ptr()) == 0
    torch.cuda.synchronize()
    out = T.cpu().numpy().reshape(2, 4, 4)
    assert np.array_equal(out[0], np.identity(4)) and np.array_equal(out[1], np.identity(4))     # a cloud against itself: r = 0
    assert stats.cpu().numpy()[:, 0].tolist() == [1.0, 1.0]
    with pytest.raises(_lib.CslamHipError, match="max_dist"):
        u.registration_icp(pts, pts, 0.0, estimation=PLANE, target_normals=pref.planted_normals(40, 2))
    with pytest.raises(_lib.CslamHipError, match="invalid argument"):
        u.registration_icp(pts, np.full((5, 3), np.nan), 1.0, estimation=PLANE, target_normals=np.zeros((5, 3)))
