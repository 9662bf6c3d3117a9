"""CPU: the float64 restatement of open3d's ICP loop (tests/icp_reference.py) does what the GPU tests rely on, and
cslam_amd.lidar_pr.icp_utils has no CPU path."""
import ctypes
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

import icp_reference as ref
from conftest import ROOT
from cslam_amd import _lib

VOXEL = 0.5
SEEDS = (100, 101, 102, 103, 104, 105)
# the inputs the GPU suite compares iteration counts on (tests/test_icp_gpu.py)
GPU_STAGE_SEED = 103          # one stage at the voxel radius from the rounded yaw, 9 000 raw points
GPU_E2E_SEED = 0              # the three stages from ScanContext's yaw, 60 000 raw points


@pytest.fixture(scope="module")
def scenes():
    return {s: ref.street_scene(s, 9000, VOXEL) for s in SEEDS}


@pytest.fixture(scope="module")
def staged(scenes):
    return {s: ref.register_staged(src, dst, VOXEL, ref.yaw_init(ref.seed_yaw(yaw)))
            for s, (src, dst, _, yaw) in scenes.items()}


def errors(T, T_true):
    return ref.rotation_error_deg(T[:3, :3], T_true[:3, :3]), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


@pytest.mark.parametrize("seed", SEEDS)
def test_staged_restatement_recovers_the_ground_truth(scenes, staged, seed):
    T_true = scenes[seed][2]
    rot, tr = errors(staged[seed][-1].transformation, T_true)
    print("seed %d: rotation error %.4f deg, translation error %.4f m, fitness %.4f, iterations %s"
          % (seed, rot, tr, staged[seed][-1].fitness, [s.iterations for s in staged[seed]]))
    assert rot <= 0.1 and tr <= VOXEL / 5


@pytest.mark.parametrize("seed", SEEDS)
def test_single_stage_from_identity_fails(scenes, seed):
    """Why the yaw seed and the coarse stages exist: the reference's refinement alone, started at the identity, ends in
    a wrong alignment whose fitness is still far from zero."""
    src, dst, T_true, yaw = scenes[seed]
    r = ref.registration_icp(src, dst, VOXEL, np.identity(4), 100)
    rot, tr = errors(r.transformation, T_true)
    print("seed %d: fitness %.3f, rotation error %.1f deg (yaw %.1f)" % (seed, r.fitness, rot, yaw))
    assert r.fitness < 0.7
    assert rot > 5.0


def test_brute_force_and_kdtree_agree(scenes):
    src, dst, T_true, yaw = scenes[100]
    for T in (np.identity(4), ref.yaw_init(ref.seed_yaw(yaw)), T_true):
        p = ref.apply_T(T, src)[:700]
        ib, db = ref.nn_brute(p, dst)
        ik, dk = ref.nn_kdtree(p, cKDTree(dst))
        assert np.array_equal(ib, ik) and np.array_equal(db, dk)
    small_src, small_dst = src[:300], dst[:400]
    a = ref.registration_icp(small_src, small_dst, 4 * VOXEL, ref.yaw_init(ref.seed_yaw(yaw)), 20, brute=True)
    b = ref.registration_icp(small_src, small_dst, 4 * VOXEL, ref.yaw_init(ref.seed_yaw(yaw)), 20, brute=False)
    assert a.iterations == b.iterations and np.array_equal(a.correspondence_set, b.correspondence_set)
    assert np.array_equal(a.transformation, b.transformation)


def test_input_condition_of_the_gpu_comparisons(scenes, staged):
    """The GPU tests demand equal iteration counts.  That is a fair demand only where the stopping decisions do not hang
    on the last bits: at the stopping round and the round before it both deltas stay 1e-9 or more away from the 1e-6
    threshold (10^4 x the 4e-14 that a different summation order moves the transform by)."""
    margins = {}
    for seed in SEEDS:
        for k, stage in enumerate(staged[seed]):
            margins["staged seed %d stage %d" % (seed, k)] = ref.stop_margin(stage.history)
    src, dst, _, yaw = scenes[GPU_STAGE_SEED]
    one = ref.registration_icp(src, dst, VOXEL, ref.yaw_init(ref.seed_yaw(yaw)), 100)
    assert 3 < one.iterations < 100
    margins["one stage seed %d" % GPU_STAGE_SEED] = ref.stop_margin(one.history)
    margins["one stage seed %d capped at 3" % GPU_STAGE_SEED] = ref.stop_margin(one.history[:4])
    # the end-to-end case: yaw as this library's ScanContext reports it (the CPU oracle is what the kernels are pinned to)
    from oracle import pyoracle
    src, dst, T_true, yaw = ref.street_scene(GPU_E2E_SEED, 60000, VOXEL)
    sc_src = pyoracle.ptcloud2sc(src).reshape(1, 20, 60)
    sc_dst = pyoracle.ptcloud2sc(dst).reshape(1, 20, 60)
    found = pyoracle.sc_search(sc_dst, sc_src, 10)
    assert found["best_idx"][0] == 0
    yaw_diff = float(found["best_yaw"][0]) * ref.SECTOR_DEG
    assert abs((360.0 - yaw_diff) - yaw) <= ref.SECTOR_DEG, "ScanContext's yaw is more than a sector off: scene too symmetric"
    from cslam_amd.lidar_pr.icp_utils import yaw_seed
    e2e = ref.register_staged(src, dst, VOXEL, yaw_seed(yaw_diff))
    rot, tr = errors(e2e[-1].transformation, T_true)
    assert rot <= 0.1 and tr <= 0.1
    for k, stage in enumerate(e2e):
        margins["end to end seed %d stage %d" % (GPU_E2E_SEED, k)] = ref.stop_margin(stage.history)
    for name, m in margins.items():
        print("%-36s margin %.2e" % (name, m))
    assert min(margins.values()) >= 1e-9, min(margins, key=margins.get)


def test_voxel_average_rule():
    pts = np.array([[0.0, 0.0, 0.0], [0.2, 0.1, 0.0], [0.3, 0.3, 0.0], [1.0, 1.0, 1.0], [np.nan, 0.0, 0.0]])
    out = ref.voxel_average(pts, 0.5)               # origin -0.25: [-0.25, 0.25) holds the first two, then 0.3, then 1.0
    assert out.shape == (3, 3)
    assert np.allclose(out[0], [0.1, 0.05, 0.0]) and np.allclose(out[1], [0.3, 0.3, 0.0]) and np.allclose(out[2], 1.0)


def _no_gpu():
    n = ctypes.c_int(0)
    return _lib.load().cslam_device_count(ctypes.byref(n)) != 0 or n.value == 0


def test_module_imports_without_a_gpu_and_helpers_work():
    from cslam_amd.lidar_pr import icp_utils
    assert icp_utils.DEFAULT_STAGES == ((4.0, 30), (2.0, 30), (1.0, 100)) == ref.DEFAULT_STAGES
    kernel = open(os.path.join(ROOT, "cslam_amd", "csrc", "icp.hip")).read()
    assert "#define ICP_CHUNK %d " % icp_utils.ICP_CHUNK in kernel      # the GPU tests size their targets around it
    assert "#define ICP_MAX_LANES %d " % icp_utils.ICP_MAX_LANES in kernel
    R = Rotation.from_euler("zyx", [40.0, -20.0, 170.0], degrees=True).as_matrix()
    T = icp_utils.Rt2T(R, [1.0, 2.0, 3.0])
    assert T.shape == (4, 4) and np.array_equal(T[:3, :3], R) and list(T[:, 3]) == [1.0, 2.0, 3.0, 1.0]
    rng = np.random.default_rng(3)
    for quat in np.concatenate([rng.standard_normal((20, 4)), np.eye(4), -np.eye(4)]):
        Rm = Rotation.from_quat(quat).as_matrix()
        msg = icp_utils.to_transform_msg([0.5, -1.5, 2.5], Rm)
        q = np.array([msg.rotation.x, msg.rotation.y, msg.rotation.z, msg.rotation.w])
        assert np.abs(Rotation.from_quat(q).as_matrix() - Rm).max() < 1e-14 and abs(np.linalg.norm(q) - 1) < 1e-14
        assert (msg.translation.x, msg.translation.y, msg.translation.z) == (0.5, -1.5, 2.5)
    # the seed is Rz(-yaw): a source that has to turn by +42 degrees matches at a yaw shift of 318
    assert np.abs(icp_utils.yaw_seed(318.0) - ref.yaw_init(42.0)).max() < 1e-15
    assert np.array_equal(icp_utils.yaw_seed(None), np.identity(4))


@pytest.mark.skipif(not _no_gpu(), reason="GPU present: covered by the -m gpu suite")
def test_registration_fails_loudly_without_gpu():
    from cslam_amd.lidar_pr import icp_utils
    pts = np.random.default_rng(0).standard_normal((50, 3))
    with pytest.raises(_lib.CslamHipError):
        icp_utils.registration_icp(pts, pts, 0.5)
    with pytest.raises(_lib.CslamHipError):
        icp_utils.register_pairs([(pts, pts)], 0.5)
    with pytest.raises(_lib.CslamHipError):
        icp_utils.compute_transform(pts, pts, 0.5, 10, init_yaw_deg=12.0)
    with pytest.raises(_lib.CslamHipError):
        icp_utils.solve_icp(pts, pts, 0.5, 10)
