"""CPU: the argument checks of cslam_voxel_downsample_dev come before anything touches HIP, the down-sampling has no CPU
path, and the facts about `icp_reference.voxel_average` that tests/test_voxel_gpu.py rests on."""
import ctypes as C
import os

import numpy as np
import pytest

import icp_reference as ref
from conftest import ROOT
from cslam_amd import _lib

VOXEL = 0.5


def _no_gpu():
    n = C.c_int(0)
    return _lib.load().cslam_device_count(C.byref(n)) != 0 or n.value == 0


def _call(voxel, n_clouds, offsets):
    """The entry point with host memory in place of every device buffer: an argument check must return before any of it
    is used.  `offsets` is given as the host copy."""
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    dummy = np.zeros(64, dtype=np.float64)
    p = dummy.ctypes.data_as(C.c_void_p)
    return _lib.load().cslam_voxel_downsample_dev(p, p, n_clouds, voxel, p, p, None, p, off.ctypes.data_as(C.c_void_p), None)


@pytest.mark.parametrize("voxel,n_clouds,offsets", [
    (0.0, 2, [0, 3, 5]), (-0.5, 2, [0, 3, 5]), (float("nan"), 2, [0, 3, 5]), (float("inf"), 2, [0, 3, 5]),
    (0.5, 0, [0]), (0.5, 65536, [0] * 65537), (0.5, 2, [0, 5, 3]), (0.5, 3, [0, 4, 4, 2]), (0.5, 2, [1, 3, 5])],
    ids=["voxel=0", "voxel<0", "voxel=nan", "voxel=inf", "n_clouds=0", "n_clouds=65536", "decreasing", "decreasing-after-empty",
         "start!=0"])
def test_argument_checks_precede_hip(voxel, n_clouds, offsets):
    assert _call(voxel, n_clouds, offsets) == -1
    assert b"invalid argument" in _lib.load().cslam_last_error()


@pytest.mark.skipif(not _no_gpu(), reason="GPU present: covered by the -m gpu suite")
def test_downsampling_fails_loudly_without_gpu():
    from cslam_amd.lidar_pr import icp_utils, keyframes
    pts = np.random.default_rng(0).standard_normal((50, 3))
    assert _call(0.5, 2, [0, 3, 5]) == -2                  # valid arguments: the first HIP call fails
    with pytest.raises(_lib.CslamHipError):
        icp_utils.downsample(pts, VOXEL)
    with pytest.raises(_lib.CslamHipError):
        icp_utils.downsample_clouds([pts, pts], VOXEL, counts=True)
    with pytest.raises(_lib.CslamHipError):
        keyframes.ingest([pts], VOXEL)


def test_constants_mirror_the_kernels():
    from cslam_amd.lidar_pr import icp_utils
    plan = open(os.path.join(ROOT, "cslam_amd", "csrc", "voxel_plan.h")).read()
    assert "#define VOXEL_TILE %d " % icp_utils.VOXEL_TILE in plan          # the GPU tests size their clouds around these
    assert "#define VOXEL_SEG_BLOCK %d " % icp_utils.VOXEL_SEG_BLOCK in plan
    assert "voxel.hip" in open(os.path.join(ROOT, "cslam_amd", "csrc", "Makefile")).read()


def test_reversed_cloud_gives_other_means():
    """The GPU test of the summation order compares against the forward cloud's result; that can see a wrong order only
    if the order matters: here it does in 9 voxels of 10."""
    pts = np.random.default_rng(5).uniform(-1.0, 1.0, (3000, 3))
    fwd, rev = ref.voxel_average(pts, VOXEL), ref.voxel_average(pts[::-1], VOXEL)
    assert fwd.shape == rev.shape == (125, 3)
    differ = np.mean((fwd != rev).any(axis=1))
    print("voxels whose mean depends on the order of the sum: %.2f" % differ)
    assert differ >= 0.5
    assert np.abs(fwd - rev).max() < 1e-15                 # and only in the last bits


def _index(p, lo, voxel):
    return np.floor((np.float64(p) - (np.float64(lo) - voxel / 2.0)) / voxel)


def test_index_values_at_the_edge_of_the_key_range():
    assert _index((2 ** 21 - 1) * VOXEL, 0.0, VOXEL) == 2 ** 21 - 1        # the last index a key holds
    assert _index(2 ** 21 * VOXEL, 0.0, VOXEL) == 2 ** 21                  # the first that is refused
    pts = np.array([[0.0, 0.0, 0.0], [(2 ** 21 - 1) * VOXEL, 0.0, 0.0]])
    assert np.array_equal(ref.voxel_average(pts[::-1], VOXEL), pts)
    # 0.25 and the double below it, minimum 0: 0.24999999999999997 + 0.25 rounds to 0.5, so both have index 1
    assert _index(0.25, 0.0, VOXEL) == 1 and _index(0.24999999999999997, 0.0, VOXEL) == 1
    assert np.float64(0.24999999999999997) < 0.25
