"""CPU: the point-to-plane estimator of the lidar ICP (csrc/plane.h, `estimation="point_to_plane"`).

Here are the input conditions of tests/test_icp_plane_gpu.py (its scenes do not hang on the last bits), csrc/plane.h itself
compiled for the host and fed the sums in the kernels' order -- against the float64 restatement near the origin, against
a numpy.longdouble update far from it, and on singular systems --, the ABI, and the argument errors, which are raised
before the GPU is touched.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import icp_plane_reference as pref
import icp_reference as iref
from conftest import ROOT
from cslam_amd import _lib

VOXEL = 0.5
# (name, seed, raw points, stages): the whole registrations the GPU suite compares with the restatement
GPU_CASES = (("scene 103, one stage", 103, 9000, ((1.0, 100),)), ("scene 21, default stages", 21, 2400, iref.DEFAULT_STAGES))
E2E_SEED = 2                  # the end-to-end pair of the GPU suite: street_scene(2), default stages
SIZES = (1, 5, 6, 63, 64, 65, 256, 257, 513)
FAR_SHIFTS = (np.array([2.0 ** 17, -2.0 ** 16, 1024.0]), np.array([2.0 ** 20, 0.0, 0.0]))


def whole_case(seed, n_raw, stages):
    """(src, dst, normals of the restatement, init, per-stage results of the restatement)."""
    src, dst, _, yaw = iref.street_scene(seed, n_raw, VOXEL)
    normals = pref.reference_normals(dst, VOXEL)
    init = iref.yaw_init(iref.seed_yaw(yaw))
    return src, dst, normals, init, pref.register_staged(src, dst, normals, VOXEL, init, stages)


@pytest.fixture(scope="module")
def whole():
    cases = {name: whole_case(seed, n_raw, stages) for name, seed, n_raw, stages in GPU_CASES}
    cases["end to end"] = whole_case(E2E_SEED, 9000, iref.DEFAULT_STAGES)
    return cases


def test_input_conditions_of_the_gpu_comparisons(whole):
    """The GPU tests demand equal iteration counts and correspondence sets.  That is fair only where no decision hangs on
    the last bits: every stage stops before its cap and after more than one update, a whole registration makes more than 3
    updates (the one-stage case: 10; the staged ones are counted over their stages, because a last stage that starts from a
    converged transform needs few: 3 on scene 21), at the stopping round and the one before both deltas stay 1e-9 away
    from the 1e-6 threshold, and every system solved is far from the determinant test (|det A| >= 1; seen: 1e22 and above)."""
    for name, (src, dst, normals, init, stages) in whole.items():
        spec = dict((n, s) for n, _, _, s in GPU_CASES).get(name, iref.DEFAULT_STAGES)
        counts = [s.iterations for s in stages]
        margins = [iref.stop_margin(s.history) for s in stages]
        dets = [abs(d) for s in stages for d in s.dets]
        print("%-26s updates %s, stop margins %s, |det A| %.1e .. %.1e, fitness %.4f"
              % (name, counts, ["%.1e" % m for m in margins], min(dets), max(dets), stages[-1].fitness))
        assert sum(counts) > 3 and all(1 < c < cap for c, (_, cap) in zip(counts, spec)), name
        assert min(margins) >= 1e-9, name
        assert min(dets) >= 1.0 and len(dets) == sum(counts), name
        assert stages[-1].fitness > 0.5, name
        assert np.abs(np.linalg.norm(normals, axis=1) - 1.0).max() <= 1e-12


def test_brute_force_and_kdtree_agree(whole):
    src, dst, normals, init, _ = whole["scene 21, default stages"]
    a = pref.registration_icp(src[:300], dst, normals, 4 * VOXEL, init, 20, brute=True)
    b = pref.registration_icp(src[:300], dst, normals, 4 * VOXEL, init, 20, brute=False)
    assert a.iterations == b.iterations > 1 and np.array_equal(a.correspondence_set, b.correspondence_set)
    assert np.array_equal(a.transformation, b.transformation)


def test_point_to_plane_needs_fewer_updates_than_point_to_point(whole):
    src, dst, normals, init, stages = whole["scene 103, one stage"]
    point = iref.registration_icp(src, dst, VOXEL, init, 100)
    print("scene 103, one stage: point-to-point %d updates, point-to-plane %d" % (point.iterations, stages[0].iterations))
    assert stages[0].iterations < point.iterations


def test_narrower_basin():
    """Why point-to-plane is not the default: scene 103 at 2400 raw points, one stage at the voxel radius from the yaw seed
    rounded to ScanContext's sector.  Point-to-point converges, point-to-plane ends 2.6 degrees off; the default stages bring
    it home."""
    src, dst, T_true, yaw = iref.street_scene(103, 2400, VOXEL)
    normals, init = pref.reference_normals(dst, VOXEL), iref.yaw_init(iref.seed_yaw(yaw))
    point = iref.registration_icp(src, dst, VOXEL, init, 100)
    one = pref.registration_icp(src, dst, normals, VOXEL, init, 100)
    stages = pref.register_staged(src, dst, normals, VOXEL, init)
    rot = [iref.rotation_error_deg(r.transformation[:3, :3], T_true[:3, :3]) for r in (point, one, stages[-1])]
    print("rotation error: point-to-point %.3f deg in %d updates, point-to-plane in one stage %.3f (fitness %.2f), through the "
          "default stages %.3f in %s" % (rot[0], point.iterations, rot[1], one.fitness, rot[2], [s.iterations for s in stages]))
    assert rot[0] <= 0.05 and rot[2] <= 0.05 and rot[1] > 1.0 and one.fitness < 0.3


# ---- plane.h itself, compiled for the host ---------------------------------------------------------------------------
WRAPPER = """
#include <math.h>
#define __host__
#define __device__
#include "horn.h"
#include "plane.h"
extern "C" int solve(const double *s, double *x, double *det) { return icp_plane_solve(s, x, det); }
extern "C" int update(const double *s, const double *o, double *U) { return icp_plane_update_from_shifted_sums(s, o, U); }
extern "C" void terms(const double *ps, const double *dq, const double *nr, double d2, double *v) { icp_plane_terms(ps, dq, nr, d2, v); }
extern "C" void origin(const double *q0, double *o) { icp_sum_origin(q0, o); }
extern "C" int nsum() { return ICP_PLANE_NSUM; }
"""


@pytest.fixture(scope="module")
def plane(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("plane")
    (tmp / "plane_host.cpp").write_text(WRAPPER)
    so = tmp / "plane_host.so"
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "cslam_amd", "csrc"),
                    str(tmp / "plane_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.terms.argtypes = [dp, dp, dp, ctypes.c_double, dp]

    def ptr(a):
        return a.ctypes.data_as(dp)

    def arr(a):
        return np.ascontiguousarray(a, dtype=np.float64)

    class Plane:
        @staticmethod
        def origin(q0):
            o = np.zeros(3)
            lib.origin(ptr(arr(q0)), ptr(o))
            return o

        @staticmethod
        def solve(s):
            x, det = np.full(6, 7.0), np.full(1, 7.0)
            ok = lib.solve(ptr(arr(s)), ptr(x), ptr(det))
            return bool(ok), x, float(det[0])

        @staticmethod
        def update(s, o=np.zeros(3)):
            U = np.full(12, 7.0)
            ok = lib.update(ptr(arr(s)), ptr(arr(o)), ptr(U))
            return bool(ok), np.concatenate([U, [0.0, 0.0, 0.0, 1.0]]).reshape(4, 4)

        @staticmethod
        def terms(ps, dq, nr, d2):
            v = np.zeros(pref.NSUM)
            lib.terms(ptr(arr(ps)), ptr(arr(dq)), ptr(arr(nr)), float(d2), ptr(v))
            return v

    assert lib.nsum() == pref.NSUM
    return Plane


def lattice_case(kept, noise=0.02):
    """A lattice pair with planted unit normals on the target: (moved source p, its target rows q, normals at q, kept mask)."""
    src, dst, partner = iref.lattice_pair(kept, 0, noise=noise)
    normals = pref.planted_normals(kept, kept)
    keep = partner >= 0
    sel = np.where(keep, partner, 0)
    return src, dst[sel], normals[sel], keep


def test_terms_are_the_rows_of_the_kernel_order_sums(plane):
    p, q, n, keep = lattice_case(6)
    for i in np.nonzero(keep)[0][:3]:
        d = p[i] - q[i]
        want = pref.kernel_sums(p[i:i + 1], q[i:i + 1], n[i:i + 1], np.array([True]), np.zeros(3))
        got = plane.terms(p[i], d, n[i], d[2] * d[2] + (d[1] * d[1] + d[0] * d[0]))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("kept", SIZES)
def test_host_build_update_equals_the_restatement_near_the_origin(plane, kept):
    """U of plane.h from the sums in kernel order against the restatement's update: <= 1e-9 per entry, the project's bound
    for a transform against its restatement.  Fewer than six correspondences: the identity."""
    p, q, n, keep = lattice_case(kept)
    o = plane.origin(q[0])
    assert np.array_equal(o, np.zeros(3))
    ok, U = plane.update(pref.kernel_sums(p, q, n, keep, o), o)
    want, det = pref.update(p[keep], q[keep], n[keep], o)
    if kept < 6:
        assert not ok and det == 0.0 and np.array_equal(U, np.identity(4)) and np.array_equal(want, np.identity(4))
        return
    err = np.abs(U - want).max()
    print("%d correspondences: det A %.2e, max |U - U_ref| = %.2e, update %.3f deg" % (
        kept, det, err, iref.rotation_error_deg(want[:3, :3], np.identity(3))))
    assert ok and abs(det) >= 1.0 and not np.array_equal(want, np.identity(4))
    assert err <= 1e-9
    ortho, d = iref.rotation_defects(U[:3, :3])
    assert ortho <= 1e-14 and d <= 1e-14


def dyadic_pair():
    """A pair on the 2^-10 m grid with its correspondences at the voxel radius and the restatement's normals."""
    pts, _ = iref.dyadic_scene()
    R = iref.axis_angle((0.3, -0.8, 0.52), 0.3)
    src = iref.dyadic(iref.rotated(R, pts[::2]) + np.array([0.05, -0.04, 0.02]))
    normals = pref.reference_normals(pts, VOXEL)
    idx, d2 = iref.nn_brute(src, pts)
    return src, pts, normals, idx, d2 <= VOXEL * VOXEL


def test_host_build_update_far_from_the_origin(plane):
    """The same pair at the origin, at (2^17, -2^16, 1024) m and at 2^20 m on one axis (exact shifts of a dyadic scene): the
    moved source points stay within icp_reference.ULP_BOUND (256 ulp of the largest coordinate) of the numpy.longdouble
    update about the same origin.  Measured on the host build: 0.45 ulp at the origin, 0.48 at (2^17, -2^16, 1024) m and
    below 0.01 at 2^20 m (where one ulp is eight times larger)."""
    src, dst, normals, idx, keep = dyadic_pair()
    assert 500 <= keep.sum() and np.finfo(np.longdouble).nmant >= 63
    for c in (np.zeros(3),) + FAR_SHIFTS:
        p, q = src + c, dst[idx] + c
        assert np.array_equal(p - c, src) and np.array_equal(q - c, dst[idx])                    # the shift is exact
        o = plane.origin((dst + c)[0])
        assert np.array_equal(o, pref.sum_origin((dst + c)[0])) and np.abs(o - c).max() <= 1024.0
        ok, U = plane.update(pref.kernel_sums(p, q, normals[idx], keep, o), o)
        want = pref.UpdateLD(p[keep], q[keep], normals[idx][keep], o)
        ulps = float(np.abs(iref.moved_ld(U, p) - want.moved(p)).max()) / iref.coord_ulp(p, q)
        near, det = pref.update(src[keep], dst[idx][keep], normals[idx][keep])
        same = float(np.abs(iref.moved_ld(U, p) - c.astype(iref.LD) - iref.moved_ld(near, src)).max()) / iref.coord_ulp(p, q)
        print("shift %s: det A %.3e (at the origin %.3e), moved points %.2f ulp of the largest coordinate from the "
              "longdouble update, %.2f from the float64 update at the origin" % (c.tolist(), float(want.det), det, ulps, same))
        assert ok and ulps <= iref.ULP_BOUND and same <= iref.ULP_BOUND
        assert abs(float(want.det) / det - 1.0) <= 1e-9                                           # det A does not move


def singular_cases():
    """{name: (p, q, n)}: systems whose determinant is exactly 0 in any summation order (every sum is exact, or a row of A
    is exactly zero)."""
    rng = np.random.default_rng(8000)
    grid = iref.dyadic(rng.uniform(-8, 8, (40, 2)))
    patch = np.concatenate([grid, np.full((40, 1), 0.25)], axis=1)
    cloud = iref.dyadic(rng.uniform(-8, 8, (40, 3)))
    out = {"z-patch": (patch, patch + np.array([0.0, 0.0, 0.125]), np.tile([0.0, 0.0, 1.0], (40, 1)))}
    for a in range(3):
        out["parallel-%s" % "xyz"[a]] = (cloud, cloud + 0.0625, np.tile(np.identity(3)[a], (40, 1)))
    for k in range(1, 6):
        out["count-%d" % k] = (cloud[:k], cloud[:k] + 0.0625, np.identity(3)[np.arange(k) % 3])
    return out


@pytest.mark.parametrize("name", list(singular_cases()))
def test_singular_systems_give_the_identity(plane, name):
    p, q, n = singular_cases()[name]
    keep = np.ones(len(p), dtype=bool)
    for o in (np.zeros(3), np.array([1024.0, -2048.0, 0.0])):
        s = pref.kernel_sums(p + o, q + o, n, keep, o)
        ok, x, det = plane.solve(s)
        assert not ok and det == 0.0 and np.array_equal(x, np.zeros(6)), name
        ok, U = plane.update(s, o)
        assert not ok and np.array_equal(U, np.identity(4)), name
        want, want_det = pref.update(p + o, q + o, n, o)
        assert want_det == 0.0 and np.array_equal(want, np.identity(4)), name


def test_a_nan_in_b_gives_the_identity(plane):
    p, q, n, keep = lattice_case(65)
    s = pref.kernel_sums(p, q, n, keep, np.zeros(3))
    assert plane.update(s)[0]
    for k in (23, 28):
        bad = s.copy()
        bad[k] = np.nan
        ok, U = plane.update(bad)
        assert not ok and np.array_equal(U, np.identity(4))
    for k, v in ((2, np.nan), (2, np.inf), (0, np.nan), (10, -np.inf)):              # and in A or the count
        bad = s.copy()
        bad[k] = v
        ok, U = plane.update(bad)
        assert not ok and np.array_equal(U, np.identity(4))
    small = s.copy()
    small[2:23] *= 2.0 ** -70                                                           # |det A| < 1e-6, nothing else wrong
    small[23:29] *= 2.0 ** -70
    ok, x, det = plane.solve(small)
    assert not ok and 0.0 < abs(det) < 1e-6 and np.array_equal(x, np.zeros(6))


# ---- the ABI and the host layer ----------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_plane_entry_point():
    name = "cslam_icp_register_plane_dev"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslam_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert decl and "const double *d_dst_normals" in decl.group(1)
    point = re.search(r"int\s+cslam_icp_register_dev\s*\(([^;]*)\)\s*;", header).group(1)

    def names(args):
        return [a.split()[-1].lstrip("*") for a in args.split(",")]

    assert [a for a in names(decl.group(1)) if a != "d_dst_normals"] == names(point)      # its arguments, plus the normals
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    makefile = open(os.path.join(ROOT, "cslam_amd", "csrc", "Makefile")).read()
    assert all("plane.h" in line for line in makefile.splitlines() if line.startswith("%.") and "horn.h" in line)
    from cslam_amd.lidar_pr import icp, icp_utils
    for public in ("ESTIMATIONS", "NORMALS_RADIUS", "NORMALS_MAX_NN"):
        assert getattr(icp_utils, public) is getattr(icp, public)
    assert icp.ESTIMATIONS == ("point_to_point", "point_to_plane")


def test_argument_errors_are_raised_before_the_gpu_is_touched(monkeypatch):
    from cslam_amd.lidar_pr import _batch, icp_utils as u

    def no_gpu(device):
        raise AssertionError("the GPU was touched")

    for mod in (u, u.icp, u.fpfh, u.robust):
        if hasattr(mod, "gpu"):
            monkeypatch.setattr(mod, "gpu", no_gpu)
    monkeypatch.setattr(_batch, "gpu", no_gpu)
    rng = np.random.default_rng(0)
    src, dst = rng.standard_normal((50, 3)), rng.standard_normal((40, 3))
    nr = pref.planted_normals(40, 1)
    unknown = [lambda: u.registration_icp(src, dst, 0.5, estimation="plane"),
               lambda: u.registration_icp_pairs([(src, dst)], 0.5, estimation="PointToPlane", target_normals=[nr]),
               lambda: u.register_pairs([(src, dst)], 0.5, estimation="point-to-plane"),
               lambda: u.solve_teaser_pairs([(src, dst)], 0.5, 5, estimation=None),
               lambda: u.solve_teaser(src, dst, 0.5, 5, estimation="p2l"),
               lambda: u.solve_icp(src, dst, 0.5, 5, estimation=""),
               lambda: u.solve_icp(src, dst, 0.5, 5, coarse="teaser", estimation="x"),
               lambda: u.compute_transform(src, dst, 0.5, 5, estimation="generalized"),
               lambda: u.compute_transform(src, dst, 0.5, 5, coarse="teaser", estimation="generalized")]
    for call in unknown:
        with pytest.raises(ValueError, match="estimation is 'point_to_point' or 'point_to_plane'"):
            call()
    with pytest.raises(ValueError, match="needs target_normals"):
        u.registration_icp(src, dst, 0.5, estimation="point_to_plane")
    with pytest.raises(ValueError, match="needs target_normals"):
        u.registration_icp_pairs([(src, dst)], 0.5, estimation="point_to_plane")
    for bad in (nr[:39], nr[:, :2], np.zeros((41, 3)), nr.ravel(), np.zeros((50, 3))):
        with pytest.raises(ValueError, match="target_normals of shape"):
            u.registration_icp(src, dst, 0.5, estimation="point_to_plane", target_normals=bad)
    with pytest.raises(ValueError, match="target_normals of shape"):
        u.registration_icp_pairs([(src, dst), (dst, src)], 0.5, estimation="point_to_plane", target_normals=[nr, nr])
    with pytest.raises(ValueError, match="2 entries for 1 pairs"):
        u.registration_icp_pairs([(src, dst)], 0.5, estimation="point_to_plane", target_normals=[nr, nr])
    with pytest.raises(ValueError, match="0 entries for 1 pairs"):
        u.registration_icp_pairs([(src, dst)], 0.5, estimation="point_to_plane", target_normals=[])
    with pytest.raises(ValueError, match="point_to_plane' only"):
        u.registration_icp(src, dst, 0.5, target_normals=nr)
    with pytest.raises(ValueError, match="point_to_plane' only"):
        u.registration_icp_pairs([(src, dst)], 0.5, estimation="point_to_point", target_normals=[nr])
