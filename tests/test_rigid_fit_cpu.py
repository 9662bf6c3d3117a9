"""CPU: the rigid fit of csrc/horn.h (`icp_rigid_from_sums`, every ICP update and every robust rotation) fed directly.

Here are the cases of tests/test_rigid_fit_gpu.py, the input conditions that make their comparisons well defined
(nearest-neighbour margins, GNC stopping at iteration 0, singular-value gaps, voxel occupancy, dyadic exactness), and one
test of horn.h itself: compiled for the host, fed the sums in the kernels' order, against the extended-precision centred
fit of tests/icp_reference.py.  The bound everywhere: the moved source points differ from the reference's by at most
256 ulp of the largest coordinate (icp_reference.ULP_BOUND), a multiple of the rounding the inputs themselves carry.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_reference as iref
import robust_reference as rref
from conftest import ROOT

C_H1 = 1000.0                 # noise bound of handle 1: every chain residual is far below it, so GNC stops at iteration 0
ORTHO = 1e-14
RMSE_REL = 1e-12


# ---- handle 1: robust_rotation on noise-free matches --------------------------------------------------------------------
def handle1_cases():
    """[(name, ms, md, unique)]: the rotation of the chain differences is compared when `unique`."""
    base = iref.generic_cloud(120, 0)
    out = [("angle-" + name, base, iref.rotated(R, base), True) for name, R in iref.angle_cases()]
    Rd = iref.axis_angle(*iref.DEFICIENT_R)
    out += [(name, pts, iref.rotated(Rd, pts), unique) for name, (pts, unique) in iref.deficient_clouds().items()]
    out += [("reflection-" + name, ms, md, True) for name, ms, md in iref.reflection_cases()]
    out += [("scale-%g" % f, base * f, iref.rotated(Rd, base * f), True) for f in (1e-3, 1e6)]
    return out


def handle1_reference(ms, md):
    a, b = iref.chain_all(ms, md)
    return a, b, (iref.rigid_fit_ld(a, b, centre=False) if len(a) else None)


def check_rotation(name, R, a, b, fit, unique, figures=None):
    """What is asserted of a rotation of handle 1 (R [3, 3]) against the uncentred reference fit of the differences."""
    assert np.all(np.isfinite(R)), name
    ortho, det = iref.rotation_defects(R)
    assert ortho <= ORTHO and det <= ORTHO, (name, ortho, det)
    if fit is None or len(a) == 0:                                   # one point: no measurement, the identity
        assert np.array_equal(R, np.identity(3)), name
        return
    if not unique:                                                   # any rotation of the null directions is as good
        got = float(np.sqrt(((np.asarray(b, dtype=iref.LD) - iref.moved_ld(R, a)) ** 2).sum(axis=1).mean()))
        check_rmse(name, got, fit.rmse(a, b), iref.coord_ulp(a, b))
    else:
        ulps = iref.moved_error_ulps(R, fit, a, a, b)
        if figures is not None:
            figures.append((name, ulps))
        assert ulps <= iref.ULP_BOUND, (name, ulps)


def check_rmse(name, got, want, ulp):
    """Equal to 1e-12 relative; where the reference's residual is zero (within the rounding of the inputs, 16 ulp of the
    largest coordinate) to 1e-12 absolute instead."""
    tol = RMSE_REL * want if want > 16.0 * ulp else RMSE_REL
    assert abs(got - want) <= tol, (name, got, want)


# ---- handle 2: one ICP update on a pair whose correspondences are known ------------------------------------------------
class Pair:
    """src, dst, partner (target row of every source row, -1 = none), the radius, the 4 x 4 init and whether the rotation
    of the fit is defined."""

    def __init__(self, name, src, dst, partner, radius=iref.LATTICE_RADIUS, init=None, unique=True):
        self.name, self.src, self.dst, self.partner, self.radius, self.unique = name, src, dst, partner, radius, unique
        self.init = np.identity(4) if init is None else init

    def moved(self):
        """init . src, rounded once from extended precision (the kernels' fma chain differs by an ulp at most)."""
        return iref.moved_ld(self.init, self.src).astype(np.float64)

    def shifted(self, off, by_init):
        """The same pair far from the origin: both clouds moved by `off`, or the target moved and the offset carried by
        the init with the source left where it is."""
        shift = iref.Rt2T(np.identity(3), off)
        if by_init:
            return Pair("%s+init" % self.name, self.src, self.dst + off, self.partner, self.radius, shift @ self.init, self.unique)
        init = self.init.copy()
        init[:3, 3] = self.init[:3, 3] + off - self.init[:3, :3] @ off
        return Pair("%s+both" % self.name, self.src + off, self.dst + off, self.partner, self.radius, init, self.unique)


def angle_pairs():
    """Every angle about every axis.  Up to 1 degree the update itself carries the rotation; the larger ones are carried by
    the init, with the source turned back by its inverse, and the update is the small default motion."""
    out = []
    for name, R in iref.angle_cases():
        deg = float(name.split("-", 1)[1])
        if deg <= 1.0:
            out.append(Pair("angle-" + name, *iref.lattice_pair(257, 1, R=R)))
        else:
            src, dst, partner = iref.lattice_pair(257, 1)
            out.append(Pair("angle-" + name, iref.rotated(R.T, src), dst, partner, init=iref.Rt2T(R, np.zeros(3))))
    return out


def size_pairs(noise=0.0):
    return [Pair("size-%d" % k, *iref.lattice_pair(k, 0, noise=noise), unique=k >= 3) for k in iref.SUM_SIZES]


def deficient_pairs():
    rng = np.random.default_rng(4200)
    many = rng.uniform(-5.0, 5.0, (50, 3))
    return [Pair("plane-z0", *iref.lattice_pair(100, 2, dims=2)),
            Pair("plane-z5", *iref.lattice_pair(100, 2, dims=2, lift=5.0)),
            Pair("collinear", *iref.lattice_pair(12, 3, dims=1), unique=False),
            Pair("many-to-one", many, np.array([[1.0, -2.0, 0.5]]), np.zeros(50, dtype=np.int64), radius=100.0, unique=False)]


def scale_pairs():
    return [Pair("scale-%g" % f, *iref.lattice_pair(257, 4, scale=f), radius=iref.LATTICE_RADIUS * f) for f in (1e-3, 1e6)]


def far_pairs(c):
    """Section B at the offset c . (1, 0.7, 0.01): the sizes 257 and 513 with 2 cm noise and the angle cases, each with
    the identity init and with the offset carried by the init."""
    off = c * iref.FAR_DIRECTION
    base = [Pair("size-%d-noisy" % k, *iref.lattice_pair(k, 0, noise=0.02)) for k in (257, 513)] + angle_pairs()
    return [p.shifted(off, by_init) for p in base for by_init in (False, True)]


def check_update(pair, T, figures=None, fit=None):
    """What is asserted of the result T of one ICP update of `pair` (registration_icp with max_iteration = 1)."""
    name = pair.name
    kept = pair.partner >= 0
    fit, p, q = fit or iref.known_fit(pair.src, pair.dst, pair.partner, pair.init)
    assert np.all(np.isfinite(T)) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]), name
    ortho, det = iref.rotation_defects(T[:3, :3])
    assert ortho <= ORTHO and det <= ORTHO, (name, ortho, det)
    s = pair.src[kept]
    ulp = iref.coord_ulp(p, q)
    got = iref.moved_ld(T, s)
    if len(p) == 1:                                                  # the update is exactly (I, q - p)
        assert np.array_equal(pair.init, np.identity(4)) and np.array_equal(T, iref.Rt2T(np.identity(3), (q - s)[0])), name
    centroid = float(np.abs(got.mean(axis=0) - q.astype(iref.LD).mean(axis=0)).max())
    assert centroid <= iref.ULP_BOUND * ulp, (name, centroid / ulp)
    if not pair.unique:                                              # any rotation of the null directions is as good
        rmse = float(np.sqrt(((q.astype(iref.LD) - got) ** 2).sum(axis=1).mean()))
        check_rmse(name, rmse, fit.rmse(p, q), ulp)
    else:
        ulps = float(np.abs(got - fit.moved(p)).max()) / ulp
        if figures is not None:
            figures.append((name, ulps))
        assert ulps <= iref.ULP_BOUND, (name, ulps)


def worst(figures, prefix=""):
    vals = [u for n, u in figures if n.startswith(prefix)]
    return max(vals) if vals else 0.0


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_mpmath_far_from_the_origin():
    """The longdouble fit against the same fit in 60 digits (mpmath), 2^20 m out: the reference's own error is far below
    one ulp of the coordinates."""
    mp = pytest.importorskip("mpmath")
    assert np.finfo(np.longdouble).nmant >= 63
    src, dst, partner = iref.lattice_pair(65, 0, noise=0.02)
    off = 2.0 ** 20 * iref.FAR_DIRECTION
    p, q = src[partner >= 0] + off, dst[partner[partner >= 0]] + off
    fit = iref.rigid_fit_ld(p, q)
    old = mp.mp.dps
    mp.mp.dps = 60
    try:
        P, Q = mp.matrix(p.tolist()), mp.matrix(q.tolist())
        n = len(p)
        mP = [sum(P[i, a] for i in range(n)) / n for a in range(3)]
        mQ = [sum(Q[i, a] for i in range(n)) / n for a in range(3)]
        S = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                S[a, b] = sum((Q[i, a] - mQ[a]) * (P[i, b] - mP[b]) for i in range(n)) / n
        U, sv, V = mp.svd_r(S)
        R = U * V
        if mp.det(R) < 0:
            R = U * mp.diag([1, 1, -1]) * V
        got = fit.moved(p)
        hi = got.astype(np.float64)
        lo = (got - hi.astype(iref.LD)).astype(np.float64)          # a longdouble as two float64, exactly
        worst_err = max(abs(sum(R[a, b] * (P[i, b] - mP[b]) for b in range(3)) + mQ[a] - (mp.mpf(hi[i, a]) + mp.mpf(lo[i, a])))
                        for i in range(n) for a in range(3))
    finally:
        mp.mp.dps = old
    assert float(worst_err) <= 0.01 * iref.coord_ulp(p, q), float(worst_err)
    assert np.allclose([float(x) for x in sv], fit.sv, rtol=1e-12)
    R_f64, t_f64 = iref.umeyama_rigid(p - off, q - off)                 # and the float64 form at the origin
    assert np.abs(R_f64 - fit.R).max() <= 1e-12


def test_reference_forms():
    """Weights, the reflection correction and the form without centring."""
    rng = np.random.default_rng(1)
    p = rng.standard_normal((30, 3))
    R = iref.axis_angle((1.0, 2.0, -0.5), 77.0)
    q = iref.rotated(R, p) + np.array([3.0, -1.0, 2.0])
    fit = iref.rigid_fit_ld(p, q)
    assert np.abs(fit.R - R).max() <= 1e-14 and np.abs(fit.t - [3.0, -1.0, 2.0]).max() <= 1e-14
    w = rng.uniform(0.0, 1.0, 30)
    w[:5] = 0.0
    q2 = q.copy()
    q2[:5] += 10.0                                                   # weight 0: not seen
    assert np.abs(iref.rigid_fit_ld(p, q2, w).R - R).max() <= 1e-14
    plain = iref.rigid_fit_ld(p, iref.rotated(R, p), centre=False)
    assert np.abs(plain.R - R).max() <= 1e-14 and np.array_equal(plain.t, np.zeros(3))
    assert np.abs(plain.R - rref.horn_rotation(p, iref.rotated(R, p), np.ones(30))).max() <= 1e-13
    mirrored = iref.rigid_fit_ld(p, p @ np.diag([1.0, 1.0, -1.0]))
    assert abs(np.linalg.det(mirrored.R) - 1.0) <= 1e-14
    for deg in (0.0, 90.0, 180.0):                                   # exact where the sine and cosine are
        Rz = iref.axis_angle((0.0, 0.0, 1.0), deg)
        assert set(np.abs(Rz).ravel().tolist()) == {0.0, 1.0}


# ---- input conditions ---------------------------------------------------------------------------------------------------
def test_handle1_cases_stop_at_iteration_zero_with_unit_weights():
    for name, ms, md, _ in handle1_cases():
        R, w, iterations = rref.gnc_rotation(ms, md, np.arange(len(ms)), C_H1)
        assert iterations == 0 and np.array_equal(w, np.ones(max(len(ms) - 1, 0))), name
        if len(ms) >= 2:
            a, b = iref.chain_all(ms, md)
            r = b - a @ R.T
            assert (r * r).sum(axis=1).max() <= 1e-2 * (4.0 * C_H1 * C_H1) / 2.0, name      # 100 times inside mu <= 0


def test_reflection_cases_have_separated_singular_values():
    for name, ms, md in iref.reflection_cases():
        a, b, fit = handle1_reference(ms, md)
        gaps = -np.diff(fit.sv) / fit.sv[0]
        assert gaps.min() >= 0.01, (name, fit.sv)
        U, _, Vt = np.linalg.svd(((b[:, :, None] * a[:, None, :]).sum(axis=0)))
        assert np.linalg.det(U @ Vt) < 0, name                       # the best orthogonal map IS a reflection


def all_handle2_pairs():
    out = angle_pairs() + size_pairs() + deficient_pairs() + scale_pairs()
    for c in iref.FAR_OFFSETS:
        out += far_pairs(c)
    return out


def test_handle2_correspondences_cannot_turn():
    """Every moved source point's nearest target is its partner, within the radius, and the second-nearest is at least one
    radius farther; a source row without a partner has no target within 1.5 radii."""
    seen = 0
    for pair in all_handle2_pairs():
        scale = pair.radius / iref.LATTICE_RADIUS if pair.name.startswith("scale") else 1.0
        first, gap, lone = iref.nearest_margin(pair.moved() / scale, pair.dst / scale, pair.partner)
        if pair.name.startswith("many-to-one"):
            assert first <= pair.radius / 5.0
            continue
        assert first <= 0.8 * iref.LATTICE_RADIUS and gap >= 1.0 and lone >= 1.5 * iref.LATTICE_RADIUS, (pair.name, first, gap, lone)
        kept = int((pair.partner >= 0).sum())
        assert len(pair.src) == kept + kept // 3 and len(pair.dst) == kept
        seen += 1
    assert seen >= 40
    src, dst, _ = iref.lattice_pair(513, 0)
    d = np.sqrt(((src[:, None] - src[None]) ** 2).sum(axis=-1)) + 10.0 * np.identity(len(src))
    assert d.min() >= 2.0


def test_street_crop_registration_does_not_hang_on_the_last_bits():
    src, dst = iref.street_crop()
    assert len(src) == 600 and len(dst) == 600
    for c in (0.0,) + iref.FAR_OFFSETS:
        off = c * iref.FAR_DIRECTION
        want = iref.registration_icp_ld(src + off, dst + off, 0.5)
        assert 5 < want.iterations < 100 and want.fitness > 0.5
        assert iref.stop_margin(want.history) > 1e-8, c


def test_dyadic_scene_is_exact_in_both_frames():
    pts, view = iref.dyadic_scene()
    assert 1400 <= len(pts) <= 1500 and len(np.unique(pts, axis=0)) == len(pts)
    assert np.array_equal(iref.dyadic(pts), pts)
    far = pts + iref.FAR_C
    assert np.array_equal(far.astype(iref.LD), pts.astype(iref.LD) + iref.FAR_C.astype(iref.LD))     # p + c is exact
    assert np.array_equal(far - iref.FAR_C, pts) and np.array_equal((view + iref.FAR_C) - iref.FAR_C, view)
    d_near = pts[:50, None, :] - pts[None, :, :]
    d_far = far[:50, None, :] - far[None, :, :]
    assert np.array_equal(d_near, d_far)                             # every difference is the same float64 number
    for cloud in (pts, far):                                         # voxel 0.5: at most 64 points per voxel
        origin = cloud.min(axis=0) - 0.25
        _, cnt = np.unique(np.floor((cloud - origin) / 0.5).astype(np.int64), axis=0, return_counts=True)
        assert cnt.max() <= 64


def robust_far_case():
    """The `planted` case of the far robust stages, on the dyadic grid: (ms, md, T, inliers, c)."""
    ms, md, T, inliers = rref.planted(300, 300, 30)
    return iref.dyadic(ms), iref.dyadic(md), T, inliers, 0.05


def test_far_robust_case_has_a_consensus_margin():
    ms, md, T, inliers, c = robust_far_case()
    for m_s, m_d in ((ms, md), (ms + iref.FAR_C, md + iref.FAR_C)):
        adj, margin = rref.consistency_graph(m_s, m_d, c, return_margin=True)
        clique, unique = rref.max_clique(adj)
        assert unique and clique == inliers.tolist() and margin > 1e-9
        R = rref.gnc_rotation(m_s, m_d, clique, c)[0]
        xs = rref.translation_scalars(m_s, m_d, clique, R)
        for a in range(3):
            assert rref.scalar_tls(xs[a], c, return_margin=True)[2] > 1e-6


# ---- horn.h itself, compiled for the host -------------------------------------------------------------------------------
WRAPPER = """
#include <math.h>
#define __host__
#define __device__
#include "horn.h"
extern "C" void fit(const double *s, const double *o, double *U) { icp_rigid_from_shifted_sums(s, o, U); }
extern "C" void fit_plain(const double *s, double *U) { icp_rigid_from_sums(s, U); }
extern "C" void origin(const double *q0, double *o) { icp_sum_origin(q0, o); }
"""


@pytest.fixture(scope="module")
def horn(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("horn")
    (tmp / "horn_host.cpp").write_text(WRAPPER)
    so = tmp / "horn_host.so"
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "cslam_amd", "csrc"),
                    str(tmp / "horn_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    dp = ctypes.POINTER(ctypes.c_double)

    def ptr(a):
        return a.ctypes.data_as(dp)

    class Horn:
        @staticmethod
        def origin(q0):
            o = np.zeros(3)
            lib.origin(ptr(np.ascontiguousarray(q0, dtype=np.float64)), ptr(o))
            return o

        @staticmethod
        def fit(s, o=np.zeros(3)):
            U = np.zeros(12)
            lib.fit(ptr(np.ascontiguousarray(s, dtype=np.float64)), ptr(np.ascontiguousarray(o, dtype=np.float64)), ptr(U))
            return np.concatenate([U, [0.0, 0.0, 0.0, 1.0]]).reshape(4, 4)

        @staticmethod
        def fit_plain(s):
            """icp_rigid_from_sums as csrc/robust.hip calls it: n = 1, zero means, the 9 sums of the chain."""
            U = np.zeros(12)
            lib.fit_plain(ptr(np.ascontiguousarray(s, dtype=np.float64)), ptr(U))
            return np.concatenate([U, [0.0, 0.0, 0.0, 1.0]]).reshape(4, 4)

        @classmethod
        def update(cls, pair):
            """One ICP update of a pair of handle 2 on the host: the kernels' sums in numpy, the fit, T <- U . T."""
            p = pair.moved()
            kept = pair.partner >= 0
            q = pair.dst[np.where(kept, pair.partner, 0)]
            o = cls.origin(pair.dst[0])
            return iref.compose(cls.fit(iref.kernel_sums(p, q, kept, o), o), pair.init)

    return Horn


def test_sums_origin_is_zero_near_the_frame_origin_and_exact(horn):
    assert np.array_equal(horn.origin([511.9, -511.9, 30.0]), np.zeros(3))
    assert np.array_equal(horn.origin([2.0 ** 20 + 700.0, -0.7 * 2.0 ** 20, 10485.76]), [2.0 ** 20 + 1024.0, -734208.0, 10240.0])
    assert np.array_equal(horn.origin([1e300, -1e300, 0.0]), [1e300, -1e300, 0.0])


def test_host_build_rotations_of_handle1(horn):
    figures = []
    for name, ms, md, unique in handle1_cases():
        a, b, fit = handle1_reference(ms, md)
        R = horn.fit_plain(iref.chain_sums(a, b))[:3, :3] if len(a) else np.identity(3)
        check_rotation(name, R, a, b, fit, unique, figures)
    print("host build, handle 1, worst moved-point error in ulp of the largest coordinate: angles %.1f, planes %.1f, "
          "reflections %.1f, scales %.1f" % (worst(figures, "angle"), worst(figures, "plane"), worst(figures, "reflection"),
                                             worst(figures, "scale")))
    s = iref.kernel_sums(np.array([[1.1, 2.3, 3.7]]), np.array([[1.6, 2.3, 2.7]]), np.array([True]), np.zeros(3))
    s[7:16] *= 1.0 + 2.0 ** -52                                      # what a fused q p - q mean p leaves on the device
    assert np.array_equal(horn.fit(s), iref.Rt2T(np.identity(3), s[4:7] - s[1:4]))      # one correspondence: R = I exactly


def test_host_build_updates_of_handle2_at_the_origin(horn):
    figures = []
    for pair in angle_pairs() + size_pairs() + deficient_pairs() + scale_pairs():
        check_update(pair, horn.update(pair), figures)
    print("host build, handle 2 at the origin, worst ulp: angles %.1f, sizes %.1f, planes %.1f, scales %.1f"
          % (worst(figures, "angle"), worst(figures, "size"), worst(figures, "plane"), worst(figures, "scale")))


@pytest.mark.parametrize("c", iref.FAR_OFFSETS, ids=lambda c: "2^%d" % int(np.log2(c)))
def test_host_build_updates_of_handle2_far_from_the_origin(horn, c):
    figures = []
    for pair in far_pairs(c):
        check_update(pair, horn.update(pair), figures)
    print("host build, handle 2 at %g m, worst ulp: sizes %.1f, angles %.1f" % (c, worst(figures, "size"), worst(figures, "angle")))


def test_host_build_weighted_chain_is_a_function_of_its_sums_only(horn):
    """robust.hip's call: n = 1, zero means.  No origin enters."""
    ms, md, c = rref.rotation_case(65, 0.2, 14)
    a, b = iref.chain_all(ms, md)
    w = np.random.default_rng(2).uniform(0.0, 1.0, len(a))
    s = iref.chain_sums(a, b, w)
    R = horn.fit_plain(s)[:3, :3]
    assert np.abs(R - iref.rigid_fit_ld(a, b, w, centre=False).R).max() <= 1e-13
    assert np.array_equal(horn.fit_plain(s)[:3, 3], np.zeros(3))
