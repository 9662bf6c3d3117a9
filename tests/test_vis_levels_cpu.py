"""CPU: the level-aware PnP rules of csrc/pnp.h against their restatement (tests/vis_levels_reference.py), and what the
feature is for, on the restatements alone.

  * sigma2, the weighted inlier rule at errors placed a relative 1e-9 inside and outside thr sigma_l for every level, the
    weighted 27 Gauss-Newton sums
  * the level functions once more as a stand-alone program under -fsanitize=address,undefined (never loaded into Python)
  * the two-distance scene of feat_pyramid_reference in both directions: sub-pixel keypoints and level-aware PnP against the
    integer keyframes and the uniform PnP
  * the argument checks of the Python layer and of the C entry points, which refuse before any launch
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import feat_pyramid_reference as pyr_ref
import feat_subpixel_reference as sub_ref
import vis_levels_reference as ref
import vis_reference as vr
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
DP = ctypes.POINTER(ctypes.c_double)
EPS = np.finfo(np.float64).eps
# the translation error of the new path is at most this share of the parent path's on the same scene (measured 0.52 and 0.35)
SCENE_GAIN = 0.6
SCENE_GUARD = 1e-6
# the header's sums against the restatement's where 8 eps sum | terms | cannot hold: the tolerance of test_vis_cpu.py's GN_SUM_TOL
GN_SUM_TOL = 8 * 64 * EPS

LEVELS_WRAPPER = r"""
#define __host__
#define __device__
#include "pnp.h"
extern "C" double w_sigma2(int l) { return pnp_level_sigma2(l); }
extern "C" int w_inlier_level(const double *R, const double *t, const double *cam, const double *x, double u, double v, double thr2,
                              double sigma2) {
    return pnp_inlier_level(R, t, cam, x, u, v, thr2, sigma2) ? 1 : 0;
}
extern "C" void w_gn_sums_level(const double *R, const double *t, const double *cam, const double *X, const double *uv, const double *w,
                                int n, double *s) {
    for (int e = 0; e < PNP_NSUM; ++e) s[e] = 0.0;
    for (int k = 0; k < n; ++k) pnp_gn_accumulate_level(R, t, cam, X + 3 * k, uv[2 * k], uv[2 * k + 1], w[k], s);
}
extern "C" void w_gn_sums(const double *R, const double *t, const double *cam, const double *X, const double *uv, int n, double *s) {
    for (int e = 0; e < PNP_NSUM; ++e) s[e] = 0.0;
    for (int k = 0; k < n; ++k) pnp_gn_accumulate(R, t, cam, X + 3 * k, uv[2 * k], uv[2 * k + 1], s);
}
extern "C" int w_max_level() { return PNP_MAX_LEVEL; }
"""

LEVELS_MAIN = r"""
#include <stdio.h>
#include <vector>
#define __host__
#define __device__
#include "pnp.h"
int main() {
    long long checks = 0;
    double prev = 0.0;
    for (int l = 0; l <= PNP_MAX_LEVEL; ++l) {
        const double s = pnp_level_sigma2(l);
        if (!(s > prev) || (l == 0 && s != 1.0) || (l == 1 && s != 1.44)) return 3;
        prev = s;
        ++checks;
    }
    const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0.1, -0.2, 0.3}, cam[4] = {525.0, 525.0, 319.5, 239.5};
    std::vector<double> X, uv, w;
    for (int k = 0; k < 64; ++k) {
        X.push_back(0.1 * (k % 9) - 0.4); X.push_back(0.07 * (k % 7) - 0.2); X.push_back(k % 13 == 0 ? -1.0 : 1.0 + 0.1 * k);
        uv.push_back(10.0 * (k % 60)); uv.push_back(7.0 * (k % 50));
        w.push_back(1.0 / pnp_level_sigma2(k % (PNP_MAX_LEVEL + 1)));
    }
    double s[PNP_NSUM] = {0}, s1[PNP_NSUM] = {0}, s2[PNP_NSUM] = {0};
    int in = 0;
    for (int k = 0; k < 64; ++k) {
        pnp_gn_accumulate_level(R, t, cam, &X[3 * k], uv[2 * k], uv[2 * k + 1], w[k], s);
        pnp_gn_accumulate_level(R, t, cam, &X[3 * k], uv[2 * k], uv[2 * k + 1], 1.0, s1);
        pnp_gn_accumulate(R, t, cam, &X[3 * k], uv[2 * k], uv[2 * k + 1], s2);
        in += pnp_inlier_level(R, t, cam, &X[3 * k], uv[2 * k], uv[2 * k + 1], 1e4, 1.0 / w[k]) ? 1 : 0;
        ++checks;
    }
    for (int e = 0; e < PNP_NSUM; ++e) if (s1[e] != s2[e] || !pnp_finite(s[e])) return 4;      // weight 1 is the uniform rule
    if (in < 1 || in > 59) return 5;                                                            // five points lie behind the camera
    printf("pnp levels ok: %lld checks\n", checks);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


def _p(a):
    return a.ctypes.data_as(DP)


@pytest.fixture(scope="module")
def pnp(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pnp_levels")
    (tmp / "levels_host.cpp").write_text(LEVELS_WRAPPER)
    so = tmp / "levels_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "levels_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.w_sigma2.restype = ctypes.c_double
    lib.w_inlier_level.argtypes = [DP, DP, DP, DP, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double]

    class Pnp:
        sigma2, max_level = lib.w_sigma2, lib.w_max_level

        @staticmethod
        def inlier(R, t, cam, x, u, v, thr2, s2):
            a = [np.ascontiguousarray(q, dtype=np.float64) for q in (R, t, cam, x)]
            return bool(lib.w_inlier_level(*[_p(q) for q in a], u, v, thr2, s2))

        @staticmethod
        def gn_sums(R, t, cam, X, uv, w=None):
            a = [np.ascontiguousarray(q, dtype=np.float64) for q in (R, t, cam, X, uv)]
            s = np.zeros(27)
            if w is None:
                lib.w_gn_sums(*[_p(q) for q in a], len(a[3]), _p(s))
            else:
                lib.w_gn_sums_level(*[_p(q) for q in a], _p(np.ascontiguousarray(w, dtype=np.float64)), len(a[3]), _p(s))
            return s
    return Pnp


# ---- pnp.h ---------------------------------------------------------------------------------------------------------
def test_sigma2_equals_the_restatement(pnp):
    assert pnp.max_level() == ref.MAX_LEVEL == 7
    got = np.array([pnp.sigma2(l) for l in range(8)])
    assert np.array_equal(got.view(np.uint64), ref.SIGMA2.view(np.uint64))
    assert got[0] == 1.0 and got[1] == 1.44 and np.all(np.abs(got - 1.2 ** (2 * np.arange(8))) <= 8 * EPS * got)


def test_weighted_inlier_rule_at_the_threshold_of_every_level(pnp):
    """Errors placed at thr sigma_l (1 -+ 1e-9), in several directions: inside is an inlier, outside is not, for the header and
    the restatement alike; a point behind the camera never is."""
    R, t = vr.random_rotation(np.random.default_rng(3), 20.0), np.array([0.2, -0.1, 0.3])
    x = np.array([0.4, -0.3, 3.0])
    P = R @ x + t
    pu, pv = vr.CAM[0] * P[0] / P[2] + vr.CAM[2], vr.CAM[1] * P[1] / P[2] + vr.CAM[3]
    n = 0
    for l in range(8):
        s2 = ref.SIGMA2[l]
        for thr in (2.0, 0.5, 3.7):
            for ang in np.linspace(0.0, 2 * np.pi, 7, endpoint=False):
                for rel, want in ((1.0 - 1e-9, True), (1.0 + 1e-9, False)):
                    d = thr * np.sqrt(s2) * rel
                    u, v = pu - d * np.cos(ang), pv - d * np.sin(ang)
                    e2 = vr.reproj_e2(R, t, vr.CAM, x[None], np.array([[u, v]]))
                    assert bool(ref.inliers(e2, np.array([s2]), thr)[0]) is want, (l, thr, ang, rel)
                    assert pnp.inlier(R, t, vr.CAM, x, u, v, thr * thr, s2) is want, (l, thr, ang, rel)
                    # the uniform threshold would decide otherwise from level 1 on
                    if l >= 1 and want:
                        assert not pnp.inlier(R, t, vr.CAM, x, u, v, thr * thr, 1.0)
                    n += 1
    assert n == 8 * 3 * 7 * 2
    behind = (np.array([0.0, 0.0, -3.0]) - t) @ R
    assert not pnp.inlier(R, t, vr.CAM, behind, 100.0, 100.0, 1e30, ref.SIGMA2[7])
    assert not ref.inliers(vr.reproj_e2(R, t, vr.CAM, behind[None], np.array([[100.0, 100.0]])), ref.SIGMA2[7:], 1e15)[0]


def _gn_cases():
    out = []
    for seed in range(12):
        X, uv, lv, T, _ = ref.planted_level_scene(300 + seed, M=40, outliers=0.0)
        rng = np.random.default_rng(seed)
        Re, te = vr.se3_exp(np.concatenate([0.01 * rng.standard_normal(3), 0.02 * rng.standard_normal(3)]))
        out.append((X, uv, lv if seed else np.arange(40) % 8, Re @ T[:3, :3], Re @ T[:3, 3] + te))
    return out


def test_weighted_gauss_newton_sums_stay_within_8_eps_of_their_terms(pnp):
    """The 27 weighted sums within 8 eps sum | terms |, the terms being the 27 per correspondence, in the three comparisons
    that can be made:

      * what the weight adds: pnp_gn_accumulate_level against sum_k w_k term_k with the header's own terms (pnp_gn_accumulate
        of one correspondence on a zeroed s), all 27 sums.  Measured: equal to the last bit.
      * the header against the restatement on the sums of J^T J.  Measured: worst share of the bound 0.36 on 20 of the 21.
        The sum (2, 5) is left to the next point: its term is a^2 px py / pz - b^2 px py / pz, which is zero for a camera
        with fx = fy as here, so sum | terms | is the rounding of an exact cancellation (1e-26 where the entries are 1e5)
        and bounds nothing.
      * the header against the restatement on that sum and on the six sums of J^T r: these MISS the bound, by up to 4.6 times
        on J^T r.  Header and restatement form the residual in another order (x (1 / z) against x / z), and a residual of
        half a pixel is the difference of coordinates of hundreds of pixels, so each term carries their rounding; no
        summation order can meet 8 eps sum | terms | there.  They are held to the tolerance test_vis_cpu.py holds the
        uniform sums to (GN_SUM_TOL: 8 x 64 eps relative to the largest entry; measured 7.5e-15 of 1.1e-13).

    With every weight 1 the weighted form is the uniform one bit for bit."""
    worst_own, worst_a, worst_b, worst_rel = 0.0, 0.0, 0.0, 0.0
    flat = 14                                              # the sum (2, 5) of the upper triangle row by row
    for X, uv, lv, R, t in _gn_cases():
        w = 1.0 / ref.SIGMA2[lv]
        got = pnp.gn_sums(R, t, vr.CAM, X, uv, w)
        own = np.stack([pnp.gn_sums(R, t, vr.CAM, X[k:k + 1], uv[k:k + 1]) for k in range(len(X))]) * w[:, None]
        err, bound = np.abs(got - own.sum(axis=0)), 8 * EPS * np.abs(own).sum(axis=0)
        assert np.all(err <= bound)
        worst_own = max(worst_own, float((err[bound > 0] / bound[bound > 0]).max()))
        terms = ref.gn_terms(R, t, vr.CAM, X, uv, w)
        err, bound = np.abs(got - terms.sum(axis=0)), 8 * EPS * np.abs(terms).sum(axis=0)
        jtj = np.array([e for e in range(21) if e != flat and bound[e] > 0])
        assert len(jtj) >= 18 and not err[:21][bound[:21] == 0].any()      # J has entries that are zero for every correspondence
        assert np.all(err[jtj] <= bound[jtj]), (err[jtj] / bound[jtj]).max()
        worst_a = max(worst_a, float((err[jtj] / bound[jtj]).max()))
        worst_b = max(worst_b, float((err[21:] / bound[21:]).max()))
        A, b = ref.gn_sums(R, t, vr.CAM, X, uv, w)
        rel = max(err[:21].max() / np.abs(A).max(), err[21:].max() / np.abs(b).max())
        worst_rel = max(worst_rel, float(rel))
        assert rel <= GN_SUM_TOL
        assert np.array_equal(A, A.T) and np.array_equal(A[np.triu_indices(6)], terms.sum(axis=0)[:21]) and np.array_equal(b, terms.sum(axis=0)[21:])
        assert np.array_equal(pnp.gn_sums(R, t, vr.CAM, X, uv, np.ones(len(X))), pnp.gn_sums(R, t, vr.CAM, X, uv))
        A1, b1 = ref.gn_sums(R, t, vr.CAM, X, uv, np.ones(len(X)))
        A0, b0 = vr.gn_sums(R, t, vr.CAM, X, uv)
        assert np.abs(A1 - A0).max() <= 64 * EPS * np.abs(A0).max() and np.abs(b1 - b0).max() <= 64 * EPS * np.abs(b0).max()
    print("weighted sums: against the header's own terms, worst share of 8 eps sum |terms| %.3g; header against restatement: J^T J %.3g, "
          "J^T r %.3g of it, %.3g relative to the largest entry" % (worst_own, worst_a, worst_b, worst_rel))


def test_restatement_with_every_level_0_is_the_uniform_restatement():
    X, uv, T, _ = vr.planted_scene(1)
    a = vr.pnp_ransac(X, uv, vr.CAM)
    b = ref.pnp_ransac(X, uv, np.zeros(len(X), dtype=np.int64), vr.CAM)
    assert a["status"] == b["status"] == 0 and a["best_hypothesis"] == b["best_hypothesis"]
    assert np.array_equal(a["inliers"], b["inliers"]) and np.array_equal(a["hyp"]["count"], b["hyp"]["count"])
    assert np.abs(a["T"] - b["T"]).max() <= 1e-12
    for cap_case, status in ((3, 2), (19, 2), (2049, 3)):
        Xs, uvs, _, _ = vr.planted_scene(2, M=cap_case, outliers=0.0)
        assert ref.pnp_ransac(Xs, uvs, np.arange(cap_case) % 4, vr.CAM)["status"] == status


def test_pnp_level_functions_under_sanitizers(tmp_path):
    """The level functions of pnp.h in a stand-alone program with its own main, built with -fsanitize=address,undefined.
    Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "levels_main.cpp").write_text(LEVELS_MAIN)
    exe = tmp_path / "levels_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "levels_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pnp levels ok:" in r.stdout


# ---- the scene -----------------------------------------------------------------------------------------------------
def scene_errors(T, want):
    """(translation error: the largest component in metres, rotation angle in radians) of T against the plant."""
    return float(np.abs(T[:3, 3] - want[:3, 3]).max()), float(np.arccos(np.clip((np.trace(T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def scene_directions():
    """(name, index of the "from" view, index of the "to" view, planted T) of the two directions: A is view 0, B view 1."""
    W = pyr_ref.scene_transform()
    return (("B->A", 1, 0, W), ("A->B", 0, 1, np.linalg.inv(W)))


@pytest.mark.parametrize("direction", [0, 1], ids=["B_to_A", "A_to_B"])
def test_scene_sub_pixel_and_level_aware_halve_the_translation_error(direction):
    """The plane seen from 2.88 m (A) and 2.0 m (B), 4 levels, 300 hypotheses, 2 px, seed 0, on the restatements alone.
    Measured, integer keyframes and uniform PnP against sub-pixel keyframes and level-aware PnP: B->A 0.0257 m / 0.0124 rad
    against 0.0133 m / 0.0066 rad (share 0.52, 86 inliers of 91 matches, guard 0.65 px); A->B 0.0357 m / 0.0124 rad (outside
    the bound of 0.0346 m) against 0.0125 m / 0.0044 rad (share 0.35, 88 of 93, guard 0.096 px).  The guard here is the smallest
    distance from the threshold over the final recounts and over the inlier set of the best hypothesis, which is a decision
    the kernel makes too; over the recounts alone it is 0.95 px for B->A, and the best hypothesis' set brings it to 0.65 px."""
    name, i_from, i_to, want = scene_directions()[direction]
    cam = np.array(pyr_ref.SCENE_CAMERA)
    kf = lambda f: (np.asarray(f["keypoints"], dtype=np.float64), f["points"], f["descriptors"], f["levels"])
    plain, fine = pyr_ref.scene_features(4), sub_ref.scene_features(4)
    m0, rec0 = vr.register(kf(plain[i_from])[:3], kf(plain[i_to])[:3], cam)
    m1, rec1 = ref.register(kf(fine[i_from]), kf(fine[i_to]), cam)
    (t0, r0), (t1, r1) = scene_errors(rec0["T"], want), scene_errors(rec1["T"], want)
    t_bound, r_bound = pyr_ref.scene_bounds()
    print("%s: integer + uniform %d matches, %d inliers, %.4f m / %.4f rad; sub-pixel + level-aware %d matches, %d inliers, "
          "%.4f m / %.4f rad; share %.3f, guard %.3g px (bounds %.4f m, %.4f rad)"
          % (name, len(m0), rec0["inliers"].sum(), t0, r0, len(m1), rec1["inliers"].sum(), t1, r1, t1 / t0, rec1["guard"], t_bound, r_bound))
    assert np.array_equal(m0, m1)                          # the match is unchanged: descriptors do not move
    assert rec1["status"] == 0
    assert t1 <= t_bound and r1 <= r_bound
    assert t1 <= SCENE_GAIN * t0
    assert rec1["guard"] >= SCENE_GUARD


# ---- argument checks -----------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import visual_registration as reg
    d = np.zeros((5, 32), dtype=np.uint8)
    X, uv, lv = np.zeros((5, 3)), np.zeros((5, 2)), np.zeros(5, dtype=np.uint8)
    kf, plain = reg.LevelKeyframe(uv, X, d, lv), reg.Keyframe(uv, X, d)
    cam = vr.CAM
    bad = [lambda: reg.pnp_ransac_level_pairs([(X, uv)], [np.array([0, 1, 2, 3, 8])], cam),      # out of range
           lambda: reg.pnp_ransac_level_pairs([(X, uv)], [np.array([0, -1, 2, 3, 4])], cam),
           lambda: reg.pnp_ransac_level_pairs([(X, uv)], [np.zeros(4, dtype=np.int32)], cam),    # one level per pixel
           lambda: reg.pnp_ransac_level_pairs([(X, uv)], [np.zeros((5, 1), dtype=np.int32)], cam),
           lambda: reg.pnp_ransac_level_pairs([(X, uv)], [np.zeros(5)], cam),                    # whole numbers
           lambda: reg.pnp_ransac_level_pairs([(X, uv)], [], cam),                               # one array per pair
           lambda: reg.pnp_ransac_level_pairs([(X, uv)], [lv], cam, iterations=0),
           lambda: reg.register_level_pairs([(kf, plain)], cam),                                 # a plain Keyframe
           lambda: reg.register_level_pairs([(plain, kf)], cam),
           lambda: reg.compute_level_transformation(plain, plain, cam),
           lambda: reg.compute_level_transformation(kf, reg.LevelKeyframe(uv, X, d, lv[:4]), cam),
           lambda: reg.compute_level_transformation(kf, reg.LevelKeyframe(uv, X, d, np.full(5, 8, dtype=np.uint8)), cam),
           lambda: reg.compute_level_transformation(kf, reg.LevelKeyframe(uv, X[:4], d, lv), cam),
           lambda: reg.compute_level_transformation(kf, kf, cam, nndr=2.0)]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)
    assert reg.VIS_MAX_LEVEL == ref.MAX_LEVEL
    assert reg.LevelKeyframe._fields == reg.Keyframe._fields + ("levels",)


def test_c_entry_points_refuse_levels_out_of_range_before_any_launch():
    """cslam_vis_pnp_levels_dev and cslam_vis_register_levels_dev check the host copy of the levels before they touch the
    device: the buffers here are host memory, which no launch could take."""
    from cslam_amd import _lib
    lib = _lib.load()
    buf = np.zeros(256, dtype=np.float64)
    ptr = buf.ctypes.data
    off = np.array([0, 5], dtype=np.int64)
    for bad in (8, -1):
        lv = np.array([0, 1, 2, bad, 3], dtype=np.int32)
        rc = lib.cslam_vis_pnp_levels_dev(ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, ptr, 1, 300, 2.0, 20, 10, 2, 0, ptr, ptr, ptr,
                                          off.ctypes.data, lv.ctypes.data, None)
        assert rc == -1 and b"levels must be in [0, 7]" in lib.cslam_last_error()
        rc = lib.cslam_vis_register_levels_dev(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, 32, 0.8, 300, 2.0, 20, 10, 2, 0, ptr, ptr, ptr, ptr, ptr,
                                               off.ctypes.data, off.ctypes.data, lv.ctypes.data, None)
        assert rc == -1 and b"levels must be in [0, 7]" in lib.cslam_last_error()
    lv = np.zeros(5, dtype=np.int32)
    rc = lib.cslam_vis_pnp_levels_dev(ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, ptr, 1, 300, 2.0, 20, 10, 2, 0, ptr, ptr, ptr, off.ctypes.data,
                                      None, None)
    assert rc == -1                                        # the host copy is required
