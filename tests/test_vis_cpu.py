"""CPU: the host pieces of the visual verification and its float64 restatement (tests/vis_reference.py).

  * csrc/pnp.h compiled by the host C++ compiler: the sampler integer for integer, P3P on planted triples and on degenerate
    input, the Gauss-Newton sums, step and singularity rule
  * the same header once more as a stand-alone program under -fsanitize=address,undefined (never loaded into Python)
  * the argument checks of cslam_amd.front_end.visual_registration and `to_edge`
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import vis_reference as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int32)

# Tolerances: 8 x the restatement's own worst error on the same input (contraction and summation order differ between the
# header and numpy).  Measured on the 1000 triples of `triples()`:
#   some root against the plant (largest entry of R - R*, t - t*): restatement 3.66e-11, header 2.51e-11
#   reprojection of the three points by every root:                restatement 1.13e-11 px, header 2.2e-11 px
#   |R^T R - I| and |det R - 1| of every root:                     restatement 6.7e-13, header 1.38e-12
P3P_PLANT_TOL = 8 * 3.66e-11
P3P_REPROJ_TOL = 8 * 1.13e-11
P3P_ORTHO_TOL = 8 * 6.7e-13
# Gauss-Newton on the 12 scenes of `gn_cases()`: the restatement's step against the step from a central-difference Jacobian
# (h = 1e-6): worst relative difference 2.15e-10 (the header: 2.15e-10); the header's sums against the restatement's: both are
# float64 sums of the same 40 terms in another order, allowed 8 x 64 eps relative to the largest entry (measured 9.6e-15)
GN_STEP_TOL = 8 * 2.15e-10
GN_SUM_TOL = 8 * 64 * 2.2e-16

PNP_WRAPPER = r"""
#define __host__
#define __device__
#include "pnp.h"
extern "C" void w_sample(unsigned long long seed, unsigned h, int M, int *idx) { pnp_sample(seed, h, M, idx); }
extern "C" int w_p3p(const double *X, const double *Yb, double *Rs, double *ts) { return pnp_p3p(X, Yb, Rs, ts); }
extern "C" int w_hypothesis(const double *X4, const double *uv4, const double *cam, double *R, double *t) {
    return pnp_hypothesis(X4, uv4, cam, R, t) ? 1 : 0;
}
extern "C" void w_gn_sums(const double *R, const double *t, const double *cam, const double *X, const double *uv, int n, double *s) {
    for (int e = 0; e < PNP_NSUM; ++e) s[e] = 0.0;
    for (int k = 0; k < n; ++k) pnp_gn_accumulate(R, t, cam, X + 3 * k, uv[2 * k], uv[2 * k + 1], s);
}
extern "C" int w_gn_solve(const double *s, double *x) { return pnp_gn_solve(s, x) ? 1 : 0; }
extern "C" double w_gn_apply(const double *delta, double *R, double *t) { return pnp_gn_apply(delta, R, t); }
extern "C" int w_inlier(const double *R, const double *t, const double *cam, const double *x, double u, double v, double thr2) {
    return pnp_inlier(R, t, cam, x, u, v, thr2) ? 1 : 0;
}
"""

# stand-alone: per case of the file 12 point coordinates, 8 pixel coordinates; every function of pnp.h runs on it
PNP_MAIN = r"""
#include <stdio.h>
#define __host__
#define __device__
#include "pnp.h"
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    const double cam[4] = {525.0, 525.0, 319.5, 239.5};
    double X4[12], uv4[8];
    int cases = 0, roots = 0, solved = 0;
    while (true) {
        int got = 0;
        for (int e = 0; e < 12; ++e) got += fscanf(f, "%lf", &X4[e]) == 1;
        for (int e = 0; e < 8; ++e) got += fscanf(f, "%lf", &uv4[e]) == 1;
        if (got != 20) break;
        double Yb[9], Rs[36], ts[12], R[9], t[3];
        for (int i = 0; i < 3; ++i) { Yb[3 * i] = (uv4[2 * i] - cam[2]) / cam[0]; Yb[3 * i + 1] = (uv4[2 * i + 1] - cam[3]) / cam[1]; Yb[3 * i + 2] = 1.0; }
        const int n = pnp_p3p(X4, Yb, Rs, ts);
        if (n < 0 || n > 4) return 3;
        for (int e = 0; e < 9 * n; ++e) if (!pnp_finite(Rs[e])) return 4;
        for (int e = 0; e < 3 * n; ++e) if (!pnp_finite(ts[e])) return 4;
        roots += n;
        const int k = pnp_select(n, Rs, ts, cam, X4 + 9, uv4[6], uv4[7]);
        if ((n == 0) != (k < 0) || k >= n) return 5;
        if (pnp_hypothesis(X4, uv4, cam, R, t)) {
            double s[PNP_NSUM], delta[6], e2;
            for (int e = 0; e < PNP_NSUM; ++e) s[e] = 0.0;
            for (int j = 0; j < 4; ++j) {
                pnp_gn_accumulate(R, t, cam, X4 + 3 * j, uv4[2 * j], uv4[2 * j + 1], s);
                pnp_reproject(R, t, cam, X4 + 3 * j, uv4[2 * j], uv4[2 * j + 1], &e2);
                (void)pnp_inlier(R, t, cam, X4 + 3 * j, uv4[2 * j], uv4[2 * j + 1], 4.0);
            }
            if (pnp_gn_solve(s, delta)) {
                const double nd = pnp_gn_apply(delta, R, t);
                if (!pnp_finite(nd)) return 6;
                ++solved;
            } else {
                for (int e = 0; e < 6; ++e) if (delta[e] != 0.0) return 7;
            }
        }
        const int Ms[4] = {4, 5, 6, 2048};
        for (int m = 0; m < 4; ++m) {
            int idx[4];
            pnp_sample(0x1234567ull + cases, (unsigned)cases, Ms[m], idx);
            for (int a = 0; a < 4; ++a) {
                if (idx[a] < 0 || idx[a] >= Ms[m]) return 8;
                for (int b = 0; b < a; ++b) if (idx[a] == idx[b]) return 9;
            }
        }
        ++cases;
    }
    fclose(f);
    printf("pnp ok: %d cases, %d roots, %d steps\n", cases, roots, solved);
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
    tmp = tmp_path_factory.mktemp("pnp")
    (tmp / "pnp_host.cpp").write_text(PNP_WRAPPER)
    so = tmp / "pnp_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "pnp_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.w_gn_apply.restype = ctypes.c_double
    lib.w_sample.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, IP]
    lib.w_inlier.argtypes = [DP, DP, DP, DP, ctypes.c_double, ctypes.c_double, ctypes.c_double]

    class Pnp:
        @staticmethod
        def sample(seed, h, M):
            idx = np.zeros(4, dtype=np.int32)
            lib.w_sample(seed, h, M, idx.ctypes.data_as(IP))
            return [int(i) for i in idx]

        @staticmethod
        def p3p(X, Yb):
            X, Yb = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Yb, dtype=np.float64)
            Rs, ts = np.full((4, 3, 3), np.nan), np.full((4, 3), np.nan)
            n = lib.w_p3p(_p(X), _p(Yb), _p(Rs), _p(ts))
            return [(Rs[k].copy(), ts[k].copy()) for k in range(n)]

        @staticmethod
        def gn_sums(R, t, cam, X, uv):
            a = [np.ascontiguousarray(x, dtype=np.float64) for x in (R, t, cam, X, uv)]
            s = np.zeros(27)
            lib.w_gn_sums(*[_p(x) for x in a], len(a[3]), _p(s))
            A = np.zeros((6, 6))
            A[np.triu_indices(6)] = s[:21]
            return A + np.triu(A, 1).T, s[21:].copy(), s

        @staticmethod
        def gn_solve(s):
            x = np.full(6, np.nan)
            ok = lib.w_gn_solve(_p(np.ascontiguousarray(s)), _p(x))
            return bool(ok), x

        @staticmethod
        def gn_apply(delta, R, t):
            R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
            n = lib.w_gn_apply(_p(np.ascontiguousarray(delta)), _p(R), _p(t))
            return R, t, n
    return Pnp


# ---- sampler -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 5, 6, 2048])
def test_sampler_equals_the_restatement_and_is_distinct(pnp, M):
    for seed in (0, 1, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15):
        for h in list(range(300)) + [65535, 2 ** 24 - 1]:
            idx = pnp.sample(seed, h, M)
            assert idx == ref.sample(seed, h, M), (seed, h, M)
            assert len(set(idx)) == 4 and all(0 <= i < M for i in idx)
            if M == 4:
                assert sorted(idx) == [0, 1, 2, 3]


def test_sampler_takes_the_lowest_unused_index_after_16_attempts():
    """M = 4 exhausts the 16 attempts of the last slot with probability (3/4)^16 ~ 1 %: among 3000 hypotheses some do, and
    the restatement (which the header equals integer for integer) then takes the one index left."""
    fell = 0
    for h in range(3000):
        s = ref.mix64(7)
        idx = ref.sample(7, h, 4)
        draws = [ref.mix64((s + ((h << 6) | (3 << 4) | a)) & ref.MASK) % 4 for a in range(16)]
        if all(d in idx[:3] for d in draws):
            fell += 1
            assert idx[3] == min(set(range(4)) - set(idx[:3]))
    assert fell > 0


# ---- P3P -----------------------------------------------------------------------------------------------------------
def triples(n=1000, seed=5):
    """Well-conditioned triples with planted poses: pixels at least 60 px apart, depths 1-10 m, rotations up to 60 deg."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        X, uv, T, _ = ref.planted_scene(int(rng.integers(1 << 30)), M=3, outliers=0.0, noise=0.0, max_deg=60.0)
        d = [np.linalg.norm(uv[a] - uv[b]) for a, b in ((0, 1), (0, 2), (1, 2))]
        e1, e2 = uv[1] - uv[0], uv[2] - uv[0]
        area = abs(e1[0] * e2[1] - e1[1] * e2[0])
        if min(d) >= 60.0 and area >= 3000.0:
            Yb = np.stack([(uv[:, 0] - ref.CAM[2]) / ref.CAM[0], (uv[:, 1] - ref.CAM[3]) / ref.CAM[1], np.ones(3)], axis=1)
            out.append((X, Yb, uv, T))
    return out


def p3p_errors(solver, cases):
    plant, reproj, ortho = 0.0, 0.0, 0.0
    for X, Yb, uv, T in cases:
        roots = solver(X, Yb)
        assert 1 <= len(roots) <= 4
        plant = max(plant, min(max(np.abs(R - T[:3, :3]).max(), np.abs(t - T[:3, 3]).max()) for R, t in roots))
        for R, t in roots:
            assert np.all(np.isfinite(R)) and np.all(np.isfinite(t))
            reproj = max(reproj, float(np.sqrt(ref.reproj_e2(R, t, ref.CAM, X, uv).max())))
            ortho = max(ortho, np.abs(R.T @ R - np.identity(3)).max(), abs(np.linalg.det(R) - 1.0))
    return plant, reproj, ortho


def test_p3p_on_planted_triples(pnp):
    cases = triples()
    r_plant, r_reproj, r_ortho = p3p_errors(lambda X, Yb: ref.p3p(X, Yb)[0], cases)
    print("restatement: plant %.3g reprojection %.3g px orthonormality %.3g" % (r_plant, r_reproj, r_ortho))
    plant, reproj, ortho = p3p_errors(pnp.p3p, cases)
    print("pnp.h:       plant %.3g reprojection %.3g px orthonormality %.3g" % (plant, reproj, ortho))
    assert plant <= P3P_PLANT_TOL and reproj <= P3P_REPROJ_TOL and ortho <= P3P_ORTHO_TOL


def degenerate_cases():
    rng = np.random.default_rng(11)
    Yb = np.array([[0.1, 0.0, 1.0], [-0.2, 0.1, 1.0], [0.05, -0.3, 1.0]])
    line = np.array([0.0, 0.0, 4.0]) + np.array([-1.0, 0.0, 1.0])[:, None] * np.array([1.0, 0.5, 0.2])
    cases = [("collinear", line, Yb), ("coincident", np.tile([1.0, 2.0, 5.0], (3, 1)), Yb),
             ("two coincident", np.array([[1.0, 2.0, 5.0], [1.0, 2.0, 5.0], [0.0, 1.0, 4.0]]), Yb),
             ("zero bearing", rng.standard_normal((3, 3)), np.zeros((3, 3))),
             ("equal bearings", rng.standard_normal((3, 3)) + [0, 0, 5], np.tile([0.1, 0.2, 1.0], (3, 1))),
             ("huge", 1e200 * rng.standard_normal((3, 3)), Yb), ("nan", np.full((3, 3), np.nan), Yb),
             ("inf", np.full((3, 3), np.inf), Yb)]
    for k in range(20):                                     # points behind the camera: the plant puts them at negative depth
        X, uv, T, _ = ref.planted_scene(100 + k, M=3, outliers=0.0, noise=0.0)
        P = X @ T[:3, :3].T + T[:3, 3]
        Xb = (-P - T[:3, 3]) @ T[:3, :3]
        cases.append(("behind %d" % k, Xb, np.stack([(uv[:, 0] - ref.CAM[2]) / ref.CAM[0], (uv[:, 1] - ref.CAM[3]) / ref.CAM[1], np.ones(3)], axis=1)))
    return cases


def test_p3p_degenerate_input_gives_no_root_or_finite_roots(pnp):
    for name, X, Yb in degenerate_cases():
        for solver in (pnp.p3p, lambda X, Yb: ref.p3p(X, Yb)[0]):
            roots = solver(X, Yb)
            assert 0 <= len(roots) <= 4, name
            for R, t in roots:
                assert np.all(np.isfinite(R)) and np.all(np.isfinite(t)), name
        if name in ("collinear", "coincident", "two coincident", "zero bearing", "nan", "inf"):
            assert pnp.p3p(X, Yb) == [], name


# ---- Gauss-Newton --------------------------------------------------------------------------------------------------
def gn_cases():
    out = []
    for seed in range(12):
        X, uv, T, _ = ref.planted_scene(300 + seed, M=40, outliers=0.0, noise=0.5)
        rng = np.random.default_rng(seed)
        Re, te = ref.se3_exp(np.concatenate([0.01 * rng.standard_normal(3), 0.02 * rng.standard_normal(3)]))
        out.append((X, uv, Re @ T[:3, :3], Re @ T[:3, 3] + te))
    return out


def numeric_step(R, t, X, uv, h=1e-6):
    def residual(d):
        Re, te = ref.se3_exp(d)
        Rn, tn = Re @ R, Re @ t + te
        P = X @ Rn.T + tn
        return np.stack([ref.CAM[0] * P[:, 0] / P[:, 2] + ref.CAM[2] - uv[:, 0], ref.CAM[1] * P[:, 1] / P[:, 2] + ref.CAM[3] - uv[:, 1]], axis=1).reshape(-1)
    J = np.stack([(residual(h * e) - residual(-h * e)) / (2 * h) for e in np.identity(6)], axis=1)
    return -np.linalg.solve(J.T @ J, J.T @ residual(np.zeros(6)))


def test_gauss_newton_sums_and_step(pnp):
    worst_ref, worst_hdr, worst_sum = 0.0, 0.0, 0.0
    for X, uv, R, t in gn_cases():
        A_ref, b_ref = ref.gn_sums(R, t, ref.CAM, X, uv)
        A, b, s = pnp.gn_sums(R, t, ref.CAM, X, uv)
        worst_sum = max(worst_sum, np.abs(A - A_ref).max() / np.abs(A_ref).max(), np.abs(b - b_ref).max() / np.abs(b_ref).max())
        num = numeric_step(R, t, X, uv)
        d_ref = ref.gn_solve(A_ref, b_ref)
        ok, d = pnp.gn_solve(s)
        assert ok and d_ref is not None
        worst_ref = max(worst_ref, np.abs(d_ref - num).max() / np.abs(num).max())
        worst_hdr = max(worst_hdr, np.abs(d - num).max() / np.abs(num).max())
        # the step is applied on the left: Exp(delta) T
        Rn, tn, nd = pnp.gn_apply(d, R, t)
        Re, te = ref.se3_exp(d)
        assert np.abs(Rn - Re @ R).max() < 1e-14 and np.abs(tn - (Re @ t + te)).max() < 1e-13 and abs(nd - np.linalg.norm(d)) < 1e-15
    print("sums: header against restatement %.3g; step against central differences: restatement %.3g, header %.3g"
          % (worst_sum, worst_ref, worst_hdr))
    assert worst_sum <= GN_SUM_TOL and worst_hdr <= GN_STEP_TOL


def test_gauss_newton_reports_singular_on_a_line(pnp):
    X, uv, T, _ = ref.planted_scene(21, M=30, outliers=0.0, noise=0.3, shape="line")
    A, b, s = pnp.gn_sums(T[:3, :3], T[:3, 3], ref.CAM, X, uv)
    ok, d = pnp.gn_solve(s)
    assert not ok and np.array_equal(d, np.zeros(6))
    assert ref.gn_solve(*ref.gn_sums(T[:3, :3], T[:3, 3], ref.CAM, X, uv)) is None
    ok, d = pnp.gn_solve(np.zeros(27))                      # no correspondence at all
    assert not ok and np.array_equal(d, np.zeros(6))
    bad = s.copy()
    bad[3] = np.nan
    ok, d = pnp.gn_solve(bad)
    assert not ok and np.array_equal(d, np.zeros(6))


def test_a_point_behind_the_camera_adds_nothing(pnp):
    X, uv, R, t = gn_cases()[0]
    _, _, s0 = pnp.gn_sums(R, t, ref.CAM, X, uv)
    Xb = np.concatenate([X, (np.array([[0.0, 0.0, -3.0]]) - t) @ R])
    _, _, s1 = pnp.gn_sums(R, t, ref.CAM, Xb, np.concatenate([uv, [[100.0, 100.0]]]))
    assert np.array_equal(s0, s1)


# ---- the restatement alone -----------------------------------------------------------------------------------------
def test_restatement_solves_a_planted_scene():
    X, uv, T, out = ref.planted_scene(1)
    r = ref.pnp_ransac(X, uv, ref.CAM)
    assert r["status"] == 0 and not np.any(r["inliers"] & out) and r["inliers"].sum() >= 90
    assert np.abs(r["T"] - T).max() < 5e-3


def test_restatement_matcher_rules():
    rng = np.random.default_rng(0)
    b = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    a = b[[3, 3, 1]].copy()
    a[1, 0] ^= 1                                            # rows 0 and 1 both claim "to" row 3: distance 0 beats 1
    assert ref.match(a, b).tolist() == [[0, 3], [2, 1]]
    assert ref.match(a, b[:1]).shape == (0, 2)              # a ratio test needs two rows
    assert ref.match(b[:2], np.concatenate([b[:1], b[:1]]), 0.8).tolist() == [[0, 0]]       # 0 <= 0.8 * 0


@pytest.mark.parametrize("M", ref.HYP_SIZES)
def test_restatement_keeps_the_hypothesis_scenes_within_the_guard_share(M):
    """The scenes of the per-hypothesis GPU test, on the restatement alone: at most 5 % of the 300 hypotheses lie below the
    conditioning guard (measured: 0, 0, 1.0, 2.0, 2.7, 2.7 %), and no (hypothesis, point) error is within 1e-6 px of the
    threshold, so the best hypothesis and its inlier set never depend on the guard."""
    X, uv, _, _ = ref.hyp_scene(M)
    h = ref.hypotheses(X, uv, ref.CAM, 300, 2.0, M)
    low = (h["guard_roots"] < ref.HYP_GUARD) | (h["guard_threshold"] < ref.HYP_GUARD)
    print("M %d: %.1f %% below the guard" % (M, 100 * low.mean()))
    assert low.mean() <= 0.05
    assert np.all(h["guard_threshold"][h["valid"]] >= 1e-6)


# ---- stand-alone under sanitizers ----------------------------------------------------------------------------------
def test_pnp_header_under_sanitizers(tmp_path):
    """Every function of pnp.h in a stand-alone program with its own main, built with -fsanitize=address,undefined, run once
    over the planted triples (with a fourth point), the degenerate cases and the line scene.  Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "pnp_main.cpp").write_text(PNP_MAIN)
    exe = tmp_path / "pnp_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "pnp_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    cases = []
    for k in range(200):
        X, uv, _, _ = ref.planted_scene(500 + k, M=4, outliers=0.25 if k % 4 == 0 else 0.0, noise=0.5)
        cases.append((X, uv))
    for name, X, Yb in degenerate_cases():
        if np.all(np.isfinite(X)):
            uv = np.stack([Yb[:, 0] * ref.CAM[0] + ref.CAM[2], Yb[:, 1] * ref.CAM[1] + ref.CAM[3]], axis=1)
            cases.append((np.concatenate([X, [[0.3, 0.2, 3.0]]]), np.concatenate([uv, [[300.0, 200.0]]])))
    X, uv, _, _ = ref.planted_scene(21, M=4, outliers=0.0, noise=0.3, shape="line")
    cases.append((X, uv))
    with open(tmp_path / "cases.txt", "w") as f:
        for X, uv in cases:
            f.write(" ".join("%.17g" % v for v in np.concatenate([X.reshape(-1), uv.reshape(-1)])) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pnp ok: %d cases" % len(cases) in r.stdout


# ---- host checks of the Python layer -------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import visual_registration as vr
    d = np.zeros((5, 32), dtype=np.uint8)
    X, uv = np.zeros((5, 3)), np.zeros((5, 2))
    kf = vr.Keyframe(uv, X, d)
    cam = ref.CAM
    bad = [lambda: vr.match_descriptors(np.zeros((5, 64), dtype=np.uint8), d),              # descriptor width
           lambda: vr.match_descriptors(d, np.zeros((5, 31), dtype=np.uint8)),
           lambda: vr.match_descriptors(d.astype(np.float32), d),                           # not bytes
           lambda: vr.match_descriptors(d.reshape(-1), d),                                  # shape
           lambda: vr.match_descriptors(d, d, nndr=1.5),
           lambda: vr.match_descriptors(d, d, nndr=-0.1),
           lambda: vr.pnp_ransac_pairs([(np.zeros((5, 2)), uv)], cam),                      # shapes
           lambda: vr.pnp_ransac_pairs([(X, np.zeros((5, 3)))], cam),
           lambda: vr.pnp_ransac_pairs([(X, np.zeros((4, 2)))], cam),
           lambda: vr.pnp_ransac_pairs([(X, uv)], [0.0, 525.0, 320.0, 240.0]),              # intrinsics
           lambda: vr.pnp_ransac_pairs([(X, uv)], [525.0, -1.0, 320.0, 240.0]),
           lambda: vr.pnp_ransac_pairs([(X, uv)], [525.0, 525.0, np.nan, 240.0]),
           lambda: vr.pnp_ransac_pairs([(X, uv)], np.ones((2, 4))),                         # one camera per pair
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, iterations=0),
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, reproj_error=0.0),
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, reproj_error=-2.0),
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, reproj_error=np.inf),
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, min_inliers=0),
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, refine_iterations=-1),
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, refine_rounds=-1),
           lambda: vr.pnp_ransac_pairs([(X, uv)], cam, seed=-1),
           lambda: vr.hypotheses((X, uv), cam, iterations=0),
           lambda: vr.hypotheses((X, uv), cam, reproj_error=0.0),
           lambda: vr.compute_transformation(kf, vr.Keyframe(uv, X[:4], d), cam),            # a keyframe's rows disagree
           lambda: vr.compute_transformation(kf, vr.Keyframe(uv, X, np.zeros((5, 16), dtype=np.uint8)), cam),
           lambda: vr.compute_transformation(kf, kf, cam, iterations=0),
           lambda: vr.compute_transformation(kf, kf, cam, nndr=2.0),
           lambda: vr.register_pairs([(kf, kf)], [525.0, 525.0, 320.0])]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)
    assert (vr.VIS_MATCH_BLOCK, vr.VIS_MATCH_CHUNK, vr.VIS_MAX_CORR) == (256, 256, 2048)


def test_to_edge_round_trip_and_refusal():
    from cslam_amd.back_end.pose_graph import DEFAULT_NOISE_STD, PoseGraphEdge, _edge
    from cslam_amd.front_end.visual_registration import VisualRegistration
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = ref.random_rotation(np.random.default_rng(3), 30.0), [0.3, -0.2, 1.0]
    reg = VisualRegistration(T, True, 0, np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=bool), 0, 7)
    e = reg.to_edge((0, 12), (1, 5))
    assert isinstance(e, PoseGraphEdge) and e.key_from == (0, 12) and e.key_to == (1, 5)
    assert np.array_equal(e.noise_std, DEFAULT_NOISE_STD)
    # the between factor measures pose(from)^-1 pose(to); T = pose(to)^-1 pose(from) maps "from" points into "to"
    assert np.abs(e.measurement @ T - np.identity(4)).max() < 1e-15
    pose_from = np.identity(4)
    pose_from[:3, :3], pose_from[:3, 3] = ref.random_rotation(np.random.default_rng(4), 90.0), [5.0, 1.0, -2.0]
    pose_to = pose_from @ np.linalg.inv(T)
    assert np.abs(np.linalg.inv(pose_from) @ pose_to - e.measurement).max() < 1e-14
    kf, kt, meas, std = _edge(e)
    assert kf == (0, 12) and kt == (1, 5) and meas is e.measurement
    assert reg.to_edge((0, 1), (0, 9), noise_std=[1, 1, 1, 2, 2, 2]).noise_std.tolist() == [1, 1, 1, 2, 2, 2]
    for status in (1, 2, 3):
        with pytest.raises(ValueError):
            VisualRegistration(T, False, status, np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=bool), 0, -1).to_edge((0, 1), (0, 9))
