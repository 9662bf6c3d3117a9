"""CPU: the host pieces of the scale pyramid of the keyframe features and their restatement (tests/feat_pyramid_reference.py).

  * csrc/feat_pyr.h compiled by the host C++ compiler against the restatement: level sizes, the taps of every output
    index of every adjacent level pair, the budgets, the level-0 pixel and coordinate rule, the blend of a constant image
  * the same header once more as a stand-alone program under -fsanitize=address,undefined (never loaded into Python)
  * the argument checks of cslam_amd.front_end.visual_pyramid
  * the finding the pyramid exists for, on the restatement alone: the same plane seen from 2.88 m and from 2.0 m gives the
    single-scale chain fewer than 20 matches and the 4-level chain a registration
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import feat_pyramid_reference as ref
import vis_reference
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
N_LO, N_HI = 2, 700

PYR_WRAPPER = r"""
#define __host__
#define __device__
#include "feat_pyr.h"
extern "C" void w_sizes(int n_lo, int n_hi, int *out) {
    for (int n = n_lo; n <= n_hi; ++n) for (int l = 0; l < FEAT_PYR_MAX_LEVELS; ++l) *out++ = feat_pyr_size(n, l);
}
extern "C" void w_taps(int n_l, int n_prev, int *out) {
    for (int x = 0; x < n_l; ++x) feat_pyr_tap(x, n_l, n_prev, out + 3 * x, out + 3 * x + 1, out + 3 * x + 2);
}
extern "C" void w_budgets(int max_features, int levels, int *out) { feat_pyr_budgets(max_features, levels, out); }
extern "C" void w_base(int n_0, int n_l, int *px, double *coord) {
    for (int x = 0; x < n_l; ++x) { px[x] = feat_pyr_base_pixel(x, n_0, n_l); coord[x] = feat_pyr_base_coord(x, n_0, n_l); }
}
extern "C" int w_blend(int g00, int g01, int g10, int g11, int a, int b) { return feat_pyr_blend(g00, g01, g10, g11, a, b); }
extern "C" int w_blend_constant(int g) {
    int wrong = 0;
    for (int a = 0; a < FEAT_PYR_ONE; ++a) for (int b = 0; b < FEAT_PYR_ONE; ++b) wrong += feat_pyr_blend(g, g, g, g, a, b) != g;
    return wrong;
}
extern "C" void w_point(double kx, double ky, double Z, const double *cam, double *p) { feat_pyr_point(kx, ky, Z, cam[0], cam[1], cam[2], cam[3], p); }
extern "C" int w_constants(int *out) { out[0] = FEAT_PYR_MAX_LEVELS; out[1] = FEAT_PYR_MAX_SIDE; out[2] = FEAT_PYR_ONE; return 3; }
"""

# stand-alone: the taps of every adjacent level pair index a buffer of the source's size, the blend stays a byte, the
# level-0 pixel stays inside, the budgets sum
PYR_MAIN = r"""
#include <stdio.h>
#include <vector>
#define __host__
#define __device__
#include "feat_pyr.h"
int main() {
    long long checks = 0;
    for (int n = 2; n <= 700; ++n)
        for (int l = 1; l < FEAT_PYR_MAX_LEVELS; ++l) {
            const int n_prev = feat_pyr_size(n, l - 1), n_l = feat_pyr_size(n, l);
            if (n_l < 1 || n_l > n_prev) return 3;
            std::vector<unsigned char> row((size_t)n_prev, 255), base((size_t)n, 1);
            for (int x = 0; x < n_l; ++x) {
                int i0, i1, a;
                feat_pyr_tap(x, n_l, n_prev, &i0, &i1, &a);
                if (a < 0 || a >= FEAT_PYR_ONE) return 4;
                const int v = feat_pyr_blend(row[i0], row[i1], row[i0], row[i1], a, a);
                if (v != 255) return 5;
                if (base[feat_pyr_base_pixel(x, n, n_l)] != 1) return 6;
                const double k = feat_pyr_base_coord(x, n, n_l);
                if (!(k > -0.5 && k < n - 0.5)) return 7;
                ++checks;
            }
        }
    for (int side : {FEAT_PYR_MAX_SIDE, FEAT_PYR_MAX_SIDE - 1}) {
        const int top = feat_pyr_size(side, 1);
        int i0, i1, a;
        feat_pyr_tap(top - 1, top, side, &i0, &i1, &a);
        if (i0 < 0 || i1 > side - 1 || feat_pyr_base_pixel(top - 1, side, top) > side - 1) return 8;
        ++checks;
    }
    for (int mf = 1; mf <= 65535; mf += 13)
        for (int L = 1; L <= FEAT_PYR_MAX_LEVELS; ++L) {
            int b[FEAT_PYR_MAX_LEVELS], sum = 0;
            feat_pyr_budgets(mf, L, b);
            for (int l = 0; l < L; ++l) { if (b[l] < 0 || (l && b[l] > b[l - 1])) return 9; sum += b[l]; }
            if (sum != mf) return 10;
            ++checks;
        }
    double p[3];
    feat_pyr_point(1.5, 2.5, 0.0, 100.0, 100.0, 3.0, 4.0, p);
    if (p[0] == p[0] || p[2] == p[2]) return 11;
    feat_pyr_point(1.5, 2.5, 2.0, 100.0, 100.0, 3.0, 4.0, p);
    if (p[0] != -0.03 || p[1] != -0.03 || p[2] != 2.0) return 12;
    printf("feat_pyr ok: %lld checks\n", checks);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def pyr(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("feat_pyr")
    (tmp / "pyr_host.cpp").write_text(PYR_WRAPPER)
    so = tmp / "pyr_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "pyr_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    IP, DP = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    lib.w_point.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, DP, DP]

    class Pyr:
        blend, blend_constant = lib.w_blend, lib.w_blend_constant

        @staticmethod
        def sizes():
            out = np.zeros((N_HI - N_LO + 1, 8), dtype=np.int32)
            lib.w_sizes(N_LO, N_HI, out.ctypes.data_as(IP))
            return out

        @staticmethod
        def taps(n_l, n_prev):
            out = np.zeros((n_l, 3), dtype=np.int32)
            lib.w_taps(n_l, n_prev, out.ctypes.data_as(IP))
            return out

        @staticmethod
        def budgets(mf, L):
            out = np.zeros(8, dtype=np.int32)
            lib.w_budgets(mf, L, out.ctypes.data_as(IP))
            return out[:L].tolist()

        @staticmethod
        def base(n_0, n_l):
            px, coord = np.zeros(n_l, dtype=np.int32), np.zeros(n_l, dtype=np.float64)
            lib.w_base(n_0, n_l, px.ctypes.data_as(IP), coord.ctypes.data_as(DP))
            return px, coord

        @staticmethod
        def point(kx, ky, Z, cam):
            cam, p = np.asarray(cam, dtype=np.float64), np.zeros(3, dtype=np.float64)
            lib.w_point(kx, ky, Z, cam.ctypes.data_as(DP), p.ctypes.data_as(DP))
            return p

        @staticmethod
        def constants():
            out = np.zeros(3, dtype=np.int32)
            lib.w_constants(out.ctypes.data_as(IP))
            return out.tolist()
    return Pyr


# ---- feat_pyr.h ----------------------------------------------------------------------------------------------------
def test_level_sizes_equal_the_restatement(pyr):
    got = pyr.sizes()
    want = np.array([[ref.level_size(n, l) for l in range(8)] for n in range(N_LO, N_HI + 1)])
    assert np.array_equal(got, want)
    assert np.all(got[:, 0] == np.arange(N_LO, N_HI + 1)) and np.all(np.diff(got, axis=1) <= 0)
    assert ref.level_sizes((480, 640), 4) == [(480, 640), (400, 533), (333, 444), (278, 370)]
    assert np.all(np.abs(want * 1.2 ** np.arange(8) - want[:, :1]) <= 0.5 * 1.2 ** np.arange(8) + 1e-9)     # n_l is n / 1.2^l rounded
    assert pyr.constants() == [8, 1 << 20, 1024]


def test_taps_of_every_adjacent_level_pair_equal_the_restatement(pyr):
    sizes, pairs = pyr.sizes(), set()
    for row in sizes:
        pairs |= {(int(row[l]), int(row[l - 1])) for l in range(1, 8) if row[l] >= 1}
    assert len(pairs) > 1000
    for n_l, n_prev in sorted(pairs):
        got = pyr.taps(n_l, n_prev)
        i0, i1, a = ref.taps(n_l, n_prev)
        assert np.array_equal(got, np.stack([i0, i1, a], axis=1)), (n_l, n_prev)
        assert got[:, 0].min() >= 0 and got[:, 1].max() <= n_prev - 1 and np.all(np.diff(got[:, 0]) >= 0)
        assert np.all(got[:, 1] - got[:, 0] <= 1)
        if n_l == n_prev:                                  # the same size: the image itself
            assert np.array_equal(got[:, 0], np.arange(n_l)) and not got[:, 2].any()
    # the ratio stays below 2: a 2 x 2 footprint leaves no source pixel between two outputs unread by both
    for n_l, n_prev in sorted(pairs):
        if n_l >= 2:
            assert n_prev < 2 * n_l and np.all(np.diff(pyr.taps(n_l, n_prev)[:, 0]) <= 2)


def test_budgets_sum_and_never_increase_with_the_level(pyr):
    for L in range(1, 9):
        for mf in range(1, 2001):
            b = pyr.budgets(mf, L)
            assert b == ref.budgets(mf, L), (mf, L)
            assert sum(b) == mf and all(x >= y for x, y in zip(b, b[1:])) and min(b) >= 0
    assert pyr.budgets(1000, 4) == [323, 268, 223, 186]
    assert pyr.budgets(1000, 1) == [1000] and pyr.budgets(3, 8) == [3, 0, 0, 0, 0, 0, 0, 0]
    assert pyr.budgets(65535, 8) == ref.budgets(65535, 8)


def test_level_0_pixel_and_coordinate_rule(pyr):
    for n_0 in (2, 3, 39, 40, 49, 144, 192, 480, 640, 700, 1 << 20):
        for l in range(8):
            n_l = ref.level_size(n_0, l)
            if n_l < 1:
                continue
            px, coord = pyr.base(n_0, n_l)
            x = np.arange(n_l)
            assert np.array_equal(px, ref.base_pixel(x, n_0, n_l))
            assert np.array_equal(coord.view(np.uint64), ref.base_coord(x, n_0, n_l).view(np.uint64))
            assert px.min() >= 0 and px.max() <= n_0 - 1
            assert np.all(np.abs(coord - px) <= 0.5)       # the pixel is the one the coordinate lies in
            if l == 0:
                assert np.array_equal(coord, x.astype(np.float64)) and np.array_equal(px, x)


def test_point_rule_equals_the_restatement(pyr):
    cam = (523.7, 519.1, 27.37, 19.81)
    kp = np.array([[3.25, 7.5], [0.0, 0.0], [100.1, 55.9], [12.5, 12.5], [1.0, 2.0], [1.0, 2.0], [1.0, 2.0]])
    Z = np.array([1.5, 2.25, 0.3, 0.0, -1.0, np.nan, np.inf])
    want = ref.points(kp, Z, cam)
    got = np.stack([pyr.point(kp[i, 0], kp[i, 1], Z[i], cam) for i in range(len(kp))])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[3:]).all() and not np.isnan(got[:3]).any()
    assert np.array_equal(got[:3].view(np.uint64), want[:3].view(np.uint64))


def test_a_constant_image_stays_constant(pyr):
    assert pyr.blend_constant(255) == 0 and pyr.blend_constant(0) == 0 and pyr.blend_constant(77) == 0
    assert pyr.blend(255, 255, 255, 255, 1023, 1023) == 255 and pyr.blend(0, 255, 0, 255, 512, 0) == 128
    for value in (0, 255):
        for shape in ((2, 2), (3, 7), (40, 49), (144, 192)):
            levels = ref.pyramid(np.full(shape, value, dtype=np.uint8), 4 if min(shape) > 3 else 2)
            assert all(np.all(g == value) for g in levels)
            assert [g.shape for g in levels] == ref.level_sizes(shape, len(levels))
    rng = np.random.default_rng(0)
    g = rng.integers(0, 256, (17, 15), dtype=np.uint8)
    for l, lev in enumerate(ref.pyramid(g, 5)):            # a blend of four neighbours lies between them
        assert g.min() <= lev.min() and lev.max() <= g.max()
    assert np.array_equal(ref.resample(g, g.shape), g)


# ---- stand-alone under sanitizers ----------------------------------------------------------------------------------
def test_feat_pyr_header_under_sanitizers(tmp_path):
    """Every function of feat_pyr.h in a stand-alone program with its own main, built with -fsanitize=address,undefined:
    the taps of every adjacent level pair of n = 2 .. 700 index a row of the source's size, the level-0 pixel a row of the
    image's, the largest side stays inside int64, the budgets over the whole range of max_features.  Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "pyr_main.cpp").write_text(PYR_MAIN)
    exe = tmp_path / "pyr_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "pyr_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "feat_pyr ok:" in r.stdout


# ---- host rules of the Python layer --------------------------------------------------------------------------------
def test_python_rules_equal_the_restatement():
    from cslam_amd.front_end import visual_pyramid as vp
    for shape in ((2, 2), (39, 39), (40, 49), (144, 192), (480, 640)):
        for L in range(1, 9):
            assert vp.level_sizes(shape, L) == ref.level_sizes(shape, L)
    for mf in (1, 7, 1000, 65535):
        for L in range(1, 9):
            assert vp.level_budgets(mf, L) == ref.budgets(mf, L)
    assert (vp.MAX_LEVELS, vp.LEVEL_RUN, vp.LEVEL_BLOCK) == (8, 4, 256)


def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import visual_pyramid as vp
    img, bgr = np.zeros((48, 64), dtype=np.uint8), np.zeros((48, 64, 3), dtype=np.uint8)
    depth = np.ones((48, 64), dtype=np.float32)
    cam, scam = (100.0, 100.0, 32.0, 24.0), (100.0, 100.0, 32.0, 24.0, 0.1)
    big = np.zeros((68, 68), dtype=np.uint8)               # level 3 of 68 is 39 = 2 * 19 + 1, level 4 is 33
    bad = [lambda: vp.level_sizes((48, 64), 0),
           lambda: vp.level_sizes((48, 64), 9),
           lambda: vp.level_sizes((48, 64), 2.5),
           lambda: vp.level_budgets(1000, 0),
           lambda: vp.level_budgets(0, 4),
           lambda: vp.level_budgets(65536, 4),
           lambda: vp.build_pyramid([img], 0),
           lambda: vp.build_pyramid([img], 9),
           lambda: vp.build_pyramid([bgr], 2),                                               # grey only
           lambda: vp.build_pyramid([img.astype(np.float32)], 2),
           lambda: vp.build_pyramid([np.zeros((2, 2), dtype=np.uint8)], 3),                  # level 2 of 2 is 1
           lambda: vp.build_pyramid([np.zeros((3, 40), dtype=np.uint8)], 5),                 # level 4 of 3 is 1
           lambda: vp.build_pyramid([img], 2, depths=[depth[:, :60]]),
           lambda: vp.build_pyramid([img], 2, depths=[depth, depth]),
           lambda: vp.build_pyramid([img], 2, depths=[depth.astype(np.float64)]),
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=0),
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=9),
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=True),
           lambda: vp.extract_keyframes_pyramid([big], [np.ones((68, 68), dtype=np.float32)], cam, levels=5),
           lambda: vp.extract_keyframes_pyramid([big, img], [np.ones((68, 68), dtype=np.float32), depth], cam, levels=3),   # the second
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=3),              # level 2 of 48 is 33 < 39
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=1, border=17),
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=1, border=24),   # 48 < 2 * 24 + 1
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=1, min_distance=0),
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=1, max_features=0),
           lambda: vp.extract_keyframes_pyramid([img], [depth], cam, levels=1, quality_level=1.5),
           lambda: vp.extract_keyframes_pyramid([img], [depth[:, :60]], cam, levels=1),
           lambda: vp.extract_keyframes_pyramid([img], [depth, depth], cam, levels=1),
           lambda: vp.extract_keyframes_pyramid([img], [depth], (100.0, 100.0, 32.0), levels=1),
           lambda: vp.extract_keyframes_stereo_pyramid([img], [img], scam, levels=0),
           lambda: vp.extract_keyframes_stereo_pyramid([img], [img], scam, levels=3),        # too small for level 2
           lambda: vp.extract_keyframes_stereo_pyramid([img], [img[:, :60]], scam, levels=1),
           lambda: vp.extract_keyframes_stereo_pyramid([img], [img], cam, levels=1),         # four numbers: no baseline
           lambda: vp.extract_keyframes_stereo_pyramid([img], [img], scam, levels=1, max_disparity=256),
           lambda: vp.extract_keyframes_stereo_pyramid([img], [img], scam, levels=1, border=17),
           lambda: vp.merge_levels([(48, 64)], [], cam),
           lambda: vp.merge_levels([(48, 64)], [[dict(keypoints=np.array([[64, 3]]), responses=[1], bins=[0],
                                                      descriptors=np.zeros((1, 32), dtype=np.uint8), z=[1.0])]], cam),
           lambda: vp.merge_levels([(48, 64)], [[dict(keypoints=np.array([[5, 3]]), responses=[1, 2], bins=[0],
                                                      descriptors=np.zeros((1, 32), dtype=np.uint8), z=[1.0])]], cam)]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)


# ---- the finding the pyramid exists for ----------------------------------------------------------------------------
def _matches_near_the_plant(a, b):
    rows = vis_reference.match(a["descriptors"], b["descriptors"])
    d = np.linalg.norm(ref.scene_map(np.asarray(a["keypoints"], dtype=np.float64)[rows[:, 0]]) - b["keypoints"][rows[:, 1]], axis=1)
    return rows, d <= 2.0


def test_two_distances_defeat_one_scale_and_not_four_levels():
    """The plane of random cells seen from 2.88 m (blocks of 10 pixels) and from 2.0 m (14.4 pixels), 144 x 192, on the
    restatement alone.  Measured: one scale 173 and 74 keypoints, 5 matches, 1 within 2 px of the planted map; 4 levels 397
    and 244 keypoints, 93 matches, 87 within 2 px, of which 57 pair level 0 of the far view with level 2 of the near one and
    26 level 1 with level 3 (1.2^2 = 1.44).  PnP RANSAC of the restatement from the near view to the far one: 86 inliers of 91
    usable matches, translation 0.0257 m from the plant (bound 0.0346 m), rotation 0.0124 rad (bound 0.036 rad)."""
    sa, sb = ref.scene_features(0)
    rows, near = _matches_near_the_plant(sa, sb)
    print("one scale: %d and %d keypoints, %d matches, %d within 2 px" % (len(sa["keypoints"]), len(sb["keypoints"]), len(rows), near.sum()))
    assert len(rows) < 20
    pa, pb = ref.scene_features(4)
    rows, near = _matches_near_the_plant(pa, pb)
    pairs, counts = np.unique(np.stack([pa["levels"][rows[near, 0]], pb["levels"][rows[near, 1]]], axis=1), axis=0, return_counts=True)
    print("4 levels: %d and %d keypoints, %d matches, %d within 2 px, level pairs %s x %s"
          % (len(pa["keypoints"]), len(pb["keypoints"]), len(rows), near.sum(), pairs.tolist(), counts.tolist()))
    assert near.sum() >= 20
    assert counts[pairs[:, 1] - pairs[:, 0] == 2].sum() > near.sum() // 2
    # the restatement itself stays inside the bound of the GPU end-to-end test
    kf = lambda f: (np.asarray(f["keypoints"], dtype=np.float64), f["points"], f["descriptors"])
    m, rec = vis_reference.register(kf(pb), kf(pa), np.array(ref.SCENE_CAMERA))
    T, want = rec["T"], ref.scene_transform()
    t_err = np.abs(T[:3, 3] - want[:3, 3]).max()
    angle = float(np.arccos(np.clip((np.trace(T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    t_bound, r_bound = ref.scene_bounds()
    print("registration near -> far: status %d, %d matches, %d inliers, translation error %.3g m (bound %.3g), rotation %.3g rad (bound %.3g)"
          % (rec["status"], len(m), rec["inliers"].sum(), t_err, t_bound, angle, r_bound))
    assert rec["status"] == 0 and rec["inliers"].sum() >= 20
    assert t_err <= t_bound and angle <= r_bound
    m1, rec1 = vis_reference.register(kf(sb), kf(sa), np.array(ref.SCENE_CAMERA))
    assert rec1["status"] != 0                             # one scale verifies nothing
