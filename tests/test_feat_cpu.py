"""CPU: the host pieces of the keyframe features and their integer restatement (tests/feat_reference.py).

  * csrc/feat.h compiled by the host C++ compiler: the generator and the pattern integer for integer, the 32 rotated
    patterns, the quarter turns, the bin rule, the grey rule, the exact integer square root and the response
  * the same header once more as a stand-alone program under -fsanitize=address,undefined (never loaded into Python)
  * the argument checks of cslam_amd.front_end.visual_features, `is_new_keyframe`, the uint16 depth conversion
"""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import feat_reference as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
D_BOUND = 440_000_000_000_000      # (a - c)^2 + 4 b^2 <= 5 * 9363600^2 = 4.4e14

FEAT_WRAPPER = r"""
#define __host__
#define __device__
#include "feat.h"
static const FeatPattern g_pat = feat_make_pattern();
extern "C" unsigned long long w_mix64(unsigned long long z) { return feat_mix64(z); }
extern "C" void w_pattern(int *out) { for (int i = 0; i < FEAT_PAIRS; ++i) for (int e = 0; e < 4; ++e) out[4 * i + e] = g_pat.v[i][e]; }
extern "C" void w_rotate(int x, int y, int k, int *out) { feat_rotate(x, y, k, out, out + 1); }
extern "C" void w_direction(int k, int *out) { feat_direction(k, out, out + 1); }
extern "C" int w_bin(long long m10, long long m01) { return feat_bin(m10, m01); }
extern "C" int w_gray(int b, int g, int r) { return feat_gray(b, g, r); }
extern "C" long long w_isqrt(long long d) { return feat_isqrt(d); }
extern "C" int w_response(long long a, long long b, long long c) { return feat_response(a, b, c); }
extern "C" int w_constants(int *out) {
    out[0] = FEAT_PATCH_RADIUS; out[1] = FEAT_BLUR_RADIUS; out[2] = FEAT_MIN_BORDER; out[3] = FEAT_PATTERN_RADIUS;
    out[4] = FEAT_PAIRS; out[5] = FEAT_DESC_BYTES; out[6] = FEAT_BINS; out[7] = FEAT_R_MAX;
    return 8;
}
"""

# stand-alone: every function of feat.h over its whole domain of small arguments and the edges of the large ones
FEAT_MAIN = r"""
#include <stdio.h>
#include <initializer_list>
#define __host__
#define __device__
#include "feat.h"
int main() {
    static const FeatPattern pat = feat_make_pattern();
    long long checks = 0;
    for (int k = 0; k < FEAT_BINS; ++k)
        for (int i = 0; i < FEAT_PAIRS; ++i)
            for (int e = 0; e < 4; e += 2) {
                int x, y;
                feat_rotate(pat.v[i][e], pat.v[i][e + 1], k, &x, &y);
                if (x * x + y * y > FEAT_PATCH_RADIUS * FEAT_PATCH_RADIUS) return 3;
                static int blurred[(2 * FEAT_PATCH_RADIUS + 1) * (2 * FEAT_PATCH_RADIUS + 1)];
                blurred[(y + FEAT_PATCH_RADIUS) * (2 * FEAT_PATCH_RADIUS + 1) + x + FEAT_PATCH_RADIUS] += 1;   // the kernel's index
                ++checks;
            }
    const long long sums[] = {0, 1, 1020, 9363600};
    for (long long a : sums) for (long long c : sums) for (long long b : {-9363600ll, -1ll, 0ll, 1ll, 9363600ll}) {
        if (b * b > a * c && !(a == 0 && c == 0 && b == 0)) continue;          // not a sum of squares (Cauchy-Schwarz)
        const int r = feat_response(a, b, c);
        if (r < 0 || r > FEAT_R_MAX) return 4;
        ++checks;
    }
    for (long long s = 0; s <= 20976177; s += 997) {
        const long long d = s * s;
        if (feat_isqrt(d) != s || (d > 0 && feat_isqrt(d - 1) != s - 1) || feat_isqrt(d + 1) != (s == 0 ? 1 : s)) return 5;
        ++checks;
    }
    if (feat_isqrt(440000000000000ll) != 20976176) return 6;
    const long long m[] = {-1200000, -1, 0, 1, 1200000};
    for (long long m10 : m) for (long long m01 : m) { const int k = feat_bin(m10, m01); if (k < 0 || k >= FEAT_BINS) return 7; ++checks; }
    for (int v = 0; v < 256; v += 5) if (feat_gray(v, 255 - v, v) < 0 || feat_gray(v, 255 - v, v) > 255) return 8;
    if (feat_gray(255, 255, 255) != 255 || feat_gray(0, 0, 0) != 0) return 9;
    printf("feat ok: %lld checks\n", checks);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def feat(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("feat")
    (tmp / "feat_host.cpp").write_text(FEAT_WRAPPER)
    so = tmp / "feat_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "feat_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.w_mix64.restype, lib.w_mix64.argtypes = ctypes.c_uint64, [ctypes.c_uint64]
    lib.w_isqrt.restype, lib.w_isqrt.argtypes = ctypes.c_int64, [ctypes.c_int64]
    lib.w_bin.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.w_response.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    IP = ctypes.POINTER(ctypes.c_int)

    class Feat:
        mix64, isqrt, bin, gray, response = lib.w_mix64, lib.w_isqrt, lib.w_bin, lib.w_gray, lib.w_response

        @staticmethod
        def pattern():
            out = np.zeros((256, 4), dtype=np.int32)
            lib.w_pattern(out.ctypes.data_as(IP))
            return out

        @staticmethod
        def rotate(x, y, k):
            out = np.zeros(2, dtype=np.int32)
            lib.w_rotate(int(x), int(y), k, out.ctypes.data_as(IP))
            return int(out[0]), int(out[1])

        @staticmethod
        def direction(k):
            out = np.zeros(2, dtype=np.int32)
            lib.w_direction(k, out.ctypes.data_as(IP))
            return int(out[0]), int(out[1])

        @staticmethod
        def constants():
            out = np.zeros(8, dtype=np.int32)
            lib.w_constants(out.ctypes.data_as(IP))
            return out.tolist()
    return Feat


# ---- feat.h --------------------------------------------------------------------------------------------------------
def test_generator_and_pattern_equal_the_restatement(feat):
    for z in (0, 1, ref.SEED, ref.MASK, 0x9E3779B97F4A7C15):
        assert feat.mix64(z) == ref.mix64(z)
    pat = feat.pattern()
    assert np.array_equal(pat, ref.base_pattern())
    assert np.all(pat[:, 0] ** 2 + pat[:, 1] ** 2 <= 169) and np.all(pat[:, 2] ** 2 + pat[:, 3] ** 2 <= 169)
    assert np.all((pat[:, 0] != pat[:, 2]) | (pat[:, 1] != pat[:, 3]))
    assert feat.constants() == [15, 3, 18, 13, 256, 32, 32, 18727200]


def test_rotated_patterns_stay_in_the_patch_and_near_the_true_rotation(feat):
    pat = ref.base_pattern()
    worst = 0.0
    for k in range(32):
        th = 2.0 * math.pi * k / 32
        for x, y in np.concatenate([pat[:, :2], pat[:, 2:]]):
            u, v = feat.rotate(x, y, k)
            assert (u, v) == ref.rotate(int(x), int(y), k)
            assert u * u + v * v <= 15 * 15
            tu, tv = x * math.cos(th) - y * math.sin(th), x * math.sin(th) + y * math.cos(th)
            worst = max(worst, abs(u - tu), abs(v - tv))
    print("largest distance of a rotated point from the true rotation, per axis: %.4f px" % worst)
    assert worst <= 0.51


def test_bins_above_7_are_exact_quarter_turns(feat):
    pat = ref.base_pattern()
    for k in range(24):
        c, s = feat.direction(k)
        assert feat.direction(k + 8) == (-s, c) and (c, s) == ref.direction(k)
        for x, y in pat[:, :2]:
            u, v = feat.rotate(x, y, k)
            assert feat.rotate(x, y, k + 8) == (-v, u)
    for k in range(8):
        assert feat.direction(k) == ref.CS8[k]
        c, s = feat.direction(k)
        assert abs(c - 16384 * math.cos(2 * math.pi * k / 32)) <= 0.5 and abs(s - 16384 * math.sin(2 * math.pi * k / 32)) <= 0.5


def test_bin_rule_and_its_tie_rule(feat):
    rng = np.random.default_rng(0)
    cases = [(0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (1200000, -1200000)]
    cases += [tuple(int(v) for v in rng.integers(-1200000, 1200001, 2)) for _ in range(2000)]
    for m10, m01 in cases:
        sc = ref.bin_scores(m10, m01)
        assert feat.bin(m10, m01) == sc.index(max(sc)), (m10, m01)
    assert feat.bin(0, 0) == 0                              # every bin ties: the lowest
    assert feat.bin(1, 1) == 4 and feat.bin(-1, 1) == 12 and feat.bin(0, -5) == 24


def test_gray_rule(feat):
    assert feat.gray(255, 255, 255) == 255 and feat.gray(0, 0, 0) == 0
    rng = np.random.default_rng(1)
    px = rng.integers(0, 256, (500, 1, 3), dtype=np.uint8)
    assert [feat.gray(*(int(v) for v in p[0])) for p in px] == ref.gray(px)[:, 0].tolist()


def test_isqrt_is_exact(feat):
    top = math.isqrt(D_BOUND)
    roots = list(range(0, 2000)) + list(range(top - 2000, top + 1)) + [int(v) for v in np.random.default_rng(2).integers(0, top, 5000)]
    for s in roots:
        d = s * s
        for v in (d - 1, d, d + 1):
            if 0 <= v <= D_BOUND:
                assert feat.isqrt(v) == math.isqrt(v), v
    assert feat.isqrt(D_BOUND) == math.isqrt(D_BOUND)
    # float64 rounds these square roots up to the next integer: the fix-up has to step back
    for s in (94906267, 67108865, 2 ** 26 + 1):
        assert feat.isqrt(s * s - 1) == s - 1
    d = np.array([0, 1, 2, 3, 4, D_BOUND, D_BOUND - 1, top * top, top * top - 1], dtype=np.int64)
    assert ref.isqrt(d).tolist() == [math.isqrt(int(v)) for v in d]


def test_response_equals_the_restatement(feat):
    rng = np.random.default_rng(3)
    for g in (ref.block_texture(24, 24, 1), (rng.integers(0, 2, (24, 24)) * 255).astype(np.uint8)):
        a, b, c, D = ref.response(g, parts=True)
        R, rmax = ref.response(g)
        assert D.max() <= D_BOUND and max(a.max(), c.max(), np.abs(b).max()) <= 9363600
        got = [feat.response(int(x), int(y), int(z)) for x, y, z in zip(a.reshape(-1), b.reshape(-1), c.reshape(-1))]
        assert got == R.reshape(-1).tolist() and rmax == max(got)


def test_restatement_selection_is_the_greedy_rule():
    R = np.zeros((60, 60), dtype=np.int32)
    R[30, 20], R[30, 24], R[30, 27] = 100, 90, 80           # 24 lies 4 from 20: rejected; 27 lies 7 from 20: accepted
    kp, resp = ref.select(R)
    assert kp.tolist() == [[20, 30], [27, 30]] and resp.tolist() == [100, 80]
    assert ref.select(np.zeros((60, 60), dtype=np.int32))[0].shape == (0, 2)


# ---- stand-alone under sanitizers ----------------------------------------------------------------------------------
def test_feat_header_under_sanitizers(tmp_path):
    """Every function of feat.h in a stand-alone program with its own main, built with -fsanitize=address,undefined: all
    32 x 512 rotated points index the blurred patch as the kernel does, the response at the extremes of the box sums, the
    square root along its whole range.  Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "feat_main.cpp").write_text(FEAT_MAIN)
    exe = tmp_path / "feat_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "feat_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "feat ok:" in r.stdout


# ---- host rules of the Python layer --------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import visual_features as vf
    img, bgr = np.zeros((48, 64), dtype=np.uint8), np.zeros((48, 64, 3), dtype=np.uint8)
    depth = np.ones((48, 64), dtype=np.float32)
    R = np.zeros((48, 64), dtype=np.int32)
    cam = (100.0, 100.0, 32.0, 24.0)
    kp = np.array([[30, 20]], dtype=np.int32)
    bad = [lambda: vf.to_gray(img.astype(np.float32)),                                       # dtype
           lambda: vf.to_gray(np.zeros((48, 64, 4), dtype=np.uint8)),                        # channels
           lambda: vf.to_gray(np.zeros(48, dtype=np.uint8)),
           lambda: vf.to_gray(np.zeros((1, 64), dtype=np.uint8)),
           lambda: vf.corner_response(bgr),                                                  # grey only
           lambda: vf.corner_response(img.astype(np.int32)),
           lambda: vf.select_keypoints(R.astype(np.int64)),
           lambda: vf.select_keypoints(R, border=17),
           lambda: vf.select_keypoints(R, border=24),                                        # 48 < 2 * 24 + 1
           lambda: vf.select_keypoints(R[:, :38]),                                           # 38 < 2 * 19 + 1
           lambda: vf.select_keypoints(R, min_distance=0),
           lambda: vf.select_keypoints(R, max_features=0),
           lambda: vf.select_keypoints(R, quality_level=-0.1),
           lambda: vf.select_keypoints(R, quality_level=1.5),
           lambda: vf.select_keypoints(R, valid=np.ones((48, 63), dtype=bool)),
           lambda: vf.select_keypoints(R - 1),                                               # a negative response
           lambda: vf.describe(bgr, kp),
           lambda: vf.describe(img, np.array([[17, 20]])),                                   # nearer than 18 to an edge
           lambda: vf.describe(img, np.array([[30, 30]])),                                   # 30 > 48 - 1 - 18
           lambda: vf.describe(img, np.array([[46, 20]])),
           lambda: vf.describe(img, np.array([[30.5, 20.0]])),                               # whole pixels
           lambda: vf.describe(img, np.array([30, 20])),
           lambda: vf.back_project(depth, np.array([[64, 20]]), cam),                        # outside
           lambda: vf.back_project(depth, np.array([[-1, 20]]), cam),
           lambda: vf.back_project(depth.astype(np.float64), kp, cam),
           lambda: vf.back_project(depth, kp, (0.0, 100.0, 32.0, 24.0)),
           lambda: vf.back_project(depth, kp, (100.0, 100.0, 32.0)),
           lambda: vf.extract_keyframes([img], [depth[:, :60]], cam),                        # depth of another size
           lambda: vf.extract_keyframes([img], [depth, depth], cam),
           lambda: vf.extract_keyframes([img], [depth.astype(np.int32)], cam),
           lambda: vf.extract_keyframes([img], [depth], cam, border=17),
           lambda: vf.extract_keyframes([img[:38]], [depth[:38]], cam),
           lambda: vf.extract_keyframes([img], [depth], cam, min_distance=0),
           lambda: vf.extract_keyframes([img], [depth], np.ones((2, 4)))]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)
    assert (vf.FEAT_TILE, vf.FEAT_MIN_BORDER, vf.FEAT_DESC_BYTES) == (16, 18, 32)


def test_is_new_keyframe_rule():
    from cslam_amd.front_end.visual_features import is_new_keyframe
    from cslam_amd.front_end.visual_registration import VisualRegistration

    def reg(status, inliers, matches=100):
        flags = np.arange(matches) < inliers
        return VisualRegistration(np.identity(4), status == 0, status, np.zeros((matches, 2), dtype=np.int64), flags, 0, 0)
    assert is_new_keyframe(reg(0, 31), 100, 0.3) is False   # 31 > 30
    assert is_new_keyframe(reg(0, 30), 100, 0.3) is True    # strictly more is needed
    assert is_new_keyframe(reg(1, 90), 100, 0.3) is True    # a failed registration is a null transform
    assert is_new_keyframe(reg(2, 0), 100, 0.3) is True
    assert is_new_keyframe(reg(0, 100), 100, 0.999) is True  # above 0.99: every frame is a keyframe
    assert is_new_keyframe(reg(0, 100), 100, 0.99) is False
    assert is_new_keyframe(reg(0, 1), 0, 0.3) is False      # 1 > 0


def test_uint16_depth_is_converted_in_float32():
    from cslam_amd.front_end.visual_features import depth_metres
    mm = np.array([[0, 1, 999, 1000], [2000, 2001, 12345, 65535]], dtype=np.uint16)
    m = depth_metres(mm)
    assert m.dtype == np.float32
    assert np.array_equal(m, mm.astype(np.float32) * np.float32(0.001))
    assert m[0, 0] == 0.0 and m[1, 0] == np.float32(2000.0) * np.float32(0.001)
    f = np.ones((2, 2), dtype=np.float32)
    assert depth_metres(f) is f
    with pytest.raises(ValueError):
        depth_metres(np.ones((2, 2), dtype=np.float64))
