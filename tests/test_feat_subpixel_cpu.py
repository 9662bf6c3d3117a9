"""CPU: the sub-pixel rules of csrc/feat_pyr.h against their restatement (tests/feat_subpixel_reference.py).

  * the offset rule, compiled by the host C++ compiler, bit for bit: all triples of int32 extremes (den and num need int64),
    plateaus, non-maxima, a missing neighbour on every side
  * the coordinate rule: base_coord bit for bit at offset 0, the restatement at +-0.5, +-2^-40 and random offsets
  * the same header functions once more as a stand-alone program under -fsanitize=address,undefined (never loaded into Python)
  * the argument checks of the Python layer
"""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import feat_pyramid_reference as pyr_ref
import feat_subpixel_reference as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
I32 = (-2 ** 31, -1, 0, 1, 7, 2 ** 31 - 1)
SIDES = (2, 3, 39, 40, 49, 144, 192, 480, 640, 700, 1 << 20)      # the sides of test_feat_pyramid_cpu's level-0 test

SUB_WRAPPER = r"""
#define __host__
#define __device__
#include "feat_pyr.h"
extern "C" double w_offset(int m, int c, int p) { return feat_pyr_subpix_offset(m, c, p); }
extern "C" void w_subpix(const int *R, int H, int W, const int *kp, int k, double *off) {
    for (int i = 0; i < k; ++i) feat_pyr_subpix(R, H, W, kp[2 * i], kp[2 * i + 1], off + 2 * i);
}
extern "C" void w_coord(int n_0, int n_l, const int *x, const double *off, int k, double *out) {
    for (int i = 0; i < k; ++i) out[i] = feat_pyr_subpix_coord(x[i], off[i], n_0, n_l);
}
"""

# stand-alone: every keypoint of maps of the edge shapes (each a buffer of exactly H W values, so a read past a missing
# neighbour is a heap overflow), the int32 extremes (signed overflow is undefined), the coordinate at the largest side
SUB_MAIN = r"""
#include <stdio.h>
#include <limits.h>
#include <vector>
#define __host__
#define __device__
#include "feat_pyr.h"
int main() {
    long long checks = 0;
    const int v[6] = {INT_MIN, -1, 0, 1, 7, INT_MAX};
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) for (int c = 0; c < 6; ++c) {
        const double o = feat_pyr_subpix_offset(v[a], v[b], v[c]);
        if (!(o >= -0.5 && o <= 0.5)) return 3;
        ++checks;
    }
    const int shapes[6][2] = {{1, 1}, {2, 2}, {3, 7}, {16, 16}, {17, 15}, {40, 49}};
    for (auto &s : shapes) {
        const int H = s[0], W = s[1];
        std::vector<int> R((size_t)H * W);
        for (size_t i = 0; i < R.size(); ++i) R[i] = v[(i * 7 + i / 5) % 6];
        for (int y = -1; y <= H; ++y) for (int x = -1; x <= W; ++x) {
            double off[2];
            feat_pyr_subpix(R.data(), H, W, x, y, off);
            if (!(off[0] >= -0.5 && off[0] <= 0.5 && off[1] >= -0.5 && off[1] <= 0.5)) return 4;
            if ((x <= 0 || x >= W - 1) && off[0] != 0.0) return 5;
            if ((y <= 0 || y >= H - 1) && off[1] != 0.0) return 6;
            ++checks;
        }
    }
    for (int side : {FEAT_PYR_MAX_SIDE, 700, 2})
        for (int l = 0; l < FEAT_PYR_MAX_LEVELS; ++l) {
            const int n_l = feat_pyr_size(side, l);
            if (n_l < 1) continue;
            for (int x : {0, n_l - 1}) {
                if (feat_pyr_subpix_coord(x, 0.0, side, n_l) != feat_pyr_base_coord(x, side, n_l)) return 7;
                const double lo = feat_pyr_subpix_coord(x, -0.5, side, n_l), hi = feat_pyr_subpix_coord(x, 0.5, side, n_l);
                if (!(lo < hi && lo >= -0.5 && hi <= side - 0.5)) return 8;
                ++checks;
            }
        }
    printf("feat_pyr subpix ok: %lld checks\n", checks);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def sub(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("feat_subpix")
    (tmp / "sub_host.cpp").write_text(SUB_WRAPPER)
    so = tmp / "sub_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "sub_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    IP, DP = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    lib.w_offset.restype = ctypes.c_double
    lib.w_offset.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]

    class Sub:
        offset = lib.w_offset

        @staticmethod
        def offsets(R, kp):
            R, kp = np.ascontiguousarray(R, dtype=np.int32), np.ascontiguousarray(kp, dtype=np.int32).reshape(-1, 2)
            out = np.full((len(kp), 2), np.nan)
            lib.w_subpix(R.ctypes.data_as(IP), R.shape[0], R.shape[1], kp.ctypes.data_as(IP), len(kp), out.ctypes.data_as(DP))
            return out

        @staticmethod
        def coord(x, off, n_0, n_l):
            x, off = np.ascontiguousarray(x, dtype=np.int32), np.ascontiguousarray(off, dtype=np.float64)
            out = np.full(len(x), np.nan)
            lib.w_coord(n_0, n_l, x.ctypes.data_as(IP), off.ctypes.data_as(DP), len(x), out.ctypes.data_as(DP))
            return out
    return Sub


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _every_pixel(shape):
    H, W = shape
    return np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2)


# ---- the offset rule -----------------------------------------------------------------------------------------------
def test_offset_rule_on_int32_extremes_equals_the_restatement(sub):
    seen = set()
    for m, c, p in itertools.product(I32, repeat=3):
        got, want = sub.offset(m, c, p), ref.offset(m, c, p)
        assert _bits([got]) == _bits([want]), (m, c, p, got, want)
        assert -0.5 <= got <= 0.5
        if m - 2 * c + p >= 0:
            assert got == 0.0
        seen.add(got)
    assert {-0.5, 0.0, 0.5} <= seen and len(seen) > 10     # clamped on both sides, and values in between
    # den and num leave int32: an evaluation in int32 would wrap
    lo, hi = -2 ** 31, 2 ** 31 - 1
    assert sub.offset(hi, hi, lo) == -0.5 and sub.offset(lo, hi, hi) == 0.5  # num = +-(2^32 - 1), den = -(2^32 - 1)
    assert sub.offset(lo, hi, lo) == 0.0                                     # num = 0, den = -(2^33 - 2)
    assert sub.offset(hi, lo, hi) == 0.0                                     # den = 2^33 - 2: no maximum


def test_plateaus_and_non_maxima_give_no_offset(sub):
    for m, c, p in ((5, 5, 5), (0, 0, 0), (4, 5, 6), (6, 5, 4), (7, 5, 7), (5, 5, 4), (4, 5, 5), (6, 5, 6), (-3, -3, -3)):
        want = ref.offset(m, c, p)
        assert sub.offset(m, c, p) == want
        if m - 2 * c + p >= 0:
            assert want == 0.0
    # a one-sided plateau is still a maximum along the axis (den < 0): half a pixel towards the equal neighbour
    assert sub.offset(5, 5, 4) == -0.5 and sub.offset(4, 5, 5) == 0.5
    # a symmetric peak stays; the parabola of (1, 7, 4): num -3, den -9
    assert sub.offset(3, 9, 3) == 0.0 and sub.offset(1, 7, 4) == np.float64(-3.0) / np.float64(-18.0)


@pytest.mark.parametrize("shape", [(2, 2), (3, 7), (16, 16), (17, 15), (40, 49)])
def test_offsets_of_every_pixel_with_missing_neighbours_equal_the_restatement(sub, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for R in (rng.integers(0, 1 << 24, shape).astype(np.int32),
              rng.choice(np.array(I32, dtype=np.int64), shape).astype(np.int32),
              np.full(shape, 9, dtype=np.int32)):
        kp = _every_pixel(shape)
        got, want = sub.offsets(R, kp), ref.offsets(R, kp)
        assert np.array_equal(_bits(got), _bits(want))
        H, W = shape
        edge_x, edge_y = (kp[:, 0] == 0) | (kp[:, 0] == W - 1), (kp[:, 1] == 0) | (kp[:, 1] == H - 1)
        assert not got[edge_x, 0].any() and not got[edge_y, 1].any()
    outside = np.array([[-1, 0], [0, -1], [shape[1], 0], [0, shape[0]]])
    assert not sub.offsets(R, outside).any() and not ref.offsets(R, outside).any()


# ---- the coordinate rule -------------------------------------------------------------------------------------------
def test_coordinate_at_offset_0_is_the_base_coordinate_bit_for_bit(sub):
    for n_0 in SIDES:
        for l in range(8):
            n_l = pyr_ref.level_size(n_0, l)
            if n_l < 1:
                continue
            x = np.arange(n_l)
            want = pyr_ref.base_coord(x, n_0, n_l)
            assert np.array_equal(_bits(sub.coord(x, np.zeros(n_l), n_0, n_l)), _bits(want))
            assert np.array_equal(_bits(ref.coord(x, np.zeros(n_l), n_0, n_l)), _bits(want))


def test_coordinate_at_offsets_equals_the_restatement(sub):
    rng = np.random.default_rng(5)
    for n_0 in SIDES:
        for l in range(8):
            n_l = pyr_ref.level_size(n_0, l)
            if n_l < 1:
                continue
            x = np.arange(n_l) if n_l <= 700 else np.concatenate([np.arange(350), n_l - 1 - np.arange(350)])
            base = pyr_ref.base_coord(x, n_0, n_l)
            for off in (np.full(len(x), 0.5), np.full(len(x), -0.5), np.full(len(x), 2.0 ** -40), np.full(len(x), -2.0 ** -40),
                        rng.uniform(-0.5, 0.5, len(x))):
                got = sub.coord(x, off, n_0, n_l)
                assert np.array_equal(_bits(got), _bits(ref.coord(x, off, n_0, n_l)))
                # the keypoint moves by off level pixels, n_0 / n_l level-0 pixels each, and stays inside its level pixel
                assert np.all(np.abs((got - base) - off * n_0 / n_l) <= 4 * np.finfo(np.float64).eps * (np.abs(base) + 1.0))
                assert np.all(got >= -0.5) and np.all(got <= n_0 - 0.5)


# ---- stand-alone under sanitizers ----------------------------------------------------------------------------------
def test_feat_pyr_subpixel_functions_under_sanitizers(tmp_path):
    """The sub-pixel functions of feat_pyr.h in a stand-alone program with its own main, built with
    -fsanitize=address,undefined: every pixel (and the ring around the image) of maps that are buffers of exactly H W values,
    int32 extremes in the maps, the coordinate rule at the largest side.  Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "sub_main.cpp").write_text(SUB_MAIN)
    exe = tmp_path / "sub_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "sub_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "feat_pyr subpix ok:" in r.stdout


# ---- the restatement and the Python layer --------------------------------------------------------------------------
def test_restatement_keeps_every_integer_output_of_the_pyramid():
    """Sub-pixel keypoints move keypoints and points only: on the two-distance scene every other key is the pyramid's, Z is
    its Z, and each keypoint stays inside its level pixel."""
    for plain, fine in zip(pyr_ref.scene_features(4), ref.scene_features(4)):
        for key in ("level_keypoints", "levels", "responses", "bins", "descriptors"):
            assert np.array_equal(plain[key], fine[key])
        assert np.array_equal(_bits(plain["points"][:, 2]), _bits(fine["points"][:, 2]))
        scale = 1.2 ** fine["levels"][:, None]
        assert np.all(np.abs(fine["keypoints"] - plain["keypoints"]) <= 0.5 * scale * (1 + 1e-2))
        assert np.abs(fine["offsets"]).max() <= 0.5 and np.count_nonzero(fine["offsets"]) > len(fine["offsets"])
        zero = ~fine["offsets"].any(axis=1)
        assert np.array_equal(_bits(plain["keypoints"][zero]), _bits(fine["keypoints"][zero]))


def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import visual_pyramid as vp
    R = np.zeros((8, 9), dtype=np.int32)
    bad = [lambda: vp.subpixel_offsets([R], []),
           lambda: vp.subpixel_offsets([R.astype(np.int64)], [np.zeros((0, 2), dtype=np.int32)]),
           lambda: vp.subpixel_offsets([R.reshape(-1)], [np.zeros((0, 2), dtype=np.int32)]),
           lambda: vp.subpixel_offsets([R[:1]], [np.zeros((0, 2), dtype=np.int32)]),
           lambda: vp.subpixel_offsets([R], [np.zeros((3, 3), dtype=np.int32)]),
           lambda: vp.subpixel_offsets([R], [np.array([[1.5, 2.0]])]),
           lambda: vp.extract_level_keyframes([np.zeros((48, 64), dtype=np.uint8)], [np.ones((48, 64), dtype=np.float32)],
                                              (100.0, 100.0, 32.0, 24.0), levels=3),          # too small for level 2
           lambda: vp.extract_level_keyframes_stereo([np.zeros((48, 64), dtype=np.uint8)], [np.zeros((48, 64), dtype=np.uint8)],
                                                     (100.0, 100.0, 32.0, 24.0), levels=1)]   # four numbers: no baseline
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)
