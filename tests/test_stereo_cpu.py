"""CPU: the host pieces of the stereo rule and its numpy restatement (tests/stereo_reference.py).

  * csrc/stereo.h compiled by the host C++ compiler: key packing, range rule, uniqueness predicate, parabola and
    triangulation value for value against the restatement
  * the same header once more as a stand-alone program under -fsanitize=address,undefined (never loaded into Python)
  * the argument checks of cslam_amd.front_end.visual_stereo
  * the restatement on planted scenes whose answer is known
"""
import ctypes
import functools
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

import stereo_reference as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")

STEREO_WRAPPER = r"""
#define __host__
#define __device__
#include "stereo.h"
extern "C" int w_key(int cost, int d) { return stereo_key(cost, d); }
extern "C" int w_key_cost(int key) { return stereo_key_cost(key); }
extern "C" int w_key_d(int key) { return stereo_key_d(key); }
extern "C" int w_inside(int u, int v, int H, int W) { return stereo_inside(u, v, H, W) ? 1 : 0; }
extern "C" int w_range(int u, int dmin, int dmax, int *out) { return stereo_range(u, dmin, dmax, out, out + 1) ? 1 : 0; }
extern "C" int w_range_back(int ur, int W, int dmax) { return stereo_range_back(ur, W, dmax); }
extern "C" int w_not_unique(int second, int best, int uniqueness) { return stereo_not_unique(second, best, uniqueness) ? 1 : 0; }
extern "C" double w_parabola(int d, int a, int b, int c) { return stereo_parabola(d, a, b, c); }
extern "C" void w_point(int u, int v, double disparity, const double *cam, double *out) {
    stereo_point(u, v, disparity, cam[0], cam[1], cam[2], cam[3], cam[4], out);
}
extern "C" int w_constants(int *out) {
    out[0] = STEREO_HALF_W; out[1] = STEREO_HALF_H; out[2] = STEREO_WIN_W; out[3] = STEREO_WIN_H; out[4] = STEREO_MAX_DISPARITY;
    out[5] = STEREO_MAX_RANGE; out[6] = STEREO_STRIP_W; out[7] = STEREO_COST_MAX; out[8] = STEREO_KEY_SHIFT;
    out[9] = STEREO_ACCEPTED; out[10] = STEREO_OUTSIDE; out[11] = STEREO_NO_RANGE; out[12] = STEREO_EDGE; out[13] = STEREO_NOT_UNIQUE;
    out[14] = STEREO_LEFT_RIGHT;
    return 15;
}
"""

# stand-alone: every function of stereo.h at the edges of its arguments; the strip and cost indices the kernel forms from
# the range rule are written into arrays of the kernel's sizes, so an index outside them is the sanitizer's to report
STEREO_MAIN = r"""
#include <stdio.h>
#include <math.h>
#include <initializer_list>
#define __host__
#define __device__
#include "stereo.h"
int main() {
    long long checks = 0;
    const int costs[] = {0, 1, 2, 65025, STEREO_COST_MAX - 1, STEREO_COST_MAX};
    for (int cost : costs)
        for (int d = 0; d <= STEREO_MAX_DISPARITY + 1; ++d) {
            const int32_t k = stereo_key(cost, d);
            if (k < 0 || stereo_key_cost(k) != cost || stereo_key_d(k) != d) return 3;
            if (cost > 0 && !(stereo_key(cost - 1, STEREO_MAX_DISPARITY + 1) < k)) return 4;       // the cost decides first
            if (d > 0 && !(stereo_key(cost, d - 1) < k)) return 5;                                 // then the lower d
            ++checks;
        }
    static unsigned char strip[STEREO_WIN_H][STEREO_STRIP_W];
    static int cost_of[STEREO_MAX_RANGE];
    const int widths[] = {15, 16, 17, 18, 22, 23, 24, 100, 271, 272, 273, 600};
    const int lows[] = {1, 2, 5, 63, 64, 128, 254, 255}, highs[] = {1, 2, 3, 5, 7, 64, 65, 128, 129, 254, 255};
    for (int W : widths)
        for (int dmin : lows)
            for (int dmax : highs)
                for (int u = -2; u <= W + 1; ++u) {
                    if (dmax < dmin) continue;
                    if (!stereo_inside(u, 1, 3, W)) { if (u >= STEREO_HALF_W && u <= W - 1 - STEREO_HALF_W) return 6; continue; }
                    int lo, hi;
                    if (!stereo_range(u, dmin, dmax, &lo, &hi)) { if (hi - lo >= 2) return 7; continue; }
                    const int count = hi - lo + 1, first = u - hi - STEREO_HALF_W, last = u - lo + STEREO_HALF_W;
                    if (count < 3 || count > STEREO_MAX_RANGE || lo < 0 || first < 0 || last > W - 1) return 8;
                    strip[STEREO_WIN_H - 1][count - 1 + STEREO_WIN_W - 1] += 1;       // the last byte the kernel stages
                    cost_of[count - 1] += 1;
                    for (int ds = lo + 1; ds <= hi - 1; ds += (hi - lo > 8 && ds > lo + 2 && ds < hi - 3) ? 5 : 1) {
                        const int ur = u - ds, e_hi = stereo_range_back(ur, W, dmax), count2 = e_hi - lo + 1;
                        if (e_hi < ds || count2 > STEREO_MAX_RANGE || ur + lo - STEREO_HALF_W < 0 || ur + e_hi + STEREO_HALF_W > W - 1) return 9;
                        strip[STEREO_WIN_H - 1][count2 - 1 + STEREO_WIN_W - 1] += 1;
                        strip[0][hi - ds] += 1;                                       // where the right window starts in the strip
                        cost_of[count2 - 1] += 1;
                        ++checks;
                    }
                }
    for (int u : {0, 50, 100})
        for (int s : {0, 1, STEREO_COST_MAX}) for (int b : {0, 1, STEREO_COST_MAX}) {
            if (stereo_not_unique(s, b, u) != ((long long)s * 100 <= (long long)b * (100 + u))) return 10;
            ++checks;
        }
    const int abc[][3] = {{1, 0, 0}, {1, 0, 1}, {2, 1, 1}, {STEREO_COST_MAX, 0, STEREO_COST_MAX}, {STEREO_COST_MAX, 0, 0},
                          {STEREO_COST_MAX, STEREO_COST_MAX - 1, STEREO_COST_MAX - 1}, {1, 0, STEREO_COST_MAX}};
    for (const int *t : abc)
        for (int d : {1, 128, 255}) {
            const double x = stereo_parabola(d, t[0], t[1], t[2]);
            if (!(x >= d - 0.5 && x <= d + 0.5)) return 11;
            double p[3];
            stereo_point(7, 1, x, 100.0, 101.0, 80.0, 60.0, 0.2, p);
            if (!(isfinite(p[0]) && isfinite(p[1]) && p[2] > 0.0)) return 12;
            ++checks;
        }
    printf("stereo ok: %lld checks\n", checks);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def stereo(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stereo")
    (tmp / "stereo_host.cpp").write_text(STEREO_WRAPPER)
    so = tmp / "stereo_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "stereo_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.w_parabola.restype = ctypes.c_double
    lib.w_point.restype = None
    DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    lib.w_point.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, DP, DP]

    class Stereo:
        key, key_cost, key_d, inside, range_back, not_unique, parabola = (lib.w_key, lib.w_key_cost, lib.w_key_d, lib.w_inside, lib.w_range_back,
                                                                          lib.w_not_unique, lib.w_parabola)

        @staticmethod
        def range(u, dmin, dmax):
            out = np.zeros(2, dtype=np.int32)
            ok = lib.w_range(u, dmin, dmax, out.ctypes.data_as(IP))
            return int(out[0]), int(out[1]), bool(ok)

        @staticmethod
        def point(u, v, disparity, camera):
            cam, out = np.array(camera, dtype=np.float64), np.zeros(3, dtype=np.float64)
            lib.w_point(u, v, float(disparity), cam.ctypes.data_as(DP), out.ctypes.data_as(DP))
            return out

        @staticmethod
        def constants():
            out = np.zeros(15, dtype=np.int32)
            lib.w_constants(out.ctypes.data_as(IP))
            return out.tolist()
    return Stereo


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


# ---- stereo.h ------------------------------------------------------------------------------------------------------
def test_constants_and_key_packing(stereo):
    assert stereo.constants() == [7, 1, 15, 3, 255, 257, 271, 2926125, 9, 0, 1, 2, 3, 4, 5]
    assert ref.COST_MAX == 2926125 < 2 ** 22
    top = stereo.key(ref.COST_MAX, 256)                    # the largest cost with the largest disparity of a range
    assert top == ref.key(ref.COST_MAX, 256) == 1498176256 and 0 < top < 2 ** 31
    rng = np.random.default_rng(0)
    cases = [(0, 0), (0, 256), (1, 0), (ref.COST_MAX, 0), (ref.COST_MAX, 256), (ref.COST_MAX - 1, 256)]
    cases += [(int(rng.integers(0, ref.COST_MAX + 1)), int(rng.integers(0, 257))) for _ in range(2000)]
    for cost, d in cases:
        k = stereo.key(cost, d)
        assert k == ref.key(cost, d) and stereo.key_cost(k) == cost and stereo.key_d(k) == d
    # the order of the keys is (cost, d): the minimum is the best cost and among equals the lowest d
    order = sorted(cases, key=lambda cd: stereo.key(*cd))
    assert order == sorted(cases)


def test_range_rule_and_inside(stereo):
    for u in list(range(-1, 30)) + [134, 135, 136, 137, 261, 262, 263, 264, 1000]:
        for dmin, dmax in ((1, 128), (1, 255), (1, 1), (5, 5), (5, 64), (6, 64), (7, 64), (128, 128), (255, 255), (1, 4)):
            assert stereo.range(u, dmin, dmax) == ref.search_range(u, dmin, dmax), (u, dmin, dmax)
    assert stereo.range(8, 1, 128) == (0, 1, False) and stereo.range(9, 1, 128) == (0, 2, True)
    assert stereo.range(1000, 1, 255) == (0, 256, True)    # the longest range: 257 disparities
    for W in (15, 18, 200):
        for ur in range(0, W):
            for dmax in (1, 4, 128, 255):
                assert stereo.range_back(ur, W, dmax) == min(dmax + 1, W - 8 - ur)
    for H, W in ((3, 15), (3, 18), (48, 200)):
        for u in range(-2, W + 2):
            for v in range(-2, H + 2):
                assert stereo.inside(u, v, H, W) == int(7 <= u <= W - 8 and 1 <= v <= H - 2)


def test_uniqueness_predicate(stereo):
    rng = np.random.default_rng(1)
    cases = [(0, 0, 0), (0, 0, 100), (1, 0, 15), (115, 100, 15), (116, 100, 15), (114, 100, 15), (100, 100, 0), (101, 100, 0),
             (200, 100, 100), (201, 100, 100), (ref.COST_MAX, ref.COST_MAX, 100), (ref.COST_MAX, ref.COST_MAX // 2, 100)]
    cases += [tuple(int(x) for x in (rng.integers(0, ref.COST_MAX + 1), rng.integers(0, ref.COST_MAX + 1), rng.integers(0, 101)))
              for _ in range(2000)]
    for second, best, uq in cases:
        assert stereo.not_unique(second, best, uq) == int(ref.not_unique(second, best, uq)), (second, best, uq)
    assert stereo.not_unique(115, 100, 15) == 1 and stereo.not_unique(116, 100, 15) == 0


def test_parabola_and_triangulation_bit_for_bit(stereo):
    rng = np.random.default_rng(2)
    M = ref.COST_MAX
    cases = [(1, 1, 0, 0), (1, 1, 0, 1), (7, 2, 1, 1), (255, M, 0, M), (255, M, 0, 0), (128, M, M - 1, M - 1), (3, 1, 0, M)]
    assert cases[0][1] - 2 * cases[0][2] + cases[0][3] == 1 and M - 2 * (M - 1) + (M - 1) == 1         # den = 1
    for _ in range(2000):
        b = int(rng.integers(0, M))
        cases.append((int(rng.integers(1, 256)), int(rng.integers(b + 1, M + 1)), b, int(rng.integers(b, M + 1))))
    cams = [(100.0, 100.0, 80.0, 60.0, 0.2), (523.7, 519.1, 317.37, 239.81, 0.1197), (1e-3, 1e4, -5.5, 1e3, 7.0)]
    for k, (d, a, b, c) in enumerate(cases):
        want = ref.parabola(d, a, b, c)
        got = stereo.parabola(d, a, b, c)
        assert bits(got) == bits(want), (d, a, b, c)
        assert d - 0.5 <= got <= d + 0.5
        cam = cams[k % 3]
        u, v = int(rng.integers(0, 2000)), int(rng.integers(0, 2000))
        assert bits(stereo.point(u, v, got, cam)) == bits(ref.triangulate(u, v, want, cam))
    assert stereo.parabola(1, 1, 0, 0) == 1.5 and stereo.parabola(1, 1, 0, 1) == 1.0
    p = stereo.point(180, 60, 10.0, (100.0, 100.0, 80.0, 60.0, 0.2))
    assert p.tolist() == [2.0, 0.0, 2.0]


# ---- stand-alone under sanitizers ----------------------------------------------------------------------------------
def test_stereo_header_under_sanitizers(tmp_path):
    """Every function of stereo.h in a stand-alone program with its own main, built with -fsanitize=address,undefined: the
    keys at the largest cost, the range rules over image widths around 15 and 272 with the strip and cost indices the
    kernel forms from them, the predicate and the parabola at their extremes.  Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "stereo_main.cpp").write_text(STEREO_MAIN)
    exe = tmp_path / "stereo_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "stereo_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stereo ok:" in r.stdout


# ---- the Python layer ----------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import visual_stereo as vs
    img, bgr = np.zeros((48, 64), dtype=np.uint8), np.zeros((48, 64, 3), dtype=np.uint8)
    cam = (100.0, 100.0, 32.0, 24.0, 0.2)
    kp = np.array([[30, 20]], dtype=np.int32)
    bad = [lambda: vs.stereo_match(img.astype(np.float32), img, kp, cam),                      # dtypes
           lambda: vs.stereo_match(img, img.astype(np.int16), kp, cam),
           lambda: vs.stereo_match(bgr, img, kp, cam),                                         # the staged call takes grey
           lambda: vs.stereo_match(img, bgr, kp, cam),
           lambda: vs.stereo_match(img, img[:, :60], kp, cam),                                 # left and right differ
           lambda: vs.stereo_match(img, img[:40], kp, cam),
           lambda: vs.stereo_match_batch([img, img], [img], [kp, kp], cam),
           lambda: vs.stereo_match_batch([img, img], [img, img], [kp], cam),
           lambda: vs.stereo_match(img, img, kp, cam, min_disparity=0),                        # parameter ranges
           lambda: vs.stereo_match(img, img, kp, cam, min_disparity=9, max_disparity=8),
           lambda: vs.stereo_match(img, img, kp, cam, max_disparity=256),
           lambda: vs.stereo_match(img, img, kp, cam, max_disparity=12.5),
           lambda: vs.stereo_match(img, img, kp, cam, uniqueness=-1),
           lambda: vs.stereo_match(img, img, kp, cam, uniqueness=101),
           lambda: vs.stereo_match(img, img, kp, cam, lr_tolerance=-2),
           lambda: vs.stereo_match(img, img, kp, cam, lr_tolerance=256),
           lambda: vs.stereo_match(img, img, kp, (100.0, 100.0, 32.0, 24.0, 0.0)),             # baseline <= 0
           lambda: vs.stereo_match(img, img, kp, (100.0, 100.0, 32.0, 24.0, -0.2)),
           lambda: vs.stereo_match(img, img, kp, (100.0, 100.0, 32.0, 24.0, np.nan)),
           lambda: vs.stereo_match(img, img, kp, (0.0, 100.0, 32.0, 24.0, 0.2)),
           lambda: vs.stereo_match(img, img, kp, (100.0, 100.0, np.inf, 24.0, 0.2)),
           lambda: vs.stereo_match(img, img, kp, (100.0, 100.0, 32.0, 24.0)),                  # no baseline
           lambda: vs.stereo_match_batch([img, img], [img, img], [kp, kp], np.ones((3, 5))),
           lambda: vs.stereo_match(img, img, np.array([[30.5, 20.0]]), cam),                   # whole pixels
           lambda: vs.stereo_match(img, img, np.array([[np.nan, 20.0]]), cam),
           lambda: vs.stereo_match(img, img, np.array([30, 20]), cam),
           lambda: vs.stereo_match(img, img, np.array([[30, 20, 1]]), cam),
           lambda: vs.extract_keyframes_stereo([img], [img[:, :60]], cam),
           lambda: vs.extract_keyframes_stereo([img], [img, img], cam),
           lambda: vs.extract_keyframes_stereo([img], [img.astype(np.float32)], cam),
           lambda: vs.extract_keyframes_stereo([np.zeros((48, 64, 4), dtype=np.uint8)], [img], cam),
           lambda: vs.extract_keyframes_stereo([img], [img], cam, border=17),
           lambda: vs.extract_keyframes_stereo([img[:38]], [img[:38]], cam),                   # 38 < 2 * 19 + 1
           lambda: vs.extract_keyframes_stereo([img], [img], cam, max_disparity=0),
           lambda: vs.extract_keyframes_stereo([img], [img], cam[:4]),
           lambda: vs.extract_features_stereo([img], [bgr], (100.0, 100.0, 32.0, 24.0, 0.0))]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)
    assert vs.STEREO_MAX_DISPARITY == 255 and len(vs.STATUS) == 6


# ---- the restatement on planted scenes -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shift5():
    L, R = ref.shifted_pair(48, 200, 5)
    assert np.array_equal(L[:, 5:], R[:, :-5])
    return L, R


def test_restatement_constant_shift():
    L, R = shift5()
    for dmax, want in ((4, 3), (5, 0), (6, 0)):
        st, d, best = ref.match_one(L, R, 100, 5, 1, dmax)
        assert st == want and best[0] == 5 and best[2] == 0
        assert (d == 5.0) if want == 0 else np.isnan(d)
    assert ref.match_one(L, R, 100, 5, 1, 4)[2][3] == -1    # d* = 5 = D_hi: no right neighbour
    for dmin, want in ((5, 0), (6, 3), (7, 3)):
        st, d, best = ref.match_one(L, R, 100, 5, dmin, 64)
        assert st == want
        if dmin == 6:
            assert best[0] == 5 and best[1] == -1           # d* = D_lo, below min_disparity
    assert [ref.match_one(L, R, u, 5, 1, 64)[0] for u in (7, 8, 9, 10)] == [2, 2, 3, 3]
    assert ref.match_one(L, R, 7, 5, 1, 64)[2] == (-1, -1, -1, -1)
    assert [ref.match_one(L, R, u, v, 1, 64)[0] for u, v in ((6, 5), (193, 5), (100, 0), (100, 47), (0, 0))] == [1] * 5


def test_restatement_stripes_and_constant_images():
    P0, P3 = ref.stripes(48, 200), ref.stripes(48, 200, 3)
    assert Counter(ref.match_one(P0, P3, u, 10, 1, 64)[0] for u in range(80, 120)) == {4: 40}
    assert Counter(ref.match_one(P0, P0, u, 10, 1, 64)[0] for u in range(80, 120)) == {3: 40}
    Z = np.full((48, 200), 77, dtype=np.uint8)
    st, d, best = ref.match_one(Z, Z, 100, 10, 1, 64)
    assert (st, best) == (3, (0, -1, 0, 0)) and np.isnan(d)


def test_restatement_foreground_over_background():
    L, R = ref.foreground_pair()
    status, band, errs = Counter(), Counter(), []
    for v in range(1, 47, 3):
        for u in range(7, 193, 3):
            st, d, _ = ref.match_one(L, R, u, v, 1, 64)
            status[st] += 1
            if 10 <= v < 40 and 70 <= u < 90:
                band[st] += 1
            if st == 0:
                errs.append(abs(d - (20 if 10 <= v < 40 and 90 <= u < 130 else 5)))
    assert status[0] == 857 and status[5] == 61
    assert sum(band.values()) == 70 and band[5] == 33 and band[4] == 20
    assert np.mean(np.array(errs) > 0.5) < 0.02             # the accepted ones are right but for the block's outline


def test_restatement_batch_form_and_triangulation():
    L, R = shift5()
    cam = (100.0, 100.0, 80.0, 24.0, 0.2)
    m = ref.match(L, R, [[100, 5], [7, 5], [0, 0], [9, 5]], cam, 1, 64)
    assert m["status"].tolist() == [0, 2, 1, 3] and m["disparity"].dtype == np.float64 and m["best"].dtype == np.int32
    assert m["points"][0].tolist() == [((100 - 80.0) * 4.0) / 100.0, ((5 - 24.0) * 4.0) / 100.0, 4.0]
    assert np.isnan(m["points"][1:]).all() and np.isnan(m["disparity"][1:]).all()
    assert m["best"][1].tolist() == [-1, -1, -1, -1]
