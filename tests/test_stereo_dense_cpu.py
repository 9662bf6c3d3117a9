"""CPU: the dense stereo rule (tests/stereo_dense_reference.py) and the host pieces of its kernel.

  * the dense restatement equals stereo_reference.match at every pixel of the twelve scenes (status, disparity bits, best),
    and every scene keeps the per-status pixel counts it was chosen for
  * its float32 depth is np.float32 of the sparse restatement's triangulated Z
  * csrc/stereo_dense.h compiled by the host C++ compiler and run in the kernel's own schedule, one thread after another
    and one phase after another, with arrays of the kernel's LDS sizes: equal to the restatement on the twelve scenes and at
    the tile edges
  * the same once more as a stand-alone program under -fsanitize=address,undefined (never loaded into Python), against a
    per-pixel search written straight from stereo.h
  * the argument checks of cslam_amd.front_end.stereo_depth
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import stereo_dense_reference as dref
import stereo_reference as sr
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")

# The schedule of stereo_dense_kernel with a loop over t where the kernel has 256 threads and a new loop where it has a
# barrier.  The arrays are heap blocks of exactly the kernel's sizes, so an index outside them is the sanitizer's to report.
DENSE_HOST = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __host__
#define __device__
#include "stereo_dense.h"

static void dense_frame(const uint8_t *L, const uint8_t *R, int H, int W, int dmin, int dmax, int uniq, int lr, const double *cam,
                        uint8_t *status, float *disparity, float *depth, int32_t *best) {
    const int T = STEREO_DENSE_T;
    std::vector<uint32_t> l(STEREO_DENSE_LW), r(STEREO_DENSE_RW), sa(T), sb(STEREO_DENSE_SBW);
    std::vector<int32_t> slab(STEREO_DENSE_SLAB), rkey(W);
    std::vector<int> dstar(W);
    std::vector<StereoDenseBook> bk(T);
    for (int v = 0; v < H; ++v) {
        const size_t row = (size_t)v * W;
        if (!stereo_dense_row_searched(v, H, W)) {
            for (int u = 0; u < W; ++u) {
                status[row + u] = STEREO_OUTSIDE; disparity[row + u] = depth[row + u] = NAN;
                for (int k = 0; k < 4; ++k) best[4 * (row + u) + k] = -1;
            }
            continue;
        }
        const StereoDenseRow q = {L, R, H, W, v, dmin, dmax, uniq, lr};
        const StereoDenseTile s = {l.data(), r.data(), sa.data(), sb.data(), slab.data()};
        const int n_dt = stereo_dense_d_tiles(dmin, dmax), d_lo = dmin - 1;
        for (int u = 0; u < W; ++u) rkey[u] = STEREO_DENSE_NO_KEY;
        for (int u0 = 0; u0 < W; u0 += T) {
            memset(slab.data(), 0x7f, slab.size() * 4);                // what no phase may read: a huge cost
            for (int t = 0; t < T; ++t) stereo_dense_stage(&q, &s, u0, t);
            for (int t = 0; t < T; ++t) { stereo_dense_squares(&q, &s, t); stereo_dense_book_init(&bk[t]); }
            for (int dt = 0; dt < n_dt; ++dt) {
                const int e0 = d_lo + dt * STEREO_DENSE_TD;
                for (int t = 0; t < T; ++t) stereo_dense_costs(&q, &s, u0, e0, t);
                for (int t = 0; t < T; ++t) { stereo_dense_left(&q, &s, u0, e0, t, &bk[t]); stereo_dense_right(&q, &s, u0, e0, t, rkey.data()); }
            }
            for (int t = 0; t < T; ++t) {
                const int u = u0 + t;
                if (u >= W) continue;
                const StereoDensePixel p = stereo_dense_pixel(&q, &bk[t], u, cam);
                status[row + u] = (uint8_t)p.status; disparity[row + u] = p.disparity; depth[row + u] = p.depth; dstar[u] = p.await;
                best[4 * (row + u)] = p.ds; best[4 * (row + u) + 1] = p.ca; best[4 * (row + u) + 2] = p.cb; best[4 * (row + u) + 3] = p.cc;
            }
        }
        for (int u = 0; u < W; ++u)
            if (dstar[u] >= 0 && stereo_dense_left_right_fails(&q, rkey.data(), u, dstar[u])) {
                status[row + u] = STEREO_LEFT_RIGHT; disparity[row + u] = depth[row + u] = NAN;
            }
    }
}

extern "C" void w_dense(const uint8_t *L, const uint8_t *R, int H, int W, int dmin, int dmax, int uniq, int lr, const double *cam,
                        uint8_t *status, float *disparity, float *depth, int32_t *best) {
    dense_frame(L, R, H, W, dmin, dmax, uniq, lr, cam, status, disparity, depth, best);
}
extern "C" int w_constants(int *out) {
    out[0] = STEREO_DENSE_T; out[1] = STEREO_DENSE_TD; out[2] = STEREO_DENSE_SEG;
    return 3;
}

#ifdef DENSE_MAIN
// one pixel, straight from stereo.h: the sparse rule
static int32_t cost_at(const uint8_t *A, const uint8_t *B, int W, int v, int ua, int ub) {
    int32_t c = 0;
    for (int dy = -STEREO_HALF_H; dy <= STEREO_HALF_H; ++dy)
        for (int dx = -STEREO_HALF_W; dx <= STEREO_HALF_W; ++dx) {
            const int e = (int)A[(v + dy) * W + ua + dx] - (int)B[(v + dy) * W + ub + dx];
            c += e * e;
        }
    return c;
}
static void pixel(const uint8_t *L, const uint8_t *R, int H, int W, int u, int v, int dmin, int dmax, int uniq, int lr, int *st, double *disp,
                  int32_t b[4]) {
    b[0] = b[1] = b[2] = b[3] = -1;
    *disp = NAN;
    int lo, hi;
    if (!stereo_inside(u, v, H, W)) { *st = STEREO_OUTSIDE; return; }
    if (!stereo_range(u, dmin, dmax, &lo, &hi)) { *st = STEREO_NO_RANGE; return; }
    std::vector<int32_t> C(hi - lo + 1);
    int32_t key = STEREO_DENSE_NO_KEY;
    for (int d = lo; d <= hi; ++d) {
        C[d - lo] = cost_at(L, R, W, v, u, u - d);
        const int32_t k = stereo_key(C[d - lo], d);
        if (k < key) key = k;
    }
    const int ds = stereo_key_d(key);
    b[0] = ds; b[2] = C[ds - lo];
    if (ds > lo) b[1] = C[ds - 1 - lo];
    if (ds < hi) b[3] = C[ds + 1 - lo];
    if (ds == lo || ds == hi) { *st = STEREO_EDGE; return; }
    int32_t second = STEREO_DENSE_NO_KEY;
    for (int d = lo; d <= hi; ++d)
        if ((d - ds >= 2 || d - ds <= -2) && C[d - lo] < second) second = C[d - lo];
    if (second != STEREO_DENSE_NO_KEY && stereo_not_unique(second, b[2], uniq)) { *st = STEREO_NOT_UNIQUE; return; }
    if (lr >= 0) {
        const int ur = u - ds, e_hi = stereo_range_back(ur, W, dmax);
        int32_t k2 = STEREO_DENSE_NO_KEY;
        for (int e = lo; e <= e_hi; ++e) {
            const int32_t k = stereo_key(cost_at(R, L, W, v, ur, ur + e), e);
            if (k < k2) k2 = k;
        }
        const int es = stereo_key_d(k2);
        if ((es > ds ? es - ds : ds - es) > lr) { *st = STEREO_LEFT_RIGHT; return; }
    }
    *st = STEREO_ACCEPTED;
    *disp = stereo_parabola(ds, b[1], b[2], b[3]);
}

int main() {
    const double cam[5] = {100.0, 110.0, 31.5, 2.25, 0.2};
    const int T = STEREO_DENSE_T, TD = STEREO_DENSE_TD, SEG = STEREO_DENSE_SEG;
    const int widths[] = {15, 16, 17, 18, SEG + 13, SEG + 14, SEG + 15, 63, 64, 65, 141, 142, 143, T - 1, T, T + 1, T + 13, T + 14, T + 15,
                          300, 2 * T + 14};
    const int ranges[][2] = {{1, 1}, {1, 4}, {1, TD - 2}, {1, TD - 1}, {1, TD}, {1, TD + 1}, {1, 62}, {1, 63}, {1, 64}, {1, 65}, {1, 126},
                             {1, 254}, {1, 255}, {5, 40}, {TD, 2 * TD}, {255, 255}};
    long long pixels = 0, seen[6] = {0, 0, 0, 0, 0, 0};
    unsigned rng = 12345u;
    int n_case = 0;
    for (int W : widths)
        for (const int *mm : ranges) {
            ++n_case;
            const bool wide = W == 300 || W == 2 * T + 14 || W == T + 14;
            if (!wide && n_case % 3 != 0) continue;                    // every width meets a third of the ranges, three meet all
            const int H = 3 + n_case % 2, shift = 3 + n_case % 17, uniq = (n_case % 4) * 15, lr = n_case % 5 - 1;
            std::vector<uint8_t> L((size_t)H * W), R((size_t)H * W);
            std::vector<uint8_t> tex(W + 64);
            for (size_t i = 0; i < tex.size(); ++i) {
                if (i % 3 == 0) rng = rng * 1664525u + 1013904223u;    // blocks of three columns
                tex[i] = (uint8_t)(rng >> 24);
            }
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    rng = rng * 1664525u + 1013904223u;
                    L[(size_t)y * W + x] = tex[x + shift];
                    R[(size_t)y * W + x] = (uint8_t)(tex[x + 2 * shift] ^ ((rng >> 28) == 0 ? 16 : 0));
                }
            std::vector<uint8_t> st((size_t)H * W);
            std::vector<float> disp((size_t)H * W), depth((size_t)H * W);
            std::vector<int32_t> best((size_t)4 * H * W);
            dense_frame(L.data(), R.data(), H, W, mm[0], mm[1], uniq, lr, cam, st.data(), disp.data(), depth.data(), best.data());
            for (int v = 0; v < H; ++v)
                for (int u = 0; u < W; ++u) {
                    int want;
                    double d;
                    int32_t b[4];
                    pixel(L.data(), R.data(), H, W, u, v, mm[0], mm[1], uniq, lr, &want, &d, b);
                    const size_t i = (size_t)v * W + u;
                    const float fd = (float)d;
                    double p[3] = {NAN, NAN, NAN};
                    if (want == STEREO_ACCEPTED) stereo_point(u, v, d, cam[0], cam[1], cam[2], cam[3], cam[4], p);
                    const float fz = (float)p[2];
                    if (st[i] != want || memcmp(&best[4 * i], b, 16) != 0 || memcmp(&disp[i], &fd, 4) != 0 || memcmp(&depth[i], &fz, 4) != 0) {
                        printf("W %d range %d..%d uniq %d lr %d pixel (%d, %d): status %d, want %d\n", W, mm[0], mm[1], uniq, lr, u, v, st[i], want);
                        return 3;
                    }
                    ++pixels;
                    ++seen[want];
                }
        }
    for (int k = 0; k < 6; ++k)
        if (seen[k] == 0) { printf("no pixel with status %d\n", k); return 4; }
    printf("dense ok: %lld pixels\n", pixels);
    return 0;
}
#endif
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stereo_dense")
    (tmp / "dense_host.cpp").write_text(DENSE_HOST)
    so = tmp / "dense_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "dense_host.cpp"), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def host_dense(lib, L, R, camera, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1):
    H, W = L.shape
    L, R, cam = np.ascontiguousarray(L), np.ascontiguousarray(R), np.ascontiguousarray(camera, dtype=np.float64)
    status, disp, depth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    best = np.zeros((H, W, 4), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.w_dense(p(L), p(R), H, W, min_disparity, max_disparity, uniqueness, lr_tolerance, p(cam), p(status), p(disp), p(depth), p(best))
    return dict(status=status, disparity32=disp, depth=depth, best=best)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def dense_scenes():
    """The restatement on the twelve scenes, computed once and left unchanged."""
    out = []
    for k in range(len(dref.SCENES)):
        L, R, params, want = dref.scene(k)
        out.append((L, R, params, want, dref.dense(L, R, dref.CAMERA, **params)))
    return out


@pytest.mark.parametrize("k", range(len(dref.SCENES)), ids=[s[0] for s in dref.SCENES])
def test_dense_restatement_equals_the_sparse_one_at_every_pixel(dense_scenes, k):
    L, R, params, want, d = dense_scenes[k]
    m = dref.sparse_everywhere(L, R, dref.CAMERA, **params)
    assert np.array_equal(d["status"], m["status"])
    assert np.array_equal(bits(d["disparity"]), bits(m["disparity"]))
    assert np.array_equal(d["best"], m["best"])
    assert dref.counts(d["status"]) == want, "the scene no longer exercises the statuses it was chosen for"
    # the float32 depth is the sparse restatement's Z, rounded once
    assert np.array_equal(bits(d["depth"]), bits(m["z"].astype(np.float32)))
    ok = d["status"] == sr.ACCEPTED
    assert np.all(np.isnan(d["depth"][~ok])) and np.all(np.isfinite(d["depth"][ok]))
    for v, u in np.argwhere(ok)[:5]:
        assert d["depth"][v, u] == np.float32(sr.triangulate(u, v, d["disparity"][v, u], dref.CAMERA)[2])


def same_as_restatement(got, want):
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["best"], want["best"])
    assert np.array_equal(bits(got["disparity32"]), bits(want["disparity32"]))
    assert np.array_equal(bits(got["depth"]), bits(want["depth"]))


@pytest.mark.parametrize("k", range(len(dref.SCENES)), ids=[s[0] for s in dref.SCENES])
def test_header_in_the_kernels_schedule_equals_the_restatement(host, dense_scenes, k):
    L, R, params, _, d = dense_scenes[k]
    same_as_restatement(host_dense(host, L, R, dref.CAMERA, **params), d)


def test_header_at_the_tile_edges(host):
    """Widths around the column tile T and the segment, ranges around the disparity tile TD: where the plan can go wrong."""
    out = (ctypes.c_int * 3)()
    assert host.w_constants(out) == 3
    T, TD, SEG = out[0], out[1], out[2]
    assert (T, TD, SEG) == dref.TILE
    for W, dmax in [(T + 14, TD - 1), (T + 15, TD), (2 * T + 14, TD + 1), (T + 13, 64), (SEG + 15, TD - 2), (143, 126)]:
        L, R = sr.shifted_pair(3, W, 9)
        same_as_restatement(host_dense(host, L, R, dref.CAMERA, max_disparity=dmax), dref.dense(L, R, dref.CAMERA, max_disparity=dmax))


def test_header_standalone_under_sanitizers(tmp_path):
    (tmp_path / "dense_main.cpp").write_text(DENSE_HOST)
    exe = tmp_path / "dense_main"
    base = [_cxx(), "-O1", "-g", "-std=c++17", "-DDENSE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "dense_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("dense ok")


def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import stereo_depth as sd
    img, bgr = np.zeros((48, 64), dtype=np.uint8), np.zeros((48, 64, 3), dtype=np.uint8)
    cam = (100.0, 100.0, 32.0, 24.0, 0.2)
    bad = [lambda: sd.dense_disparity(img.astype(np.float32), img, cam),                       # dtypes and shapes
           lambda: sd.dense_disparity(img, img.astype(np.int16), cam),
           lambda: sd.dense_disparity(np.zeros((48, 64, 4), dtype=np.uint8), img, cam),
           lambda: sd.dense_disparity(img, img[:, :60], cam),                                  # left and right differ
           lambda: sd.dense_disparity(bgr, img[:40], cam),
           lambda: sd.dense_disparity_batch([img, img], [img], cam),
           lambda: sd.dense_disparity(img, img, cam, min_disparity=0),                         # parameter ranges
           lambda: sd.dense_disparity(img, img, cam, min_disparity=9, max_disparity=8),
           lambda: sd.dense_disparity(img, img, cam, max_disparity=256),
           lambda: sd.dense_disparity(img, img, cam, max_disparity=12.5),
           lambda: sd.dense_disparity(img, img, cam, uniqueness=-1),
           lambda: sd.dense_disparity(img, img, cam, uniqueness=101),
           lambda: sd.dense_disparity(img, img, cam, lr_tolerance=-2),
           lambda: sd.dense_disparity(img, img, cam, lr_tolerance=256),
           lambda: sd.dense_disparity(img, img, (100.0, 100.0, 32.0, 24.0, 0.0)),              # cameras
           lambda: sd.dense_disparity(img, img, (100.0, 100.0, 32.0, 24.0, np.nan)),
           lambda: sd.dense_disparity(img, img, (0.0, 100.0, 32.0, 24.0, 0.2)),
           lambda: sd.dense_disparity(img, img, (100.0, 100.0, 32.0, 24.0)),
           lambda: sd.dense_disparity_batch([img, img], [img, img], np.ones((3, 5))),
           lambda: sd.keyframe_clouds_stereo([img], [img[:, :60]], cam),
           lambda: sd.keyframe_clouds_stereo([img], [img, img], cam),
           lambda: sd.keyframe_clouds_stereo([img], [bgr.astype(np.float32)], cam),
           lambda: sd.keyframe_clouds_stereo([img], [img], cam[:4]),
           lambda: sd.keyframe_clouds_stereo([img], [img], cam, max_disparity=0),
           lambda: sd.keyframe_clouds_stereo([img], [img], cam, voxel_size=np.inf),
           lambda: sd.keyframe_clouds_stereo([img], [img], cam, voxel_size=np.nan),
           lambda: sd.keyframe_clouds_stereo([img], [img], cam, max_range=-1.0),
           lambda: sd.keyframe_clouds_stereo([img], [img], cam, max_range=np.nan)]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)


def test_no_cpu_path():
    """Without a GPU the functions raise CslamHipError once the arguments are right; with one this test has nothing to say."""
    import torch
    from cslam_amd import _lib
    from cslam_amd.front_end import stereo_depth as sd
    if torch.cuda.is_available():
        return
    img = np.zeros((48, 64), dtype=np.uint8)
    cam = (100.0, 100.0, 32.0, 24.0, 0.2)
    for f in (lambda: sd.dense_disparity(img, img, cam), lambda: sd.keyframe_clouds_stereo([img], [img], cam)):
        with pytest.raises(_lib.CslamHipError):
            f()
