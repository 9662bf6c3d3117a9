"""CPU: the rule of csrc/rectify.h against its numpy restatement (tests/rectify_reference.py), and the host pieces of
cslam_amd.front_end.rectify.

  * csrc/rectify.h compiled by the host C++ compiler with -ffp-contract=off into a stand-alone program that runs the
    kernels' per-thread functions in the kernels' schedule (whole workgroups, one thread after another) on heap blocks of
    exactly the kernels' buffer sizes: equal to the restatement bit for bit on every case of the GPU test
  * the same program once more under -fsanitize=address,undefined (its own main, never loaded into Python)
  * the argument checks of cslam_amd.front_end.rectify
  * the end-to-end scene through the restatement alone: the bounds and the recorded counts the GPU test relies on
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rectify_reference as ref
import stereo_reference
import vis_reference
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")

# Jobs are read from argv[1] and their results written to argv[2].  A job is four int32 (kind, n, n_maps, flags) and its
# arrays; every device buffer of the kernels is a heap block of exactly its size here, filled with 0xAA where a kernel
# has to write, so an index outside is the sanitizer's to report and a pixel left out shows in the comparison.
RECTIFY_HOST = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#define __host__
#define __device__
#include "rectify.h"

template <typename T> static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(5); }
    return v;
}
template <typename T> static void wr(FILE *f, const std::vector<T> &v) {
    if (v.size() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(6);
}
static std::vector<int64_t> prefix(const std::vector<int64_t> &len) {
    std::vector<int64_t> off(len.size() + 1, 0);
    for (size_t c = 0; c < len.size(); ++c) off[c + 1] = off[c] + len[c];
    return off;
}
static std::vector<int64_t> pixels(const std::vector<int32_t> &hw) {
    std::vector<int64_t> len(hw.size() / 2);
    for (size_t c = 0; c < len.size(); ++c) len[c] = (int64_t)hw[2 * c] * hw[2 * c + 1];
    return len;
}
static int64_t blocks_for(int64_t most) { return (most + RECTIFY_BLOCK - 1) / RECTIFY_BLOCK; }

template <typename T> static void nearest_job(FILE *in, FILE *out, const RectifyFrames &f, const std::vector<int64_t> &src_off, int n, int64_t total,
                                              int64_t largest, bool masked) {
    const std::vector<T> src = rd<T>(in, (size_t)src_off[n]);
    const std::vector<uint8_t> mask = rd<uint8_t>(in, masked ? (size_t)total : 0);
    std::vector<T> dst((size_t)total);
    memset(dst.data(), 0xAA, dst.size() * sizeof(T));
    for (int c = 0; c < n; ++c)
        for (int64_t b = 0; b < blocks_for(largest); ++b)
            for (int t = 0; t < RECTIFY_BLOCK; ++t)
                rectify_nearest_thread<T>(&f, src.data(), masked ? mask.data() : nullptr, c, b * RECTIFY_BLOCK + t, dst.data());
    wr(out, dst);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t head[4];
    int jobs = 0;
    while (fread(head, 4, 4, in) == 4) {
        const int kind = head[0], n = head[1], n_maps = head[2], flags = head[3];
        if (kind == 0) {                                            // rectify_map_kernel
            const std::vector<double> cams = rd<double>(in, (size_t)RECTIFY_CAM * n);
            const std::vector<int32_t> hw = rd<int32_t>(in, (size_t)2 * n);
            const std::vector<int64_t> len = pixels(hw), off = prefix(len);
            int64_t largest = 0;
            for (int64_t l : len) largest = l > largest ? l : largest;
            std::vector<int32_t> map((size_t)2 * off[n], (int32_t)0xAAAAAAAA);
            for (int c = 0; c < n; ++c)
                for (int64_t b = 0; b < blocks_for(largest); ++b)
                    for (int t = 0; t < RECTIFY_BLOCK; ++t) rectify_map_thread(cams.data(), off.data(), hw.data(), c, b * RECTIFY_BLOCK + t, map.data());
            wr(out, map);
        } else {                                                    // 1 rectify_remap_kernel, 2 / 3 rectify_nearest_kernel<uint16_t / float>
            const std::vector<int32_t> map_hw = rd<int32_t>(in, (size_t)2 * n_maps);
            const std::vector<int64_t> map_off = prefix(pixels(map_hw));
            const std::vector<int32_t> map = rd<int32_t>(in, (size_t)2 * map_off[n_maps]);
            const std::vector<int32_t> idx = rd<int32_t>(in, (size_t)n), src_hw = rd<int32_t>(in, (size_t)2 * n), ch = rd<int32_t>(in, (size_t)n);
            std::vector<int32_t> hw((size_t)2 * n);
            std::vector<int64_t> src_len(n), dst_len(n);
            for (int c = 0; c < n; ++c) { hw[2 * c] = map_hw[2 * idx[c]]; hw[2 * c + 1] = map_hw[2 * idx[c] + 1]; }
            const std::vector<int64_t> len = pixels(hw), off = prefix(len);
            int64_t largest = 0, most_runs = 0;
            for (int c = 0; c < n; ++c) {
                src_len[c] = (int64_t)ch[c] * src_hw[2 * c] * src_hw[2 * c + 1];
                dst_len[c] = ch[c] * len[c];
                largest = len[c] > largest ? len[c] : largest;
                const int64_t runs = (int64_t)hw[2 * c] * ((hw[2 * c + 1] + RECTIFY_RUN - 1) / RECTIFY_RUN);
                most_runs = runs > most_runs ? runs : most_runs;
            }
            const std::vector<int64_t> src_off = prefix(src_len), dst_off = prefix(dst_len);
            const RectifyFrames f = {map.data(), map_off.data(), idx.data(), off.data(), hw.data(), src_off.data(), src_hw.data(),
                                     kind == 1 ? dst_off.data() : nullptr};
            if (kind == 1) {
                const std::vector<uint8_t> src = rd<uint8_t>(in, (size_t)src_off[n]);
                std::vector<uint8_t> dst((size_t)dst_off[n], (uint8_t)0xAA), valid((size_t)off[n], (uint8_t)0xAA);
                for (int c = 0; c < n; ++c)
                    for (int64_t b = 0; b < blocks_for(most_runs); ++b)
                        for (int t = 0; t < RECTIFY_BLOCK; ++t) rectify_remap_thread(&f, src.data(), c, b * RECTIFY_BLOCK + t, dst.data(), valid.data());
                wr(out, dst);
                wr(out, valid);
            } else if (kind == 2) {
                nearest_job<uint16_t>(in, out, f, src_off, n, off[n], largest, flags & 1);
            } else {
                nearest_job<float>(in, out, f, src_off, n, off[n], largest, flags & 1);
            }
        }
        ++jobs;
    }
    fclose(out);
    printf("rectify ok: %d jobs\n", jobs);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


# ---- jobs ------------------------------------------------------------------------------------------------------------
def map_job(cams, sizes):
    return dict(kind=0, n=len(cams), n_maps=0, flags=0, sizes=sizes,
                data=[np.ascontiguousarray(cams, dtype=np.float64), np.ascontiguousarray(sizes, dtype=np.int32)])


def frames_job(kind, sources, maps, index, mask=None):
    """kind 1: uint8 images through `rectify_remap_thread`; 2, 3: uint16, float32 depth through `rectify_nearest_thread`."""
    index = np.ascontiguousarray(index, dtype=np.int32)
    data = [np.array([m.shape[:2] for m in maps], dtype=np.int32), np.concatenate([m.reshape(-1) for m in maps]).astype(np.int32), index,
            np.array([s.shape[:2] for s in sources], dtype=np.int32), np.array([s.shape[2] if s.ndim == 3 else 1 for s in sources], dtype=np.int32),
            np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in sources])]
    if mask is not None:
        data.append(np.concatenate([np.ascontiguousarray(m, dtype=np.uint8).reshape(-1) for m in mask]))
    return dict(kind=kind, n=len(sources), n_maps=len(maps), flags=0 if mask is None else 1, data=data, sources=sources,
                shapes=[maps[m].shape[:2] for m in index])


def run_jobs(exe, tmp, jobs):
    """The results of the jobs: a map job gives the maps, a remap job (images, valids), a nearest job the depth images."""
    with open(tmp / "jobs.bin", "wb") as f:
        for j in jobs:
            f.write(np.array([j["kind"], j["n"], j["n_maps"], j["flags"]], dtype=np.int32).tobytes())
            for a in j["data"]:
                f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(exe), str(tmp / "jobs.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("rectify ok: %d jobs" % len(jobs))
    raw = np.fromfile(tmp / "out.bin", dtype=np.uint8)
    at, out = 0, []

    def take(shape, dtype):
        nonlocal at
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = raw[at:at + size].view(dtype).reshape(shape).copy()
        at += size
        return a

    for j in jobs:
        if j["kind"] == 0:
            out.append([take((h, w, 2), np.int32) for h, w in j["sizes"]])
        elif j["kind"] == 1:
            imgs = [take(tuple(s) + ((3,) if src.ndim == 3 else ()), np.uint8) for s, src in zip(j["shapes"], j["sources"])]
            out.append((imgs, [take(tuple(s), np.uint8) for s in j["shapes"]]))
        else:
            out.append([take(tuple(s), j["sources"][0].dtype) for s in j["shapes"]])
    assert at == len(raw)
    return out


def all_jobs():
    """(jobs, what the restatement gives for each): every case of the GPU test, one by one and as batches."""
    jobs, want = [], []
    cases = ref.map_cases()
    for _, cam, H, W in cases:
        jobs.append(map_job([cam], [(H, W)]))
        want.append([ref.rect_map(cam, H, W)])
    jobs.append(map_job([c[1] for c in cases], [(c[2], c[3]) for c in cases]))                  # the ragged batch of all cameras
    want.append([w[0] for w in want[:len(cases)]])
    for _, src, q in ref.remap_cases():
        jobs.append(frames_job(1, [src], [q], [0]))
        img, valid = ref.bilinear(src, q)
        want.append(([img], [valid]))
    sources, maps, index = ref.batch_case()
    jobs.append(frames_job(1, sources, maps, index))
    both = [ref.bilinear(s, maps[m]) for s, m in zip(sources, index)]
    want.append(([b[0] for b in both], [b[1] for b in both]))
    for _, src, q in ref.nearest_cases():
        kind = 2 if src.dtype == np.uint16 else 3
        jobs.append(frames_job(kind, [src], [q], [0]))
        want.append([ref.nearest(src, q)])
        mask = (np.arange(q.shape[0] * q.shape[1]).reshape(q.shape[:2]) % 3 != 0).astype(np.uint8)
        jobs.append(frames_job(kind, [src], [q], [0], [mask]))
        want.append([ref.nearest(src, q, mask)])
    grey = [s for s in sources if s.ndim == 2]
    depth = [s.astype(np.uint16) * 257 for s in grey]
    gidx = [m for s, m in zip(sources, index) if s.ndim == 2]
    jobs.append(frames_job(2, depth, maps, gidx))
    want.append([ref.nearest(d, maps[m]) for d, m in zip(depth, gidx)])
    return jobs, want


def same_bytes(got, want):
    if isinstance(want, (list, tuple)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            same_bytes(g, w)
    else:
        assert got.dtype == want.dtype and got.shape == want.shape
        assert got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def expected():
    return all_jobs()


def build(tmp, flags):
    (tmp / "rectify_main.cpp").write_text(RECTIFY_HOST)
    exe = tmp / "rectify_main"
    return exe, [_cxx(), "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(tmp / "rectify_main.cpp"), "-o", str(exe)] + flags


def test_header_in_the_kernels_schedule_equals_the_restatement(tmp_path, expected):
    exe, cmd = build(tmp_path, ["-O2"])
    subprocess.run(cmd, check=True)
    jobs, want = expected
    got = run_jobs(exe, tmp_path, jobs)
    for j, g, w in zip(jobs, got, want):
        same_bytes(g, w)


def test_header_standalone_under_sanitizers(tmp_path, expected):
    exe, base = build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    jobs, want = expected
    for g, w in zip(run_jobs(exe, tmp_path, jobs), want):
        same_bytes(g, w)


def test_cases_meet_the_rules_they_were_chosen_for():
    """The restatement on its own cases: identity, sentinels, the three remainders, ties, bits."""
    cases = {name: (cam, H, W) for name, cam, H, W in ref.map_cases()}
    q = ref.rect_map(*cases["identity"])
    v, u = np.meshgrid(np.arange(40), np.arange(49), indexing="ij")
    assert np.array_equal(q[..., 0], 32 * u) and np.array_equal(q[..., 1], 32 * v)
    q = ref.rect_map(*cases["behind"])
    assert np.all(q[:, :20] == ref.NONE) and np.all(q[:, 30:] != ref.NONE)
    for name in ("0 / 0", "2 / 0"):
        q = ref.rect_map(*cases[name])
        assert np.argwhere(q[..., 0] == ref.NONE).tolist() == [[5, 6]] and q[5, 6, 1] == ref.NONE
    for name, axis in (("far x", 0), ("far y", 1)):
        q = ref.rect_map(*cases[name])
        inside = q[..., 0] != ref.NONE
        assert inside.any() and (~inside).any() and np.abs(q[inside].astype(np.int64)).max() < 2 ** 26
        assert np.abs(q[inside][:, axis].astype(np.int64)).max() > 2 ** 25
    remap = {name: (src, m) for name, src, m in ref.remap_cases()}
    for target, value in ((511, 0), (512, 1), (513, 1)):                       # (1024 k + r + 512) >> 10 = k + (r >= 512)
        src, m = remap["remainder %d" % target]
        total = 961 * int(src[0, 0]) + 31 * int(src[0, 1]) + 31 * int(src[1, 0]) + int(src[1, 1])
        img, valid = ref.bilinear(src, m)
        assert total % 1024 == target and img[0, 0] == total // 1024 + value and valid[0, 0] == 1
    src, m = remap["all 255, 3 channels"]
    img, valid = ref.bilinear(src, m)
    assert np.all(img[valid == 1] == 255) and np.all(img[m[..., 0] == ref.NONE] == 0)
    # nearest: .5 rounds up on both sides of zero; the bits of NaN, the infinities and -0.0 come through
    src = np.arange(12, dtype=np.uint16).reshape(3, 4) + 1
    line = lambda qs: np.array([[(a, 0) for a in qs], [(a, 32) for a in qs]], dtype=np.int32)
    assert ref.nearest(src, line([-17, -16, -15, 15, 16, 17, 48, 111, 112]))[0].tolist() == [0, 1, 1, 1, 2, 2, 3, 4, 0]
    f32 = dict((n, s) for n, s, _ in ref.nearest_cases())["float32 grid"]
    got = ref.nearest(f32, line([0, 32, 64, 96, 128, 160, 192]))
    assert np.array_equal(got[0].view(np.uint32), f32[0].view(np.uint32)) and np.isnan(got[0, :3]).all()


def test_identity_camera_reproduces_the_input_bytes():
    rng = np.random.default_rng(3)
    for shape in ((40, 49), (40, 49, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        out, valid = ref.rectify(ref.identity_camera(ref.BASE_P), 40, 49, img)
        assert np.array_equal(out, img) and valid.all()
    depth = rng.standard_normal((40, 49)).astype(np.float32)
    assert np.array_equal(ref.nearest(depth, ref.rect_map(ref.identity_camera(ref.BASE_P), 40, 49)), depth)


# ---- the end-to-end scene, by the restatements alone -------------------------------------------------------------------
def scene_chain(lefts, rights):
    cam = ref.SCENE_P + (ref.SCENE_BASELINE,)
    want = [stereo_reference.extract_stereo(l, r, cam) for l, r in zip(lefts, rights)]
    kfs = [(w["keypoints"].astype(np.float64), w["points"], w["descriptors"]) for w in want]
    rows, reg = vis_reference.register(kfs[0], kfs[1], np.array(ref.SCENE_P))
    T = reg["T"]
    counts = dict(keypoints=[len(w["keypoints"]) for w in want], accepted=[int((w["status"] == 0).sum()) for w in want], matches=len(rows),
                  inliers=int(reg["inliers"].sum()))
    d_err = max(float(np.nanmax(np.abs(w["disparity"] - 10.0))) for w in want)
    t_err = float(np.abs(T[:3, 3] - ref.SCENE_PLANT).max())
    angle = float(np.arccos(np.clip((np.trace(T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return reg["status"], counts, d_err, t_err, angle


def test_scene_needs_rectification_and_is_registered_with_it():
    """Two stereo views of one block texture 16 columns apart behind mildly distorted, slightly rotated raw cameras.  Rectified
    by the restatement: 110 and 115 keypoints, 110 and 114 accepted, largest |d - 10| 0.493, 77 matches, 76 inliers,
    0.0088 m and 0.0041 rad from the plant (-0.32, 0, 0), inside the 0.04 m and 0.025 rad of the stereo end-to-end test.
    The raw frames as they are: 76 of 109 and 68 of 107 accepted, 39 inliers, 0.060 m, outside the bound."""
    lefts, rights, lc, rc = ref.scene()
    H, W = ref.SCENE_SIZE
    rl, rr_ = [ref.rectify(lc, H, W, x) for x in lefts], [ref.rectify(rc, H, W, x) for x in rights]
    assert all(v.all() for _, v in rl + rr_)
    status, counts, d_err, t_err, angle = scene_chain([x for x, _ in rl], [x for x, _ in rr_])
    print("rectified: %s, largest |d - 10| %.3f, translation error %.4f m, rotation %.4f rad" % (counts, d_err, t_err, angle))
    assert status == 0 and counts == ref.SCENE_RECTIFIED
    assert d_err <= 0.5 and t_err <= 0.04 and angle <= 0.025
    status, counts, d_err, t_err, angle = scene_chain(lefts, rights)
    print("raw: %s, translation error %.4f m, rotation %.4f rad" % (counts, t_err, angle))
    assert counts == ref.SCENE_RAW
    assert t_err > 0.04


# ---- the Python layer --------------------------------------------------------------------------------------------------
def test_raw_camera_layouts():
    from cslam_amd.front_end import rectify as rc
    R = ref.rotation(ref.BASE_R)
    a = rc.RawCamera(ref.BASE_K, ref.BASE_D, R, ref.BASE_P, (40, 49))
    assert np.array_equal(a.values, ref.camera(ref.BASE_K, ref.BASE_D, R, ref.BASE_P)) and (a.height, a.width) == (40, 49)
    K9 = [31.0, 0, 20.25, 0, 29.5, 17.5, 0, 0, 1]
    P12 = [33.0, 0, 24.5, -6.6, 0, 32.0, 19.75, 0, 0, 0, 1, 0]
    b = rc.RawCamera.from_camera_info(K9, ref.BASE_D[:5], R, P12, 49, 40)
    want = ref.camera(ref.BASE_K, ref.BASE_D[:5], R, ref.BASE_P, tx=-6.6)      # a 5-coefficient D: k4, k5, k6 are zero
    assert np.array_equal(b.values, want) and np.all(b.values[9:12] == 0.0) and b.values[8] == ref.BASE_D[4]
    assert b.projection == ref.BASE_P
    assert rc.stereo_camera(a, b) == ref.BASE_P + (6.6 / 33.0,)
    for bad in (lambda: rc.stereo_camera(a, a),                                                  # no baseline
                lambda: rc.stereo_camera(a, rc.RawCamera(ref.BASE_K, [], R, (33.0, 32.0, 24.5, 20.0, -6.6), (40, 49))),   # cy' differs
                lambda: rc.stereo_camera(a, rc.RawCamera(ref.BASE_K, [], R, ref.BASE_P + (-6.6,), (40, 48))),
                lambda: rc.stereo_camera(a, ref.BASE_P)):
        with pytest.raises(ValueError):
            bad()


def test_argument_errors_raise_before_any_launch():
    """Every one of these raises from the argument checks: none reaches the library, so none needs a GPU."""
    from cslam_amd.front_end import rectify as rc
    eye, K, P = np.identity(3), ref.BASE_K, ref.BASE_P
    skew = np.identity(3)
    skew[0, 1] = 1e-6
    cam = rc.RawCamera(K, [], eye, P, (48, 64))
    right = rc.RawCamera(K, [], eye, P + (-10.0,), (48, 64))
    img, depth = np.zeros((48, 64), dtype=np.uint8), np.zeros((48, 64), dtype=np.float32)
    maps = rc.RectifyMaps.__new__(rc.RectifyMaps)                              # checks come before anything touches the device
    maps.n, maps.device, maps.cameras = 2, 0, [cam, cam]
    bad = [lambda: rc.RawCamera(K[:3], [], eye, P, (48, 64)),                                     # layouts
           lambda: rc.RawCamera(K, [0.1] * 6, eye, P, (48, 64)),
           lambda: rc.RawCamera(K, [], eye[:2], P, (48, 64)),
           lambda: rc.RawCamera(K, [], eye, P[:3], (48, 64)),
           lambda: rc.RawCamera(K, [], eye, P, (48,)),
           lambda: rc.RawCamera(K, [], eye, P, (48.5, 64)),
           lambda: rc.RawCamera(K, [], eye, P, (1, 64)),                                          # sizes
           lambda: rc.RawCamera(K, [], eye, P, (1 << 16, 1 << 15)),
           lambda: rc.RawCamera((np.nan,) + K[1:], [], eye, P, (48, 64)),                         # finite, positive
           lambda: rc.RawCamera(K, [np.inf, 0, 0, 0], eye, P, (48, 64)),
           lambda: rc.RawCamera((0.0,) + K[1:], [], eye, P, (48, 64)),
           lambda: rc.RawCamera(K, [], eye, (33.0, -32.0, 24.5, 19.75), (48, 64)),
           lambda: rc.RawCamera(K, [], skew, P, (48, 64)),                                        # R
           lambda: rc.RawCamera(K, [], 1.001 * eye, P, (48, 64)),
           lambda: rc.RawCamera(K, [], np.diag([1.0, 1.0, -1.0]), P, (48, 64)),
           lambda: rc.RawCamera.from_camera_info([31.0, 0.5, 20.0, 0, 29.5, 17.5, 0, 0, 1], [], eye, [33.0, 0, 24.5, 0, 0, 32.0, 19.75, 0, 0, 0, 1, 0],
                                                 64, 48),
           lambda: rc.RawCamera.from_camera_info(K, [], eye, P, 64, 48),
           lambda: rc.rectify_maps([]),
           lambda: rc.rectify_maps([K]),
           lambda: rc.rectify_images([img], None),                                                # staged calls
           lambda: rc.rectify_images([img.astype(np.float32)], maps),
           lambda: rc.rectify_images([np.zeros((48, 64, 4), dtype=np.uint8)], maps),
           lambda: rc.rectify_images([img, img, img], maps),
           lambda: rc.rectify_images([img], maps, [2]),
           lambda: rc.rectify_images([img], maps, [-1]),
           lambda: rc.rectify_images([img], maps, [0.5]),
           lambda: rc.rectify_images([img], maps, [0, 1]),
           lambda: rc.rectify_depths([img], maps, [0]),
           lambda: rc.rectify_depths([depth, depth.astype(np.uint16)], maps),
           lambda: rc.rectify_depths([depth[:1]], maps, [0]),
           lambda: rc.extract_keyframes_stereo_raw([img], [img, img], cam, right),               # chains
           lambda: rc.extract_keyframes_stereo_raw([img], [img], cam, cam),
           lambda: rc.extract_keyframes_stereo_raw([img], [img], [cam, cam], right),
           lambda: rc.extract_keyframes_stereo_raw([img], [img], cam, right, max_disparity=256),
           lambda: rc.extract_keyframes_stereo_raw([img], [img], cam, right, border=3),
           lambda: rc.extract_keyframes_stereo_raw([img], [img], K, right),
           lambda: rc.keyframe_clouds_stereo_raw([img], [img], cam, right, voxel_size=np.nan),
           lambda: rc.keyframe_clouds_stereo_raw([img], [img], cam, right, max_range=-1.0),
           lambda: rc.keyframe_clouds_stereo_raw([img], [img.astype(np.int8)], cam, right),
           lambda: rc.extract_keyframes_raw([img], [], cam),
           lambda: rc.extract_keyframes_raw([img], [depth[:, :60]], cam),
           lambda: rc.extract_keyframes_raw([img], [depth.astype(np.float64)], cam),
           lambda: rc.extract_keyframes_raw([img], [depth], cam, max_features=0),
           lambda: rc.extract_keyframes_raw([img], [depth], rc.RawCamera(K, [], eye, P, (30, 64)))]        # smaller than 2 border + 1
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d did not raise" % k)


def test_no_cpu_path():
    """Without a GPU the functions raise CslamHipError once the arguments are right; with one this test has nothing to say."""
    import torch
    from cslam_amd import _lib
    from cslam_amd.front_end import rectify as rc
    if torch.cuda.is_available():
        return
    cam = rc.RawCamera(ref.BASE_K, [], np.identity(3), ref.BASE_P, (48, 64))
    right = rc.RawCamera(ref.BASE_K, [], np.identity(3), ref.BASE_P + (-10.0,), (48, 64))
    img, depth = np.zeros((48, 64), dtype=np.uint8), np.ones((48, 64), dtype=np.float32)
    for f in (lambda: rc.rectify_maps([cam]), lambda: rc.extract_keyframes_stereo_raw([img], [img], cam, right),
              lambda: rc.keyframe_clouds_stereo_raw([img], [img], cam, right), lambda: rc.extract_keyframes_raw([img], [depth], cam)):
        with pytest.raises(_lib.CslamHipError):
            f()
