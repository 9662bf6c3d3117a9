"""CPU: the host side of the keyframe clouds and the swarm map.

  * the argument checks of the four entry points of csrc/cloud.hip come before anything touches HIP; no CPU path
  * the constants in Python mirror csrc/cloud.h
  * the facts about tests/cloud_reference.py that tests/test_cloud_gpu.py rests on, each asserted and printed
  * csrc/cloud.h and the plan (csrc/voxel_plan.h) as a stand-alone program under -fsanitize=address,undefined, whose
    projected points are compared with the numpy restatement bit for bit (never loaded into Python); in the same program
    the open3d rule of the lidar filter (GridOpen3d) against the indices of icp_reference.voxel_average
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_reference as ref
from conftest import ROOT
from cslam_amd import _lib

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
F = np.float32


def _no_gpu():
    n = C.c_int(0)
    return _lib.load().cslam_device_count(C.byref(n)) != 0 or n.value == 0


def _p(arr):
    return arr.ctypes.data_as(C.c_void_p)


_DUMMY = np.zeros(64, dtype=np.float64)
P = _p(_DUMMY)                                             # host memory in place of every device buffer: a check returns before it is used


def _voxel(leaf=0.05, max_range=2.0, n=2, offsets=(0, 3, 5), null=()):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    a = dict(points=P, rgb=P, off=P, out=P, out_rgb=P, counts=P, out_off=P, status=P, h_off=_p(off))
    a.update({k: None for k in null})
    return _lib.load().cslam_cloud_voxel_dev(a["points"], a["rgb"], a["off"], n, leaf, max_range, a["out"], a["out_rgb"], a["counts"],
                                             a["out_off"], a["status"], a["h_off"], None)


def _frames(chain, n=2, offsets=(0, 6, 10), hw=((2, 3), (2, 2)), channels=3, depth_type=0, leaf=0.05, max_range=2.0, null=()):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    hw = np.ascontiguousarray(hw, dtype=np.int32)
    a = dict(image=P, depth=P, off=P, hw=P, cam=P, h_off=_p(off), h_hw=_p(hw), out=P, out_rgb=P)
    a.update({k: None for k in null})
    lib = _lib.load()
    if chain:
        return lib.cslam_cloud_keyframes_dev(a["image"], channels, a["depth"], depth_type, a["off"], a["hw"], a["cam"], n, leaf, max_range,
                                             a["out"], a["out_rgb"], P, P, P, a["h_off"], a["h_hw"], None)
    return lib.cslam_cloud_from_depth_dev(a["image"], channels, a["depth"], depth_type, a["off"], a["hw"], a["cam"], n, a["out"], a["out_rgb"],
                                          a["h_off"], a["h_hw"], None)


def _map(voxel=0.1, n=2, offsets=(0, 3, 5), dtype=0, null=()):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    a = dict(points=P, off=P, poses=P, out=P, h_off=_p(off))
    a.update({k: None for k in null})
    return _lib.load().cslam_map_assemble_dev(a["points"], dtype, P, a["off"], a["poses"], n, voxel, a["out"], P, P, P, P, a["h_off"], None)


BAD_LEAF = [0.0, -0.05, float("nan"), float("inf")]
BAD_SHAPES = [dict(n=0, offsets=[0]), dict(n=65536, offsets=[0] * 65537), dict(offsets=[0, 5, 3]), dict(offsets=[1, 3, 5])]
SHAPE_IDS = ["n=0", "n=65536", "decreasing", "start!=0"]


def _invalid(rc):
    assert rc == -1
    assert b"invalid argument" in _lib.load().cslam_last_error()


@pytest.mark.parametrize("leaf", BAD_LEAF)
def test_a_filter_refuses_a_bad_voxel_before_hip(leaf):
    _invalid(_voxel(leaf=leaf))
    _invalid(_frames(True, leaf=leaf))
    _invalid(_map(voxel=leaf))


@pytest.mark.parametrize("kw", BAD_SHAPES, ids=SHAPE_IDS)
def test_shape_checks_precede_hip(kw):
    _invalid(_voxel(**kw))
    _invalid(_map(**kw))
    fk = dict(kw)
    if fk.get("n", 2) != 2:
        fk["hw"] = [(1, 1)] * max(fk["n"], 1)
    _invalid(_frames(False, **fk))
    _invalid(_frames(True, **fk))


@pytest.mark.parametrize("null", ["points", "off", "out", "h_off"])
def test_null_pointers_are_refused_before_hip(null):
    _invalid(_voxel(null=(null,)))
    _invalid(_map(null=(null,)))


@pytest.mark.parametrize("chain", [False, True], ids=["from_depth", "keyframes"])
def test_frame_checks_precede_hip(chain):
    for null in ("image", "depth", "off", "hw", "cam", "h_off", "h_hw", "out", "out_rgb"):
        _invalid(_frames(chain, null=(null,)))
    _invalid(_frames(chain, channels=2))
    _invalid(_frames(chain, depth_type=2))
    _invalid(_frames(chain, hw=((2, 3), (2, 3))))                                   # offsets say 4 pixels, the size 6
    _invalid(_frames(chain, hw=((2, 3), (0, 4)), offsets=(0, 6, 6)))                # an empty frame


def test_other_argument_checks():
    _invalid(_voxel(max_range=-1.0))
    _invalid(_voxel(max_range=float("nan")))
    _invalid(_frames(True, max_range=-1.0))
    _invalid(_map(dtype=2))
    lib = _lib.load()
    assert lib.cslam_cloud_profile_read(None, None) == -1


@pytest.mark.skipif(not _no_gpu(), reason="GPU present: covered by the -m gpu suite")
def test_everything_fails_loudly_without_gpu():
    from cslam_amd.back_end import swarm_map
    from cslam_amd.front_end import keyframe_clouds as kc
    assert _voxel() == -2 and _map() == -2 and _frames(False) == -2 and _frames(True) == -2      # valid: the first HIP call fails
    img, d = ref.scene_image(4, 4), ref.scene_depth(4, 4)
    pts = np.random.default_rng(0).standard_normal((20, 3)).astype(F)
    col = np.zeros((20, 3), dtype=np.uint8)
    for call in (lambda: kc.create_colored_pointcloud(img, d, ref.SCENE_CAMERA), lambda: kc.create_colored_pointclouds([img], [d], ref.SCENE_CAMERA),
                 lambda: kc.voxel_subsample(pts, col), lambda: kc.voxel_subsample_batch([(pts, col)]), lambda: kc.voxel_subsample(pts, col, 0.0),
                 lambda: kc.keyframe_clouds([img], [d], ref.SCENE_CAMERA), lambda: kc.keyframe_clouds([img], [d], ref.SCENE_CAMERA, voxel_size=0),
                 lambda: swarm_map.assemble_map({0: pts}, {0: np.identity(4)}, 0.1)):
        with pytest.raises(_lib.CslamHipError):
            call()


def test_python_argument_checks_come_first():
    from cslam_amd.back_end import swarm_map
    from cslam_amd.front_end import keyframe_clouds as kc
    img, d = ref.scene_image(4, 4), ref.scene_depth(4, 4)
    with pytest.raises(ValueError, match="empty cloud"):
        kc.create_colored_pointcloud(img, d[:3], ref.SCENE_CAMERA)                  # the reference returns an empty cloud
    with pytest.raises(ValueError):
        kc.keyframe_clouds([img], [d.astype(np.float64)], ref.SCENE_CAMERA)
    with pytest.raises(ValueError):
        kc.voxel_subsample(np.zeros((3, 3), dtype=F), np.zeros((2, 3), dtype=np.uint8))
    with pytest.raises(KeyError):
        swarm_map.assemble_map({0: np.zeros((3, 3)), 1: np.zeros((3, 3))}, {0: np.identity(4)}, 0.1)
    bad = np.identity(4)
    bad[0, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        swarm_map.assemble_map({0: np.zeros((3, 3))}, {0: bad}, 0.1)
    with pytest.raises(ValueError):
        swarm_map.assemble_map({0: np.zeros((3, 3))}, {0: np.identity(4)}, 0.0)


def test_constants_mirror_the_kernels():
    from cslam_amd.front_end import keyframe_clouds as kc
    from cslam_amd.lidar_pr import icp_utils
    head = open(os.path.join(CSRC, "cloud.h")).read()
    assert "#define CLOUD_DEPTH_U16 %d " % kc.CLOUD_DEPTH_U16 in head
    assert "#define CLOUD_DEPTH_F32 %d " % kc.CLOUD_DEPTH_F32 in head
    assert "#define CLOUD_BOUNDS_BLOCK %d " % kc.CLOUD_BOUNDS_BLOCK in head
    assert "#define CLOUD_CELL_LIMIT %.1f " % ref.CELL_LIMIT in head
    plan = open(os.path.join(CSRC, "voxel_plan.h")).read()
    assert "#define VOXEL_AXIS_BITS 21 " in plan and ref.AXIS_LIMIT == 2 ** 21
    assert "#define VOXEL_TILE %d " % icp_utils.VOXEL_TILE in plan
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "cloud.hip" in make and "cloud.h " in make and "voxel_engine.h" in make
    assert _lib.F32 == 0 and _lib.F64 == 1
    w = kc.pack_colors(np.array([[1, 2, 3]], dtype=np.uint8))
    assert w.tolist() == [1 | 2 << 8 | 3 << 16] and kc.unpack_colors(w).tolist() == [[1, 2, 3]]


# ---- facts the GPU tests rest on -------------------------------------------------------------------------------------
def test_fact_a_the_folded_constant_gives_other_bits_than_metres_first():
    d = ref.scene_depth()
    valid = d.reshape(-1) != 0
    p, _ = ref.back_project(ref.scene_image(), d, ref.SCENE_CAMERA)
    q = ref.back_project_metres_first(d, ref.SCENE_CAMERA)
    dx = np.mean(p[valid, 0] != q[valid, 0])
    any_axis = np.mean((p[valid] != q[valid]).any(axis=1))
    print("valid pixels whose x differs from metres-first: %.3f (any coordinate: %.3f)" % (dx, any_axis))
    assert dx >= 0.25                                      # measured 0.477
    assert np.abs(p[valid] - q[valid]).max() < 1e-6        # and only in the last bits


def test_fact_b_the_filter_depends_on_the_order_of_the_sum():
    p, c = ref.back_project(ref.scene_image(), ref.scene_depth(), ref.SCENE_CAMERA)
    fwd, _, cnt = ref.voxel_filter(p, c, 0.1)
    rev, _, cnt_r = ref.voxel_filter(p[::-1], c[::-1], 0.1)
    differ = np.mean((fwd != rev).any(axis=1))
    print("leaf 0.1: %d voxels, largest %d points, %.2f hold more than one; centroid changes under reversal: %.3f"
          % (len(fwd), cnt.max(), np.mean(cnt > 1), differ))
    assert len(fwd) == 457 and cnt.max() == 16 and abs(np.mean(cnt > 1) - 0.87) < 0.005
    assert np.array_equal(cnt, cnt_r)
    assert differ >= 0.4                                   # measured 0.556


def test_fact_c_the_map_depends_on_the_order_of_the_sum():
    k1, k2 = ref.scene_keyframes()
    T1, T2 = ref.scene_poses()
    assert len(k1[0]) == 1518 and len(k2[0]) == 1541
    fwd = ref.assemble_map([k1[:2], k2[:2]], [T1, T2], 0.1)
    rev = ref.assemble_map([(k2[0][::-1], k2[1][::-1]), (k1[0][::-1], k1[1][::-1])], [T2, T1], 0.1)
    swap = ref.assemble_map([k2[:2], k1[:2]], [T2, T1], 0.1)
    differ, differ_swap = np.mean((fwd[0] != rev[0]).any(axis=1)), np.mean((fwd[0] != swap[0]).any(axis=1))
    print("map voxel 0.1: %d rows, largest %d points; centroid changes under full reversal: %.3f, under a swap of the keyframes: %.3f"
          % (len(fwd[0]), fwd[2].max(), differ, differ_swap))
    assert len(fwd[0]) == 839 and fwd[2].max() == 11
    assert np.array_equal(fwd[2], rev[2]) and np.array_equal(fwd[1], rev[1])       # integer sums do not depend on the order
    assert differ >= 0.15                                  # measured 0.236
    assert differ_swap < 0.1                               # measured 0.04: too few, so the GPU test uses the full reversal


def test_fact_d_index_values_at_the_edge_of_the_key_range():
    # keyframe rule, leaf 0.5: inv = 2 exactly
    pts = np.array([[0.0, 0.0, 0.0], [(2 ** 21 - 1) * 0.5, 0.0, 0.0]], dtype=F)
    assert ref.grid_indices(pts, F(1) / F(0.5))[1, 0] == 2 ** 21 - 1               # the last index a key holds
    pts[1, 0] = 2 ** 21 * 0.5
    with pytest.raises(ref.RangeError):
        ref.grid_indices(pts, F(1) / F(0.5))                                       # the first that is refused
    with pytest.raises(ref.RangeError):
        ref.grid_indices(np.array([[-3e9, 0, 0]], dtype=F), F(1))                  # a cell that PCL's int does not hold
    with pytest.raises(ref.RangeError), np.errstate(over="ignore"):
        ref.grid_indices(np.array([[1.0, 0, 0]], dtype=F), F(1) / F(1e-45))         # inv = inf
    # PCL's rule: floor(p * inv), not a division: 0.3f * (1 / 0.1f) lands on 3, the true quotient below it
    assert np.floor(F(0.3) * (F(1) / F(0.1))) == 3.0 and np.floor(0.3 / 0.1) == 2.0
    # map rule: a true division in float64, anchored at the world origin and negative below it
    pw = np.array([[1000.0, -0.05, 0.0], [1000.0 + (2 ** 21 - 1) * 0.5, 0.3, 0.0]])
    assert ref.grid_indices(pw, np.float64(0.5))[1, 0] == 2 ** 21 - 1
    assert ref._cells(pw[:, 1], np.float64(0.1)).tolist() == [-1.0, 2.0]
    pw[1, 0] += 0.5
    with pytest.raises(ref.RangeError):
        ref.grid_indices(pw, np.float64(0.5))
    # the grid does not move with the cloud: a point keeps its cell when another keyframe extends the map below it
    assert ref._cells(np.array([1000.26]), np.float64(0.1))[0] == 10002.0


# ---- stand-alone under sanitizers ----------------------------------------------------------------------------------
CLOUD_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cloud.h"

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

template <typename S> static size_t write_head(int n_clouds, int64_t n_pts, int64_t n_mid) {
    const int nb = cloud_bounds_blocks(n_clouds);
    CloudHead<S> h;
    Carver size;
    cloud_head_layout<S>(size, n_clouds, nb, n_pts, n_mid, &h);
    char *block = (char *)malloc(h.bytes ? h.bytes : 1);
    Carver place(block);
    cloud_head_layout<S>(place, n_clouds, nb, n_pts, n_mid, &h);
    if (place.at != size.at) { printf("layout drift\n"); exit(1); }
    // every piece to its full length: an overlap or an overrun is the sanitizer's to find
    for (int64_t i = 0; i < 3 * n_pts; ++i) h.pts[i] = (S)1;
    for (int64_t i = 0; i < n_pts; ++i) h.rgb[i] = 2u;
    for (int64_t i = 0; i < (int64_t)n_clouds * nb * CLOUD_NPART; ++i) h.part[i] = (S)3;
    for (int64_t i = 0; i < (int64_t)n_clouds * nb; ++i) h.part_missing[i] = 4u;
    for (int64_t i = 0; i < 3 * (int64_t)n_clouds; ++i) h.base[i] = (S)5;
    for (int64_t i = 0; i < 4 * (int64_t)n_clouds; ++i) h.meta[i] = 6;
    h.head[0] = h.head[1] = 7; h.kept[0] = 8u; h.one_off[0] = h.one_off[1] = 9;
    for (int64_t i = 0; i < 3 * n_mid; ++i) h.mid[i] = (S)10;
    for (int64_t i = 0; i < n_mid; ++i) { h.mid_rgb[i] = 11u; h.mid_counts[i] = 12; }
    for (int64_t i = 0; i <= n_clouds; ++i) h.mid_off[i] = 13;
    size_t sum = 0;
    for (int64_t i = 0; i < 3 * n_pts; ++i) sum += (size_t)h.pts[i];
    for (int64_t i = 0; i < n_mid; ++i) sum += h.mid_rgb[i];
    const size_t bytes = h.bytes;
    free(block);
    return sum + bytes;
}

// open3d's rule on the clouds of a file (per cloud: int64 n, double voxel, n rows of 3 doubles): "G status bx by bz", then
// per row "P ix iy iz key".  The bounds are taken as the bounds kernel takes them; a refused cloud prints no rows.
static void open3d_clouds(const char *path) {
    FILE *fp = fopen(path, "rb");
    if (!fp) { printf("no clouds file\n"); exit(1); }
    int64_t n;
    while (fread(&n, 8, 1, fp) == 1) {
        double voxel;
        if (fread(&voxel, 8, 1, fp) != 1) exit(1);
        double *p = (double *)malloc((size_t)(n ? n : 1) * 24);
        if (fread(p, 24, (size_t)n, fp) != (size_t)n) exit(1);
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, base[3];
        for (int64_t i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], p[3 * i + a]); hi[a] = fmax(hi[a], p[3 * i + a]); }
        const GridOpen3d::P g = {voxel, voxel / 2.0};
        int b[3];
        const int over = GridOpen3d::range(lo, hi, g, base, b);
        printf("G %d %d %d %d\n", over, b[0], b[1], b[2]);
        for (int64_t i = 0; i < n && !over; ++i) {
            uint32_t k[3];
            for (int a = 0; a < 3; ++a) k[a] = GridOpen3d::index(p[3 * i + a], g, base[a]);
            printf("P %u %u %u %llx\n", k[0], k[1], k[2],
                   (unsigned long long)GridOpen3d::key(k[0], k[1], k[2], b[1] + b[2 - GridOpen3d::MAJOR], b[2 - GridOpen3d::MAJOR]));
        }
        free(p);
    }
    fclose(fp);
}

int main(int argc, char **argv) {
    if (argc > 1) open3d_clouds(argv[1]);
    // projected points of a small frame in both depth types, for the comparison with the numpy restatement
    const double cam[4] = {60.0, 61.0, 31.5, 23.5};
    float k[4], p[3];
    cloud_constants(cam, CLOUD_DEPTH_U16, k);
    for (int v = 0; v < 5; ++v)
        for (int u = 0; u < 7; ++u) {
            const uint16_t d = (uint16_t)((u * 7 + v * 3) % 5 == 0 ? 0 : 1500 + 8 * u + 5 * v);
            cloud_project(u, v, d, k, p);
            printf("U %d %d %08x %08x %08x\n", u, v, bits(p[0]), bits(p[1]), bits(p[2]));
        }
    cloud_constants(cam, CLOUD_DEPTH_F32, k);
    const float fd[6] = {1.25f, 0.0f, -2.0f, INFINITY, NAN, 3.1f};
    for (int u = 0; u < 6; ++u) {
        cloud_project(u, 2, fd[u], k, p);
        printf("F %d %08x %08x %08x\n", u, bits(p[0]), bits(p[1]), bits(p[2]));
    }
    // ranges: the last index a key holds, the first that is refused, a cell beyond int, an infinite scale
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {(float)((1 << 21) - 1) * 0.5f, 0.f, 3.f}, base[3];
    int b[3];
    int over = cloud_axis_range(lo, hi, 2.0f, base, b);
    printf("R %d %d %d %d\n", over, b[0], b[1], b[2]);
    const uint64_t key = cloud_key(cloud_index(hi[0], 2.0f, base[0]), 0, cloud_index(hi[2], 2.0f, base[2]), b[0], b[0] + b[1]);
    printf("K %llx\n", (unsigned long long)key);
    hi[0] = (float)(1 << 21) * 0.5f;
    printf("R %d\n", cloud_axis_range(lo, hi, 2.0f, base, b));
    lo[0] = -3e9f; hi[0] = -3e9f;
    printf("R %d\n", cloud_axis_range(lo, hi, 1.0f, base, b));
    lo[0] = 1.f; hi[0] = 1.f;
    printf("R %d\n", cloud_axis_range(lo, hi, INFINITY, base, b));
    double dlo[3] = {1000.0, -0.05, 0.0}, dhi[3] = {1000.0 + ((1 << 21) - 1) * 0.5, 0.3, 0.0}, dbase[3];
    over = cloud_axis_range(dlo, dhi, 0.5, dbase, b);
    printf("R %d %d\n", over, b[0]);
    dlo[0] = dhi[0] = 1e300;
    printf("R %d\n", cloud_axis_range(dlo, dhi, 1e-300, dbase, b));
    printf("C %d %d %d\n", (int)cloud_clip_keep(0.0f, 2.0f), (int)cloud_clip_keep(2.0f, 2.0f), (int)cloud_clip_keep(NAN, 2.0f));
    // the scratch layouts and the plan they go with
    size_t sum = 0;
    const int64_t sizes[5] = {0, 1, 2047, 2048, 6149};
    for (int s = 0; s < 5; ++s)
        for (int n_clouds = 1; n_clouds <= 300; n_clouds += 299) {
            sum += write_head<float>(n_clouds, sizes[s], sizes[s]);
            sum += write_head<double>(n_clouds, sizes[s], 0);
            VoxelPlan pl;
            if (voxel_make_plan(sizes[s], n_clouds, 40, 1, nullptr, &pl)) { printf("plan refused\n"); return 1; }
            char *block = (char *)malloc(pl.bytes ? pl.bytes : 1);
            voxel_make_plan(sizes[s], n_clouds, 40, 1, block, &pl);
            for (int64_t i = 0; i < sizes[s]; ++i) { pl.flags[i] = 1; pl.rank[i] = 2u; pl.seg_start[i] = 3u; pl.seg_end[i] = 4u; }
            for (int64_t i = 0; i < pl.flag_tiles; ++i) pl.tile_count[i] = 5u;
            pl.rows[0] = 6u;
            sum += pl.bytes;
            free(block);
        }
    printf("cloud ok: %zu\n", sum);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


def _sanitizer_flags(cxx, tmp_path):
    """The flags with which this compiler builds and runs a trivial program under both sanitizers; skips when it has no
    sanitizer runtime.  Asked before the program under test is compiled, so that a failure there is a failure."""
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        flags = ["-fsanitize=address,undefined"] + extra
        r = subprocess.run([cxx, str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")] + flags, capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            return flags
    pytest.skip("this compiler has no sanitizer runtime")


@pytest.fixture(scope="module")
def cloud_main(tmp_path_factory):
    """The stand-alone program, built once with -fsanitize=address,undefined."""
    tmp_path = tmp_path_factory.mktemp("cloud_main")
    cxx = _cxx()
    flags = _sanitizer_flags(cxx, tmp_path)
    (tmp_path / "cloud_main.cpp").write_text(CLOUD_MAIN)
    exe = tmp_path / "cloud_main"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "cloud_main.cpp"), "-o", str(exe)]
                       + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _open3d_clouds():
    """(cloud, voxel) pairs for the open3d rule: seeded rows with negative coordinates, rows exactly on cell faces, one row,
    all three axes at the widest index a key holds (shifts of 42 and 21), a span of 2^21 - 1 cells and one of 2^21."""
    rng = np.random.default_rng(33)
    faces = np.concatenate([[[-1.75, -1.75, -1.75]], rng.integers(-3, 5, (200, 3)) * 0.5])      # minimum -1.75: faces at multiples of 0.5
    top = (2 ** 21 - 1) * 0.5
    wide = np.concatenate([[[0.0, 0.0, 0.0], [top, top, top]], rng.integers(0, 2 ** 21, (60, 3)) * 0.5])
    return [(rng.uniform(-3.0, 2.0, (300, 3)), 0.3), (faces, 0.5), (np.array([[0.1, -7.0, 3.0]]), 0.5), (wide, 0.5),
            (np.array([[0.0, 0.0, 0.0], [0.0, top, 0.0]]), 0.5), (np.array([[0.0, 0.0, 0.0], [0.0, 2 ** 21 * 0.5, 0.0]]), 0.5)]


def test_open3d_rule_under_sanitizers(cloud_main, tmp_path):
    """GridOpen3d's range, index and key in the stand-alone program against the indices of icp_reference.voxel_average:
    the same integers row by row, keys that pack them with the cloud's own widths, and, grouped by those keys in key order,
    voxel_average's very rows."""
    import icp_reference
    clouds = _open3d_clouds()
    with open(tmp_path / "clouds.bin", "wb") as fp:
        for pts, voxel in clouds:
            fp.write(np.int64(len(pts)).tobytes() + np.float64(voxel).tobytes() + np.ascontiguousarray(pts, dtype=np.float64).tobytes())
    r = subprocess.run([str(cloud_main), str(tmp_path / "clouds.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    heads = [k for k, ln in enumerate(lines) if ln[0] == "G"]
    assert len(heads) == len(clouds)
    statuses = []
    for (pts, voxel), at in zip(clouds, heads):
        origin = pts.min(axis=0) - voxel / 2.0                                      # voxel_average's own two lines
        want = np.floor((pts - origin) / voxel).astype(np.int64)
        over = int((want.max(axis=0) >= 2 ** 21).any())
        statuses.append(over)
        bits = [0 if over and q >= 2 ** 21 else int(q).bit_length() for q in want.max(axis=0)]
        assert [int(x) for x in lines[at][1:]] == [over] + bits, lines[at]
        rows = lines[at + 1:at + 1 + len(pts)]
        if over:
            assert at + 1 == len(lines) or lines[at + 1][0] != "P"
            continue
        assert all(ln[0] == "P" for ln in rows) and len(rows) == len(pts)
        got = np.array([[int(x) for x in ln[1:4]] for ln in rows], dtype=np.int64)
        assert np.array_equal(got, want)
        keys = [int(ln[4], 16) for ln in rows]
        assert keys == [(int(i) << (bits[1] + bits[2])) | (int(j) << bits[2]) | int(k) for i, j, k in want]
        uniq, inv, cnt = np.unique(np.array(keys, dtype=np.uint64), return_inverse=True, return_counts=True)
        out = np.zeros((len(uniq), 3))
        np.add.at(out, inv.reshape(-1), pts)
        assert np.array_equal(out / cnt[:, None], icp_reference.voxel_average(pts, voxel))
    assert statuses == [0, 0, 0, 0, 0, 1]
    assert lines[heads[3]][1:] == ["0", "21", "21", "21"] and lines[heads[4]][1:] == ["0", "0", "21", "0"]
    faces = clouds[1][0]
    assert np.array_equal((faces[1:] + 2.0) / 0.5, np.floor((faces[1:] + 2.0) / 0.5))      # origin -2: those rows ARE on cell faces


def test_cloud_header_under_sanitizers(cloud_main):
    """cloud.h and the plan in a stand-alone program with its own main, built with -fsanitize=address,undefined: the
    projection in both depth types (compared with the restatement bit for bit), the range rule at its edges, every piece of
    every scratch layout written to its full length.  Not loaded into Python."""
    r = subprocess.run([str(cloud_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cloud ok:" in r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    # the same frame in numpy
    u, v = np.meshgrid(np.arange(7), np.arange(5))
    d = np.where((u * 7 + v * 3) % 5 == 0, 0, 1500 + 8 * u + 5 * v).astype(np.uint16)
    want, _ = ref.back_project(np.zeros((5, 7), dtype=np.uint8), d, ref.SCENE_CAMERA)
    got = {(int(ln[1]), int(ln[2])): [int(x, 16) for x in ln[3:]] for ln in lines if ln[0] == "U"}
    assert len(got) == 35
    for (uu, vv), w in got.items():
        assert w == want[vv * 7 + uu].view(np.uint32).tolist(), (uu, vv)
    fd = np.zeros((3, 6), dtype=F)
    fd[2] = [1.25, 0.0, -2.0, np.inf, np.nan, 3.1]
    want, _ = ref.back_project(np.zeros((3, 6), dtype=np.uint8), fd, ref.SCENE_CAMERA)
    got = {int(ln[1]): [int(x, 16) for x in ln[2:]] for ln in lines if ln[0] == "F"}
    for uu in range(6):
        row = want[2 * 6 + uu]
        if np.isnan(row).any():
            assert all(np.isnan(np.array(got[uu], dtype=np.uint32).view(F))), uu
        else:
            assert got[uu] == row.view(np.uint32).tolist(), uu
    assert np.isfinite(want[2 * 6 + 1]).all() and np.isfinite(want[2 * 6 + 2]).all()       # depths 0 and -2 are valid
    ranges = [ln[1:] for ln in lines if ln[0] == "R"]
    assert ranges == [["0", "21", "0", "3"], ["1"], ["1"], ["1"], ["0", "21"], ["1"]]
    assert [ln[1] for ln in lines if ln[0] == "K"] == ["%x" % ((6 << 21) | (2 ** 21 - 1))]
    assert [ln[1:] for ln in lines if ln[0] == "C"] == [["1", "1", "0"]]


# ---- write_ply -------------------------------------------------------------------------------------------------------
def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    dtype = np.dtype([(name, {"double": "<f8", "float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    assert len(body) == n * dtype.itemsize
    return np.frombuffer(body, dtype=dtype), [name for _, name in props]


@pytest.mark.parametrize("colors", [True, False])
def test_write_ply_round_trip(tmp_path, colors):
    from cslam_amd.back_end import swarm_map
    from cslam_amd.front_end import keyframe_clouds as kc
    rng = np.random.default_rng(7)
    pts = rng.standard_normal((37, 3))
    col = rng.integers(0, 256, (37, 3), dtype=np.uint8) if colors else None
    swarm_map.write_ply(tmp_path / "map.ply", swarm_map.SwarmMap(pts, col, np.ones(37, dtype=np.int64)))
    rec, names = _read_ply(tmp_path / "map.ply")
    assert names == ["x", "y", "z"] + (["red", "green", "blue"] if colors else [])
    assert rec["x"].dtype == np.float64 and np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], axis=1), pts)
    if colors:
        assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], axis=1), col)
    # a keyframe cloud keeps its float32
    swarm_map.write_ply(tmp_path / "kf.ply", kc.KeyframeCloud(pts.astype(F), col, None))
    rec, _ = _read_ply(tmp_path / "kf.ply")
    assert rec["x"].dtype == F and np.array_equal(rec["z"], pts[:, 2].astype(F))
    swarm_map.write_ply(tmp_path / "empty.ply", swarm_map.SwarmMap(np.zeros((0, 3)), None, np.zeros(0, dtype=np.int64)))
    assert len(_read_ply(tmp_path / "empty.ply")[0]) == 0
