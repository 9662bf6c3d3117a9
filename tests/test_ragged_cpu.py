"""CPU: csrc/ragged.h compiled for the host: the one offsets rule of the registration entry points against its statement in
numpy, the scratch carver, and `voxel_make_plan` (csrc/voxel_plan.h), which carves with it.  The same code once more as a
stand-alone program under -fsanitize=address,undefined, which writes every piece of every layout to its full length
(never loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
LP = ctypes.POINTER(ctypes.c_int64)
OK, E_START, E_DECREASE = 0, 1, 2

# shared by the wrapper and the stand-alone program: a layout of `k` pieces of counts[q] elements of elem[q] bytes, and
# the pieces of a voxel plan with their lengths in bytes
COMMON = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "ragged.h"
#include "voxel_plan.h"
static void layout(Carver &cv, int k, const int64_t *counts, const int *elem, int64_t slack, char **piece) {
    for (int q = 0; q < k; ++q) {
        const size_t c = (size_t)counts[q], s = (size_t)slack;
        piece[q] = elem[q] == 8 ? (char *)cv.take<uint64_t>(c, s) : elem[q] == 4 ? (char *)cv.take<uint32_t>(c, s)
                 : elem[q] == 2 ? (char *)cv.take<uint16_t>(c, s) : (char *)cv.take<uint8_t>(c, s);
    }
}
enum { VOXEL_PIECES = 13 };
static void voxel_pieces(const VoxelPlan &p, char **piece, int64_t *len) {
    char *at[VOXEL_PIECES] = {(char *)p.keys[0], (char *)p.keys[1], (char *)p.idx[0], (char *)p.idx[1], (char *)p.cloud_of, (char *)p.flags,
                              (char *)p.rank, (char *)p.seg_start, (char *)p.seg_end, (char *)p.hist, (char *)p.totals,
                              (char *)p.tile_count, (char *)p.rows};
    const int64_t bytes[VOXEL_PIECES] = {8 * p.n, 8 * p.n, 4 * p.n, 4 * p.n, 2 * p.n, p.n, 4 * p.n, 4 * p.n, 4 * p.n,
                                         p.tiles * 4 * (1 << VOXEL_RADIX_BITS), 4 * (1 << VOXEL_RADIX_BITS), 4 * p.flag_tiles, 4};
    for (int q = 0; q < VOXEL_PIECES; ++q) { piece[q] = at[q]; len[q] = bytes[q]; }
}
"""

WRAPPER = COMMON + r"""
extern "C" int w_measure(const int64_t *off, int n, int any_start, int64_t *out) {
    RaggedShape s = {-7, -7, -7};
    const int rc = ragged_measure(off, n, any_start, &s);
    out[0] = s.total; out[1] = s.largest; out[2] = s.smallest;
    return rc;
}
// offsets of the pieces from `base` (0: the sizing pass, every piece must be null: returns -1 if one is not); returns the bytes
extern "C" int64_t w_carve(uint64_t base, int k, const int64_t *counts, const int *elem, int64_t slack, int64_t *offs) {
    Carver cv((void *)(uintptr_t)base);
    char *piece[64];
    layout(cv, k, counts, elem, slack, piece);
    for (int q = 0; q < k; ++q) {
        if (!base && piece[q]) return -1;
        offs[q] = base ? (int64_t)((uintptr_t)piece[q] - (uintptr_t)base) : 0;
    }
    return (int64_t)cv.at;
}
extern "C" int64_t w_voxel_plan(int64_t n, int n_clouds, int key_bits, int any_invalid, uint64_t base, int64_t *offs, int64_t *len) {
    VoxelPlan p;
    if (voxel_make_plan(n, n_clouds, key_bits, any_invalid, (void *)(uintptr_t)base, &p)) return -1;
    char *piece[VOXEL_PIECES];
    voxel_pieces(p, piece, len);
    for (int q = 0; q < VOXEL_PIECES; ++q) {
        if (!base && piece[q]) return -2;
        offs[q] = base ? (int64_t)((uintptr_t)piece[q] - (uintptr_t)base) : 0;
    }
    return (int64_t)p.bytes;
}
extern "C" int w_voxel_tile() { return VOXEL_TILE; }
"""

# stand-alone: "O any_start n off[0..n]" prints the measure; "C slack k (count elem)*k" and "V n n_clouds" size the layout,
# allocate exactly that, place it and write every piece to its full length
MAIN = COMMON + r"""
#include <stdio.h>
#include <vector>
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char kind;
    int lines = 0;
    while (fscanf(f, " %c", &kind) == 1) {
        if (kind == 'O') {
            int any_start, n;
            if (fscanf(f, "%d %d", &any_start, &n) != 2) return 3;
            std::vector<int64_t> off((size_t)n + 1);
            for (int64_t &v : off) { long long x; if (fscanf(f, "%lld", &x) != 1) return 3; v = x; }
            RaggedShape s = {0, 0, 0};
            const int rc = ragged_measure(off.data(), n, any_start, &s);
            printf("O %d %lld %lld %lld\n", rc, rc ? 0ll : (long long)s.total, rc ? 0ll : (long long)s.largest, rc ? 0ll : (long long)s.smallest);
        } else if (kind == 'C') {
            long long slack;
            int k;
            if (fscanf(f, "%lld %d", &slack, &k) != 2 || k > 64) return 3;
            std::vector<int64_t> counts(k);
            std::vector<int> elem(k);
            for (int q = 0; q < k; ++q) { long long c; if (fscanf(f, "%lld %d", &c, &elem[q]) != 2) return 3; counts[q] = c; }
            char *piece[64];
            Carver size;
            layout(size, k, counts.data(), elem.data(), slack, piece);
            char *block = (char *)malloc(size.at ? size.at : 1);
            Carver place(block);
            layout(place, k, counts.data(), elem.data(), slack, piece);
            if (place.at != size.at) return 4;
            for (int q = 0; q < k; ++q) memset(piece[q], q + 1, (size_t)(counts[q] * elem[q] + slack));
            for (int q = 0; q < k; ++q)
                for (int64_t b = 0; b < counts[q] * elem[q] + slack; ++b) if (piece[q][b] != (char)(q + 1)) return 5;
            free(block);
            printf("C %lld\n", (long long)size.at);
        } else if (kind == 'V') {
            long long n;
            int n_clouds;
            if (fscanf(f, "%lld %d", &n, &n_clouds) != 2) return 3;
            VoxelPlan p;
            if (voxel_make_plan(n, n_clouds, 40, 1, nullptr, &p)) return 6;
            const size_t bytes = p.bytes;
            char *block = (char *)malloc(bytes ? bytes : 1), *piece[VOXEL_PIECES];
            int64_t len[VOXEL_PIECES];
            if (voxel_make_plan(n, n_clouds, 40, 1, block, &p) || p.bytes != bytes) return 7;
            voxel_pieces(p, piece, len);
            for (int q = 0; q < VOXEL_PIECES; ++q) memset(piece[q], q + 1, (size_t)len[q]);
            for (int q = 0; q < VOXEL_PIECES; ++q)
                for (int64_t b = 0; b < len[q]; ++b) if (piece[q][b] != (char)(q + 1)) return 8;
            free(block);
            printf("V %lld\n", (long long)bytes);
        } else return 9;
        ++lines;
    }
    fclose(f);
    printf("ragged ok: %d\n", lines);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ragged")
    (tmp / "ragged_host.cpp").write_text(WRAPPER)
    so = tmp / "ragged_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "ragged_host.cpp"), "-o", str(so)],
                   check=True)
    lib = ctypes.CDLL(str(so))
    lib.w_measure.argtypes = [LP, ctypes.c_int, ctypes.c_int, LP]
    lib.w_carve.argtypes = [ctypes.c_uint64, ctypes.c_int, LP, ctypes.POINTER(ctypes.c_int), ctypes.c_int64, LP]
    lib.w_carve.restype = ctypes.c_int64
    lib.w_voxel_plan.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, LP, LP]
    lib.w_voxel_plan.restype = ctypes.c_int64
    return lib


# ---- the offsets rule ---------------------------------------------------------------------------------------------------
OFFSETS = [[0], [0, 0], [0, 5], [0, 3, 3, 7], [1, 3, 5], [-1, 3], [0, 5, 3], [0, 4, 4, 2], [0, 2 ** 31, 2 ** 40], [7], [3, 3, 2 ** 33]]


def rule(off, any_start):
    """The rule in numpy: the start, no decrease, then (total, largest, smallest)."""
    off = np.asarray(off, dtype=np.int64)
    if off[0] < 0 if any_start else off[0] != 0:
        return E_START
    if (np.diff(off) < 0).any():
        return E_DECREASE
    return OK, int(off[-1]), int(np.diff(off).max(initial=0)), int(np.diff(off).min()) if len(off) > 1 else 0


def measure(lib, off, any_start):
    a = np.asarray(off, dtype=np.int64)
    out = np.zeros(3, dtype=np.int64)
    rc = lib.w_measure(a.ctypes.data_as(LP), len(a) - 1, any_start, out.ctypes.data_as(LP))
    return rc if rc else (rc, int(out[0]), int(out[1]), int(out[2]))


@pytest.mark.parametrize("any_start", [0, 1], ids=["start=0", "start>=0"])
@pytest.mark.parametrize("off", OFFSETS, ids=[",".join(map(str, o)) for o in OFFSETS])
def test_offsets_rule(lib, off, any_start):
    assert measure(lib, off, any_start) == rule(off, any_start)


def test_offsets_rule_names_the_cases(lib):
    """The statement above agrees with the C code; this is what it says of the cases by name."""
    assert measure(lib, [0], 0) == (OK, 0, 0, 0)
    assert measure(lib, [0, 0], 0) == (OK, 0, 0, 0) and measure(lib, [0, 5], 0) == (OK, 5, 5, 5)
    assert measure(lib, [0, 3, 3, 7], 0) == (OK, 7, 4, 0)
    assert measure(lib, [1, 3, 5], 0) == E_START and measure(lib, [1, 3, 5], 1) == (OK, 5, 2, 2)
    assert measure(lib, [-1, 3], 0) == E_START and measure(lib, [-1, 3], 1) == E_START
    assert measure(lib, [0, 5, 3], 0) == E_DECREASE and measure(lib, [0, 4, 4, 2], 1) == E_DECREASE
    assert measure(lib, [0, 2 ** 31, 2 ** 40], 0) == (OK, 2 ** 40, 2 ** 40 - 2 ** 31, 2 ** 31)      # no 32-bit arithmetic


# ---- the carver ---------------------------------------------------------------------------------------------------------
LAYOUTS = [([0, 1, 255, 256, 257], [1] * 5), ([0, 1, 255, 256, 257], [4] * 5), ([257, 0, 31, 32, 33, 64, 1], [8, 8, 8, 8, 8, 2, 2]),
           ([0], [8]), ([0, 0, 0], [4, 2, 1]), ([2 ** 33, 3], [8, 4])]
BASE = 0x7f0000000000                                           # an address that is never dereferenced


def carve(lib, base, counts, elem, slack):
    c, e = np.asarray(counts, dtype=np.int64), np.asarray(elem, dtype=np.int32)
    offs = np.zeros(len(c), dtype=np.int64)
    total = lib.w_carve(base, len(c), c.ctypes.data_as(LP), e.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), slack, offs.ctypes.data_as(LP))
    return int(total), offs


def check_pieces(offs, lens, total):
    """Every piece on a multiple of 256, long enough, inside the block and clear of every other piece."""
    assert all(o % 256 == 0 for o in offs)
    spans = sorted(zip(offs, lens))
    for (o, n), (o_next, _) in zip(spans, spans[1:] + [(total, 0)]):
        assert o + n <= o_next, (spans, total)


@pytest.mark.parametrize("slack", [0, 8, 256, 512])
@pytest.mark.parametrize("counts,elem", LAYOUTS)
def test_carver(lib, counts, elem, slack):
    sized, _ = carve(lib, 0, counts, elem, slack)               # -1: a piece of the sizing pass was not null
    placed, offs = carve(lib, BASE, counts, elem, slack)
    assert sized == placed >= 0 and sized % 256 == 0
    lens = [c * e + slack for c, e in zip(counts, elem)]
    check_pieces(offs.tolist(), lens, placed)
    assert placed == sum((n + 255) // 256 * 256 for n in lens)  # and no more than the pieces rounded up


# ---- the voxel plan -----------------------------------------------------------------------------------------------------
def test_voxel_plan_covers_its_pieces(lib):
    T = lib.w_voxel_tile()
    for n in (0, 1, T, T + 1):
        for n_clouds in (1, 300):
            offs, lens = np.zeros(13, dtype=np.int64), np.zeros(13, dtype=np.int64)
            sized = lib.w_voxel_plan(n, n_clouds, 40, 1, 0, offs.ctypes.data_as(LP), lens.ctypes.data_as(LP))
            placed = lib.w_voxel_plan(n, n_clouds, 40, 1, BASE, offs.ctypes.data_as(LP), lens.ctypes.data_as(LP))
            assert sized == placed >= 256
            assert lens[0] == 8 * n and lens[5] == n and lens[9] == 1024 * ((n + T - 1) // T) and lens[12] == 4
            check_pieces(offs.tolist(), lens.tolist(), placed)
    assert lib.w_voxel_plan(-1, 1, 40, 1, 0, offs.ctypes.data_as(LP), lens.ctypes.data_as(LP)) == -1


# ---- the same under sanitizers ------------------------------------------------------------------------------------------
def test_ragged_under_sanitizers(tmp_path, lib):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined, run once: it allocates exactly what
    the sizing pass asks for and writes every placed piece to its full length.  Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "ragged_main.cpp").write_text(MAIN)
    exe = tmp_path / "ragged_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "ragged_main.cpp"), "-o", str(exe)]
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    T = lib.w_voxel_tile()
    lines, want = [], []
    for off in OFFSETS:
        for any_start in (0, 1):
            lines.append("O %d %d %s" % (any_start, len(off) - 1, " ".join(map(str, off))))
            w = rule(off, any_start)
            want.append("O %d %d %d %d" % (w if isinstance(w, tuple) else (w, 0, 0, 0)))
    for counts, elem in LAYOUTS[:-1]:                           # all but the 64 GiB one
        for slack in (0, 8, 512):
            lines.append("C %d %d %s" % (slack, len(counts), " ".join("%d %d" % ce for ce in zip(counts, elem))))
            want.append("C %d" % sum((c * e + slack + 255) // 256 * 256 for c, e in zip(counts, elem)))
    for n in (0, 1, T, T + 1):
        lines.append("V %d 3" % n)
        want.append("V %d" % lib.w_voxel_plan(n, 3, 40, 1, 0, (ctypes.c_int64 * 13)(), (ctypes.c_int64 * 13)()))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines() == want + ["ragged ok: %d" % len(lines)]
