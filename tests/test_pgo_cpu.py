"""CPU: the pose-graph back end's host pieces and its float64 restatement (tests/pgo_reference.py).

  * csrc/pose.h compiled for the host against the restatement and against central differences
  * csrc/pgo_plan.h compiled for the host: junctions, segments, determinism; the same code once more as a stand-alone
    program under -fsanitize=address,undefined (never loaded into Python)
  * the elimination the kernels perform (segment recurrence, junction system, back substitution), walked in numpy over
    the plan's own index lists, against spsolve
  * the restatement as an optimiser on the planted scene; the g2o round trip
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.sparse.linalg import spsolve

import pgo_reference as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int32)

POSE_WRAPPER = r"""
#define __host__
#define __device__
#include "pose.h"
extern "C" void w_exp(const double *xi, double *T) { double R[9], t[3]; se3_exp(xi, R, t); pose_store(R, t, T); }
extern "C" void w_log(const double *T, double *xi) { double R[9], t[3]; pose_load(T, R, t); se3_log(R, t, xi); }
extern "C" void w_inv(const double *T, double *O) { double R[9], t[3], Ri[9], ti[3]; pose_load(T, R, t); se3_inv(R, t, Ri, ti); pose_store(Ri, ti, O); }
extern "C" void w_adjoint(const double *T, double *A) { double R[9], t[3]; pose_load(T, R, t); se3_adjoint(R, t, A); }
extern "C" void w_jr_inv(const double *xi, double *J) { se3_jr_inv(xi, J); }
extern "C" void w_between(const double *Ti, const double *Tj, const double *Z, int has_i, double *e, double *Ai, double *Aj) {
    pgo_between_residual(has_i ? Ti : nullptr, Tj, Z, e, has_i ? Ai : nullptr, Aj);
}
extern "C" double w_series_theta() { return POSE_SERIES_THETA; }
"""

PLAN_FIELDS = ("pa", "pb", "pair_ptr", "pair_fac", "pose_ptr", "pose_fac", "adj_ptr", "adj_nbr", "adj_pair", "jl", "jidx", "seg_ptr",
               "seg_a", "seg_b", "seg_first", "slot_pose", "slot_link", "pose_slot", "jj_pair", "tgt_r", "tgt_c", "tgt_ptr", "tgt_ent")
PLAN_WRAPPER = r"""
#include "pgo_plan.h"
static PgoPlan g_plan;
static const std::vector<int32_t> *field(int k) {
    const std::vector<int32_t> *f[] = {%s};
    return f[k];
}
extern "C" int w_plan(long long n, long long nf, const int32_t *ei, const int32_t *ej, long long prior) { return pgo_make_plan(n, nf, ei, ej, prior, &g_plan); }
extern "C" long long w_size(int k) { return (long long)field(k)->size(); }
extern "C" void w_copy(int k, int32_t *out) { for (size_t q = 0; q < field(k)->size(); ++q) out[q] = (*field(k))[q]; }
extern "C" long long w_cut() { return g_plan.n_cut; }
extern "C" int w_seg_max() { return PGO_SEG_MAX; }
extern "C" int w_max_junctions() { return PGO_MAX_JUNCTIONS; }
""" % ", ".join("&g_plan." + f for f in PLAN_FIELDS)

# stand-alone: reads "n nf prior" then nf edge lines per graph from the file named on the command line
PLAN_MAIN = r"""
#include <stdio.h>
#include "pgo_plan.h"
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long long n, nf, prior;
    int graphs = 0;
    while (fscanf(f, "%lld %lld %lld", &n, &nf, &prior) == 3) {
        std::vector<int32_t> ei(nf), ej(nf);
        for (long long k = 0; k < nf; ++k) { int a, b; if (fscanf(f, "%d %d", &a, &b) != 2) return 3; ei[k] = a; ej[k] = b; }
        PgoPlan p, q;
        const int rc = pgo_make_plan(n, nf, ei.data(), ej.data(), prior, &p);
        if (rc != pgo_make_plan(n, nf, ei.data(), ej.data(), prior, &q)) return 4;
        if (rc == 0) {
            std::vector<int> seen(n, 0);
            for (int32_t v : p.jl) ++seen[v];
            for (int32_t v : p.slot_pose) ++seen[v];
            for (long long v = 0; v < n; ++v) if (seen[v] != 1) return 5;
            if (p.slot_pose != q.slot_pose || p.jl != q.jl || p.tgt_ent != q.tgt_ent) return 6;
        }
        printf("graph %d: rc %d junctions %lld segments %lld\n", graphs, rc, (long long)p.J(), (long long)p.S());
        ++graphs;
    }
    fclose(f);
    printf("plans ok: %d\n", graphs);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def pose(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pose")
    (tmp / "pose_host.cpp").write_text(POSE_WRAPPER)
    so = tmp / "pose_host.so"
    subprocess.run([_cxx(), "-O2", "-shared", "-fPIC", "-I", CSRC, str(tmp / "pose_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.w_series_theta.restype = ctypes.c_double

    class Pose:
        @staticmethod
        def call(fn, out_shape, *arrays):
            out = np.zeros(out_shape)
            args = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
            getattr(lib, fn)(*[a.ctypes.data_as(DP) for a in args], out.ctypes.data_as(DP))
            return out
        exp = staticmethod(lambda xi: Pose.call("w_exp", (4, 4), xi))
        log = staticmethod(lambda T: Pose.call("w_log", (6,), T))
        inv = staticmethod(lambda T: Pose.call("w_inv", (4, 4), T))
        adjoint = staticmethod(lambda T: Pose.call("w_adjoint", (6, 6), T))
        jr_inv = staticmethod(lambda xi: Pose.call("w_jr_inv", (6, 6), xi))

        @staticmethod
        def between(Ti, Tj, Z):
            e, Ai, Aj = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
            a = [np.ascontiguousarray(x, dtype=np.float64) for x in (Tj if Ti is None else Ti, Tj, Z)]
            lib.w_between(a[0].ctypes.data_as(DP), a[1].ctypes.data_as(DP), a[2].ctypes.data_as(DP), 0 if Ti is None else 1,
                          e.ctypes.data_as(DP), Ai.ctypes.data_as(DP), Aj.ctypes.data_as(DP))
            return e, (None if Ti is None else Ai), Aj
        series_theta = lib.w_series_theta()
    return Pose


class Plan:
    def __init__(self, lib, n, ei, ej, prior):
        ei, ej = np.ascontiguousarray(ei, dtype=np.int32), np.ascontiguousarray(ej, dtype=np.int32)
        self.n, self.nf, self.ei, self.ej, self.prior = n, len(ei), ei, ej, prior
        self.rc = lib.w_plan(n, len(ei), ei.ctypes.data_as(IP), ej.ctypes.data_as(IP), prior)
        for k, name in enumerate(PLAN_FIELDS):
            out = np.zeros(lib.w_size(k), dtype=np.int32)
            lib.w_copy(k, out.ctypes.data_as(IP))
            setattr(self, name, out)
        self.n_cut = lib.w_cut()

    def interiors(self):
        return [list(self.slot_pose[self.seg_ptr[s]:self.seg_ptr[s + 1]]) for s in range(len(self.seg_a))]


@pytest.fixture(scope="module")
def planlib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgo_plan")
    (tmp / "plan_host.cpp").write_text(PLAN_WRAPPER)
    so = tmp / "plan_host.so"
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(tmp / "plan_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.w_plan.argtypes = [ctypes.c_longlong, ctypes.c_longlong, IP, IP, ctypes.c_longlong]
    lib.w_size.restype = ctypes.c_longlong
    lib.w_cut.restype = ctypes.c_longlong
    return lib


# ---- pose.h ------------------------------------------------------------------------------------------------------------------------
THETAS = (0.0, 1e-10, 1e-5, 1.0, np.pi - 1e-6)
EPS = np.finfo(np.float64).eps
# the C code and the restatement evaluate the same expressions; they may differ by the rounding of sin / cos / atan2 and by
# fused multiply-adds, a few ulp of the largest term of each entry
ULP_MARGIN = 64.0


def tangent_cases():
    rng = np.random.default_rng(11)
    out = []
    for th in THETAS + (ref.SERIES_THETA * (1 - 1e-9), ref.SERIES_THETA * (1 + 1e-9), 3.0):
        for scale in (0.0, 1.0, 2.0 ** 20):
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            out.append(np.concatenate([th * axis, scale * rng.uniform(-1, 1, 3)]))
    return out


def test_pose_matches_the_restatement(pose):
    assert pose.series_theta == ref.SERIES_THETA
    for xi in tangent_cases():
        mag = max(1.0, float(np.abs(xi[3:]).max()))
        T = pose.exp(xi)
        assert np.abs(T - ref.exp(xi)).max() <= ULP_MARGIN * EPS * mag, xi
        assert np.abs(pose.jr_inv(xi) - ref.jr_inv(xi)).max() <= ULP_MARGIN * EPS * mag, xi
        assert np.abs(pose.adjoint(T) - ref.adjoint(T)).max() <= ULP_MARGIN * EPS * mag
        assert np.abs(pose.inv(T) - ref.inv(T)).max() <= ULP_MARGIN * EPS * mag
        # Log of the same matrix: the rotation part is conditioned like 1 (quaternion form), the translation like |t|
        assert np.abs(pose.log(T) - ref.log(T)).max() <= ULP_MARGIN * EPS * mag, xi


def test_exp_log_round_trip(pose):
    """Log(Exp(xi)) == xi.  The rotation loses nothing to the angle (pi - 1e-6 included); v carries the rounding of
    t = V v times |V^-1| <= 1 + theta / 2 + d theta^2 < 4 on [0, pi]."""
    for xi in tangent_cases():
        back = pose.log(pose.exp(xi))
        mag = max(1.0, float(np.abs(xi[3:]).max()))
        assert np.abs(back[:3] - xi[:3]).max() <= ULP_MARGIN * EPS * np.pi, xi
        assert np.abs(back[3:] - xi[3:]).max() <= 4 * ULP_MARGIN * EPS * mag, xi
        assert np.abs(ref.log(ref.exp(xi)) - xi).max() <= 4 * ULP_MARGIN * EPS * mag


def central_diff(f, x0, h):
    cols = []
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        cols.append((f(d) - f(-d)) / (2 * h))
    return np.stack(cols, axis=1)


FD_H = 1e-5
FD_MARGIN = 4.0      # the C code may miss central differences by this many times what the restatement itself misses them by


def test_jacobians_against_central_differences(pose):
    """Jr_inv: Log(Exp(xi) Exp(d)) = xi + Jr_inv(xi) d.  Between: e(Ti Exp(di), Tj Exp(dj)) = e + Ai di + Aj dj.
    Central differences with h = 1e-5 carry h^2 truncation and eps / h rounding, about 1e-10 relative; the bound is what the
    restatement achieves against the same differences, times FD_MARGIN, plus that floor."""
    rng = np.random.default_rng(5)
    for th in (0.0, 1e-5, 0.3, 1.0, 2.5):
        axis = rng.standard_normal(3)
        xi = np.concatenate([th * axis / np.linalg.norm(axis), rng.uniform(-3, 3, 3)])
        num = central_diff(lambda d: ref.log(ref.exp(xi) @ ref.exp(d)), xi, FD_H)
        floor = 1e-9 * max(1.0, np.abs(num).max())
        err_ref = np.abs(ref.jr_inv(xi) - num).max()
        assert err_ref <= 10 * floor, (th, err_ref)
        assert np.abs(pose.jr_inv(xi) - num).max() <= FD_MARGIN * err_ref + floor, th
    for k in range(6):
        Ti, Tj = (ref.exp(np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-10, 10, 3)])) for _ in range(2))
        Z = ref.inv(Ti) @ Tj @ ref.exp(rng.standard_normal(6) * (0.0 if k == 0 else 0.5))
        e, Ai, Aj = pose.between(Ti, Tj, Z)
        re, rAi, rAj = ref.between(Ti, Tj, Z)
        num_i = central_diff(lambda d: ref.between(Ti @ ref.exp(d), Tj, Z, jac=False)[0], None, FD_H)
        num_j = central_diff(lambda d: ref.between(Ti, Tj @ ref.exp(d), Z, jac=False)[0], None, FD_H)
        for got, want, num in ((Ai, rAi, num_i), (Aj, rAj, num_j)):
            floor = 1e-9 * max(1.0, np.abs(num).max())
            err_ref = np.abs(want - num).max()
            assert err_ref <= 10 * floor, (k, err_ref)
            assert np.abs(got - num).max() <= FD_MARGIN * err_ref + floor
        assert np.abs(e - re).max() <= ULP_MARGIN * EPS * 32
        pe, pAi, pAj = pose.between(None, Tj, Z)
        assert pAi is None and np.abs(pAj - ref.between(None, Tj, Z)[2]).max() <= ULP_MARGIN * EPS * 32


# ---- pgo_plan.h ----------------------------------------------------------------------------------------------------------------------
def check_plan(p):
    """What holds of every plan."""
    assert p.rc == 0
    nbrs = [set() for _ in range(p.n)]
    for i, j in zip(p.ei, p.ej):
        nbrs[i].add(int(j)); nbrs[j].add(int(i))
    isj = p.jidx >= 0
    assert isj[p.prior]
    for v in range(p.n):
        if len(nbrs[v]) != 2:
            assert isj[v], "a pose without exactly two neighbours is a junction"
        assert sorted(nbrs[v]) == list(p.adj_nbr[p.adj_ptr[v]:p.adj_ptr[v + 1]])
    # every pose exactly once: a junction or one interior slot
    count = np.zeros(p.n, dtype=int)
    np.add.at(count, p.jl, 1)
    np.add.at(count, p.slot_pose, 1)
    assert np.array_equal(count, np.ones(p.n, dtype=int))
    assert np.array_equal(p.jl, np.flatnonzero(isj)) and np.array_equal(p.jidx[p.jl], np.arange(len(p.jl)))
    for s, path in enumerate(p.interiors()):
        assert 1 <= len(path) <= SEG_MAX
        a, b = p.jl[p.seg_a[s]], p.jl[p.seg_b[s]]
        walk = [a] + path + [b]
        for u, v in zip(walk[:-1], walk[1:]):
            assert v in nbrs[u]
        for q, v in enumerate(path):
            assert p.pose_slot[v] == p.seg_ptr[s] + q and not isj[v]
            link = p.slot_link[p.seg_ptr[s] + q]
            assert {int(p.pa[link >> 1]), int(p.pb[link >> 1])} == {v, walk[q + 2]} and (link & 1) == (v > walk[q + 2])
        first = p.seg_first[s]
        assert {int(p.pa[first >> 1]), int(p.pb[first >> 1])} == {path[0], a} and (first & 1) == (path[0] > a)
    pairs = sorted({(min(i, j), max(i, j)) for i, j in zip(p.ei.tolist(), p.ej.tolist())})
    assert pairs == list(zip(p.pa.tolist(), p.pb.tolist()))
    for q, (a, b) in enumerate(pairs):
        facs = p.pair_fac[p.pair_ptr[q]:p.pair_ptr[q + 1]]
        want = [k for k in range(p.nf) if {int(p.ei[k]), int(p.ej[k])} == {a, b}]
        assert [f >> 1 for f in facs] == want and all((f & 1) == (p.ei[f >> 1] > p.ej[f >> 1]) for f in facs)
    for v in range(p.n):
        facs = p.pose_fac[p.pose_ptr[v]:p.pose_ptr[v + 1]]
        want = [k for k in range(p.nf) if v in (p.ei[k], p.ej[k])] + ([p.nf] if v == p.prior else [])
        assert [f >> 2 for f in facs] == want
    assert sorted(p.jj_pair.tolist()) == [q for q, (a, b) in enumerate(pairs) if isj[a] and isj[b]]


SEG_MAX = 64


def test_plan_constants(planlib):
    assert planlib.w_seg_max() == SEG_MAX


@pytest.mark.parametrize("name", sorted(ref.plan_graphs(SEG_MAX)))
def test_plan_structure(planlib, name):
    n, ei, ej, prior = ref.plan_graphs(SEG_MAX)[name]
    p = Plan(planlib, n, ei, ej, prior)
    check_plan(p)
    again = Plan(planlib, n, ei, ej, prior)
    for f in PLAN_FIELDS:
        assert np.array_equal(getattr(p, f), getattr(again, f)), "the plan is a pure function of its input"
    J, S = len(p.jl), len(p.seg_a)
    if name == "chain2":
        assert (J, S) == (2, 0) and list(p.jj_pair) == [0]
    if name == "ring":
        assert list(p.jl) == [3] and p.interiors() == [[2, 1, 0, 6, 5, 4]] and p.seg_a[0] == p.seg_b[0] == 0
    if name == "ring-no-prior-junction":
        assert list(p.jl) == [0, 5]                 # 0: prior and degree 3; 5: degree 3; both rings hang on a junction
    if name == "star":
        assert (J, S) == (9, 0)
    if name == "complete8":
        assert (J, S) == (8, 0) and len(p.jj_pair) == 28
    if name == "adjacent-junctions":
        assert {0, 3, 4, 5, 7, 8} == set(p.jl.tolist()) and [6] in p.interiors()
    if name == "dangling":
        assert {0, 2, 5, 7} == set(p.jl.tolist())
    if name == "parallel":
        assert len(p.pa) == 6 and list(p.pair_fac[p.pair_ptr[3]:p.pair_ptr[4]]) == [2 * 2, 5 * 2, 6 * 2 + 1]   # pair (2, 3)
    if name == "segment-%d" % (SEG_MAX - 1) or name == "segment-%d" % SEG_MAX:
        assert p.n_cut == 0 and S == 1
    if name == "segment-%d" % (SEG_MAX + 1):
        assert p.n_cut == 1 and S == 1 and len(p.interiors()[0]) == SEG_MAX      # the promoted pose is next to the end junction
    if name == "segment-%d" % (2 * SEG_MAX + 2):
        assert p.n_cut == 2 and sorted(len(x) for x in p.interiors()) == [SEG_MAX, SEG_MAX]
    if name == "two-components":
        assert {0, 4, 8, 10} == set(p.jl.tolist())          # the ring 5-6-7-8 hangs on 8; nothing ties it to the prior
    kinds = p.tgt_ent & 3
    lists = np.diff(p.tgt_ptr)
    if name == "complete16":
        assert (J, S) == (16, 0) and len(p.jj_pair) == 120                       # N = 96: two exact panels of the dense factor
    if name == "complete17":
        assert (J, S) == (17, 0) and len(p.jj_pair) == 136                       # N = 102: a 6-row remainder after them
    if name == "grid7x8":
        assert (J, S) == (52, 4) and sorted(p.interiors()) == [[0], [7], [48], [55]]         # N = 312; the corners are segments
        assert len(p.jj_pair) == 97 - 8                                           # every lattice edge that touches no corner
    if name == "subdivided9":
        assert p.n == 45 and (J, S) == (9, 24) and list(p.jl) == list(range(9)) and len(p.jj_pair) == 12
        # a segment is walked from its lower junction, so between two junctions it enters the block (b, a) as BA whichever way
        # its edges are listed (AB is the kind of a ring that starts and ends on one junction, as in "ring"); the listing order
        # reaches the plan as the reversed bit of the pair's factors, and both values occur
        off = np.concatenate([kinds[p.tgt_ptr[T]:p.tgt_ptr[T + 1]] for T in range(len(p.tgt_r)) if p.tgt_r[T] != p.tgt_c[T]])
        assert len(off) == 24 and np.all(off == 3), "PGO_KIND_BA"
        assert set((p.pair_fac & 1).tolist()) == {0, 1} and set((p.slot_link & 1).tolist()) == {0, 1}
        # a junction is the first end of some segments and the last of others: AA and BB in one diagonal list
        assert any({0, 1} <= set(kinds[p.tgt_ptr[T]:p.tgt_ptr[T + 1]].tolist()) for T in range(len(p.tgt_r)))
    if name == "bundle":
        assert p.n == 13 and (J, S) == (2, 4) and sorted(len(x) for x in p.interiors()) == [1, 2, 3, 5]
        assert list(zip(p.tgt_r.tolist(), p.tgt_c.tolist())) == [(0, 0), (1, 0), (1, 1)] and list(lists) == [4, 4, 4]
        assert list(p.jj_pair) == [0] and list(p.pair_fac[p.pair_ptr[0]:p.pair_ptr[1]]) == [0, 3]   # (0, 1) and its reversed twin
        assert set((p.pair_fac & 1).tolist()) == {0, 1}


def test_plan_promotes_one_pose_of_a_cycle_without_junction(planlib):
    """A ring that holds neither the prior nor a branching pose: its lowest pose becomes the junction."""
    n = 9
    ed = [(0, 1), (1, 2)] + [(k, k + 1) for k in range(3, 8)] + [(8, 3)]
    p = Plan(planlib, n, [e[0] for e in ed], [e[1] for e in ed], 1)
    check_plan(p)
    assert set(p.jl.tolist()) == {0, 1, 2, 3} and [4, 5, 6, 7, 8] in p.interiors()


def test_plan_argument_errors_and_cap(planlib):
    assert Plan(planlib, 3, [0, 1], [1, 1], 0).rc == -1                      # i == j
    assert Plan(planlib, 3, [0, 1], [1, 3], 0).rc == -1                      # index out of range
    assert Plan(planlib, 3, [0, 1], [1, 2], 3).rc == -1                      # prior outside the poses
    cap = planlib.w_max_junctions()
    star = Plan(planlib, cap + 1, np.zeros(cap, dtype=np.int32), np.arange(1, cap + 1, dtype=np.int32), 0)
    assert star.rc == -2
    assert Plan(planlib, cap, np.zeros(cap - 1, dtype=np.int32), np.arange(1, cap, dtype=np.int32), 0).rc == 0


def test_plan_under_sanitizers(tmp_path):
    """The same header in a stand-alone program with its own main, built with -fsanitize=address,undefined, run once over
    the test graphs (and the three argument errors).  Not loaded into Python."""
    cxx = _cxx()
    (tmp_path / "plan_main.cpp").write_text(PLAN_MAIN)
    exe = tmp_path / "plan_main"
    base = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            str(tmp_path / "plan_main.cpp"), "-o", str(exe)]
    # the sanitizer runtimes linked into the program itself where the compiler can (gcc's spelling)
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    graphs = list(ref.plan_graphs(SEG_MAX).values())
    graphs += [(3, np.array([0, 1]), np.array([1, 1]), 0), (3, np.array([0, 1]), np.array([1, 3]), 0), (3, np.array([0]), np.array([1]), 5)]
    with open(tmp_path / "graphs.txt", "w") as f:
        for n, ei, ej, prior in graphs:
            f.write("%d %d %d\n" % (n, len(ei), prior))
            for a, b in zip(ei, ej):
                f.write("%d %d\n" % (a, b))
    r = subprocess.run([str(exe), str(tmp_path / "graphs.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "plans ok: %d" % len(graphs) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- the elimination, in numpy over the plan's lists -------------------------------------------------------------------------------
def block(Hoff, link):
    B = Hoff[link >> 1]
    return B.T if link & 1 else B


def eliminate(p, Hd, g, Hoff, lam):
    """What pgo_segment_kernel, the junction kernels, the dense factor and pgo_backsub_kernel compute, in that order."""
    J, S = len(p.jl), len(p.seg_a)
    Sd, rhs = np.zeros((6 * J, 6 * J)), np.zeros(6 * J)
    Y = np.zeros((len(p.slot_pose), 19, 6))
    con = np.zeros((S, 120))
    for s in range(S):
        s0, m = p.seg_ptr[s], p.seg_ptr[s + 1] - p.seg_ptr[s]
        Ca = block(Hoff, p.seg_first[s])
        Uprev, Wprev, zprev = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((6, 13))
        for k in range(m):
            v = p.slot_pose[s0 + k]
            L = Hd[v] + lam * np.identity(6) - Uprev.T @ Wprev
            U = block(Hoff, p.slot_link[s0 + k])
            B = np.zeros((6, 19))
            B[:, 0] = -g[v]
            if k == 0:
                B[:, 1:7] = Ca
            if k == m - 1:
                B[:, 7:13] = U
            else:
                B[:, 13:19] = U
            B[:, :13] -= Uprev.T @ zprev
            Z = np.linalg.solve(L, B)
            Y[s0 + k] = Z.T
            Uprev, Wprev, zprev = U, Z[:, 13:19], Z[:, :13]
        y = Y[s0 + m - 1, :13].T
        for k in range(m - 2, -1, -1):
            y = Y[s0 + k, :13].T - Y[s0 + k, 13:19].T @ y
            Y[s0 + k, :13] = y.T
        Y1, Ym, Cb = Y[s0], Y[s0 + m - 1], Uprev
        con[s, 0:36] = (Ca.T @ Y1[1:7].T).ravel()
        con[s, 36:72] = (Ca.T @ Y1[7:13].T).ravel()
        con[s, 72:108] = (Cb.T @ Ym[7:13].T).ravel()
        con[s, 108:114] = Ca.T @ Y1[0]
        con[s, 114:120] = Cb.T @ Ym[0]
    for j, v in enumerate(p.jl):
        Sd[6 * j:6 * j + 6, 6 * j:6 * j + 6] = Hd[v] + lam * np.identity(6)
        rhs[6 * j:6 * j + 6] = -g[v]
    for q in p.jj_pair:
        ja, jb = p.jidx[p.pa[q]], p.jidx[p.pb[q]]
        Sd[6 * jb:6 * jb + 6, 6 * ja:6 * ja + 6] = Hoff[q].T
    for T in range(len(p.tgt_r)):
        r, c = p.tgt_r[T], p.tgt_c[T]
        assert r >= c
        for ent in p.tgt_ent[p.tgt_ptr[T]:p.tgt_ptr[T + 1]]:
            s, kind = ent >> 2, ent & 3
            sub = {0: con[s, 0:36], 1: con[s, 72:108], 2: con[s, 36:72], 3: con[s, 36:72]}[kind].reshape(6, 6)
            Sd[6 * r:6 * r + 6, 6 * c:6 * c + 6] -= sub.T if kind == 3 else sub
            if kind == 0:
                rhs[6 * r:6 * r + 6] -= con[s, 108:114]
            if kind == 1:
                rhs[6 * r:6 * r + 6] -= con[s, 114:120]
    full = np.tril(Sd) + np.tril(Sd, -1).T                       # only the lower triangle is read
    xj = np.linalg.solve(full, rhs)
    delta = np.zeros((p.n, 6))
    for j, v in enumerate(p.jl):
        delta[v] = xj[6 * j:6 * j + 6]
    for s in range(S):
        xa, xb = xj[6 * p.seg_a[s]:6 * p.seg_a[s] + 6], xj[6 * p.seg_b[s]:6 * p.seg_b[s] + 6]
        for slot in range(p.seg_ptr[s], p.seg_ptr[s + 1]):
            delta[p.slot_pose[slot]] = Y[slot, 0] - Y[slot, 1:7].T @ xa - Y[slot, 7:13].T @ xb
    return delta


@pytest.mark.parametrize("name", sorted(ref.plan_graphs(SEG_MAX)))
def test_plan_lists_carry_the_elimination(planlib, name):
    n, ei, ej, prior = ref.plan_graphs(SEG_MAX)[name]
    p = Plan(planlib, n, ei, ej, prior)
    poses, meas, sig = ref.random_graph_values(n, ei, ej, 3)
    gr = ref.Graph(n, ei, ej, meas, sig, prior)
    _, Hd, g, Ho = ref.linearize(gr, poses, np.ones(gr.nf + 1))
    Hoff = np.stack([Ho[(int(a), int(b))] for a, b in zip(p.pa, p.pb)])
    for lam in (1e-5, 1e5):
        A = ref.assemble(n, Hd, Ho, lam)
        want = spsolve(A, -g.ravel())
        got = eliminate(p, Hd, g, Hoff, lam).ravel()
        res = lambda x: np.linalg.norm(A @ x + g.ravel()) / np.linalg.norm(g)
        assert res(got) <= 10 * res(want) + 1e-13, (name, lam, res(got), res(want))


# ---- the integer systems of the GPU's exact tests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,density", [(1, 1.0), (49, 1.0), (102, 0.1), (354, 1.0), (354, 0.1)])
def test_integer_systems_are_exact_in_float64(N, density):
    """The right-looking factor in 48-column panels and the two triangular solves, in float64 with numpy's own summation
    orders, return L and x of ref.integer_system exactly: what tests/test_pgo_gpu.py then asks of the kernels bit for bit."""
    from scipy.linalg import solve_triangular
    L, A, x, b = ref.integer_system(N, 7, density)
    assert np.array_equal(A, A.T) and np.array_equal(np.triu(L, 1), np.zeros_like(L)) and np.abs(b).max() < 2 ** 31
    if N > 100:
        fill = np.count_nonzero(np.tril(L, -1)) / (N * (N - 1) / 2)
        assert (0.07 < fill < 0.13) if density < 1.0 else (0.75 < fill < 0.85)      # a fifth of {-2 .. 2} is 0
    S = A.astype(np.float64)
    for k0 in range(0, N, 48):
        k1 = min(N, k0 + 48)
        S[k0:k1, k0:k1] = np.linalg.cholesky(S[k0:k1, k0:k1])
        if k1 < N:
            S[k1:, k0:k1] = solve_triangular(S[k0:k1, k0:k1], S[k1:, k0:k1].T, lower=True).T
            S[k1:, k1:] -= S[k1:, k0:k1] @ S[k1:, k0:k1].T
    F = np.tril(S)
    assert np.array_equal(F, L.astype(np.float64))
    y = solve_triangular(F, b.astype(np.float64), lower=True)
    assert np.array_equal(solve_triangular(F.T, y, lower=False), x.astype(np.float64))


# ---- the restatement as an optimiser -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    out = {}
    for seed, kw in ((1, {}), (2, {}), (5, dict(n_true=8, n_out=3))):
        sc = ref.planted_scene(seed, **kw)
        out[seed] = (sc, ref.gnc(sc.graph, sc.init, known=sc.known))
    return out


@pytest.mark.parametrize("seed", (1, 2, 5))
def test_restatement_rejects_the_planted_outliers(planted, seed):
    sc, res = planted[seed]
    w = res["weights"]
    assert np.all(w[sc.outliers] == 0.0), w[sc.outliers]
    assert np.all(w[~sc.outliers] == 1.0), w[~sc.outliers]
    assert 1 <= res["rounds"] <= 100
    err = max(np.abs(ref.log(ref.inv(sc.truth[v]) @ res["poses"][v])[3:]).max() for v in range(sc.graph.n))
    # metres, against the noise-free truth: a chain of 30 noisy steps drifts by about 0.1 sqrt(30) = 0.55 m in translation plus
    # 0.01 sqrt(30) rad over a 30 m lever = 1.6 m; gross outliers left in would move poses by several metres
    assert err < 3.0, err


def test_g2o_round_trip(tmp_path):
    from cslam_amd.back_end import pose_graph as pg
    sc = ref.planted_scene(1)
    gr = sc.graph
    values = {(v // 30, v % 30): sc.init[v] for v in range(gr.n)}
    keys = sorted(values)
    edges = [pg.PoseGraphEdge(keys[gr.ei[k]], keys[gr.ej[k]], gr.meas[k], gr.sig[k]) for k in range(gr.nf)]
    path = str(tmp_path / "graph.g2o")
    pg.write_g2o(path, values, edges)
    v2, e2 = pg.read_g2o(path)
    assert sorted(v2) == keys and len(e2) == len(edges)
    for k in keys:
        assert np.abs(v2[k] - values[k]).max() <= 1e-12 * max(1.0, np.abs(values[k]).max())
    for a, b in zip(edges, e2):
        assert (a.key_from, a.key_to) == (b.key_from, b.key_to)
        assert np.abs(a.measurement - b.measurement).max() <= 1e-12 * max(1.0, np.abs(a.measurement).max())
        assert np.allclose(a.noise_std, b.noise_std, rtol=1e-12, atol=0)
    # a full information matrix: only its diagonal is taken
    lines = open(path).read().splitlines()
    k = next(i for i, ln in enumerate(lines) if ln.startswith("EDGE_SE3:QUAT"))
    tok = lines[k].split()
    tok[11] = "123.0"                                               # information (0, 1), off the diagonal
    lines[k] = " ".join(tok)
    open(path, "w").write("\n".join(lines) + "\n")
    _, e3 = pg.read_g2o(path)
    assert np.allclose(e3[0].noise_std, e2[0].noise_std, rtol=1e-15, atol=0)


def test_pose_graph_argument_errors_come_before_any_launch():
    from cslam_amd.back_end import pose_graph as pg
    I = np.identity(4)
    values = {(0, 0): I, (0, 1): I}
    with pytest.raises(KeyError):
        pg.optimize(values, [((0, 0), (0, 7), I, ref.SIGMAS)])
    with pytest.raises(ValueError):
        pg.optimize(values, [((0, 0), (0, 0), I, ref.SIGMAS)])
    with pytest.raises(ValueError):
        pg.optimize(values, [((0, 0), (0, 1), I, np.array([0.01, 0.01, 0.0, 0.1, 0.1, 0.1]))])
    with pytest.raises(ValueError):
        pg.optimize(values, [((0, 0), (0, 1), I, -ref.SIGMAS)])
