"""CPU: the two-view bundle adjustment after PnP.

  * the restatement (tests/vis_ba_reference.py) against the plant: the accuracy condition on the far scene
  * csrc/ba.h compiled by the host C++ compiler into a stand-alone program that runs vis_ba_kernel's schedule (member k on
    thread k mod 256, the shuffle tree per wave, the waves in wave order, thread 0 solving) on heap blocks of exactly the
    kernel's buffer sizes, against the restatement on every case of the GPU test
  * the same program once more under -fsanitize=address,undefined (its own main, never loaded into Python)
  * the argument checks of cslam_amd.front_end.visual_registration's adjusted entry points
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import vis_ba_reference as ba
from conftest import ROOT
from cslam_amd import _lib
from cslam_amd.front_end import visual_registration as vr

CSRC = os.path.join(ROOT, "cslam_amd", "csrc")

# A job is ten int32 (na, nb, K, has_la, has_lb, min_inliers, iterations, rounds, pnp_status, 0), 27 float64 (reproj_error,
# cam_a, cam_b, baselines, T0) and its arrays; the result is T, cost, info, flags, points.  Every LDS array of the kernel is
# a heap block of BA_MAX_CORR entries here, the scratch and the outputs heap blocks of exactly their sizes, so an index
# outside is the sanitizer's to report.
BA_HOST = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __host__
#define __device__
#include "ba.h"

#define BLOCK 256
#define WAVES 4
template <typename T> static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(5); }
    return v;
}
template <typename T> static void wr(FILE *f, const std::vector<T> &v) {
    if (v.size() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(6);
}
// the workgroup's sum of one value per thread: __shfl_down tree per wave (lane 0's result), then the waves in wave order
static double block_sum(const double *v) {
    double w[WAVES];
    for (int wave = 0; wave < WAVES; ++wave) {
        double x[64], y[64];
        for (int l = 0; l < 64; ++l) x[l] = v[64 * wave + l];
        for (int o = 32; o >= 1; o >>= 1) {
            for (int l = 0; l < 64; ++l) y[l] = x[l] + (l + o < 64 ? x[l + o] : x[l]);
            memcpy(x, y, sizeof x);
        }
        w[wave] = x[0];
    }
    double a = w[0];
    for (int k = 1; k < WAVES; ++k) a += w[k];
    return a;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t head[10];
    int jobs = 0;
    const double nan = NAN;
    while (fread(head, 4, 10, in) == 10) {
        const int na = head[0], nb = head[1], K = head[2], min_inliers = head[5], iterations = head[6], rounds = head[7], pnp_status = head[8];
        const std::vector<double> par = rd<double>(in, 27);
        const double thr2 = par[0] * par[0];
        const std::vector<double> kp_a = rd<double>(in, 2 * (size_t)na), pts_a = rd<double>(in, 3 * (size_t)na), kp_b = rd<double>(in, 2 * (size_t)nb),
                                  pts_b = rd<double>(in, 3 * (size_t)nb);
        const std::vector<int32_t> lvl_a = rd<int32_t>(in, head[3] ? na : 0), lvl_b = rd<int32_t>(in, head[4] ? nb : 0);
        const std::vector<int32_t> rows = rd<int32_t>(in, 2 * (size_t)K), flags0 = rd<int32_t>(in, (size_t)K);
        std::vector<double> T(16, nan), cost(2, nan), points(3 * (size_t)K, nan), Y(3 * (size_t)K), Ys(3 * (size_t)K);
        std::vector<int32_t> info(8, -1), flags((size_t)K, -1);
        std::vector<double> sUa(BA_MAX_CORR), sVa(BA_MAX_CORR), sIa(BA_MAX_CORR), sUb(BA_MAX_CORR), sVb(BA_MAX_CORR), sIb(BA_MAX_CORR);
        std::vector<int32_t> s_src(BA_MAX_CORR);
        std::vector<uint8_t> s_la(BA_MAX_CORR), s_lb(BA_MAX_CORR), s_in(BA_MAX_CORR);
        double s_sig[PNP_MAX_LEVEL + 1];
        for (int l = 0; l <= PNP_MAX_LEVEL; ++l) s_sig[l] = pnp_level_sigma2(l);
        const int cap = K, given = K;
        for (int k = 0; k < cap; ++k) flags[k] = flags0[k];
        const bool adjust = pnp_status == 0 && rounds > 0 && iterations > 0;
        int M = 0;
        for (int c0 = 0; c0 < given && adjust; c0 += BLOCK) {
            int n_ok = 0;
            for (int t = 0; t < BLOCK; ++t) {
                const int k = c0 + t;
                bool ok = false;
                double ua = 0, va = 0, ia = 0, ub = 0, vb = 0, ib = 0;
                int la = 0, lb = 0;
                if (k < given && flags0[k] != 0) {
                    const int64_t i = rows[2 * k], j = rows[2 * k + 1];
                    if (i >= 0 && i < na && j >= 0 && j < nb) {
                        ua = kp_a[2 * i]; va = kp_a[2 * i + 1]; ub = kp_b[2 * j]; vb = kp_b[2 * j + 1];
                        const double xa = pts_a[3 * i], ya = pts_a[3 * i + 1];
                        ia = ba_inv_depth(pts_a[3 * i + 2]);
                        ib = ba_inv_depth(pts_b[3 * j + 2]);
                        if (head[3]) la = lvl_a[i];
                        if (head[4]) lb = lvl_b[j];
                        la = la < 0 ? 0 : (la > PNP_MAX_LEVEL ? PNP_MAX_LEVEL : la);
                        lb = lb < 0 ? 0 : (lb > PNP_MAX_LEVEL ? PNP_MAX_LEVEL : lb);
                        ok = pnp_finite(ua) && pnp_finite(va) && pnp_finite(ub) && pnp_finite(vb) && pnp_finite(xa) && pnp_finite(ya) && ia != 0.0;
                    }
                    if (!ok) flags[k] = 0;
                }
                const int at = M + n_ok;
                if (ok && at < BA_MAX_CORR) {
                    sUa[at] = ua; sVa[at] = va; sIa[at] = ia; sUb[at] = ub; sVb[at] = vb; sIb[at] = ib;
                    s_src[at] = k; s_la[at] = (uint8_t)la; s_lb[at] = (uint8_t)lb; s_in[at] = 1;
                }
                n_ok += ok ? 1 : 0;
            }
            M += n_ok;
        }
        if (!adjust || M > BA_MAX_CORR) {
            for (int e = 0; e < 16; ++e) T[e] = par[11 + e];
            if (adjust) for (int k = 0; k < cap; ++k) flags[k] = flags0[k];
            int n0 = 0;
            for (int k = 0; k < K; ++k) n0 += flags0[k] != 0;
            info = {adjust ? 3 : pnp_status, adjust ? M : n0, adjust ? M : n0, 0, 0, 0, pnp_status, 0};
        } else {
            const BaView ca = {par[1], par[2], par[3], par[4], par[1] * par[9]}, cb = {par[5], par[6], par[7], par[8], par[5] * par[10]};
            double R[9], tt[3];
            pose_load(par.data() + 11, R, tt);
            double *Yx = Y.data(), *Yy = Yx + cap, *Yz = Yy + cap, *Sx = Ys.data(), *Sy = Sx + cap, *Sz = Sy + cap;
            for (int k = 0; k < M; ++k) {
                const int64_t i = rows[2 * s_src[k]];
                Yx[k] = pts_a[3 * i]; Yy[k] = pts_a[3 * i + 1]; Yz[k] = pts_a[3 * i + 2];
            }
#define OBS(k) const BaObs o = {sUa[k], sVa[k], sIa[k], sUb[k], sVb[k], sIb[k], 1.0 / s_sig[s_la[k]], 1.0 / s_sig[s_lb[k]]}
            int kept = M, steps = 0, discarded = 0, held = 0;
            double cost_first = 0, cost_last = 0, lane[BLOCK];
            auto total_cost = [&](bool save) {
                for (int t = 0; t < BLOCK; ++t) {
                    double c = 0;
                    for (int k = t; k < M; k += BLOCK)
                        if (s_in[k]) {
                            OBS(k);
                            const double P[3] = {Yx[k], Yy[k], Yz[k]};
                            if (save) { Sx[k] = P[0]; Sy[k] = P[1]; Sz[k] = P[2]; }
                            c += ba_cost(R, tt, ca, cb, o, P);
                        }
                    lane[t] = c;
                }
                return block_sum(lane);
            };
            for (int round = 0; round < rounds; ++round) {
                double R0[9], t0[3];
                memcpy(R0, R, sizeof R0); memcpy(t0, tt, sizeof t0);
                const double cost0 = total_cost(true);
                if (round == 0) cost_first = cost0;
                for (int it = 0; it < iterations; ++it) {
                    static double s[BLOCK][PNP_NSUM];
                    memset(s, 0, sizeof s);
                    for (int t = 0; t < BLOCK; ++t)
                        for (int k = t; k < M; k += BLOCK)
                            if (s_in[k]) {
                                OBS(k);
                                const double P[3] = {Yx[k], Yy[k], Yz[k]};
                                held += ba_accumulate(R, tt, ca, cb, o, P, s[t]) == BA_HELD ? 1 : 0;
                            }
                    double tot[PNP_NSUM], delta[6], Rn[9], tn[3];
                    for (int e = 0; e < PNP_NSUM; ++e) {
                        for (int t = 0; t < BLOCK; ++t) lane[t] = s[t][e];
                        tot[e] = block_sum(lane);
                    }
                    const int stop = ba_pose_step(tot, R, tt, delta, Rn, tn);
                    if (stop != 1) {
                        for (int k = 0; k < M; ++k)
                            if (s_in[k]) {
                                OBS(k);
                                double P[3] = {Yx[k], Yy[k], Yz[k]};
                                if (ba_back_substitute(R, tt, ca, cb, o, delta, P) == BA_FREE) { Yx[k] = P[0]; Yy[k] = P[1]; Yz[k] = P[2]; }
                            }
                        memcpy(R, Rn, sizeof R); memcpy(tt, tn, sizeof tt);
                        ++steps;
                    }
                    if (stop) break;
                }
                double cost1 = total_cost(false);
                if (ba_round_rejected(cost0, cost1)) {
                    memcpy(R, R0, sizeof R); memcpy(tt, t0, sizeof tt);
                    for (int k = 0; k < M; ++k)
                        if (s_in[k]) { Yx[k] = Sx[k]; Yy[k] = Sy[k]; Yz[k] = Sz[k]; }
                    ++discarded;
                    cost1 = cost0;
                }
                cost_last = cost1;
                kept = 0;
                for (int k = 0; k < M; ++k)
                    if (s_in[k]) {
                        OBS(k);
                        const double P[3] = {Yx[k], Yy[k], Yz[k]};
                        s_in[k] = ba_keep(R, tt, ca, cb, o, P, thr2, s_sig[s_la[k]], s_sig[s_lb[k]]) ? 1 : 0;
                        kept += s_in[k];
                    }
            }
            for (int k = 0; k < M; ++k) {
                const int row = s_src[k];
                flags[row] = s_in[k];
                if (s_in[k]) { points[3 * row] = Yx[k]; points[3 * row + 1] = Yy[k]; points[3 * row + 2] = Yz[k]; }
            }
            pose_store(R, tt, T.data());
            info = {kept >= min_inliers ? 0 : 1, M, kept, steps, discarded, held, pnp_status, 0};
            cost[0] = cost_first; cost[1] = cost_last;
        }
        wr(out, T); wr(out, cost); wr(out, info); wr(out, flags); wr(out, points);
        ++jobs;
    }
    fclose(out);
    printf("ba ok: %d jobs\n", jobs);
    return 0;
}
"""


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


def build(tmp, flags):
    (tmp / "ba_main.cpp").write_text(BA_HOST)
    exe = tmp / "ba_main"
    return exe, [_cxx(), "-std=c++17", "-I", CSRC, str(tmp / "ba_main.cpp"), "-o", str(exe)] + flags


def run_jobs(exe, tmp, cases):
    """The host program's result for every case (a dict as `vis_ba_reference.planted_case` gives, plus optional settings)."""
    with open(tmp / "jobs.bin", "wb") as f:
        for c in cases:
            na, nb, K = len(c["kp_a"]), len(c["kp_b"]), len(c["rows"])
            la, lb = c.get("lv_a"), c.get("lv_b")
            f.write(np.array([na, nb, K, la is not None, lb is not None, c.get("min_inliers", 20), c.get("ba_iterations", 10),
                              c.get("ba_rounds", 2), c.get("pnp_status", 0), 0], dtype=np.int32).tobytes())
            par = np.concatenate([[c.get("reproj_error", 2.0)], c.get("cam_a", ba.CAM), c.get("cam_b", ba.CAM),
                                  [c.get("base_a", ba.BASELINE), c.get("base_b", ba.BASELINE)], np.asarray(c["T0"]).reshape(16)])
            f.write(par.astype(np.float64).tobytes())
            for key in ("kp_a", "pts_a", "kp_b", "pts_b"):
                f.write(np.ascontiguousarray(c[key], dtype=np.float64).tobytes())
            for l in (la, lb):
                if l is not None:
                    f.write(np.ascontiguousarray(l, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(c["rows"], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(c["flags"]).astype(np.int32).tobytes())
    r = subprocess.run([str(exe), str(tmp / "jobs.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("ba ok: %d jobs" % len(cases))
    raw = np.fromfile(tmp / "out.bin", dtype=np.uint8)
    at, out = 0, []

    def take(shape, dtype):
        nonlocal at
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = raw[at:at + size].view(dtype).reshape(shape).copy()
        at += size
        return a

    for c in cases:
        K = len(c["rows"])
        T, cost, info = take((4, 4), np.float64), take((2,), np.float64), take((8,), np.int32)
        out.append(dict(T=T, cost=cost, info=info, flags=take((K,), np.int32).astype(bool), points=take((K, 3), np.float64)))
    assert at == len(raw)
    return out


@functools.lru_cache(maxsize=None)
def cases_and_records():
    cases = ba.all_cases()
    return cases, [ba.run_case(c, **ba.settings(c)) for c in cases]


# ---- the restatement against the plant -------------------------------------------------------------------------------
def test_restatement_beats_the_pnp_fit_on_the_far_scene():
    """20 seeds of the far scene (150 correspondences, fx = 100, baseline 0.2 m, depths 3 - 8 m, +-0.5 px on u, v and the
    disparity of both views, no outliers), started at the Gauss-Newton PnP fit: the adjusted transform is closer to the plant
    in at least 14 of 20 seeds for translation and for rotation, and the ratios of the median errors are <= 0.8.
    The restatement gives 20 and 20 of 20, ratios 0.43 (0.0111 m -> 0.0048 m) and 0.53 (0.124 deg -> 0.066 deg)."""
    et, er = [], []
    for seed in range(20):
        s, T0, ok = ba.far_scene(seed)
        rows = np.repeat(np.arange(len(ok))[:, None], 2, axis=1)
        rec = ba.adjust(s["kp_a"], s["pts_a"], s["kp_b"], s["pts_b"], rows, T0, ok, ba.FAR_CAM, ba.FAR_CAM, ba.FAR_BASELINE, ba.FAR_BASELINE,
                        reproj_error=1e9, min_inliers=1)
        assert rec["status"] == 0 and rec["discarded"] == 0 and rec["held"] == 0 and rec["set_out"] == 150
        assert rec["cost"][1] < rec["cost"][0]
        a, b = ba.pose_errors(T0, s["T"]), ba.pose_errors(rec["T"], s["T"])
        et.append((a[0], b[0]))
        er.append((a[1], b[1]))
    et, er = np.array(et), np.array(er)
    better_t, better_r = int((et[:, 1] < et[:, 0]).sum()), int((er[:, 1] < er[:, 0]).sum())
    ratio_t, ratio_r = np.median(et[:, 1]) / np.median(et[:, 0]), np.median(er[:, 1]) / np.median(er[:, 0])
    print("better in %d (translation) and %d (rotation) of 20; medians %.4f -> %.4f m (%.2f), %.3f -> %.3f deg (%.2f)" % (
        better_t, better_r, np.median(et[:, 0]), np.median(et[:, 1]), ratio_t, np.median(er[:, 0]), np.median(er[:, 1]), ratio_r))
    assert better_t >= 14 and better_r >= 14
    assert ratio_t <= 0.8 and ratio_r <= 0.8


def test_restatement_step_is_the_dense_gauss_newton_step():
    """The Schur-complement step equals the step of the dense (6 + 3 M)-square normal equations."""
    c = ba.planted_case(20)
    want = ba.run_case(c, ba_iterations=1, ba_rounds=1)
    pr = want["problem"]
    R, t = c["T0"][:3, :3], c["T0"][:3, 3]
    Y = c["pts_a"][c["rows"][want["src"], 0]]
    member = np.ones(len(Y), dtype=bool)
    idx, Hpp, gp, Hcp, Hcc, gc, _, _ = pr.blocks(R, t, Y, member)
    H = pr.dense_normal(R, t, Y, member)
    g = np.concatenate([gc.sum(axis=0), gp.reshape(-1)])
    x = -np.linalg.solve(H, g)
    Rn, tn, Yn, nd, held = pr.step(R, t, Y, member)
    Re, te = ba.se3_exp(x[:6])
    assert held == 0 and len(idx) == 20
    assert np.abs(Re @ R - Rn).max() <= 1e-9 and np.abs(Re @ t + te - tn).max() <= 1e-9
    assert np.abs(Y + x[6:].reshape(-1, 3) - Yn).max() <= 1e-7


def test_cases_meet_the_rules_they_were_chosen_for():
    cases, recs = cases_and_records()
    by = {c["name"]: (c, r) for c, r in zip(cases, recs)}
    for size in ba.SET_SIZES:
        c, r = by["size %d" % size]
        assert r["set_in"] == size and r["status"] == 0 and r["discarded"] == 0 and r["guard_recount"] >= ba.RECOUNT_GUARD
        assert r["cost"][1] < r["cost"][0] and 0.05 * size <= np.isnan(c["pts_b"][c["rows"][c["flags"], 1], 2]).sum() <= 0.2 * size + 2
        assert set(np.unique(c["lv_a"])) == set(np.unique(c["lv_b"])) == {0, 1, 2, 3}
        assert np.abs(r["T"] - c["T"]).max() < 0.05
    c, r = by["displaced from keypoint"]
    k = c["displaced"]
    assert c["flags"][k] and not r["flags"][k] and r["set_out"] == r["set_in"] - 1 and r["guard_recount"] >= ba.RECOUNT_GUARD
    c, r = by["no to depth"]
    assert np.isnan(c["pts_b"]).all() and r["status"] == 0 and r["set_out"] == r["set_in"] and np.abs(r["T"] - c["T"]).max() < 0.05
    c, r = by["behind at T0"]
    k = c["behind"]
    assert c["flags"][k] and not r["flags"][k] and r["set_out"] == r["set_in"] - 1
    c, r = by["held by the pivot rule"]
    assert r["held"] >= r["set_in"] and r["steps"] >= 1 and r["status"] == 0
    for st in (1, 2, 3):
        assert by["pnp status %d" % st][1]["status"] == st
    assert by["no rounds"][1]["status"] == 0 == by["no iterations"][1]["status"]
    assert by["above the cap"][1]["status"] == 3 and by["too few remain"][1]["status"] == 1


def check_program(exe, tmp):
    cases, recs = cases_and_records()
    got = run_jobs(exe, tmp, cases)
    for c, g, w in zip(cases, got, recs):
        ba.compare(c, g, w, c["name"])


def test_header_in_the_kernels_schedule_equals_the_restatement(tmp_path):
    exe, cmd = build(tmp_path, ["-O2"])
    subprocess.run(cmd, check=True)
    check_program(exe, tmp_path)


def test_header_standalone_under_sanitizers(tmp_path):
    exe, base = build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout:
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    check_program(exe, tmp_path)


# ---- the Python layer ------------------------------------------------------------------------------------------------
def _kf(n, levels=None):
    kf = (np.zeros((n, 2)), np.ones((n, 3)), np.zeros((n, 32), np.uint8))
    return vr.Keyframe(*kf) if levels is None else vr.LevelKeyframe(*kf, levels)


def test_argument_errors_raise_before_any_launch():
    """Every one of these raises ValueError: on a machine without a GPU a call that got past its checks raises CslamHipError."""
    ok = [(_kf(5), _kf(6))]
    reg = [vr.VisualRegistration(np.identity(4), True, 0, np.zeros((3, 2), np.int64), np.ones(3, bool), 0, 0)]
    bad_lv = [(_kf(5, np.array([0, 1, 2, 3, 8])), _kf(6, np.zeros(6, np.int32)))]
    neg_lv = [(_kf(5, np.zeros(5, np.int32)), _kf(6, np.array([0, 0, -1, 0, 0, 0])))]
    short = [(vr.Keyframe(np.zeros((5, 2)), np.ones((4, 3)), np.zeros((5, 32), np.uint8)), _kf(6))]
    for call in (lambda p, **kw: vr.register_pairs_ba(p, ba.CAM, **kw), lambda p, **kw: vr.bundle_adjust_pairs(p, reg, ba.CAM, **kw)):
        for pairs in (bad_lv, neg_lv, short):
            with pytest.raises(ValueError):
                call(pairs)
        for kw in (dict(baselines=0.0), dict(baselines=-0.1), dict(baselines=np.nan), dict(baselines=[0.1, 0.0]), dict(baselines=np.ones((2, 2))),
                   dict(ba_iterations=-1), dict(ba_rounds=-1), dict(reproj_error=0.0), dict(min_inliers=0), dict(cameras_to=np.ones((2, 4)))):
            with pytest.raises(ValueError):
                call(ok, **kw)
    with pytest.raises(ValueError):
        vr.bundle_adjust_pairs(ok, reg + reg, ba.CAM)       # mismatched lengths
    with pytest.raises(ValueError):
        vr.bundle_adjust_pairs(ok, [vr.VisualRegistration(np.identity(4), True, 0, np.zeros((3, 2), np.int64), np.ones(2, bool), 0, 0)], ba.CAM)
    with pytest.raises(ValueError):
        vr.register_pairs_ba(ok, np.ones((2, 4)))
    with pytest.raises(ValueError):
        vr.register_pairs_ba(ok, ba.CAM, nndr=1.5)
    with pytest.raises(ValueError):
        vr.compute_transformation_ba(_kf(5), _kf(6), ba.CAM, iterations=0)


def test_no_cpu_path():
    import ctypes
    n = ctypes.c_int(0)
    if _lib.load().cslam_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("GPU present: covered by the -m gpu suite")
    with pytest.raises(_lib.CslamHipError):
        vr.register_pairs_ba([(_kf(5), _kf(6))], ba.CAM)
    with pytest.raises(_lib.CslamHipError):
        vr.register_pairs_ba([], ba.CAM)


def test_refined_registration_is_a_visual_registration():
    pnp = vr.VisualRegistration(np.identity(4), True, 0, np.zeros((3, 2), np.int64), np.ones(3, bool), 1, 7)
    T = np.identity(4)
    T[0, 3] = 0.5
    r = vr.RefinedRegistration(pnp, T, 0, np.array([True, False, True]), np.zeros((3, 3)), 2.0, 1.0, 3, 5, 0, 0)
    assert isinstance(r, vr.VisualRegistration) and r.success and r.pnp is pnp and r.best_hypothesis == 7 and r.dropped_no_depth == 1
    assert np.allclose(r.to_edge((0, 1), (1, 2)).measurement, np.linalg.inv(T))
    bad = vr.RefinedRegistration(pnp, T, 1, np.zeros(3, bool), np.full((3, 3), np.nan), 2.0, 1.0, 3, 5, 0, 0)
    with pytest.raises(ValueError):
        bad.to_edge((0, 1), (1, 2))
