#!/usr/bin/env python
"""The robust coarse fit of lidar loop closures on the GPU box, stage by stage, the numpy restatement beside it.

    python tools/perf_robust.py [--batch 16] [--reps 20] [--batch-reps 5] [--cap-n 8000] [--parts single,batch,cap,whole,dense] [--cpu 1]

Inputs: the mutual FPFH matches of the street scenes of tests/icp_reference.py (9000 raw points, 0.5 m voxels: the scenes
of the tests, about 1.1k matches per pair), and a planted input near the cap (tests/robust_reference.planted).  Times are
HIP events around the C entry points on device-resident matched points with host copies of offsets and counts (no host
wait inside the calls), after warm-up calls, median and extremes over the repetitions (the figures of the whole batch, whose clique search takes seconds per call,
over --batch-reps calls; every figure prints its number of calls).  The whole `solve_teaser_pairs`
figure is wall time from host arrays to results.  The CPU figures are tests/robust_reference.py on one core of the same
box: a restatement written for clarity, not TEASER++, and no speed-up over TEASER++ is claimed.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def timed(torch, run, reps):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return "median %.3f ms, min %.3f, max %.3f over %d calls" % (np.median(ms), ms.min(), ms.max(), reps), float(np.median(ms))


class Staged:
    """Device-resident matched points of a batch and the outputs of every stage."""

    def __init__(self, torch, lib, u, pairs, c, budget):
        self.torch, self.lib, self.c, self.budget, self.n = torch, lib, c, budget, len(pairs)
        dev = torch.device("cuda", 0)
        from cslam_amd.lidar_pr import robust
        ms, md, self.off = robust.matched_points(pairs)
        used, words = robust.used(self.off)
        self.h_off = self.off.ctypes.data_as(C.c_void_p)
        self.t_ms, self.t_md, self.t_off = (torch.from_numpy(x).to(dev) for x in (ms, md, self.off))
        total = int(self.off[-1])
        self.t_adj = torch.zeros(int(words[-1]) + 1, dtype=torch.int64, device=dev)
        self.t_adj_off = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.t_deg = torch.zeros(total, dtype=torch.int32, device=dev)
        self.t_clique = torch.zeros(total, dtype=torch.int32, device=dev)
        self.t_small = torch.zeros((3, self.n), dtype=torch.int32, device=dev)
        self.t_nodes = torch.zeros(self.n, dtype=torch.int64, device=dev)
        self.t_R = torch.zeros((self.n, 9), dtype=torch.float64, device=dev)
        self.t_w = torch.zeros(total, dtype=torch.float64, device=dev)
        self.t_t = torch.zeros((self.n, 3), dtype=torch.float64, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream

    def graph(self):
        from cslam_amd import _lib
        _lib.check(self.lib.cslam_robust_graph_dev(self.t_ms.data_ptr(), self.t_md.data_ptr(), self.t_off.data_ptr(), None, self.n, self.c,
                                                   self.t_adj.data_ptr(), self.t_adj_off.data_ptr(), self.t_deg.data_ptr(), self.h_off, None,
                                                   self.st))

    def clique(self, budget=None):
        from cslam_amd import _lib
        _lib.check(self.lib.cslam_robust_clique_dev(self.t_adj.data_ptr(), self.t_adj_off.data_ptr(), self.t_deg.data_ptr(),
                                                    self.t_off.data_ptr(), None, self.n, budget or self.budget, self.t_clique.data_ptr(),
                                                    self.t_small[0].data_ptr(), self.t_small[1].data_ptr(), self.t_nodes.data_ptr(),
                                                    self.h_off, None, self.st))

    def rotation(self):
        from cslam_amd import _lib
        _lib.check(self.lib.cslam_robust_rotation_dev(self.t_ms.data_ptr(), self.t_md.data_ptr(), self.t_off.data_ptr(),
                                                      self.t_clique.data_ptr(), self.t_small[0].data_ptr(), self.n, self.c, self.t_R.data_ptr(),
                                                      self.t_w.data_ptr(), self.t_small[2].data_ptr(), self.h_off, self.st))

    def translation(self):
        from cslam_amd import _lib
        _lib.check(self.lib.cslam_robust_translation_dev(self.t_ms.data_ptr(), self.t_md.data_ptr(), self.t_off.data_ptr(),
                                                         self.t_clique.data_ptr(), self.t_small[0].data_ptr(), self.t_R.data_ptr(), self.n,
                                                         self.c, self.t_t.data_ptr(), None, self.h_off, self.st))

    def all(self):
        self.graph()
        self.clique()
        self.rotation()
        self.translation()


def report(torch, lib, u, label, pairs, c, budget, reps):
    s = Staged(torch, lib, u, pairs, c, budget)
    n = len(pairs)
    sizes = [len(a) for a, _ in pairs]
    for name, run in (("consistency graph", s.graph), ("maximum clique", s.clique), ("rotation (GNC-TLS)", s.rotation),
                      ("translation (TLS)", s.translation), ("the four stages back to back", s.all)):
        text, med = timed(torch, run, reps)
        print("%s, N = %d .. %d: %s: %s = %.3f ms per pair" % (label, min(sizes), max(sizes), name, text, med / n))
    small, nodes = s.t_small.cpu().numpy(), s.t_nodes.cpu().numpy()
    print("%s: clique sizes %s, certified %s, nodes %s of a budget of %d, rotation iterations %s"
          % (label, small[0].tolist(), small[1].tolist(), nodes.tolist(), budget, small[2].tolist()))
    fit = lambda: u.robust_fit_pairs(pairs, c, budget)
    fit()
    t0 = time.perf_counter()
    for _ in range(reps):
        fit()
    print("%s: robust_fit_pairs (host arrays in, results out) %.2f ms per call" % (label, 1e3 * (time.perf_counter() - t0) / reps))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cap-n", type=int, default=8000)
    ap.add_argument("--cpu", type=int, default=1, help="0: leave the CPU restatement out")
    ap.add_argument("--parts", default="single,batch,cap,whole,dense", help="which parts to run")
    ap.add_argument("--batch-reps", type=int, default=5, help="calls per figure of the whole batch (its clique search takes seconds)")
    ap.add_argument("--whole-batch-reps", type=int, default=3, help="calls of solve_teaser_pairs on the whole batch (seconds each)")
    args = ap.parse_args()
    parts = args.parts.split(",")
    import torch
    import icp_reference as iref
    import robust_reference as ref
    from cslam_amd import _lib
    from cslam_amd.lidar_pr import icp_utils as u

    _lib.require_gpu()
    lib = _lib.load()
    voxel, budget = 0.5, u.ROBUST_DEFAULT_NODE_BUDGET
    scenes = [iref.street_scene(seed)[:2] for seed in range(1, args.batch + 1)]
    feats = u.extract_fpfh_clouds([c for pair in scenes for c in pair], voxel)
    corr = u.find_correspondences_pairs([(feats[2 * p], feats[2 * p + 1]) for p in range(len(scenes))])
    matched = [(scenes[p][0][i0], scenes[p][1][i1]) for p, (i0, i1) in enumerate(corr)]
    print("street scenes 1 .. %d: %d .. %d points per cloud, %d .. %d mutual matches; noise bound %.2f m" % (
        len(scenes), min(len(c) for pair in scenes for c in pair), max(len(c) for pair in scenes for c in pair),
        min(len(a) for a, _ in matched), max(len(a) for a, _ in matched), voxel))
    if "single" in parts:
        report(torch, lib, u, "1 pair (street scene 1)", matched[:1], voxel, budget, args.reps)
        report(torch, lib, u, "1 pair (street scene 2)", matched[1:2], voxel, budget, args.reps)
    if "batch" in parts:
        report(torch, lib, u, "%d pairs" % len(matched), matched, voxel, budget, args.batch_reps)
    if "cap" in parts:
        ms, md, T, inliers = ref.planted(1, args.cap_n, args.cap_n // 20)
        report(torch, lib, u, "1 pair (planted, %d inliers)" % len(inliers), [(ms, md)], 0.05, budget, args.reps)

    whole = lambda pairs: u.solve_teaser_pairs(pairs, voxel, 50)
    for pairs, label, reps in ((scenes[:1], "street scene 1", args.reps), (scenes[1:2], "street scene 2", args.reps),
                               (scenes, "%d pairs" % len(scenes), args.whole_batch_reps)):
        if "whole" not in parts:
            break
        whole(pairs)
        t0 = time.perf_counter()
        for _ in range(reps):
            res = whole(pairs)
        per = 1e3 * (time.perf_counter() - t0) / reps
        print("%s: solve_teaser_pairs (host arrays in: FPFH, matches, robust fit, ICP; results out) %.2f ms per call over %d calls = %.2f ms "
              "per pair; valid %d of %d" % (label, per, reps, per / len(pairs), sum(bool(r[0]) for r in res), len(pairs)))
    if "dense" in parts:
        ms, md = ref.dense_case()
        s = Staged(torch, lib, u, [(ms, md)], 0.5, budget)
        s.graph()
        for b in (budget, 16384, 4096, 256, 16):
            text, _ = timed(torch, lambda: s.clique(b), args.reps)
            small, nodes = s.t_small.cpu().numpy(), s.t_nodes.cpu().numpy()
            print("dense case (N = 128, edge share 0.85), budget %d: %s; clique %d, certified %d, nodes %d"
                  % (b, text, small[0, 0], small[1, 0], nodes[0]))

    if args.cpu:
        for p in (0, 1):
            a, b = matched[p]
            t0 = time.perf_counter()
            adj = ref.consistency_graph(a, b, voxel)
            t1 = time.perf_counter()
            clique, _ = ref.max_clique(adj)
            t2 = time.perf_counter()
            R, _, it = ref.gnc_rotation(a, b, clique, voxel)
            t3 = time.perf_counter()
            ref.tls_translation(a, b, clique, R, voxel)
            t4 = time.perf_counter()
            print("restatement (numpy / Python ints, one core of this box), street scene %d, N = %d: graph %.0f ms, clique (%d) %.0f ms, "
                  "rotation (%d iterations) %.0f ms, translation %.0f ms" % (p + 1, len(a), 1e3 * (t1 - t0), len(clique), 1e3 * (t2 - t1), it,
                                                                            1e3 * (t3 - t2), 1e3 * (t4 - t3)))


if __name__ == "__main__":
    main()
