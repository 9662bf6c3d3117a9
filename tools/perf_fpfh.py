#!/usr/bin/env python
"""FPFH features and mutual matches of down-sampled lidar keyframes on the GPU box, the numpy / cKDTree restatement beside them.

    python tools/perf_fpfh.py [--raw 60000] [--batch 16] [--reps 30]

Clouds: the 15k-point recipe of tools/perf_icp.py (the synthetic street of tests/icp_reference.py from 60 000 raw points,
voxel-averaged at 0.5 m), which is what registering a pair is timed on.  Times are HIP events around the C entry points
on device-resident clouds and features with host copies of the offsets (no host wait inside the calls), after warm-up
calls, median and extremes over the repetitions.  Stages: the neighbour search at (5 voxels, 100), the normals from the
prefix of its lists at (2 voxels, 30), SPFH + FPFH; then all three back to back, which is what `extract_fpfh_clouds`
enqueues.  The host-API figures include the copies.  The CPU figures are tests/fpfh_reference.py (numpy, and
scipy's cKDTree as the reference's find_knn_cpu uses it) on one core of the same box; they are a restatement written
for clarity, not open3d, and no speed-up over open3d is claimed.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw", type=int, default=60000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu", type=int, default=1, help="0: leave the CPU restatement out")
    args = ap.parse_args()
    import torch
    import fpfh_reference as fref
    import icp_reference as ref
    from cslam_amd import _lib
    from cslam_amd.lidar_pr import icp_utils as u
    from cslam_amd.lidar_pr._batch import upload

    _lib.require_gpu()
    lib = _lib.load()
    voxel = 0.5
    pairs = [ref.street_scene(seed, args.raw, voxel)[:2] for seed in range(args.batch)]
    clouds = [p[0] for p in pairs]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    host = lambda a: a.ctypes.data_as(C.c_void_p)
    print(f"clouds: street scenes from {args.raw} raw points at {voxel} m voxels, {min(len(c) for c in clouds)} .. "
          f"{max(len(c) for c in clouds)} points; search chunk {u.KNN_CHUNK}, candidate buffer {u.KNN_CAND}, "
          f"matching block {u.FM_BLOCK} x chunk {u.FM_CHUNK}")

    for name, sel in (("1 cloud", clouds[:1]), (f"{args.batch} clouds", clouds)):
        cl = upload(sel, dev)
        n, total, off = len(sel), int(cl.off[-1]), cl.off
        pts, d_off = cl.rows, cl.d_off
        idx = torch.empty((total, 100), dtype=torch.int32, device=dev)
        d2 = torch.empty((total, 100), dtype=torch.float64, device=dev)
        cnt = torch.empty(total, dtype=torch.int32, device=dev)
        nrm = torch.empty((total, 3), dtype=torch.float64, device=dev)
        feat = torch.empty((total, 33), dtype=torch.float64, device=dev)

        def knn():
            _lib.check(lib.cslam_knn_radius_dev(pts, d_off, n, 5 * voxel, 100, idx.data_ptr(), d2.data_ptr(), cnt.data_ptr(), host(off), st))

        def normals():
            _lib.check(lib.cslam_normals_dev(pts, d_off, n, idx.data_ptr(), d2.data_ptr(), cnt.data_ptr(), 100, 2 * voxel, 30, None,
                                             nrm.data_ptr(), host(off), st))

        def fpfh():
            _lib.check(lib.cslam_fpfh_dev(pts, nrm.data_ptr(), d_off, n, idx.data_ptr(), d2.data_ptr(), cnt.data_ptr(), 100,
                                          feat.data_ptr(), None, host(off), st))

        def all_three():
            knn()
            normals()
            fpfh()

        pair_tests = sum(len(c) ** 2 for c in sel)
        for stage, run in (("neighbour search (5 voxels, 100)", knn), ("normals (2 voxels, 30, prefix)", normals), ("SPFH + FPFH", fpfh),
                           ("all three back to back", all_three)):
            text, med = timed(torch, run, args.reps)
            extra = f" = {pair_tests / med / 1e9:.2f} T point pairs/s" if run is knn else ""
            extra = f" = {med / n:.3f} ms per cloud" if run is all_three else extra
            print(f"{name}: {stage}: {text}{extra}")
        c = cnt.cpu().numpy()
        print(f"{name}: {total} points; list entries: mean {c.mean():.1f}, cut at 100 for {100 * (c == 100).mean():.1f} %, "
              f"fewer than 3 within 2 voxels for {100 * ((d2[:, :3] <= (2 * voxel) ** 2).sum(dim=1) < 3).float().mean().item():.1f} %")
    u.extract_fpfh_clouds(clouds[:1], voxel)
    for name, n in (("1 cloud", 1), (f"{args.batch} clouds", args.batch)):
        t0 = time.perf_counter()
        for _ in range(5):
            feats = u.extract_fpfh_clouds(clouds[:n], voxel)
        print(f"{name}: extract_fpfh_clouds (host arrays in, features out) {(time.perf_counter() - t0) / 5 * 1e3:.2f} ms per call")

    # matching: the features of the (source, target) clouds of every scene
    f_src = feats
    f_dst = u.extract_fpfh_clouds([p[1] for p in pairs], voxel)
    for name, m in (("1 pair", 1), (f"{args.batch} pairs", args.batch)):
        a_off = np.zeros(m + 1, dtype=np.int64)
        b_off = np.zeros(m + 1, dtype=np.int64)
        a_off[1:] = np.cumsum([len(f) for f in f_src[:m]])
        b_off[1:] = np.cumsum([len(f) for f in f_dst[:m]])
        t_a = torch.from_numpy(np.concatenate(f_src[:m])).to(dev)
        t_b = torch.from_numpy(np.concatenate(f_dst[:m])).to(dev)
        t_ao, t_bo = torch.from_numpy(a_off).to(dev), torch.from_numpy(b_off).to(dev)
        na, nb = int(a_off[-1]), int(b_off[-1])
        out = torch.empty(3 * na + nb + m, dtype=torch.int32, device=dev)
        base = out.data_ptr()

        def match():
            _lib.check(lib.cslam_feature_match_dev(t_a.data_ptr(), t_ao.data_ptr(), t_b.data_ptr(), t_bo.data_ptr(), m, 33, base,
                                                   base + 4 * na, base + 4 * (na + nb), base + 4 * (3 * na + nb), host(a_off),
                                                   host(b_off), st))
        text, med = timed(torch, match, args.reps)
        work = 2 * sum(len(a) * len(b) for a, b in zip(f_src[:m], f_dst[:m]))
        kept = out[3 * na + nb:].cpu().numpy()
        print(f"{name}: find_correspondences (both directions + mutual filter, device resident): {text} = {med / m:.3f} ms per pair, "
              f"{work / med / 1e9:.2f} T row pairs/s of 33 doubles; mutual matches {kept.min()} .. {kept.max()} of about {len(f_src[0])}")
        t0 = time.perf_counter()
        for _ in range(3):
            got = u.find_correspondences_pairs(list(zip(f_src[:m], f_dst[:m])))
        print(f"{name}: find_correspondences_pairs (host arrays in, results out) {(time.perf_counter() - t0) / 3 * 1e3:.2f} ms per call")
    if not args.cpu:
        return
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    lists = fref.radius_neighbors(clouds[0], 5 * voxel, 100)
    t1 = time.perf_counter()
    nrm = fref.estimate_normals(clouds[0], *fref.radius_neighbors(clouds[0], 2 * voxel, 30), 2 * voxel, 30)
    t2 = time.perf_counter()
    want = fref.compute_fpfh(fref.compute_spfh(clouds[0], nrm, lists[0], lists[2]), *lists)
    t3 = time.perf_counter()
    print(f"restatement (numpy, one core of this box), 1 cloud: search {(t1 - t0) * 1e3:.0f} ms, second search + normals "
          f"{(t2 - t1) * 1e3:.0f} ms, SPFH + FPFH {(t3 - t2) * 1e3:.0f} ms; largest |GPU - restatement| over the features "
          f"{np.abs(want - f_src[0]).max():.3g} (a count of a bin is {100.0 / 99:.2f} .. 100)")
    t0 = time.perf_counter()
    nn01 = fref.match_kdtree(f_src[0], f_dst[0])
    nn10 = fref.match_kdtree(f_dst[0], f_src[0])
    i0, i1 = fref.mutual(nn01, nn10)
    t1 = time.perf_counter()
    same = np.array_equal(i0, got[0][0]) and np.array_equal(i1, got[0][1])
    print(f"restatement (cKDTree as find_knn_cpu, one core), 1 pair: {(t1 - t0) * 1e3:.0f} ms; {len(i0)} mutual matches, "
          f"equal to the GPU's: {same} (features of flat ground repeat, so ties and near-ties are expected to differ)")


if __name__ == "__main__":
    main()
