#!/usr/bin/env python
"""Lidar registration on the GPU box: the staged ICP for one pair and for a batch of 16, the scipy restatement beside it.

    python tools/perf_icp.py [--raw 60000] [--batch 16] [--reps 20] [--estimation both]

Scene: the synthetic street of tests/icp_reference.py (60 000 raw points -> about 15k points per cloud at 0.5 m voxels),
seeded with the true yaw rounded to ScanContext's 6 degree sector, stages = icp_utils.DEFAULT_STAGES.  Times are HIP
events around `cslam_icp_register_dev` on device-resident clouds (what a handler that keeps its keyframes on the GPU
pays), after a warm-up call; the host-API figure includes the copies.  The restatement is float64 numpy + cKDTree on
one core of the same box.

--estimation point_to_point | point_to_plane | both (the default): with both, the two estimators are timed in the same run
on the same clouds, one after the other per case, and the point-to-plane lines carry the ratio.  The targets' normals of
point-to-plane are device resident like the clouds; what estimating them costs (the radius search at 2 voxels and the
normals, as `register_pairs` chains them) is timed on its own line.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw", type=int, default=60000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--estimation", choices=("point_to_point", "point_to_plane", "both"), default="both")
    args = ap.parse_args()
    import torch
    import icp_reference as ref
    from cslam_amd import _lib
    from cslam_amd.lidar_pr import _batch, icp, icp_utils

    _lib.require_gpu()
    lib = _lib.load()
    voxel = 0.5
    scenes = [ref.street_scene(seed, args.raw, voxel) for seed in range(args.batch)]
    yaws = [360.0 - ref.seed_yaw(s[3]) for s in scenes]
    dists = np.array([m * voxel for m, _ in icp_utils.DEFAULT_STAGES])
    iters = np.array([i for _, i in icp_utils.DEFAULT_STAGES], dtype=np.int32)
    st = torch.cuda.current_stream().cuda_stream
    estimations = icp.ESTIMATIONS if args.estimation == "both" else (args.estimation,)

    def device_call(sel, estimation="point_to_point"):
        n = len(sel)
        so = np.zeros(n + 1, dtype=np.int64)
        do = np.zeros(n + 1, dtype=np.int64)
        so[1:] = np.cumsum([len(scenes[k][0]) for k in sel])
        do[1:] = np.cumsum([len(scenes[k][1]) for k in sel])
        t = dict(src=torch.from_numpy(np.concatenate([scenes[k][0] for k in sel])).cuda(),
                 dst=torch.from_numpy(np.concatenate([scenes[k][1] for k in sel])).cuda(),
                 so=torch.from_numpy(so).cuda(), do=torch.from_numpy(do).cuda(),
                 init=torch.from_numpy(np.stack([icp_utils.yaw_seed(yaws[k]).reshape(16) for k in sel])).cuda(),
                 T=torch.empty((n, 16), dtype=torch.float64, device="cuda"),
                 stats=torch.empty((n, 4), dtype=torch.float64, device="cuda"))

        targets = _batch.Packed(t["dst"], t["dst"].data_ptr(), t["do"].data_ptr(), do)

        def normals():
            t["normals"] = icp.target_normals_enqueue(lib, targets, voxel)

        if estimation == "point_to_plane":
            normals()

        def register(first, n_stages, p_init):
            """Stages first .. first + n_stages - 1 from the transforms at p_init, by the entry point of the estimator."""
            clouds = (t["src"].data_ptr(), t["so"].data_ptr(), t["dst"].data_ptr(), t["do"].data_ptr())
            tail = (n, p_init, dists[first:].ctypes.data_as(C.c_void_p), iters[first:].ctypes.data_as(C.c_void_p), n_stages, 1e-6, 1e-6,
                    t["T"].data_ptr(), t["stats"].data_ptr(), st)
            if estimation == "point_to_plane":
                _lib.check(lib.cslam_icp_register_plane_dev(*clouds, t["normals"].data_ptr(), *tail))
            else:
                _lib.check(lib.cslam_icp_register_dev(*clouds, *tail))

        def run():
            register(0, len(dists), t["init"].data_ptr())

        def updates_per_stage():
            """[stage][pair]: the stages one call each, every one from the transforms the one before left."""
            out = []
            for k in range(len(dists)):
                register(k, 1, t["init"].data_ptr() if k == 0 else t["T"].data_ptr())
                out.append(t["stats"].cpu().numpy()[:, 3].astype(int))
            return np.array(out)

        def one_eval(idx, d2):
            _lib.check(lib.cslam_icp_correspondences_dev(
                t["src"].data_ptr(), t["so"].data_ptr(), t["dst"].data_ptr(), t["do"].data_ptr(), n, t["T"].data_ptr(),
                voxel, idx.data_ptr(), d2.data_ptr(), st))
        return (t, run, one_eval, int(so[-1]), sum(int(so[p + 1] - so[p]) * int(do[p + 1] - do[p]) for p in range(n)), normals,
                updates_per_stage)

    def events(fn, reps):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return np.array(ms)

    print(f"scene: {args.raw} raw points, voxel {voxel} m; clouds of pair 0: {len(scenes[0][0])} / {len(scenes[0][1])} points; "
          f"stages {icp_utils.DEFAULT_STAGES}")
    results = {}
    for name, sel in (("1 pair", [0]), (f"{args.batch} pairs", list(range(args.batch)))):
        base = None
        for estimation in estimations:
            t, run, one_eval, total, pairs, normals, updates_per_stage = device_call(sel, estimation)
            ms = events(run, args.reps)
            stats = t["stats"].cpu().numpy()
            T = t["T"].cpu().numpy().reshape(-1, 4, 4)
            if estimation == "point_to_point":
                results[name] = T
            rot = max(ref.rotation_error_deg(T[k][:3, :3], scenes[s][2][:3, :3]) for k, s in enumerate(sel))
            tr = max(float(np.linalg.norm(T[k][:3, 3] - scenes[s][2][:3, 3])) for k, s in enumerate(sel))
            ratio = "" if base is None else f" = {np.median(ms) / base:.2f} x point_to_point in this run"
            print(f"{name}, {estimation}: register (3 stages, device resident) median {np.median(ms):.2f} ms, min {ms.min():.2f}, "
                  f"max {ms.max():.2f} over {args.reps} calls = {np.median(ms) / len(sel):.2f} ms per pair{ratio}; last-stage "
                  f"iterations {stats[:, 3].astype(int).tolist()}, fitness {stats[:, 0].min():.4f} .. {stats[:, 0].max():.4f}; "
                  f"against the ground truth <= {rot:.4f} deg, <= {tr:.4f} m")
            ups = updates_per_stage()
            print(f"{name}, {estimation}: updates per stage of pair {sel[0]} {ups[:, 0].tolist()}; over the stages per pair "
                  f"{ups.sum(axis=0).tolist()}; the most of any pair per stage {ups.max(axis=1).tolist()}")
            if estimation == "point_to_plane":
                nm = events(normals, args.reps)
                print(f"{name}, {estimation}: the targets' normals (radius search at 2 voxels + normals, what register_pairs adds "
                      f"for this estimator) median {np.median(nm):.2f} ms")
            else:
                base = np.median(ms)
        idx = torch.empty(total, dtype=torch.int32, device="cuda")
        d2 = torch.empty(total, dtype=torch.float64, device="cuda")
        ev = events(lambda: one_eval(idx, d2), args.reps)
        print(f"{name}: one evaluation (nearest neighbours + merge, {pairs / 1e6:.0f} M point pairs) median {np.median(ev) * 1e3:.0f} us "
              f"= {pairs / (np.median(ev) * 1e-3) / 1e12:.2f} T point pairs/s (each: 3 sub, 1 mul, 2 fma, 1 compare in float64)")
    # the public host API on the same inputs (copies included)
    pairs_host = [(s[0], s[1]) for s in scenes]
    for estimation in estimations:
        icp_utils.register_pairs(pairs_host[:1], voxel, yaws[:1], estimation=estimation)
        for name, n in (("1 pair", 1), (f"{args.batch} pairs", args.batch)):
            t0 = time.perf_counter()
            for _ in range(5):
                icp_utils.register_pairs(pairs_host[:n], voxel, yaws[:n], estimation=estimation)
            dt = (time.perf_counter() - t0) / 5
            print(f"{name}, {estimation}: register_pairs (host arrays in, results out) {dt * 1e3:.2f} ms per call")
    if not results:
        return
    # accuracy of point-to-point against the ground truth and the restatement
    t_cpu, worst_rot, worst_tr, worst_dT = [], 0.0, 0.0, 0.0
    for k in range(min(args.batch, 4)):
        src, dst, T_true, _ = scenes[k]
        t0 = time.perf_counter()
        want = ref.register_staged(src, dst, voxel, icp_utils.yaw_seed(yaws[k]))
        t_cpu.append(time.perf_counter() - t0)
        T = results[f"{args.batch} pairs"][k]
        worst_rot = max(worst_rot, ref.rotation_error_deg(T[:3, :3], T_true[:3, :3]))
        worst_tr = max(worst_tr, float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])))
        worst_dT = max(worst_dT, float(np.abs(T - want[-1].transformation).max()))
        print(f"pair {k}: restatement (numpy + cKDTree, this box's CPU) {t_cpu[-1] * 1e3:.0f} ms, iterations "
              f"{[s.iterations for s in want]}")
    print(f"against the ground truth: rotation error <= {worst_rot:.4f} deg, translation error <= {worst_tr:.4f} m; "
          f"max |T - T_restatement| = {worst_dT:.2e}; batch == single bits: "
          f"{np.array_equal(results['1 pair'][0], results[f'{args.batch} pairs'][0])}")


if __name__ == "__main__":
    main()
