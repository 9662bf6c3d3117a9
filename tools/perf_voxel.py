#!/usr/bin/env python
"""Voxel down-sampling of raw lidar scans on the GPU box: one scan and a batch of 16, numpy's `voxel_average` beside it.

    python tools/perf_voxel.py [--points 130000] [--batch 16] [--reps 30]

Scans: the raw clouds of the synthetic street of tests/icp_reference.py (its generator without the final averaging),
about 130 000 points each, the size of a 64-beam sweep, at 0.5 m voxels.  Times are HIP events around
`cslam_voxel_downsample_dev` on device-resident clouds, after warm-up calls, median and extremes over the repetitions;
the events span the call's one host wait, so the figure is what a handler that keeps its clouds on the GPU waits for.
The per-stage split comes from the events `cslam_voxel_profile` has the call record at its stage boundaries.  The
host-API figure includes the copies.  The CPU figure is `voxel_average` (numpy) on one core of the same box.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

STAGES = ("bounds + meta", "host wait", "keys", "radix passes", "heads + scan", "segment sums")


def raw_scans(ref, n_clouds, points, voxel):
    """Raw street scans: street_scene with its final averaging switched off (each scene is two scans of one street)."""
    keep = ref.voxel_average
    ref.voxel_average = lambda pts, v: np.asarray(pts)
    try:
        out = []
        for seed in range((n_clouds + 1) // 2):
            src, dst, _, _ = ref.street_scene(seed, int(points / 0.6), voxel)
            out += [src, dst]
    finally:
        ref.voxel_average = keep
    return out[:n_clouds]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=130000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    import icp_reference as ref
    from cslam_amd import _lib
    from cslam_amd.lidar_pr import icp_utils
    from cslam_amd.lidar_pr._batch import upload

    _lib.require_gpu()
    lib = _lib.load()
    voxel = 0.5
    scans = raw_scans(ref, args.batch, args.points, voxel)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    print(f"scans: {len(scans)} raw clouds of {min(len(s) for s in scans)} .. {max(len(s) for s in scans)} points, voxel {voxel} m; "
          f"sort tile {icp_utils.VOXEL_TILE} keys")

    def device_call(sel):
        clouds = [scans[k] for k in sel]
        cl = upload(clouds, dev)
        n, total = len(clouds), int(cl.off[-1])
        out = torch.empty((total, 3), dtype=torch.float64, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)

        def run():
            _lib.check(lib.cslam_voxel_downsample_dev(cl.rows, cl.d_off, n, voxel, out.data_ptr(),
                                                      out_off.data_ptr(), None, status.data_ptr(),
                                                      cl.off.ctypes.data_as(C.c_void_p), st))
        return run, out, out_off, total

    for name, sel in (("1 scan", [0]), (f"{args.batch} scans", list(range(args.batch)))):
        run, out, out_off, total = device_call(sel)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ms, wall = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
        ms, wall = np.array(ms), np.array(wall)
        rows = int(out_off.cpu()[-1])
        print(f"{name}: {total} points -> {rows} voxels; device resident, events: median {np.median(ms):.3f} ms, min {ms.min():.3f}, "
              f"max {ms.max():.3f} over {args.reps} calls = {np.median(ms) / len(sel):.3f} ms per scan; wall median {np.median(wall):.3f} ms")
        _lib.check(lib.cslam_voxel_profile(1))
        split = []
        info = (C.c_int32 * 4)()
        for _ in range(args.reps):
            run()
            got = (C.c_double * 6)()
            _lib.check(lib.cslam_voxel_profile_read(C.byref(got), C.byref(info)))
            split.append(list(got))
        _lib.check(lib.cslam_voxel_profile(0))
        med = np.median(np.array(split), axis=0)
        print(f"{name}: {info[0]} key passes + {info[1]} cloud-number passes of 8 bits ({info[2]} key bits, {info[3]} sort tiles); "
              "median per stage: " + ", ".join(f"{s} {m * 1e3:.0f} us" for s, m in zip(STAGES, med))
              + f" (sum {med.sum() * 1e3:.0f} us)")
    # the public host API on the same inputs (copies included)
    icp_utils.downsample_clouds(scans[:1], voxel)
    for name, n in (("1 scan", 1), (f"{args.batch} scans", args.batch)):
        t0 = time.perf_counter()
        for _ in range(5):
            got = icp_utils.downsample_clouds(scans[:n], voxel)
        dt = (time.perf_counter() - t0) / 5
        print(f"{name}: downsample_clouds (host arrays in, results out) {dt * 1e3:.2f} ms per call")
    t_cpu = []
    for k in range(min(args.batch, 3)):
        t0 = time.perf_counter()
        want = ref.voxel_average(scans[k], voxel)
        t_cpu.append(time.perf_counter() - t0)
        assert np.array_equal(got[k], want), "the GPU result differs from voxel_average"
    print(f"voxel_average (numpy, this box's CPU): {np.median(t_cpu) * 1e3:.1f} ms per scan; GPU rows == voxel_average bit for bit "
          f"on the first {len(t_cpu)} scans")


if __name__ == "__main__":
    main()
