#!/usr/bin/env python
"""Keyframe clouds and the merged map on the GPU box: one 480 x 640 RGB-D frame and a batch of 16 through
`cslam_cloud_keyframes_dev`, then `cslam_map_assemble_dev` over 64 and 1024 keyframe clouds.

    python tools/perf_keyframe_clouds.py [--batch 16] [--reps 30] [--maps 64,1024]

Frames: a seeded synthetic room (a sloped floor of depths 0.8 .. 3.3 m with 4 cm of noise, 10 % holes), uint16 millimetres,
B, G, R images; voxel 0.05 m and max_range 2.0 m, the reference's defaults.  Times are HIP events around the call on
device-resident inputs, after warm-up calls, median and extremes over the repetitions; the events span the call's one host
wait.  The per-stage split comes from the events `cslam_cloud_profile` has the call record at its stage boundaries, in a
pass of its own.  Beside each figure, from the same run: `cslam_voxel_downsample_dev` (the lidar kernel) on the same
number of float64 points, the byte floor of every stage (the bytes it has to move, over 6.3 TB/s, the copy rate measured
on this GPU), and the numpy restatement of tests/cloud_reference.py on one core of the same box.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

STAGES = ("project / transform + bounds + meta", "host wait", "keys", "radix passes", "heads + scan", "segment sums", "clip")
HBM = 6.3e12                                               # bytes per second: the copy rate measured on an MI355X
CAMERA = (525.0, 525.0, 319.5, 239.5)
H, W = 480, 640


def room(seed):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    d = (800 + 2.5 * u + 1.8 * v + rng.integers(0, 40, (H, W))).astype(np.uint16)
    d[rng.random((H, W)) < 0.1] = 0
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), d


def timed(run, reps):
    import torch
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
    return np.array(ms)


def split(lib, _lib, run, reps):
    _lib.check(lib.cslam_cloud_profile(1))
    rows, info = [], (C.c_int32 * 4)()
    for _ in range(reps):
        run()
        got = (C.c_double * 7)()
        _lib.check(lib.cslam_cloud_profile_read(C.byref(got), C.byref(info)))
        rows.append(list(got))
    _lib.check(lib.cslam_cloud_profile(0))
    return np.median(np.array(rows), axis=0), list(info)


def floors(n, rows, passes, xyz, chain, clip):
    """Least bytes per stage: n input rows, `rows` output rows, xyz = bytes of a coordinate."""
    first = n * (2 + 3 + 3 * xyz + 4) if chain else n * (3 * 4 + 16 + 3 * xyz + 3 * xyz)      # project | transform (f32 in) + bounds
    return (first, 0, n * (3 * xyz + 8 + 4 + 2), passes * n * (12 + 12 + 12), n * (8 + 2 + 1 + 1 + 4), n * (4 + 3 * xyz + 4) + rows * (3 * xyz + 8),
            (rows * (3 * xyz + 1) + n + rows * 2 * (3 * xyz + 8)) if clip else 0)


def report(name, ms, med, info, fl, reps, per=1):
    print(f"{name}: events median {np.median(ms):.3f} ms, min {ms.min():.3f}, max {ms.max():.3f} over {reps} calls"
          f" = {np.median(ms) / per * 1e3:.1f} us per frame or keyframe")
    print(f"{name}: {info[0]} key passes + {info[1]} cloud-number passes of 8 bits ({info[2]} key bits, {info[3]} sort tiles); median per stage"
          " (byte floor): " + ", ".join(f"{s} {m * 1e3:.0f} us ({b / HBM * 1e6:.1f})" for s, m, b in zip(STAGES, med, fl))
          + f"; sum {med.sum() * 1e3:.0f} us, floor {sum(fl) / HBM * 1e6:.0f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--maps", default="64,1024")
    args = ap.parse_args()
    import torch
    import cloud_reference as ref
    from cslam_amd import _lib
    from cslam_amd.back_end import swarm_map
    from cslam_amd.front_end import keyframe_clouds as kc
    from cslam_amd.lidar_pr._batch import host, offsets, to_dev, upload

    _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    leaf, max_range = 0.05, 2.0
    frames = [room(k) for k in range(args.batch)]
    cam = np.repeat(np.array(CAMERA)[None], args.batch, axis=0)
    print(f"frames: {args.batch} of {H} x {W}, uint16 depth, B G R image; voxel {leaf} m, max_range {max_range} m")

    clouds = None
    for name, n in (("1 frame", 1), (f"{args.batch} frames", args.batch)):
        f = kc._Frames([x[0] for x in frames[:n]], [x[1] for x in frames[:n]], cam[:n], (kc.CLOUD_DEPTH_U16, 3), dev)
        t_out, lay = kc.result_buffer(n, f.b.total, 4, dev)

        def run():
            _lib.check(lib.cslam_cloud_keyframes_dev(*f.head(), leaf, max_range, *kc.result_args(t_out, lay), host(f.b.off), host(f.b.hw), st))
        ms = timed(run, args.reps)
        med, info = split(lib, _lib, run, args.reps)
        res, _ = kc.unpack_result(t_out.cpu().numpy(), lay, n, np.float32)
        rows = sum(len(r.points) for r in res)
        print(f"{name}: {f.b.total} pixels -> {rows} rows after the clip")
        report(name + ", cslam_cloud_keyframes_dev", ms, med, info, floors(f.b.total, rows, info[0] + info[1], 4, True, True), args.reps, n)
        clouds = res
        # the lidar kernel on the same number of float64 points: the finite rows of the organised clouds
        org = kc.create_colored_pointclouds([x[0] for x in frames[:n]], [x[1] for x in frames[:n]], cam[:n])
        dense = []
        for o in org:                                      # an invalid pixel takes the valid point before it: no voxel of its own
            valid = np.isfinite(o.points).all(axis=1)
            dense.append(o.points[np.maximum.accumulate(np.where(valid, np.arange(len(valid)), np.flatnonzero(valid)[0]))].astype(np.float64))
        cl = upload(dense, dev)
        out = torch.empty((f.b.total, 3), dtype=torch.float64, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)

        def run_lidar():
            _lib.check(lib.cslam_voxel_downsample_dev(cl.rows, cl.d_off, n, leaf, out.data_ptr(), out_off.data_ptr(), None, status.data_ptr(),
                                                      host(cl.off), st))
        ms = timed(run_lidar, args.reps)
        print(f"{name}: cslam_voxel_downsample_dev on the same {f.b.total} points as float64: median {np.median(ms):.3f} ms, min {ms.min():.3f}, "
              f"max {ms.max():.3f} -> {int(out_off.cpu()[-1])} voxels")
        t0 = time.perf_counter()
        for _ in range(3):
            got = kc.keyframe_clouds([x[0] for x in frames[:n]], [x[1] for x in frames[:n]], CAMERA, leaf, max_range)
        print(f"{name}: keyframe_clouds (host arrays in, results out) {(time.perf_counter() - t0) / 3 * 1e3:.2f} ms per call")
    t0 = time.perf_counter()
    want = ref.keyframe_cloud(frames[0][0], frames[0][1], CAMERA, leaf, max_range)
    t_ref = time.perf_counter() - t0
    assert all(np.array_equal(g, w) for g, w in zip(got[0], want)), "the GPU result differs from the restatement"
    print(f"numpy restatement (this box's CPU, one core): {t_ref * 1e3:.0f} ms per frame; GPU rows == restatement bit for bit on frame 0")

    # the map: the keyframe clouds above along a trajectory, one pose per keyframe
    for m in (int(x) for x in args.maps.split(",")):
        kfs = [clouds[k % len(clouds)] for k in range(m)]
        poses = np.zeros((m, 16))
        for k in range(m):
            T = np.identity(4)
            T[:3, :3] = ref.rotation((0.0, 1.0, 0.0), 0.05 * k)
            T[:3, 3] = (0.3 * k, 0.0, 0.02 * k)
            poses[k] = T.reshape(16)
        off = offsets([len(c.points) for c in kfs])
        total = int(off[-1])
        t_pts = to_dev(np.concatenate([c.points for c in kfs]), dev)
        t_rgb = to_dev(np.concatenate([kc.pack_colors(c.colors) for c in kfs]).view(np.int32), dev)
        t_off, t_T = to_dev(off, dev), to_dev(poses, dev)
        t_out, lay = kc.result_buffer(1, total, 8, dev)

        def run_map():
            _lib.check(lib.cslam_map_assemble_dev(t_pts.data_ptr(), _lib.F32, t_rgb.data_ptr(), t_off.data_ptr(), t_T.data_ptr(), m, 0.1,
                                                  *kc.result_args(t_out, lay), host(off), st))
        ms = timed(run_map, args.reps)
        med, info = split(lib, _lib, run_map, args.reps)
        res, _ = kc.unpack_result(t_out.cpu().numpy(), lay, 1, np.float64)
        name = f"map of {m} keyframes"
        print(f"{name}: {total} rows -> {len(res[0].points)} map rows at voxel 0.1 m")
        report(name + ", cslam_map_assemble_dev", ms, med, info, floors(total, len(res[0].points), info[0] + info[1], 8, False, False), args.reps, m)
        as_dict = dict(enumerate(kfs))
        pose_dict = {k: poses[k].reshape(4, 4) for k in range(m)}
        t0 = time.perf_counter()
        got = swarm_map.assemble_map(as_dict, pose_dict, 0.1)
        print(f"{name}: assemble_map (host arrays in, results out) {(time.perf_counter() - t0) * 1e3:.2f} ms")
        if m <= 64:
            t0 = time.perf_counter()
            want = ref.assemble_map([(c.points, c.colors) for c in kfs], [pose_dict[k] for k in range(m)], 0.1)
            t_ref = time.perf_counter() - t0
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the GPU map differs from the restatement"
            print(f"{name}: numpy restatement {t_ref * 1e3:.0f} ms; GPU map == restatement bit for bit")
        else:
            print(f"{name}: numpy restatement not measured at this size")


if __name__ == "__main__":
    main()
