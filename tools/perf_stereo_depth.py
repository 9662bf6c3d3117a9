#!/usr/bin/env python
"""Dense stereo depth and the stereo keyframe cloud on the GPU box: one 480 x 640 B, G, R pair and a batch of 16.

    python tools/perf_stereo_depth.py [--batch 16] [--reps 30] [--max-disparity 128]

Frames: a seeded block texture seen at a disparity that grows down the image in bands of 32 rows, 8 .. 64 pixels (7.9 m ..
0.98 m at fx 525 and a baseline of 0.12 m); voxel 0.05 m and max_range 2.0 m, the reference's defaults.  Times are HIP
events around the call on device-resident inputs, after warm-up calls, median and extremes over the repetitions.  From one
run:

  dense     `cslam_stereo_dense_dev` on the grey pair
  chain     `cslam_cloud_keyframes_stereo_dev`: grey of both sides, the dense kernel, the cloud chain with its one host wait
  rgbd      `cslam_cloud_keyframes_dev` on the same left images and the dense depth: what the chain adds to
  sparse    `cslam_feat_stereo_dev` with every pixel of every frame as a keypoint: the only route to the same depth without
            the dense kernel (one wave per pixel)

and the dense kernel's own floor: the bytes it has to move (two grey reads, 9 bytes written per pixel) over 6.3 TB/s, the
vector instructions it issues per (pixel, disparity) over the chip's 256 CUs x 64 lanes x 2.4 GHz, and beside them what it
moves through its per-pixel scratch (the back search's keys, rewritten once per pair of tiles by the row's own workgroup).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

HBM = 6.3e12                                               # bytes per second: the copy rate measured on an MI355X
LANE_OPS = 256 * 64 * 2.4e9                                # vector lane operations per second
# Instructions per (pixel, disparity) as issued, counted in the assembly hipcc -O3 makes of stereo_dense_kernel for gfx950
# (--save-temps; the three inner blocks): the unrolled walk of 46 columns is 215 vector instructions (46 of them v_dot4) and 75
# LDS instructions for 32 costs; the loop of the left book 22 vector + 1 LDS per cost; the loop of the back search, unrolled
# by two, 21 vector + 2 LDS per two costs.  Scalar instructions and waits (about 11 per cost) issue beside them.
VALU_PER_ENTRY = 215 / 32 + 22 + 21 / 2
LDS_PER_ENTRY = 75 / 32 + 1 + 1
T, TD = 256, 32                                            # csrc/stereo_dense.h: columns and disparities per tile
CAMERA = (525.0, 525.0, 319.5, 239.5, 0.12)
H, W = 480, 640


def pair(seed):
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 256, (H // 4, (W + 192) // 4, 3), dtype=np.uint8)
    tex = np.kron(cells, np.ones((4, 4, 1), np.uint8))
    left, right = np.empty((H, W, 3), np.uint8), np.empty((H, W, 3), np.uint8)
    for y0 in range(0, H, 32):
        d = 8 + (y0 // 32) * 4
        left[y0:y0 + 32] = tex[y0:y0 + 32, 64:64 + W]
        right[y0:y0 + 32] = tex[y0:y0 + 32, 64 + d:64 + d + W]
    return left, right


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


def line(name, what, ms, reps, n):
    print(f"{name}, {what}: events median {np.median(ms):.3f} ms, min {ms.min():.3f}, max {ms.max():.3f} over {reps} calls"
          f" = {np.median(ms) / n:.3f} ms per frame")
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--max-disparity", type=int, default=128)
    args = ap.parse_args()
    import torch
    import stereo_dense_reference as dref
    from cslam_amd import _lib
    from cslam_amd.front_end import keyframe_clouds as kc
    from cslam_amd.front_end import stereo_depth as sd
    from cslam_amd.lidar_pr._batch import host, offsets, to_dev

    _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    leaf, max_range = 0.05, 2.0
    params = (1, args.max_disparity, 15, 1)
    frames = [pair(k) for k in range(args.batch)]
    print(f"frames: {args.batch} pairs of {H} x {W}, B G R; disparities {params[0]} .. {params[1]}, uniqueness {params[2]}, lr_tolerance "
          f"{params[3]}; voxel {leaf} m, max_range {max_range} m")
    for name, n in (("1 frame", 1), (f"{args.batch} frames", args.batch)):
        cam = np.repeat(np.array(CAMERA)[None], n, axis=0)
        p = sd._Pairs([x[0] for x in frames[:n]], [x[1] for x in frames[:n]], cam, dev)
        b = p.b
        t_gl, t_gr = sd._gray(lib, p, p.t_left, p.t_lo, p.l_off), sd._gray(lib, p, p.t_right, p.t_ro, p.r_off)
        t_disp = torch.zeros(b.total, dtype=torch.float32, device=dev)
        t_depth = torch.zeros(b.total, dtype=torch.float32, device=dev)
        t_status = torch.zeros(b.total, dtype=torch.uint8, device=dev)

        def run_dense():
            _lib.check(lib.cslam_stereo_dense_dev(t_gl.data_ptr(), t_gr.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), n, p.t_cam.data_ptr(),
                                                  *params, t_disp.data_ptr(), t_status.data_ptr(), t_depth.data_ptr(), None, host(b.off),
                                                  host(b.hw), host(cam), st))
        t_dense = line(name, "dense (cslam_stereo_dense_dev)", timed(run_dense, args.reps), args.reps, n)
        status = t_status.cpu().numpy()
        entries = b.total * (params[1] + 2)
        pairs = n * H * -(-W // T) * ((params[1] + 1) // TD + 1)               # (column tile, disparity tile) pairs of all rows
        scratch = b.total * (4 + 2 + 2 + 4) + pairs * (T + TD - 1) * 8       # start values, d*, the last pass; keys read and written
        print(f"{name}: {b.total} pixels, accepted {float((status == 0).mean()):.3f}; floor of the dense kernel: {b.total * 11 / HBM * 1e6:.1f} us "
              f"of bytes, {entries * VALU_PER_ENTRY / LANE_OPS * 1e6:.0f} us of {VALU_PER_ENTRY:.1f} vector instructions per (pixel, disparity) "
              f"on {entries / 1e6:.1f} M of them (+ {LDS_PER_ENTRY:.1f} LDS instructions each); scratch traffic {scratch / 1e6:.1f} MB = "
              f"{scratch / b.total:.0f} bytes per pixel, {scratch / HBM * 1e6:.1f} us if none of it stayed in L2")

        t_out, lay = kc.result_buffer(n, b.total, 4, dev)

        def run_chain():
            _lib.check(lib.cslam_cloud_keyframes_stereo_dev(p.t_left.data_ptr(), p.t_lo.data_ptr(), 3, p.t_right.data_ptr(), p.t_ro.data_ptr(),
                                                            b.t_off.data_ptr(), b.t_hw.data_ptr(), p.t_cam.data_ptr(), n, *params, leaf, max_range,
                                                            *kc.result_args(t_out, lay), host(p.l_off), host(p.r_off), host(b.off), host(b.hw),
                                                            host(cam), st))
        line(name, "chain (cslam_cloud_keyframes_stereo_dev)", timed(run_chain, args.reps), args.reps, n)
        res, _ = kc.unpack_result(t_out.cpu().numpy(), lay, n, np.float32)
        print(f"{name}: {sum(len(r.points) for r in res)} cloud rows after the clip")

        t_cam4 = to_dev(cam[:, :4], dev)
        t_out2, lay2 = kc.result_buffer(n, b.total, 4, dev)

        def run_rgbd():
            _lib.check(lib.cslam_cloud_keyframes_dev(p.t_left.data_ptr(), 3, t_depth.data_ptr(), kc.CLOUD_DEPTH_F32, b.t_off.data_ptr(),
                                                     b.t_hw.data_ptr(), t_cam4.data_ptr(), n, leaf, max_range, *kc.result_args(t_out2, lay2),
                                                     host(b.off), host(b.hw), st))
        line(name, "rgbd (cslam_cloud_keyframes_dev on the dense depth)", timed(run_rgbd, args.reps), args.reps, n)
        assert t_out.cpu().numpy().tobytes() == t_out2.cpu().numpy().tobytes(), "the chain differs from the staged calls"

        kp = np.tile(dref.all_pixels(H, W), (n, 1))
        k_off = offsets([H * W] * n)
        t_kp, t_ko = to_dev(kp, dev), to_dev(k_off, dev)
        t_d64 = torch.zeros(b.total, dtype=torch.float64, device=dev)
        t_s32 = torch.zeros(b.total, dtype=torch.int32, device=dev)
        t_best = torch.zeros((b.total, 4), dtype=torch.int32, device=dev)
        t_pts = torch.zeros((b.total, 3), dtype=torch.float64, device=dev)

        def run_sparse():
            _lib.check(lib.cslam_feat_stereo_dev(t_gl.data_ptr(), t_gr.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), n, t_kp.data_ptr(),
                                                 t_ko.data_ptr(), p.t_cam.data_ptr(), *params, t_d64.data_ptr(), t_s32.data_ptr(),
                                                 t_best.data_ptr(), t_pts.data_ptr(), host(b.off), host(b.hw), host(k_off), host(cam), st))
        t_sparse = line(name, f"sparse (cslam_feat_stereo_dev, {H * W} keypoints per frame)", timed(run_sparse, args.reps), args.reps, n)
        assert np.array_equal(t_s32.cpu().numpy().astype(np.uint8), status), "the dense status differs from the sparse kernel's"
        assert np.array_equal(t_pts.cpu().numpy()[:, 2].astype(np.float32), t_depth.cpu().numpy(), equal_nan=True), \
            "the dense depth differs from the sparse kernel's"
        print(f"{name}: dense == sparse at every pixel (status and depth); dense is {t_sparse / t_dense:.1f} x faster")


if __name__ == "__main__":
    main()
