#!/usr/bin/env python
"""Rectification on the GPU box: the map of one 480 x 640 camera, the remap of one B, G, R frame and of a batch of 16, the
nearest remap of uint16 depth, and what rectifying in front of the stereo keyframe chain and the stereo cloud chain costs.

    python tools/perf_rectify.py [--batch 16] [--reps 30] [--timeout 240]

Every step runs in a fresh child process (`--step NAME`) under its own time limit; the first one that fails or runs out of
time ends the run.  Times are HIP events around the calls on device-resident inputs and preallocated outputs, after
warm-up calls, median and extremes over the repetitions.

  map        `cslam_rectify_map_dev`, one camera.  Floor: 8 bytes written per pixel.
  remap      `cslam_rectify_remap_dev`, frames sharing one map.  Floor per destination pixel: 8 bytes of map, C of source
             (read once), C written, 1 of validity = 9 + 2 C.
  nearest    `cslam_rectify_nearest_dev`, uint16: 8 + 2 + 2 bytes.
  keyframes  `cslam_feat_extract_stereo_dev` on the frames as they are, and behind two remaps (both sides) in the same run
  clouds     `cslam_cloud_keyframes_stereo_dev` likewise

The frames are the pairs of tools/perf_stereo_depth.py, taken as what a mildly distorted, slightly rotated camera gave; the
rectified chain therefore sees other pixels than the plain one, and the difference of the two times is the cost of the
remaps plus whatever the other content does to the chain.  The floors are bytes over 6.3 TB/s.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.3e12
H, W = 480, 640
STEPS = ("map", "remap", "nearest", "keyframes", "clouds")
P = (525.0, 525.0, 319.5, 239.5)
BASELINE = 0.12


def cameras():
    from cslam_amd.front_end import rectify as rc

    def rot(w):
        w = np.asarray(w, dtype=np.float64)
        t = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        return np.identity(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * (K @ K)

    left = rc.RawCamera((520.0, 522.0, 322.0, 238.0), (-0.28, 0.09, 0.0005, -0.0003, -0.01), rot([0.004, -0.006, 0.008]), P, (H, W))
    right = rc.RawCamera((521.0, 521.5, 318.0, 241.0), (-0.27, 0.085, -0.0004, 0.0006, -0.008), rot([-0.003, 0.005, -0.007]),
                         P + (-BASELINE * P[0],), (H, W))
    return left, right


def line(name, ms, n, floor_bytes=None):
    med = float(np.median(ms))
    tail = ""
    if floor_bytes is not None:
        floor_us = floor_bytes / HBM * 1e6
        tail = f"; floor {floor_bytes / 1e6:.1f} MB = {floor_us:.1f} us, measured is {med * 1e3 / floor_us:.1f} x the floor"
    print(f"{name}: events median {med:.3f} ms, min {ms.min():.3f}, max {ms.max():.3f} over {len(ms)} calls = {med / n:.3f} ms per frame{tail}",
          flush=True)
    return med


def step(name, batch, reps):
    import torch
    from perf_stereo_depth import pair, timed
    from cslam_amd import _lib
    from cslam_amd.front_end import rectify as rc
    from cslam_amd.front_end import keyframe_clouds as kc
    from cslam_amd.front_end.visual_features import FEAT_DESC_BYTES
    from cslam_amd.lidar_pr._batch import host, to_dev

    _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    left, right = cameras()
    maps = rc.rectify_maps([left, right])

    class Remap:
        """One `cslam_rectify_remap_dev` with everything allocated before."""

        def __init__(self, arrays, index):
            self.s = rc._Sources(arrays, maps, np.asarray(index, dtype=np.int32), dev)
            self.t_dst, self.dst_off, self.t_do, self.t_valid = rc._remap(lib, self.s)

        def __call__(self):
            s, b = self.s, self.s.b
            _lib.check(lib.cslam_rectify_remap_dev(s.t_src.data_ptr(), s.t_so.data_ptr(), s.t_shw.data_ptr(), *s.map_args(), b.t_off.data_ptr(),
                                                   b.t_hw.data_ptr(), b.n, self.t_dst.data_ptr(), self.t_do.data_ptr(), self.t_valid.data_ptr(),
                                                   *s.host_args(), host(self.dst_off), st))

    if name == "map":
        one = rc.rectify_maps([left])
        t_cam = to_dev(left.values[None], dev)
        values = np.ascontiguousarray(left.values[None])

        def run():
            _lib.check(lib.cslam_rectify_map_dev(t_cam.data_ptr(), one.t_off.data_ptr(), one.t_hw.data_ptr(), 1, one.t_map.data_ptr(), host(one.off),
                                                 host(one.hw), host(values), st))
        line("map, 1 camera (cslam_rectify_map_dev)", timed(run, reps), 1, H * W * 8)
        q = one.numpy()[0]
        print(f"map: {float((q[..., 0] != -2 ** 31).mean()):.3f} of the pixels have a source position", flush=True)
        return
    frames = [pair(k) for k in range(batch)]
    if name == "remap":
        for n in (1, batch):
            for C, imgs in ((3, [f[0] for f in frames[:n]]), (1, [np.ascontiguousarray(f[0][..., 1]) for f in frames[:n]])):
                r = Remap(imgs, [0] * n)
                line(f"remap, {n} frame(s) of {C} channel(s) (cslam_rectify_remap_dev)", timed(r, reps), n, n * H * W * (9 + 2 * C))
                print(f"remap: valid {float(r.t_valid.float().mean()):.3f}", flush=True)
        return
    if name == "nearest":
        rng = np.random.default_rng(0)
        for n in (1, batch):
            s = rc._Sources([rng.integers(400, 5000, (H, W)).astype(np.int16) for _ in range(n)], maps, np.zeros(n, dtype=np.int32), dev)
            t_dst = rc._nearest(lib, s, rc.RECTIFY_U16)

            def run():
                _lib.check(lib.cslam_rectify_nearest_dev(s.t_src.data_ptr(), rc.RECTIFY_U16, s.t_so.data_ptr(), s.t_shw.data_ptr(), *s.map_args(),
                                                         s.b.t_off.data_ptr(), s.b.t_hw.data_ptr(), n, None, t_dst.data_ptr(), *s.host_args(), st))
            line(f"nearest, {n} frame(s) of uint16 (cslam_rectify_nearest_dev)", timed(run, reps), n, n * H * W * 12)
        return
    cam1 = np.array(rc.stereo_camera(left, right))
    for n in (1, batch):
        cam = np.repeat(cam1[None], n, axis=0)
        t_cam = to_dev(cam, dev)
        rl, rr = Remap([f[0] for f in frames[:n]], [0] * n), Remap([f[1] for f in frames[:n]], [1] * n)
        b = rl.s.b
        if name == "keyframes":
            mf = 1000
            t_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
            t_kp, t_resp = torch.zeros((n, mf, 2), dtype=torch.int32, device=dev), torch.zeros((n, mf), dtype=torch.int32, device=dev)
            t_bins, t_desc = torch.zeros((n, mf), dtype=torch.int32, device=dev), torch.zeros((n, mf, FEAT_DESC_BYTES), dtype=torch.uint8, device=dev)
            t_pts, t_disp = torch.zeros((n, mf, 3), dtype=torch.float64, device=dev), torch.zeros((n, mf), dtype=torch.float64, device=dev)
            t_status = torch.zeros((n, mf), dtype=torch.int32, device=dev)

            def chain(t_l, t_lo, l_off, t_r, t_ro, r_off):
                _lib.check(lib.cslam_feat_extract_stereo_dev(t_l.data_ptr(), t_lo.data_ptr(), t_r.data_ptr(), t_ro.data_ptr(), b.t_off.data_ptr(),
                                                             b.t_hw.data_ptr(), t_cam.data_ptr(), n, 0.001, 7, 19, mf, 1, 128, 15, 1, t_cnt.data_ptr(),
                                                             t_kp.data_ptr(), t_resp.data_ptr(), t_bins.data_ptr(), t_desc.data_ptr(), t_pts.data_ptr(),
                                                             t_disp.data_ptr(), t_status.data_ptr(), host(l_off), host(r_off), host(b.off), host(b.hw),
                                                             host(cam), st))
            what = "stereo keyframes (cslam_feat_extract_stereo_dev)"
        else:
            t_out, lay = kc.result_buffer(n, b.total, 4, dev)

            def chain(t_l, t_lo, l_off, t_r, t_ro, r_off):
                _lib.check(lib.cslam_cloud_keyframes_stereo_dev(t_l.data_ptr(), t_lo.data_ptr(), 3, t_r.data_ptr(), t_ro.data_ptr(), b.t_off.data_ptr(),
                                                                b.t_hw.data_ptr(), t_cam.data_ptr(), n, 1, 128, 15, 1, 0.05, 2.0,
                                                                *kc.result_args(t_out, lay), host(l_off), host(r_off), host(b.off), host(b.hw), host(cam),
                                                                st))
            what = "stereo clouds (cslam_cloud_keyframes_stereo_dev)"

        def plain():
            chain(rl.s.t_src, rl.s.t_so, rl.s.src_off, rr.s.t_src, rr.s.t_so, rr.s.src_off)

        def rectified():
            rl()
            rr()
            chain(rl.t_dst, rl.t_do, rl.dst_off, rr.t_dst, rr.t_do, rr.dst_off)
        t0 = line(f"{n} frame(s), {what} on the frames as they are", timed(plain, reps), n)
        t1 = line(f"{n} frame(s), two remaps + {what}", timed(rectified, reps), n)
        print(f"{n} frame(s): rectification adds {t1 - t0:.3f} ms = {(t1 - t0) / n:.3f} ms per pair to {t0 / n:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--step", choices=STEPS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.batch, args.reps)
        return 0
    print(f"frames: {H} x {W}, batch {args.batch}; one map per side, shared by the frames; floors at {HBM / 1e12:.1f} TB/s", flush=True)
    for name in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--batch", str(args.batch), "--reps", str(args.reps)],
                               timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"step {name} ran out of its {args.timeout} s: stopping", flush=True)
            return 124
        if r.returncode != 0:
            print(f"step {name} failed with {r.returncode}: stopping", flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
