"""Chained transform vs output + input transform, per boundary class of the VGG-16 trunk at the 256-frame chunk (MI355X), interleaved:
   pair   cslam_wino4_output_scaled_dev (ReLU, max |y|) + cslam_wino4_input_h2_dev        M -> y -> V2
   chain  cslam_wino4_chain_h2_dev (csrc/wino_chain.hip)                                   M -> V2, y in LDS
The classes are the map sizes between two unpooled Winograd layers: 56 x 56 x 256 (conv3_x), 28 x 28 x 512 (conv4_x), 14 x 14 x 512
(conv5_x).  Bytes: 144 (M) + 144 (V2) per tile and channel for both, + 128 for y in the pair form.
    python tools/perf_wino_chain.py [--frames 256] [--reps 30]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cslam_amd import _lib                                                                  # noqa: E402


def p(t):
    return C.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    st = torch.cuda.current_stream().cuda_stream
    B = a.frames
    for hw, c in ((56, 256), (28, 512), (14, 512)):
        tiles = B * (-(-hw // 4)) ** 2
        M = torch.randn(36 * tiles * c, device="cuda")
        V2 = torch.empty(36 * tiles * c, device="cuda")
        y = torch.empty((B, hw, hw, c), device="cuda")
        bias = torch.randn(c, device="cuda") * 0.1
        ax = torch.full((1,), 1.0, device="cuda")
        ay, bound = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")

        def pair():
            ay.zero_()
            _lib.check(lib.cslam_wino4_output_scaled_dev(p(M), p(bias), None, B, hw, hw, c, 1, 0, p(ax), 1.0, p(ay), p(y), st))
            _lib.check(lib.cslam_wino4_input_h2_dev(p(y), B, hw, hw, c, p(ay), p(V2), st))

        def chain():
            ay.zero_()
            _lib.check(lib.cslam_wino4_chain_h2_dev(p(M), p(bias), B, hw, hw, c, p(ax), 1.0, p(ax), 300.0, 0.5, p(ay), p(bound), p(V2), st))

        times = {"pair": [], "chain": []}
        for fn in (pair, chain, pair, chain):                                               # warm-up
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in (("pair", pair), ("chain", chain)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        tc = tiles * c
        out = {"map": hw, "channels": c, "frames": B}
        for name, extra in (("pair", 128), ("chain", 0)):
            med = statistics.median(times[name])
            out[name + "_ms"] = round(med, 4)
            out[name + "_min_ms"] = round(min(times[name]), 4)
            out[name + "_max_ms"] = round(max(times[name]), 4)
            out[name + "_TBps"] = round(tc * (288 + extra) / med / 1e9, 2)
        out["chain_over_pair"] = round(out["chain_ms"] / out["pair_ms"], 3)
        print(json.dumps(out), flush=True)
        del M, V2, y


if __name__ == "__main__":
    main()
