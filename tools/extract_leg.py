#!/usr/bin/env python
"""The extract leg alone (NetVLAD VGG-16, chunks of 256 resident frames) for rocprofv3 runs:
2 warm-up passes (MIOpen find mode, workspace growth), then `--iters` steady-state passes.  Every pass
starts with `preprocess_fused_kernel`, which tools/kernel_trace_summary.py uses to cut the trace."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cslam_amd.vpr.netvlad import NetVLAD

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=4)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--backbone-conv", default="winograd")
ap.add_argument("--copy-peak", action="store_true", help="print this run's own streaming-copy rate first (bench.py's peaks_measured.hbm_copy_GBs)")
a = ap.parse_args()
torch.backends.cudnn.benchmark = True
nv = NetVLAD({"frontend.nn_checkpoint": "random", "frontend.image_crop_size": 376, "frontend.netvlad.pca_dim": 4096,
              "frontend.backbone_conv": a.backbone_conv}, None)
fr = torch.randint(0, 256, (a.batch, 480, 640, 3), device="cuda", dtype=torch.uint8)
import time
if a.copy_peak:
    import ctypes as C
    from cslam_amd import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nbytes = 2 << 30                                          # 2 GiB each way: well past the 256 MB Infinity Cache
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    best = 0.0
    for variant in (0, 1, 2):
        for rep in range(3):
            e0.record()
            for _ in range(3):
                _lib.check(lib.cslam_peak_copy_dev(src.data_ptr(), dst.data_ptr(), nbytes, variant, st))
            e1.record()
            torch.cuda.synchronize()
            if rep:                                           # first round of every variant warms up
                best = max(best, 3 * 2.0 * nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    del src, dst
    print("hbm_copy_GBs: %.1f" % best)
for _ in range(2):
    nv.compute_embeddings_device(fr)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.iters):
    nv.compute_embeddings_device(fr)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.iters
print("extract leg: %.2f ms per %d frames = %.0f frames/s" % (dt * 1e3, a.batch, a.batch / dt))
