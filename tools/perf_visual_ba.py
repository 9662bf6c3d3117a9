"""Times of the two-view bundle adjustment after PnP (csrc/vis_ba.hip) by HIP events around device-resident calls, in the
manner of tools/perf_visual_registration.py: the same pair at 1000 keypoints per keyframe, batches of 1, 16 and 64 such
pairs.  In one run: the match -> PnP chain as it was before the adjustment existed (`cslam_vis_register_dev`: the yardstick),
the chain with the adjustment (`cslam_vis_register_ba_dev`), and the adjustment kernel alone on the PnP result
(`cslam_vis_ba_dev`); medians of `--reps`.  The cost of the adjustment is reported as a fraction of the PnP chain.
Prints one JSON line.

    python tools/perf_visual_ba.py [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--baseline", type=float, default=0.1)
    args = ap.parse_args()
    import torch
    import vis_reference as ref
    from cslam_amd import _lib
    from cslam_amd.lidar_pr._batch import host, offsets, stream, to_dev
    _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n_land = args.keypoints * 3 // 4
    out = {"keypoints": args.keypoints, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for batch in (1, 16, 64):
        kfs = [ref.keyframe_pair(s, landmarks=n_land, distractors=args.keypoints - n_land)[:2] for s in range(min(batch, 4))]
        kfs = [kfs[k % len(kfs)] for k in range(batch)]
        a_off = offsets([len(a[0]) for a, _ in kfs])
        b_off = offsets([len(b[0]) for _, b in kfs])
        total = int(a_off[-1])
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dtype=dt)
        t_da, t_db = to_dev(cat([a[2] for a, _ in kfs], np.uint8), dev), to_dev(cat([b[2] for _, b in kfs], np.uint8), dev)
        t_kpa, t_pta = to_dev(cat([a[0] for a, _ in kfs], np.float64), dev), to_dev(cat([a[1] for a, _ in kfs], np.float64), dev)
        t_kpb, t_ptb = to_dev(cat([b[0] for _, b in kfs], np.float64), dev), to_dev(cat([b[1] for _, b in kfs], np.float64), dev)
        base = np.full((batch, 2), args.baseline)
        t_ao, t_bo, t_cam, t_base = to_dev(a_off, dev), to_dev(b_off, dev), to_dev(np.tile(ref.CAM, (batch, 1)), dev), to_dev(base, dev)
        t_rows = torch.zeros((total, 2), dtype=torch.int32, device=dev)
        t_cnt = torch.zeros(batch, dtype=torch.int32, device=dev)
        new = lambda: (torch.zeros((batch, 16), dtype=torch.float64, device=dev), torch.zeros((batch, 8), dtype=torch.int32, device=dev),
                       torch.zeros(total, dtype=torch.int32, device=dev))
        (t_T0, t_i0, t_f0), (t_T, t_info, t_flags) = new(), new()
        t_pts = torch.zeros((total, 3), dtype=torch.float64, device=dev)
        t_cost = torch.zeros((batch, 2), dtype=torch.float64, device=dev)

        def chain():                                        # the parent's chain: match -> PnP
            _lib.check(lib.cslam_vis_register_dev(t_da.data_ptr(), t_pta.data_ptr(), t_ao.data_ptr(), t_db.data_ptr(), t_kpb.data_ptr(),
                                                  t_bo.data_ptr(), t_cam.data_ptr(), batch, 32, 0.8, 300, 2.0, 20, 10, 2, 0,
                                                  t_rows.data_ptr(), t_cnt.data_ptr(), t_T0.data_ptr(), t_i0.data_ptr(), t_f0.data_ptr(),
                                                  host(a_off), host(b_off), stream()))

        def chain_ba():                                     # match -> PnP -> adjustment
            _lib.check(lib.cslam_vis_register_ba_dev(t_da.data_ptr(), t_kpa.data_ptr(), t_pta.data_ptr(), t_ao.data_ptr(), t_db.data_ptr(),
                                                     t_kpb.data_ptr(), t_ptb.data_ptr(), t_bo.data_ptr(), None, None, t_cam.data_ptr(),
                                                     t_cam.data_ptr(), t_base.data_ptr(), batch, 32, 0.8, 300, 2.0, 20, 10, 2, 0, 10, 2,
                                                     t_rows.data_ptr(), t_cnt.data_ptr(), t_T0.data_ptr(), t_i0.data_ptr(), t_f0.data_ptr(),
                                                     t_T.data_ptr(), t_info.data_ptr(), t_flags.data_ptr(), t_pts.data_ptr(), t_cost.data_ptr(),
                                                     host(a_off), host(b_off), None, None, host(base), stream()))

        def adjust():                                       # the adjustment kernel alone, on what the chain left
            _lib.check(lib.cslam_vis_ba_dev(t_kpa.data_ptr(), t_pta.data_ptr(), t_ao.data_ptr(), t_kpb.data_ptr(), t_ptb.data_ptr(),
                                            t_bo.data_ptr(), None, None, t_cam.data_ptr(), t_cam.data_ptr(), t_base.data_ptr(),
                                            t_rows.data_ptr(), t_ao.data_ptr(), t_cnt.data_ptr(), t_T0.data_ptr(), t_i0.data_ptr(),
                                            t_f0.data_ptr(), batch, 2.0, 20, 10, 2, t_T.data_ptr(), t_info.data_ptr(), t_flags.data_ptr(),
                                            t_pts.data_ptr(), t_cost.data_ptr(), host(a_off), host(b_off), host(a_off), None, None, host(base),
                                            stream()))

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return round(float(np.median(ms)), 4)

        # alternate the two chains so that a drift of the machine shows in both
        res = {"chain_ms": timed(chain), "chain_ba_ms": timed(chain_ba), "chain_again_ms": timed(chain), "chain_ba_again_ms": timed(chain_ba),
               "ba_alone_ms": timed(adjust)}
        info = t_info.cpu().numpy()
        res["ba_over_chain"] = round((res["chain_ba_ms"] - res["chain_ms"]) / res["chain_ms"], 3)
        res["ba_alone_over_chain"] = round(res["ba_alone_ms"] / res["chain_ms"], 3)
        res["accepted"] = int((info[:, 0] == 0).sum())
        res["set_in"] = round(float(info[:, 1].mean()), 1)
        res["set_out"] = round(float(info[:, 2].mean()), 1)
        res["steps"] = round(float(info[:, 3].mean()), 1)
        res["matches_per_pair"] = round(float(t_cnt.cpu().numpy().mean()), 1)
        out["batch_%d" % batch] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
