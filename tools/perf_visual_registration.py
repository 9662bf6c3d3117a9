"""Times of the visual verification (csrc/vis.hip) by HIP events: one pair at 1000 keypoints per keyframe, batches of 16 and
64 such pairs, the matcher and the PnP RANSAC apart and chained; beside them, in the same run, the level-aware PnP and its
chain with a level of 0 .. 3 drawn per "to" keypoint.  Prints one JSON line.

    python tools/perf_visual_registration.py [--reps 30]
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
    args = ap.parse_args()
    import torch
    import vis_reference as ref
    from cslam_amd import _lib
    from cslam_amd.front_end import visual_registration as vr
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
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dtype=dt)
        t_da, t_db = to_dev(cat([a[2] for a, _ in kfs], np.uint8), dev), to_dev(cat([b[2] for _, b in kfs], np.uint8), dev)
        t_pts, t_pix = to_dev(cat([a[1] for a, _ in kfs], np.float64), dev), to_dev(cat([b[0] for _, b in kfs], np.float64), dev)
        t_ao, t_bo, t_cam = to_dev(a_off, dev), to_dev(b_off, dev), to_dev(np.tile(ref.CAM, (batch, 1)), dev)
        t_rows = torch.zeros((int(a_off[-1]), 2), dtype=torch.int32, device=dev)
        t_cnt = torch.zeros(batch, dtype=torch.int32, device=dev)
        t_T = torch.zeros((batch, 16), dtype=torch.float64, device=dev)
        t_info = torch.zeros((batch, 8), dtype=torch.int32, device=dev)
        t_flags = torch.zeros(int(a_off[-1]), dtype=torch.int32, device=dev)
        lvl = np.random.default_rng(batch).integers(0, 4, int(b_off[-1])).astype(np.int32)
        t_lvl = to_dev(lvl, dev)

        def match():
            _lib.check(lib.cslam_vis_match_dev(t_da.data_ptr(), t_ao.data_ptr(), t_db.data_ptr(), t_bo.data_ptr(), batch, 32, 0.8,
                                               t_rows.data_ptr(), t_cnt.data_ptr(), host(a_off), host(b_off), stream()))

        def pnp():
            _lib.check(lib.cslam_vis_pnp_dev(t_pts.data_ptr(), t_ao.data_ptr(), t_pix.data_ptr(), t_bo.data_ptr(), t_rows.data_ptr(),
                                             t_ao.data_ptr(), t_cnt.data_ptr(), t_cam.data_ptr(), batch, 300, 2.0, 20, 10, 2, 0,
                                             t_T.data_ptr(), t_info.data_ptr(), t_flags.data_ptr(), stream()))

        def chain():
            _lib.check(lib.cslam_vis_register_dev(t_da.data_ptr(), t_pts.data_ptr(), t_ao.data_ptr(), t_db.data_ptr(), t_pix.data_ptr(),
                                                  t_bo.data_ptr(), t_cam.data_ptr(), batch, 32, 0.8, 300, 2.0, 20, 10, 2, 0,
                                                  t_rows.data_ptr(), t_cnt.data_ptr(), t_T.data_ptr(), t_info.data_ptr(),
                                                  t_flags.data_ptr(), host(a_off), host(b_off), stream()))

        def pnp_levels():
            _lib.check(lib.cslam_vis_pnp_levels_dev(t_pts.data_ptr(), t_ao.data_ptr(), t_pix.data_ptr(), t_bo.data_ptr(), t_lvl.data_ptr(),
                                                    t_rows.data_ptr(), t_ao.data_ptr(), t_cnt.data_ptr(), t_cam.data_ptr(), batch, 300, 2.0, 20,
                                                    10, 2, 0, t_T.data_ptr(), t_info.data_ptr(), t_flags.data_ptr(), host(b_off), host(lvl),
                                                    stream()))

        def chain_levels():
            _lib.check(lib.cslam_vis_register_levels_dev(t_da.data_ptr(), t_pts.data_ptr(), t_ao.data_ptr(), t_db.data_ptr(), t_pix.data_ptr(),
                                                         t_bo.data_ptr(), t_lvl.data_ptr(), t_cam.data_ptr(), batch, 32, 0.8, 300, 2.0, 20, 10, 2,
                                                         0, t_rows.data_ptr(), t_cnt.data_ptr(), t_T.data_ptr(), t_info.data_ptr(),
                                                         t_flags.data_ptr(), host(a_off), host(b_off), host(lvl), stream()))

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

        res = {"match_ms": timed(match), "pnp_ms": timed(pnp), "chain_ms": timed(chain)}
        info = t_info.cpu().numpy()
        res["accepted"] = int((info[:, 0] == 0).sum())
        res.update({"pnp_levels_ms": timed(pnp_levels), "chain_levels_ms": timed(chain_levels)})
        res["accepted_levels"] = int((t_info.cpu().numpy()[:, 0] == 0).sum())
        res["matches_per_pair"] = round(float(t_cnt.cpu().numpy().mean()), 1)
        out["batch_%d" % batch] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
