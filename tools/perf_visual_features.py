"""Times of the keyframe features (csrc/feat.hip) by HIP events: one 480 x 640 BGR frame and a batch of 16, each stage
apart (grey, response, selection, bins and descriptors, points) and the whole chain; then the stereo leg on the same
frames with a right image 12 columns apart: the stereo kernel alone on the selected keypoints and the chained stereo
frame.  Then, in the same run, the scale pyramid (front_end/visual_pyramid.py) at 1, 4 and 8 levels on the same frames: the
chain, the stereo chain, and its stages apart (level images with the validity maps; response, selection with the largest
level budget, bins and descriptors on the n L level images through the single-scale entries), and beside each chain its
sub-pixel form and the staged sub-pixel offsets of the selected level keypoints.  Prints one JSON line.

    python tools/perf_visual_features.py [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def frame(seed, H, W):
    """Random grey blocks of 6 .. 12 pixels, smoothed once, in three channels: some thousand corner candidates."""
    rng = np.random.default_rng(seed)
    b = 6 + seed % 7
    cells = rng.integers(0, 256, size=((H + b - 1) // b, (W + b - 1) // b)).astype(np.float32)
    g = np.kron(cells, np.ones((b, b), dtype=np.float32))[:H, :W]
    g = (g + np.roll(g, 1, axis=0) + np.roll(g, 1, axis=1) + np.roll(g, (1, 1), axis=(0, 1))) / 4 + rng.normal(0.0, 2.0, (H, W))
    g = np.clip(np.round(g), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, np.roll(g, 1, axis=1), np.roll(g, 1, axis=0)], axis=2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--max-features", type=int, default=1000)
    args = ap.parse_args()
    import torch
    from cslam_amd import _lib
    from cslam_amd.lidar_pr._batch import host, offsets, stream, to_dev
    _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    H, W, mf = args.height, args.width, args.max_features
    out = {"height": H, "width": W, "max_features": mf, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for batch in (1, 16):
        imgs = [frame(s, H, W) for s in range(min(batch, 4))]
        imgs = [imgs[k % len(imgs)] for k in range(batch)]
        rng = np.random.default_rng(0)
        depth = (1.0 + 4.0 * rng.random((batch, H, W))).astype(np.float32)
        depth[:, :, W // 3:W // 3 + 20] = 0.0
        off, src_off = offsets([H * W] * batch), offsets([3 * H * W] * batch)
        hw = np.tile(np.array([[H, W]], dtype=np.int32), (batch, 1))
        t_src, t_depth = to_dev(np.concatenate([i.reshape(-1) for i in imgs]), dev), to_dev(depth.reshape(-1), dev)
        t_off, t_so, t_hw = to_dev(off, dev), to_dev(src_off, dev), to_dev(hw, dev)
        t_cam = to_dev(np.tile(np.array([525.0, 525.0, W / 2 - 0.5, H / 2 - 0.5]), (batch, 1)), dev)
        total = batch * H * W
        t_gray = torch.zeros(total, dtype=torch.uint8, device=dev)
        t_R = torch.zeros(total, dtype=torch.int32, device=dev)
        t_max = torch.zeros(batch, dtype=torch.int32, device=dev)
        t_valid = (t_depth > 0).to(torch.uint8)
        t_cnt = torch.zeros(batch, dtype=torch.int32, device=dev)
        t_kp = torch.zeros((batch, mf, 2), dtype=torch.int32, device=dev)
        t_resp = torch.zeros((batch, mf), dtype=torch.int32, device=dev)
        t_bins = torch.zeros((batch, mf), dtype=torch.int32, device=dev)
        t_desc = torch.zeros((batch, mf, 32), dtype=torch.uint8, device=dev)
        t_pts = torch.zeros((batch, mf, 3), dtype=torch.float64, device=dev)
        k_off = offsets([mf] * batch)                      # the staged entries take the rows as ragged: here all mf per image
        t_ko = to_dev(k_off, dev)
        h = (host(off), host(hw))
        # the stereo leg: the right image is the left one seen 12 columns further left (disparity 12 everywhere)
        rights = [np.ascontiguousarray(np.roll(i, -12, axis=1)) for i in imgs]
        t_right = to_dev(np.concatenate([i.reshape(-1) for i in rights]), dev)
        t_gray_r = torch.zeros(total, dtype=torch.uint8, device=dev)
        scam = np.tile(np.array([525.0, 525.0, W / 2 - 0.5, H / 2 - 0.5, 0.12]), (batch, 1))
        t_scam = to_dev(scam, dev)
        t_disp = torch.zeros((batch, mf), dtype=torch.float64, device=dev)
        t_status = torch.zeros((batch, mf), dtype=torch.int32, device=dev)
        t_best = torch.zeros((batch, mf, 4), dtype=torch.int32, device=dev)

        def gray():
            _lib.check(lib.cslam_feat_gray_dev(t_src.data_ptr(), t_so.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch, t_gray.data_ptr(),
                                               host(src_off), *h, stream()))

        def response():
            _lib.check(lib.cslam_feat_response_dev(t_gray.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch, t_R.data_ptr(), t_max.data_ptr(),
                                                   *h, stream()))

        def select():
            _lib.check(lib.cslam_feat_select_dev(t_R.data_ptr(), t_max.data_ptr(), t_valid.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch,
                                                 0.001, 7, 19, mf, t_cnt.data_ptr(), t_kp.data_ptr(), t_resp.data_ptr(), *h, stream()))

        def describe():
            _lib.check(lib.cslam_feat_describe_dev(t_gray.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch, t_kp.data_ptr(), t_ko.data_ptr(),
                                                   t_bins.data_ptr(), t_desc.data_ptr(), *h, host(k_off), stream()))

        def points():
            _lib.check(lib.cslam_feat_points_dev(t_depth.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch, t_kp.data_ptr(), t_ko.data_ptr(),
                                                 t_cam.data_ptr(), t_pts.data_ptr(), *h, host(k_off), stream()))

        def chain():
            _lib.check(lib.cslam_feat_extract_dev(t_src.data_ptr(), t_so.data_ptr(), t_depth.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(),
                                                  t_cam.data_ptr(), batch, 0.001, 7, 19, mf, 1, t_cnt.data_ptr(), t_kp.data_ptr(),
                                                  t_resp.data_ptr(), t_bins.data_ptr(), t_desc.data_ptr(), t_pts.data_ptr(), host(src_off), *h,
                                                  stream()))

        def gray_right():
            _lib.check(lib.cslam_feat_gray_dev(t_right.data_ptr(), t_so.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch,
                                               t_gray_r.data_ptr(), host(src_off), *h, stream()))

        def stereo():
            _lib.check(lib.cslam_feat_stereo_dev(t_gray.data_ptr(), t_gray_r.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch,
                                                 t_kp.data_ptr(), t_ko.data_ptr(), t_scam.data_ptr(), 1, 128, 15, 1, t_disp.data_ptr(),
                                                 t_status.data_ptr(), t_best.data_ptr(), t_pts.data_ptr(), *h, host(k_off), host(scam),
                                                 stream()))

        def stereo_chain():
            _lib.check(lib.cslam_feat_extract_stereo_dev(t_src.data_ptr(), t_so.data_ptr(), t_right.data_ptr(), t_so.data_ptr(),
                                                         t_off.data_ptr(), t_hw.data_ptr(), t_scam.data_ptr(), batch, 0.001, 7, 19, mf, 1, 128,
                                                         15, 1, t_cnt.data_ptr(), t_kp.data_ptr(), t_resp.data_ptr(), t_bins.data_ptr(),
                                                         t_desc.data_ptr(), t_pts.data_ptr(), t_disp.data_ptr(), t_status.data_ptr(),
                                                         host(src_off), host(src_off), *h, host(scam), stream()))

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

        def pyramid(L):
            """The pyramid chain at L levels and its stages; the staged entries take the level images packed without padding."""
            from cslam_amd.front_end import visual_pyramid as vp
            lv = vp._Levels([vp.level_sizes((H, W), L)] * batch, dev)
            nl, b0 = batch * L, vp.level_budgets(mf, L)[0]
            hl = (host(lv.off), host(lv.hw))
            z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
            p_cnt, p_kp, p_lkp, p_lev = z(batch, torch.int32), z((batch, mf, 2), torch.float64), z((batch, mf, 2), torch.int32), z((batch, mf), torch.int32)
            t_lg, t_lv = z(lv.total, torch.uint8), z(lv.total, torch.uint8)
            rows = (p_cnt.data_ptr(), p_kp.data_ptr(), p_lkp.data_ptr(), p_lev.data_ptr(), t_resp.data_ptr(), t_bins.data_ptr(),
                    t_desc.data_ptr(), t_pts.data_ptr())

            def pyr_chain():
                _lib.check(lib.cslam_feat_extract_pyramid_dev(t_src.data_ptr(), t_so.data_ptr(), t_depth.data_ptr(), t_off.data_ptr(),
                                                              t_hw.data_ptr(), t_cam.data_ptr(), batch, L, lv.t_off.data_ptr(), lv.t_hw.data_ptr(),
                                                              0.001, 7, 19, mf, 1, *rows, host(src_off), *h, *hl, stream()))

            def pyr_stereo_chain():
                _lib.check(lib.cslam_feat_extract_stereo_pyramid_dev(t_src.data_ptr(), t_so.data_ptr(), t_right.data_ptr(), t_so.data_ptr(),
                                                                     t_off.data_ptr(), t_hw.data_ptr(), t_scam.data_ptr(), batch, L,
                                                                     lv.t_off.data_ptr(), lv.t_hw.data_ptr(), 0.001, 7, 19, mf, 1, 128, 15, 1,
                                                                     *rows, t_disp.data_ptr(), t_status.data_ptr(), host(src_off),
                                                                     host(src_off), *h, *hl, host(scam), stream()))

            p_offs = z((batch, mf, 2), torch.float64)

            def pyr_subpix_chain():
                _lib.check(lib.cslam_feat_extract_pyramid_subpix_dev(t_src.data_ptr(), t_so.data_ptr(), t_depth.data_ptr(), t_off.data_ptr(),
                                                                     t_hw.data_ptr(), t_cam.data_ptr(), batch, L, lv.t_off.data_ptr(),
                                                                     lv.t_hw.data_ptr(), 0.001, 7, 19, mf, 1, *rows, p_offs.data_ptr(),
                                                                     host(src_off), *h, *hl, stream()))

            def pyr_subpix_stereo_chain():
                _lib.check(lib.cslam_feat_extract_stereo_pyramid_subpix_dev(t_src.data_ptr(), t_so.data_ptr(), t_right.data_ptr(),
                                                                            t_so.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(),
                                                                            t_scam.data_ptr(), batch, L, lv.t_off.data_ptr(),
                                                                            lv.t_hw.data_ptr(), 0.001, 7, 19, mf, 1, 128, 15, 1, *rows,
                                                                            t_disp.data_ptr(), t_status.data_ptr(), p_offs.data_ptr(),
                                                                            host(src_off), host(src_off), *h, *hl, host(scam), stream()))

            def pyr_levels():
                _lib.check(lib.cslam_feat_pyramid_dev(t_gray.data_ptr(), t_off.data_ptr(), t_hw.data_ptr(), batch, L, t_depth.data_ptr(),
                                                      lv.t_off.data_ptr(), lv.t_hw.data_ptr(), t_lg.data_ptr(), t_lv.data_ptr(), *h, *hl,
                                                      stream()))

            r = {"chain_ms": timed(pyr_chain), "subpix_chain_ms": timed(pyr_subpix_chain)}
            r["offsets_not_zero"] = round(float((p_offs != 0).any(dim=2).sum().item()) / batch, 1)
            cnt = p_cnt.cpu().numpy()
            lev = p_lev.cpu().numpy()
            r["keypoints_per_image"] = round(float(cnt.mean()), 1)
            r["keypoints_per_level"] = np.round(np.mean([np.bincount(lev[c, :cnt[c]], minlength=L) for c in range(batch)], axis=0), 1).tolist()
            r["stereo_chain_ms"] = timed(pyr_stereo_chain)
            r["subpix_stereo_chain_ms"] = timed(pyr_subpix_stereo_chain)
            gray()
            r["levels_ms"] = timed(pyr_levels)
            # the level images and maps packed without padding, for the single-scale entries
            px = [int(a) * int(b) for a, b in lv.shapes]
            off_l = offsets(px)
            pack = lambda t: torch.cat([t[int(lv.off[i]):int(lv.off[i]) + px[i]] for i in range(nl)])
            q_gray, q_valid, q_off, q_hw = pack(t_lg), pack(t_lv), to_dev(off_l, dev), lv.t_hw
            q_R, q_max, q_cnt = z(int(off_l[-1]), torch.int32), z(nl, torch.int32), z(nl, torch.int32)
            q_kp, q_resp, q_bins, q_desc = z((nl, b0, 2), torch.int32), z((nl, b0), torch.int32), z((nl, b0), torch.int32), z((nl, b0, 32), torch.uint8)
            q_koff = offsets([b0] * nl)
            q_ko = to_dev(q_koff, dev)
            hq = (host(off_l), host(lv.hw))

            def pyr_response():
                _lib.check(lib.cslam_feat_response_dev(q_gray.data_ptr(), q_off.data_ptr(), q_hw.data_ptr(), nl, q_R.data_ptr(), q_max.data_ptr(),
                                                       *hq, stream()))

            def pyr_select():
                _lib.check(lib.cslam_feat_select_dev(q_R.data_ptr(), q_max.data_ptr(), q_valid.data_ptr(), q_off.data_ptr(), q_hw.data_ptr(), nl,
                                                     0.001, 7, 19, b0, q_cnt.data_ptr(), q_kp.data_ptr(), q_resp.data_ptr(), *hq, stream()))

            def pyr_describe():
                _lib.check(lib.cslam_feat_describe_dev(q_gray.data_ptr(), q_off.data_ptr(), q_hw.data_ptr(), nl, q_kp.data_ptr(), q_ko.data_ptr(),
                                                       q_bins.data_ptr(), q_desc.data_ptr(), *hq, host(q_koff), stream()))

            r.update({"response_ms": timed(pyr_response), "select_ms": timed(pyr_select)})
            # the staged describe reads all b0 rows of a level image: rows a level did not fill are moved inside it
            top = torch.from_numpy(lv.hw[:, ::-1].copy()).to(dev).view(nl, 1, 2) - 19
            q_kp.copy_(torch.minimum(torch.clamp(q_kp, min=18), top))
            r["describe_ms"] = timed(pyr_describe)
            q_offs = z((nl, b0, 2), torch.float64)

            def pyr_subpixel():
                _lib.check(lib.cslam_feat_subpixel_dev(q_R.data_ptr(), q_off.data_ptr(), q_hw.data_ptr(), nl, q_kp.data_ptr(), q_ko.data_ptr(),
                                                       q_offs.data_ptr(), *hq, host(q_koff), stream()))

            r["subpixel_ms"] = timed(pyr_subpixel)
            return r

        res = {"gray_ms": timed(gray), "response_ms": timed(response), "select_ms": timed(select)}
        cnt = t_cnt.cpu().numpy()
        if not np.all(cnt == mf):                          # the staged describe / points read all mf rows of an image
            t_kp[:, :, 0].clamp_(18, W - 19)
            t_kp[:, :, 1].clamp_(18, H - 19)
        res.update({"describe_ms": timed(describe), "points_ms": timed(points), "chain_ms": timed(chain)})
        res["keypoints_per_image"] = round(float(t_cnt.cpu().numpy().mean()), 1)
        gray_right()
        res.update({"stereo_ms": timed(stereo), "stereo_chain_ms": timed(stereo_chain)})
        n_st = t_cnt.cpu().numpy()
        st = t_status.cpu().numpy()
        res["stereo_keypoints_per_image"] = round(float(n_st.mean()), 1)
        res["stereo_accepted_per_image"] = round(float(np.mean([(st[c, :n_st[c]] == 0).sum() for c in range(batch)])), 1)
        for L in (1, 4, 8):
            res["pyramid_%d" % L] = pyramid(L)
        out["batch_%d" % batch] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
