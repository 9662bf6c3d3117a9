#!/usr/bin/env python
"""SHA-256 of what the registration entry points (voxel, FPFH and matches, robust fit and its stages, both ICP estimators,
visual registration) return on seeded inputs at the sizes of tools/perf_voxel.py, perf_fpfh.py, perf_robust.py, perf_icp.py and
perf_visual_registration.py, singles and batches of 4, with and without the host copies of the offsets where an entry takes them.
One line per result: name sha256.  For a change that must not move a bit, run it on both builds and compare:

    python tools/registration_output_hashes.py > child.log
    CSLAM_HIP_LIB=/path/to/the/other/libcslam_hip.so python tools/registration_output_hashes.py > parent.log
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def h(name, *arrays):
    m = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        m.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    print(name, m.hexdigest(), flush=True)


def main():
    import torch
    import icp_reference as iref
    import robust_reference as rref
    import vis_reference as vref
    from cslam_amd import _lib
    from cslam_amd.lidar_pr import icp_utils as u, robust
    from cslam_amd.lidar_pr._batch import upload
    from cslam_amd.front_end import visual_registration as vr
    import perf_voxel

    lib = _lib.load()
    voxel, B = 0.5, 4
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    host = lambda a: a.ctypes.data_as(C.c_void_p)

    # voxel (perf_voxel: raw scans of 130 000 points)
    scans = perf_voxel.raw_scans(iref, B, 130000, voxel)
    for name, sel in (("voxel.1", scans[:1]), ("voxel.%d" % B, scans)):
        got = u.downsample_clouds(sel, voxel, counts=True)
        h(name, *[x for g in got for x in g])
    cl = upload(scans, dev)
    total = int(cl.off[-1])
    out = torch.zeros((total, 3), dtype=torch.float64, device=dev)
    out_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(total, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.check(lib.cslam_voxel_downsample_dev(cl.rows, cl.d_off, B, voxel, out.data_ptr(), out_off.data_ptr(), cnt.data_ptr(),
                                              status.data_ptr(), None, st))
    rows = int(out_off.cpu()[-1])
    h("voxel.%d.no_host_offsets" % B, out.cpu().numpy()[:rows], out_off.cpu().numpy(), cnt.cpu().numpy()[:rows], status.cpu().numpy())

    # fpfh + match (perf_fpfh / perf_icp: street scenes from 60 000 raw points)
    scenes = [iref.street_scene(seed, 60000, voxel) for seed in range(B)]
    pairs = [(s[0], s[1]) for s in scenes]
    f_src = u.extract_fpfh_clouds([p[0] for p in pairs], voxel)
    f_dst = u.extract_fpfh_clouds([p[1] for p in pairs], voxel)
    h("fpfh.features.%d" % B, *f_src, *f_dst)
    h("fpfh.features.1", *u.extract_fpfh_clouds(pairs[0][:1], voxel))
    fp = list(zip(f_src, f_dst))
    for name, sel in (("match.1", fp[:1]), ("match.%d" % B, fp)):
        h(name, *[x for g in u.find_correspondences_pairs(sel) for x in g])
        h(name + ".plain", *[x for g in u.find_correspondences_pairs(sel, mutual_filter=False) for x in g])
    a_off = np.zeros(B + 1, dtype=np.int64); a_off[1:] = np.cumsum([len(f) for f in f_src])
    b_off = np.zeros(B + 1, dtype=np.int64); b_off[1:] = np.cumsum([len(f) for f in f_dst])
    t_a, t_b = torch.from_numpy(np.concatenate(f_src)).to(dev), torch.from_numpy(np.concatenate(f_dst)).to(dev)
    t_ao, t_bo = torch.from_numpy(a_off).to(dev), torch.from_numpy(b_off).to(dev)
    na, nb = int(a_off[-1]), int(b_off[-1])
    o = torch.zeros(3 * na + nb + B, dtype=torch.int32, device=dev)
    base = o.data_ptr()
    _lib.check(lib.cslam_feature_match_dev(t_a.data_ptr(), t_ao.data_ptr(), t_b.data_ptr(), t_bo.data_ptr(), B, 33, base, base + 4 * na,
                                           base + 4 * (na + nb), base + 4 * (3 * na + nb), None, None, st))
    kept = o[3 * na + nb:].cpu().numpy()
    pr = o[na + nb:3 * na + nb].cpu().numpy().reshape(na, 2)
    h("match.%d.no_host_offsets" % B, o[:na + nb].cpu().numpy(), kept, *[pr[a_off[p]:a_off[p] + kept[p]] for p in range(B)])

    # robust (perf_robust: the mutual matches of street scenes; the planted pair of 8000)
    small = [iref.street_scene(seed)[:2] for seed in range(1, B + 1)]          # perf_robust's scenes: 9000 raw points
    sf = u.extract_fpfh_clouds([c for pair in small for c in pair], voxel)
    corr = u.find_correspondences_pairs([(sf[2 * p], sf[2 * p + 1]) for p in range(B)])
    matched = [(small[p][0][i0], small[p][1][i1]) for p, (i0, i1) in enumerate(corr)]
    print("robust: %s matches" % [len(a) for a, _ in matched], flush=True)
    planted = [rref.planted(1, 8000, 400)[:2]]
    for name, sel, c in (("robust.1", matched[:1], voxel), ("robust.%d" % B, matched, voxel), ("robust.planted8000", planted, 0.05)):
        fits = u.robust_fit_pairs(sel, c)
        h(name + ".fit", *[x for f in fits for x in (f.transformation, f.clique, np.array([f.status, f.clique_size, f.iterations, f.certified,
                                                                                            f.nodes, f.correspondences]))])
        graphs = robust.consistency_graph_pairs(sel, c)
        cliques = robust.max_clique_graphs([g[0] for g in graphs])
        lists = [q[0] for q in cliques]
        rots = robust.robust_rotation_pairs(sel, c, lists)
        R = [r[0] for r in rots]
        trs = robust.robust_translation_pairs(sel, R, c, lists)
        flat = lambda xs: [np.asarray(y) for x in xs for y in (x if isinstance(x, (tuple, list)) else (x,))]
        h(name + ".graph", *flat(graphs))
        h(name + ".clique", *flat(cliques))
        h(name + ".rotation", *flat(rots))
        h(name + ".translation", *flat(trs))

    # icp (perf_icp)
    yaws = [360.0 - iref.seed_yaw(s[3]) for s in scenes]
    for est in ("point_to_point", "point_to_plane"):
        for name, n in (("icp.1", 1), ("icp.%d" % B, B)):
            res = u.register_pairs(pairs[:n], voxel, yaws[:n], estimation=est, correspondence_sets=True)
            h("%s.%s" % (name, est), *[x for r in res for x in (r.transformation, np.array([r.fitness, r.inlier_rmse]),
                                                               np.array([r.iterations, r.correspondences]), r.correspondence_set)])
    nc = u.nearest_correspondences(pairs, voxel)
    h("icp.%d.correspondences" % B, *[x for g in nc for x in g])

    # visual registration (perf_visual_registration: 1000 keypoints per keyframe)
    kfs = [tuple(vr.Keyframe(*k) for k in vref.keyframe_pair(s, landmarks=750, distractors=250)[:2]) for s in range(B)]
    for name, sel in (("vis.1", kfs[:1]), ("vis.%d" % B, kfs)):
        res = vr.register_pairs(sel, vref.CAM)
        h(name + ".register", *[x for r in res for x in (r.transformation, np.array([r.status, r.dropped_no_depth, r.best_hypothesis]),
                                                         r.matches, r.inliers)])
        h(name + ".match", *vr.match_descriptors_pairs([(a.descriptors, b.descriptors) for a, b in sel]))
    X, uv, _, _ = vref.planted_scene(1)
    res = vr.pnp_ransac_pairs([(X, uv)] * 3, vref.CAM)
    h("vis.pnp", *[x for r in res for x in (r.transformation, r.inliers, np.array([r.status, r.best_hypothesis]))])
    hy = vr.hypotheses((X, uv), vref.CAM)
    h("vis.hypotheses", hy.R, hy.t, hy.valid, hy.inliers, np.array([hy.best_hypothesis]), hy.best_inliers)
    print("hashes done", flush=True)


if __name__ == "__main__":
    main()
