#!/usr/bin/env python
"""Relative transform between two lidar keyframes on an MI355X: FPFH features, mutual matches, the robust coarse fit
and batched point-to-point ICP.

Counterpart of cslam/lidar_pr/icp_utils.py (`compute_transform`, called by lidar_handler_node.py:115,133 for every
accepted ScanContext match).  The reference runs FPFH + mutual nearest neighbours + TEASER++ for a coarse alignment and
then open3d's `registration_icp(src, dst, voxel_size, T, PointToPoint, max_iteration=100)` (icp_utils.py:126-134), and
accepts the match when TEASER's maximum clique has more than min_inliers members.  Both coarse alignments exist here:
  coarse="yaw" (the default of `compute_transform` / `solve_icp`): the yaw shift of the ScanContext match
      (`ScanContextMatching.last_yaw_diff_deg`), helped by two coarse ICP stages at a larger correspondence radius
      (`DEFAULT_STAGES`); accepted on a correspondence count and a fitness;
  coarse="teaser" (`solve_teaser`, `solve_teaser_pairs`): the reference's path.  `extract_fpfh` and `find_correspondences`
      (icp_utils.py:26-65; csrc/fpfh.hip, batched forms `extract_fpfh_clouds` and `find_correspondences_pairs`) give
      putative matches that do not come from the alignment under test, and the robust fit (csrc/robust.hip: `robust_fit_pairs`,
      staged `consistency_graph`, `max_clique`, `robust_rotation`, `robust_translation`) is TEASER++'s algorithm at the
      reference's parameters: the consistency graph of the matches, its exact maximum clique, GNC-TLS for the rotation and
      per-axis TLS for the translation.  It needs no yaw, and its acceptance test is the reference's: the clique size.
The refinement keeps open3d's documented semantics exactly in both.

The loop is hand-written HIP (csrc/icp.hip behind `cslam_icp_register_dev`): float64, brute-force nearest neighbours,
fixed summation order -- a pair's result is the same bits alone or in any batch.  There is no CPU path: without the
library or a GPU every registration raises `CslamHipError`.  Parity with open3d itself is not pinned (no open3d is
available to record golden vectors from); the tests hold the kernels to a float64 restatement of open3d's documented
algorithm.

Clouds are [n, >=3] arrays or anything with a `.points` attribute (an open3d cloud); they are widened to float64 and
rows with a non-finite coordinate are dropped, as the reference's `downsample` does.  The clouds the handler stores
and sends are down-sampled ones: `downsample` / `downsample_clouds` (csrc/voxel.hip behind
`cslam_voxel_downsample_dev`) are the counterpart of the reference's `downsample` (icp_utils.py:93-100, open3d's
`voxel_down_sample`), batched, and `keyframes.ingest` does it on the upload the ScanContext descriptor uses.

Yaw seed: with `matcher.add_item(descriptor(dst))`, `matcher.search(descriptor(src))`, a source that is the target
scene turned by +a degrees about z (dst ~ Rz(a) . src) matches at `last_yaw_diff_deg` = 360 - a (rounded to the 6 degree
sector).  The seed is therefore the rotation about z by MINUS `init_yaw_deg`.
"""
import ctypes as C

import numpy as np

from .. import _lib

# (multiple of voxel_size, max iterations) per stage; the last is the reference's refinement (icp_utils.py:126-131)
DEFAULT_STAGES = ((4.0, 30), (2.0, 30), (1.0, 100))
ICP_CHUNK = 1024      # target points per LDS chunk of the nearest-neighbour kernel (csrc/icp.hip); the tests size around it
ICP_MAX_LANES = 64    # chunk lanes of its grid: a target of more chunks than this is walked lane-strided
VOXEL_TILE = 2048        # keys per workgroup per radix pass of the voxel sort (csrc/voxel_plan.h); the tests size around it
VOXEL_SEG_BLOCK = 256    # threads per workgroup of the kernel that sums a voxel's points (one wave per voxel)
KNN_BLOCK = 256       # threads per workgroup of the radius search (csrc/fpfh.hip): one wave per query point, four per workgroup
KNN_CHUNK = 1024      # cloud points per LDS chunk of the radius search; the tests size around it
KNN_CAND = 512        # candidate buffer of a query: more in-radius points than this are cut to the best max_nn - 1 on the way
KNN_MAX_NN = 256      # widest neighbour list
FM_BLOCK = 64         # query rows per workgroup of the feature matching kernel
FM_CHUNK = 32         # target rows per LDS chunk of the feature matching kernel
FM_MAX_LANES = 16     # chunk lanes of its grid: a target of more chunks than this is walked lane-strided
FM_MAX_DIM = 64       # widest feature
FPFH_BINS = 33
ROBUST_MAX_N = 8192            # most correspondences of a pair the robust fit attempts (csrc/robust.hip); above it: status 2
ROBUST_GRAPH_BLOCK = 64        # rows of the consistency graph per workgroup
ROBUST_GRAPH_CHUNK = 256       # matched points per LDS chunk of the graph kernel; the tests size around it
ROBUST_STACK_DEPTH = 512       # deepest branch of the clique search below a root; deeper ends the search uncertified
ROBUST_DEFAULT_NODE_BUDGET = 2097152     # nodes of one pair's clique search (CSLAM_ROBUST_DEFAULT_NODE_BUDGET)


def Rt2T(R, t):
    T = np.identity(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def yaw_seed(init_yaw_deg):
    """4 x 4 initial transform for a ScanContext yaw shift in degrees (None -> identity): Rz(-init_yaw_deg)."""
    if init_yaw_deg is None:
        return np.identity(4)
    a = np.deg2rad(-float(init_yaw_deg))
    c, s = np.cos(a), np.sin(a)
    return Rt2T(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.zeros(3))


class RegistrationResult:
    """open3d's RegistrationResult fields, plus the number of updates the (last) stage made."""

    def __init__(self, transformation, fitness, inlier_rmse, correspondences, iterations, correspondence_set=None):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.correspondences = correspondences
        self.iterations = iterations
        self.correspondence_set = correspondence_set

    def __repr__(self):
        return ("RegistrationResult(fitness=%.6f, inlier_rmse=%.6f, correspondences=%d, iterations=%d)"
                % (self.fitness, self.inlier_rmse, self.correspondences, self.iterations))


class Success:
    """The success flag of `compute_transform`: truthy or falsy like the reference's bool, and it carries the figures
    the decision was made from (`fitness`, `inlier_rmse`, `correspondences`, `iterations`, `transformation`)."""

    def __init__(self, ok, result):
        self.ok = bool(ok)
        self.fitness = result.fitness
        self.inlier_rmse = result.inlier_rmse
        self.correspondences = result.correspondences
        self.iterations = result.iterations
        self.transformation = result.transformation

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return "Success(%s, fitness=%.4f, inlier_rmse=%.4f, correspondences=%d)" % (
            self.ok, self.fitness, self.inlier_rmse, self.correspondences)


def _points(cloud):
    pts = np.asarray(cloud.points if hasattr(cloud, "points") else cloud)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("a cloud is an [n, >=3] array, got shape %s" % (pts.shape,))
    pts = np.ascontiguousarray(pts[:, :3], dtype=np.float64)
    return pts[np.isfinite(pts).all(axis=1)]


def _rows(cloud):
    """[n, 3] float64 rows of a cloud, non-finite rows included (the down-sampling kernels leave them out themselves)."""
    pts = np.asarray(cloud.points if hasattr(cloud, "points") else cloud)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("a cloud is an [n, >=3] array, got shape %s" % (pts.shape,))
    return np.ascontiguousarray(pts[:, :3], dtype=np.float64)


def _round256(n):
    return (n + 255) // 256 * 256


def _upload_clouds(clouds, dev):
    """One host buffer, one copy: the int64 offsets, then the rows.  Returns (device bytes, host offsets, byte offset
    of the rows)."""
    import torch
    n = len(clouds)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    total, head = int(off[-1]), _round256(8 * (n + 1))
    buf = np.zeros(head + 24 * total, dtype=np.uint8)
    buf[:8 * (n + 1)].view(np.int64)[:] = off
    if total:
        np.concatenate(clouds, axis=0, out=buf[head:].view(np.float64).reshape(total, 3))
    return torch.from_numpy(buf).to(dev), off, head


def _voxel_enqueue(lib, t_in, off, head, voxel_size, counts, extra_bytes=0):
    """`cslam_voxel_downsample_dev` on uploaded clouds.  Every result lies in ONE device byte buffer, so that it comes
    back in one copy: returns (buffer, layout) with layout = byte offsets of out_offsets, status, rows, counts, extra."""
    import torch
    n, total = len(off) - 1, int(off[-1])
    lay = {"out_off": 0}
    lay["status"] = _round256(8 * (n + 1))
    lay["rows"] = lay["status"] + _round256(4 * n)
    lay["counts"] = lay["rows"] + _round256(24 * total)
    lay["extra"] = lay["counts"] + _round256(4 * total if counts else 0)
    t_out = torch.zeros(lay["extra"] + extra_bytes, dtype=torch.uint8, device=t_in.device)
    base = t_out.data_ptr()
    _lib.check(lib.cslam_voxel_downsample_dev(
        t_in.data_ptr() + head if total else None, t_in.data_ptr(), n, float(voxel_size),
        base + lay["rows"] if total else None, base + lay["out_off"], base + lay["counts"] if counts and total else None,
        base + lay["status"], off.ctypes.data_as(C.c_void_p), torch.cuda.current_stream().cuda_stream))
    return t_out, lay


class VoxelSizeError(ValueError):
    """A cloud needs a voxel index of 2^21 or more on some axis.  `failed`: the numbers of those clouds; `clouds`: the
    results of the call with None in their places (the other clouds of a batch are not affected)."""

    def __init__(self, failed, clouds):
        ValueError.__init__(self, "voxel_size is too small for cloud%s %s: a voxel index of 2^21 or more on some axis "
                            "(open3d raises 'voxel_size is too small' where its index arithmetic overflows)"
                            % ("s" if len(failed) > 1 else "", ", ".join(str(c) for c in failed)))
        self.failed = failed
        self.clouds = clouds


def _voxel_unpack(host, lay, n, counts):
    """Split the downloaded result buffer into per-cloud arrays; raises VoxelSizeError for a status of 1."""
    out_off = host[lay["out_off"]:lay["out_off"] + 8 * (n + 1)].view(np.int64)
    status = host[lay["status"]:lay["status"] + 4 * n].view(np.int32)
    m = int(out_off[-1])
    rows = host[lay["rows"]:lay["rows"] + 24 * m].view(np.float64).reshape(m, 3)
    cnt = host[lay["counts"]:lay["counts"] + 4 * m].view(np.int32) if counts else None
    res = []
    for c in range(n):
        a, b = int(out_off[c]), int(out_off[c + 1])
        pts = rows[a:b].copy()
        res.append((pts, cnt[a:b].astype(np.int64)) if counts else pts)
    failed = [c for c in range(n) if status[c] != 0]
    if failed:
        raise VoxelSizeError(failed, [None if c in failed else r for c, r in enumerate(res)])
    return res


def downsample_clouds(clouds, voxel_size, counts=False, device=0):
    """Voxel down-sampling of a list of clouds in ONE call (one upload, one download): per cloud the [m, 3] float64
    means of the occupied voxels, in ascending lexicographic voxel index; with `counts` a pair (means, points per
    voxel).  The rule is open3d's `voxel_down_sample` after the reference's filter of non-finite rows
    (icp_utils.py:93-100); the filter too runs on the GPU.  A cloud without a finite row gives [0, 3].
    Raises `VoxelSizeError` (a ValueError) naming the clouds whose index range is beyond 2^21 per axis."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    clouds = [_rows(c) for c in clouds]
    if not clouds:
        return []
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_in, off, head = _upload_clouds(clouds, dev)
        t_out, lay = _voxel_enqueue(lib, t_in, off, head, voxel_size, counts)
        host = t_out.cpu().numpy()
    return _voxel_unpack(host, lay, len(clouds), counts)


def downsample(points, voxel_size, device=0):
    """Counterpart of the reference's `downsample` (icp_utils.py:93-100): the down-sampled cloud as an [m, 3] float64
    array (every function of this module takes arrays or `.points`)."""
    return downsample_clouds([points], voxel_size, device=device)[0]


# ---- FPFH features and mutual matches (csrc/fpfh.hip) ---------------------------------------------------------------
def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _host(off):
    return off.ctypes.data_as(C.c_void_p)


def _knn_enqueue(lib, t_in, off, head, radius, max_nn):
    """`cslam_knn_radius_dev` on uploaded clouds (at least one point in all): device (idx, d2, count)."""
    import torch
    total, dev = int(off[-1]), t_in.device
    t_idx = torch.empty((total, max_nn), dtype=torch.int32, device=dev)
    t_d2 = torch.empty((total, max_nn), dtype=torch.float64, device=dev)
    t_cnt = torch.empty(total, dtype=torch.int32, device=dev)
    _lib.check(lib.cslam_knn_radius_dev(t_in.data_ptr() + head, t_in.data_ptr(), len(off) - 1, float(radius), int(max_nn),
                                        t_idx.data_ptr(), t_d2.data_ptr(), t_cnt.data_ptr(), _host(off), _stream()))
    return t_idx, t_d2, t_cnt


def _normals_enqueue(lib, t_in, off, head, lists, radius, max_nn, viewpoint):
    import torch
    t_idx, t_d2, t_cnt = lists
    view = np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
    t_n = torch.empty((int(off[-1]), 3), dtype=torch.float64, device=t_in.device)
    _lib.check(lib.cslam_normals_dev(t_in.data_ptr() + head, t_in.data_ptr(), len(off) - 1, t_idx.data_ptr(), t_d2.data_ptr(),
                                     t_cnt.data_ptr(), t_idx.shape[1], float(radius), int(max_nn), _host(view), t_n.data_ptr(),
                                     _host(off), _stream()))
    return t_n


def _fpfh_enqueue(lib, t_in, off, head, t_normals, lists, spfh):
    """Device [total, 33] FPFH, or [2, total, 33] (FPFH, SPFH) with `spfh`."""
    import torch
    t_idx, t_d2, t_cnt = lists
    total = int(off[-1])
    t_f = torch.empty((2 if spfh else 1, total, FPFH_BINS), dtype=torch.float64, device=t_in.device)
    _lib.check(lib.cslam_fpfh_dev(t_in.data_ptr() + head, t_normals.data_ptr(), t_in.data_ptr(), len(off) - 1, t_idx.data_ptr(),
                                  t_d2.data_ptr(), t_cnt.data_ptr(), t_idx.shape[1], t_f.data_ptr(),
                                  t_f[1].data_ptr() if spfh else None, _host(off), _stream()))
    return t_f if spfh else t_f[0]


def _split(rows, off):
    return [rows[int(off[c]):int(off[c + 1])].copy() for c in range(len(off) - 1)]


def radius_neighbors_clouds(clouds, radius, max_nn, device=0):
    """The neighbour lists the normals and the features are computed from (`cslam_knn_radius_dev`, the counterpart of
    open3d's KDTreeSearchParamHybrid(radius, max_nn)) for a list of clouds in one call: per cloud (idx [n, max_nn] int32,
    d2 [n, max_nn], count [n]).  The list of point i is i itself, then the other points within the radius in ascending
    (d2, index), `max_nn` entries at most; beyond the count idx is -1 and d2 is +inf."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    clouds = [_points(c) for c in clouds]
    if sum(len(c) for c in clouds) == 0:
        if not (np.isfinite(radius) and radius > 0 and 1 <= max_nn <= KNN_MAX_NN):
            raise _lib.CslamHipError("invalid argument: radius must be positive and finite, max_nn in [1, %d]" % KNN_MAX_NN)
        return [(np.zeros((0, max_nn), np.int32), np.zeros((0, max_nn)), np.zeros(0, np.int32)) for _ in clouds]
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_in, off, head = _upload_clouds(clouds, dev)
        idx, d2, cnt = (t.cpu().numpy() for t in _knn_enqueue(lib, t_in, off, head, radius, max_nn))
    return list(zip(_split(idx, off), _split(d2, off), _split(cnt, off)))


def radius_neighbors(cloud, radius, max_nn, device=0):
    return radius_neighbors_clouds([cloud], radius, max_nn, device)[0]


def estimate_normals_clouds(clouds, radius, max_nn=30, viewpoint=(0.0, 0.0, 0.0), device=0):
    """open3d's `estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))` for a list of clouds in one call: per cloud
    the [n, 3] unit normals.  The eigenvector of the smallest eigenvalue of the neighbours' covariance; (0, 0, 1) with
    fewer than 3 neighbours (the point included).  The sign is fixed, which open3d leaves to its eigen-solver: every
    normal points to the side of `viewpoint` (default: the sensor at the origin of a keyframe cloud)."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    clouds = [_points(c) for c in clouds]
    if sum(len(c) for c in clouds) == 0:
        return [np.zeros((0, 3)) for _ in clouds]
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_in, off, head = _upload_clouds(clouds, dev)
        lists = _knn_enqueue(lib, t_in, off, head, radius, max_nn)
        normals = _normals_enqueue(lib, t_in, off, head, lists, radius, max_nn, viewpoint).cpu().numpy()
    return _split(normals, off)


def estimate_normals(cloud, radius, max_nn=30, viewpoint=(0.0, 0.0, 0.0), device=0):
    return estimate_normals_clouds([cloud], radius, max_nn, viewpoint, device)[0]


def compute_fpfh_feature(cloud, normals, radius, max_nn=100, return_spfh=False, device=0):
    """open3d's `compute_fpfh_feature(cloud, KDTreeSearchParamHybrid(radius, max_nn))` with the normals given: the
    [n, 33] features, one ROW per point (the reference transposes open3d's [33, n], icp_utils.py:37); with
    `return_spfh` the pair (FPFH, SPFH)."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    pts = _points(cloud)
    nrm = np.ascontiguousarray(normals, dtype=np.float64)
    if nrm.shape != pts.shape:
        raise ValueError("normals of shape %s for %d points with finite coordinates" % (nrm.shape, len(pts)))
    if len(pts) == 0:
        return (np.zeros((0, FPFH_BINS)),) * 2 if return_spfh else np.zeros((0, FPFH_BINS))
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_in, off, head = _upload_clouds([pts], dev)
        lists = _knn_enqueue(lib, t_in, off, head, radius, max_nn)
        out = _fpfh_enqueue(lib, t_in, off, head, torch.from_numpy(nrm).to(dev), lists, return_spfh).cpu().numpy()
    return (out[0], out[1]) if return_spfh else out


def extract_fpfh_clouds(clouds, voxel_size, viewpoint=(0.0, 0.0, 0.0), device=0):
    """`extract_fpfh` for a list of clouds in ONE call (one upload, one download).  One neighbour search at
    (5 voxels, 100) serves both steps: the normals at (2 voxels, 30) use the prefix of each list, which is the list a
    search of their own returns."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    clouds = [_points(c) for c in clouds]
    if sum(len(c) for c in clouds) == 0:
        return [np.zeros((0, FPFH_BINS)) for _ in clouds]
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_in, off, head = _upload_clouds(clouds, dev)
        lists = _knn_enqueue(lib, t_in, off, head, 5.0 * voxel_size, 100)
        t_n = _normals_enqueue(lib, t_in, off, head, lists, 2.0 * voxel_size, 30, viewpoint)
        feats = _fpfh_enqueue(lib, t_in, off, head, t_n, lists, False).cpu().numpy()
    return _split(feats, off)


def extract_fpfh(cloud, voxel_size, viewpoint=(0.0, 0.0, 0.0), device=0):
    """Counterpart of the reference's `extract_fpfh` (icp_utils.py:26-37): normals from the neighbours within 2 voxels
    (30 at most), FPFH from those within 5 voxels (100 at most); [n, 33] float64."""
    return extract_fpfh_clouds([cloud], voxel_size, viewpoint, device)[0]


def _features(x):
    f = np.ascontiguousarray(x, dtype=np.float64)
    if f.ndim != 2 or not 1 <= f.shape[1] <= FM_MAX_DIM or f.shape[0] < 1:
        raise ValueError("features are an [n >= 1, 1 <= dim <= %d] array, got shape %s" % (FM_MAX_DIM, f.shape))
    return f


def _match(pairs, device):
    """`cslam_feature_match_dev`: per pair (nn01, nn10, mutual rows [m, 2]), int64."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    pairs = [(_features(a), _features(b)) for a, b in pairs]
    n = len(pairs)
    if n == 0:
        return []
    dim = pairs[0][0].shape[1]
    if any(a.shape[1] != dim or b.shape[1] != dim for a, b in pairs):
        raise ValueError("all feature arrays of a call need the same dimension")
    a_off = np.zeros(n + 1, dtype=np.int64)
    b_off = np.zeros(n + 1, dtype=np.int64)
    a_off[1:] = np.cumsum([len(a) for a, _ in pairs])
    b_off[1:] = np.cumsum([len(b) for _, b in pairs])
    na, nb = int(a_off[-1]), int(b_off[-1])
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_a = torch.from_numpy(np.concatenate([a for a, _ in pairs], axis=0)).to(dev)
        t_b = torch.from_numpy(np.concatenate([b for _, b in pairs], axis=0)).to(dev)
        t_ao = torch.from_numpy(a_off).to(dev)
        t_bo = torch.from_numpy(b_off).to(dev)
        t_out = torch.empty(3 * na + nb + n, dtype=torch.int32, device=dev)     # nn01 | nn10 | pairs | counts: one download
        base = t_out.data_ptr()
        _lib.check(lib.cslam_feature_match_dev(t_a.data_ptr(), t_ao.data_ptr(), t_b.data_ptr(), t_bo.data_ptr(), n, dim, base,
                                               base + 4 * na, base + 4 * (na + nb), base + 4 * (3 * na + nb), _host(a_off),
                                               _host(b_off), _stream()))
        out = t_out.cpu().numpy().astype(np.int64)
    rows = out[na + nb:3 * na + nb].reshape(na, 2)
    return [(out[a_off[p]:a_off[p + 1]], out[na + b_off[p]:na + b_off[p + 1]],
             rows[a_off[p]:a_off[p] + out[3 * na + nb + p]]) for p in range(n)]


def find_knn(feat0, feat1, device=0):
    """For every row of feat0 the nearest row of feat1 in squared Euclidean distance, ties -> the lower row (the
    reference's `find_knn_cpu` with knn=1, icp_utils.py:40-46), brute force on the GPU."""
    return _match([(feat0, feat1)], device)[0][0]


def find_correspondences_pairs(pairs, mutual_filter=True, device=0):
    """`find_correspondences` for a list of (feats0, feats1) in ONE call: per pair (idx0, idx1)."""
    out = []
    for nn01, _, rows in _match(pairs, device):
        out.append((rows[:, 0].copy(), rows[:, 1].copy()) if mutual_filter else (np.arange(len(nn01)), nn01))
    return out


def find_correspondences(feats0, feats1, mutual_filter=True, device=0):
    """Counterpart of the reference's `find_correspondences` (icp_utils.py:49-65): rows (idx0[k], idx1[k]) are each
    other's nearest neighbour in feature space; without the filter every row of feats0 with its nearest in feats1."""
    return find_correspondences_pairs([(feats0, feats1)], mutual_filter, device)[0]


# ---- the robust coarse fit (csrc/robust.hip) ------------------------------------------------------------------------
def _matched(pairs):
    """Matched points of a list of pairs: (ms [total, 3], md [total, 3], offsets).  A pair is (src_points, dst_points)
    with row k of one matched to row k of the other."""
    ms, md = [], []
    for a, b in pairs:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1, 3))
        if a.shape != b.shape:
            raise ValueError("matched points come in pairs: %s source rows, %s target rows" % (a.shape, b.shape))
        ms.append(a)
        md.append(b)
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in ms])
    cat = lambda xs: np.concatenate(xs, axis=0) if xs else np.zeros((0, 3))
    return cat(ms), cat(md), off


def _noise(noise_bound):
    c = float(noise_bound)
    if not (np.isfinite(c) and c > 0):
        raise _lib.CslamHipError("invalid argument: noise_bound must be positive and finite")
    return c


def _budget(node_budget):
    b = int(node_budget)
    if b < 1:
        raise _lib.CslamHipError("invalid argument: node_budget must be at least 1")
    return b


def _used(off):
    """The correspondences the stages use per pair (0 above the cap) and the word offsets of the bit matrices."""
    n = np.diff(off)
    n = np.where(n > ROBUST_MAX_N, 0, n)
    words = np.zeros(len(off), dtype=np.int64)
    words[1:] = np.cumsum(n * ((n + 63) // 64))
    return n, words


def _dev(arr, dev):
    import torch
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(dev)


def consistency_graph_pairs(pairs, noise_bound, device=0):
    """The consistency graphs of a list of (matched source points, matched target points) in ONE call
    (`cslam_robust_graph_dev`): per pair (adj [N, ceil(N / 64)] uint64, deg [N] int32).  Matches i and j are joined iff
    the distance between the two source points and that between the two target points differ by 2 noise_bound at most.
    Bit j of row i is bit j % 64 of word j // 64.  A pair of more than ROBUST_MAX_N rows gets an empty result."""
    c = _noise(noise_bound)
    ms, md, off = _matched(pairs)
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    n, words = _used(off)
    if len(pairs) == 0:
        return []
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_ms, t_md, t_off = _dev(ms, dev), _dev(md, dev), _dev(off, dev)
        t_adj = torch.zeros(max(int(words[-1]), 1), dtype=torch.int64, device=dev)
        t_adj_off = torch.zeros(len(off), dtype=torch.int64, device=dev)
        t_deg = torch.zeros(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_robust_graph_dev(t_ms.data_ptr(), t_md.data_ptr(), t_off.data_ptr(), None, len(pairs), c, t_adj.data_ptr(),
                                              t_adj_off.data_ptr(), t_deg.data_ptr(), _host(off), None, _stream()))
        adj, deg, adj_off = t_adj.cpu().numpy().view(np.uint64), t_deg.cpu().numpy(), t_adj_off.cpu().numpy()
    assert np.array_equal(adj_off, words)
    return [(adj[words[p]:words[p + 1]].reshape(int(n[p]), -1).copy() if n[p] else np.zeros((0, 0), np.uint64),
             deg[off[p]:off[p] + n[p]].copy()) for p in range(len(pairs))]


def consistency_graph(src_points, dst_points, noise_bound, device=0):
    return consistency_graph_pairs([(src_points, dst_points)], noise_bound, device)[0]


def max_clique_graphs(graphs, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0):
    """The maximum cliques of a list of bit matrices (as `consistency_graph` returns them) in ONE call
    (`cslam_robust_clique_dev`): per graph (clique: ascending int64 indices, certified, nodes).  The search is exact;
    `certified` is False when `node_budget` nodes did not finish it (or a branch went deeper than ROBUST_STACK_DEPTH below
    its root): the clique is then the best found, never smaller than the greedy one.  Of equal cliques the greedy one wins,
    then the first that the search of the lowest root in the (core number, index) order meets."""
    budget = _budget(node_budget)
    graphs = [np.ascontiguousarray(g, dtype=np.uint64) for g in graphs]
    for g in graphs:
        if g.ndim != 2 or g.shape[1] != (g.shape[0] + 63) // 64 or g.shape[0] > ROBUST_MAX_N:
            raise ValueError("a graph is an [N <= %d, ceil(N / 64)] uint64 bit matrix, got shape %s" % (ROBUST_MAX_N, g.shape))
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    if not graphs:
        return []
    npairs = len(graphs)
    off = np.zeros(npairs + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(g) for g in graphs])
    n, words = _used(off)
    adj = np.concatenate([g.reshape(-1) for g in graphs]) if words[-1] else np.zeros(1, np.uint64)
    deg = np.concatenate([np.unpackbits(g.view(np.uint8).reshape(len(g), 8 * g.shape[1]), axis=1).sum(axis=1, dtype=np.int32) for g in graphs])
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_adj, t_words, t_deg, t_off = _dev(adj.view(np.int64), dev), _dev(words, dev), _dev(deg.astype(np.int32), dev), _dev(off, dev)
        t_clique = torch.zeros(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
        t_small = torch.zeros((2, npairs), dtype=torch.int32, device=dev)
        t_nodes = torch.zeros(npairs, dtype=torch.int64, device=dev)
        _lib.check(lib.cslam_robust_clique_dev(t_adj.data_ptr(), t_words.data_ptr(), t_deg.data_ptr(), t_off.data_ptr(), None, npairs, budget,
                                               t_clique.data_ptr(), t_small[0].data_ptr(), t_small[1].data_ptr(), t_nodes.data_ptr(),
                                               _host(off), None, _stream()))
        clique, small, nodes = t_clique.cpu().numpy(), t_small.cpu().numpy(), t_nodes.cpu().numpy()
    return [(clique[off[p]:off[p] + small[0, p]].astype(np.int64), bool(small[1, p]), int(nodes[p])) for p in range(npairs)]


def max_clique(graph, node_budget=ROBUST_DEFAULT_NODE_BUDGET, return_info=False, device=0):
    """The maximum clique of one bit matrix: ascending indices; with `return_info` (clique, certified, nodes)."""
    out = max_clique_graphs([graph], node_budget, device)[0]
    return out if return_info else out[0]


def _index_lists(cliques, off):
    """Per-pair index lists in the capacity layout (None = all rows in order): (int32 [total], sizes int32 [n])."""
    total = int(off[-1])
    flat = np.zeros(max(total, 1), dtype=np.int32)
    sizes = np.zeros(len(off) - 1, dtype=np.int32)
    for p in range(len(off) - 1):
        cap = int(off[p + 1] - off[p])
        q = np.arange(cap) if cliques is None or cliques[p] is None else np.asarray(cliques[p], dtype=np.int64).reshape(-1)
        if len(q) > cap or (len(q) and (q.min() < 0 or q.max() >= cap)):
            raise ValueError("an index list addresses rows outside its pair")
        flat[off[p]:off[p] + len(q)] = q
        sizes[p] = len(q)
    return flat, sizes


def robust_rotation_pairs(pairs, noise_bound, cliques=None, device=0):
    """GNC-TLS rotations of a list of (matched source points, matched target points) in ONE call
    (`cslam_robust_rotation_dev`), each on the chain of its index list (`cliques[p]`, None = every row in order): per pair
    (R [3, 3], weights [K - 1], iterations)."""
    c = _noise(noise_bound)
    ms, md, off = _matched(pairs)
    flat, sizes = _index_lists(cliques, off)
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    if not pairs:
        return []
    npairs = len(pairs)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_ms, t_md, t_off, t_q, t_k = _dev(ms, dev), _dev(md, dev), _dev(off, dev), _dev(flat, dev), _dev(sizes, dev)
        t_R = torch.zeros((npairs, 9), dtype=torch.float64, device=dev)
        t_w = torch.zeros(len(flat), dtype=torch.float64, device=dev)
        t_it = torch.zeros(npairs, dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_robust_rotation_dev(t_ms.data_ptr(), t_md.data_ptr(), t_off.data_ptr(), t_q.data_ptr(), t_k.data_ptr(), npairs,
                                                 c, t_R.data_ptr(), t_w.data_ptr(), t_it.data_ptr(), _host(off), _stream()))
        R, w, it = t_R.cpu().numpy(), t_w.cpu().numpy(), t_it.cpu().numpy()
    return [(R[p].reshape(3, 3).copy(), w[off[p]:off[p] + max(int(sizes[p]) - 1, 0)].copy(), int(it[p])) for p in range(npairs)]


def robust_rotation(src_points, dst_points, noise_bound, clique=None, device=0):
    return robust_rotation_pairs([(src_points, dst_points)], noise_bound, [clique], device)[0]


def robust_translation_pairs(pairs, rotations, noise_bound, cliques=None, device=0):
    """Per-axis TLS translations of a list of (matched source points, matched target points) under the given rotations in
    ONE call (`cslam_robust_translation_dev`): per pair (t [3], sets [3, K] bool: the consensus set of each axis)."""
    c = _noise(noise_bound)
    ms, md, off = _matched(pairs)
    flat, sizes = _index_lists(cliques, off)
    if len(rotations) != len(pairs):
        raise ValueError("%d rotations for %d pairs" % (len(rotations), len(pairs)))
    R = np.stack([np.asarray(r, dtype=np.float64).reshape(9) for r in rotations]) if pairs else np.zeros((0, 9))
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    if not pairs:
        return []
    npairs, total = len(pairs), max(int(off[-1]), 1)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_ms, t_md, t_off, t_q, t_k, t_R = (_dev(x, dev) for x in (ms, md, off, flat, sizes, R))
        t_t = torch.zeros((npairs, 3), dtype=torch.float64, device=dev)
        t_set = torch.zeros((3, total), dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_robust_translation_dev(t_ms.data_ptr(), t_md.data_ptr(), t_off.data_ptr(), t_q.data_ptr(), t_k.data_ptr(),
                                                    t_R.data_ptr(), npairs, c, t_t.data_ptr(), t_set.data_ptr() if off[-1] else None,
                                                    _host(off), _stream()))
        t, sets = t_t.cpu().numpy(), t_set.cpu().numpy()
    return [(t[p].copy(), sets[:, off[p]:off[p] + sizes[p]].astype(bool)) for p in range(npairs)]


def robust_translation(src_points, dst_points, rotation, noise_bound, clique=None, device=0):
    return robust_translation_pairs([(src_points, dst_points)], [rotation], noise_bound, [clique], device)[0]


class RobustFit:
    """The robust fit of one pair: `transformation` (4 x 4, source -> target), `status` (0 solved; 1 fewer than 3 clique
    members: the identity, never a fit; 2 more than ROBUST_MAX_N correspondences: not attempted), `clique` (ascending
    correspondence indices), `clique_size`, `iterations` of the rotation, `certified`, `nodes` of the clique search and
    `correspondences` given."""

    def __init__(self, transformation, status, clique, clique_size, iterations, certified, nodes, correspondences):
        self.transformation = transformation
        self.status = status
        self.clique = clique
        self.clique_size = clique_size
        self.iterations = iterations
        self.certified = certified
        self.nodes = nodes
        self.correspondences = correspondences

    def __repr__(self):
        return "RobustFit(status=%d, clique_size=%d of %d, iterations=%d, certified=%s, nodes=%d)" % (
            self.status, self.clique_size, self.correspondences, self.iterations, self.certified, self.nodes)


def _fit_enqueue(lib, p_src, p_src_off, p_dst, p_dst_off, p_rows, p_row_off, p_count, n, c, budget, row_off, h_count, dev):
    """`cslam_robust_fit_dev` on device pointers: device (T [n, 16], info [n, 6], clique [total rows])."""
    import torch
    t_T = torch.zeros((n, 16), dtype=torch.float64, device=dev)
    t_info = torch.zeros((n, 6), dtype=torch.int64, device=dev)
    t_clique = torch.zeros(max(int(row_off[-1]), 1), dtype=torch.int32, device=dev)
    _lib.check(lib.cslam_robust_fit_dev(p_src, p_src_off, p_dst, p_dst_off, p_rows, p_row_off, p_count, n, c, budget, t_T.data_ptr(),
                                        t_info.data_ptr(), t_clique.data_ptr(), _host(row_off),
                                        _host(h_count) if h_count is not None else None, _stream()))
    return t_T, t_info, t_clique


def _fits(T, info, clique, row_off):
    return [RobustFit(T[p].reshape(4, 4).copy(), int(info[p, 0]), clique[row_off[p]:row_off[p] + info[p, 1]].astype(np.int64),
                      int(info[p, 1]), int(info[p, 2]), bool(info[p, 3]), int(info[p, 4]), int(info[p, 5])) for p in range(len(T))]


def robust_fit_pairs(pairs, noise_bound, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0):
    """The robust fit (consistency graph, maximum clique, GNC-TLS rotation, per-axis TLS translation: TEASER++ with the
    reference's parameters, icp_utils.py:68-83,116-121) for a list of pairs in ONE batched call (`cslam_robust_fit_dev`).
    A pair is (matched source points, matched target points), or (source cloud, target cloud, rows) with rows [N, 2] =
    (source row, target row) as `find_correspondences` gives them.  Returns one `RobustFit` per pair."""
    c, budget = _noise(noise_bound), _budget(node_budget)
    srcs, dsts, rows = [], [], []
    for pr in pairs:
        a, b = _rows(pr[0]), _rows(pr[1])
        if len(pr) == 2:
            if a.shape != b.shape:
                raise ValueError("matched points come in pairs: %s source rows, %s target rows" % (a.shape, b.shape))
            r = np.repeat(np.arange(len(a), dtype=np.int32)[:, None], 2, axis=1)
        else:
            r = np.asarray(pr[2])
            r = (np.stack(r, axis=1) if isinstance(pr[2], tuple) else r).astype(np.int32).reshape(-1, 2)
        srcs.append(a)
        dsts.append(b)
        rows.append(r)
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    n = len(srcs)
    if n == 0:
        return []
    cum = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    s_off, d_off, r_off = cum(srcs), cum(dsts), cum(rows)
    count = np.diff(r_off).astype(np.int32)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_src, t_dst = _dev(np.concatenate(srcs), dev), _dev(np.concatenate(dsts), dev)
        t_rows = _dev(np.concatenate(rows), dev)
        t_so, t_do, t_ro, t_cnt = _dev(s_off, dev), _dev(d_off, dev), _dev(r_off, dev), _dev(count, dev)
        t_T, t_info, t_clique = _fit_enqueue(lib, t_src.data_ptr(), t_so.data_ptr(), t_dst.data_ptr(), t_do.data_ptr(), t_rows.data_ptr(),
                                             t_ro.data_ptr(), t_cnt.data_ptr(), n, c, budget, r_off, count, dev)
        T, info, clique = t_T.cpu().numpy(), t_info.cpu().numpy(), t_clique.cpu().numpy()
    return _fits(T, info, clique, r_off)


class TeaserSuccess(Success):
    """The success flag of `solve_teaser` / `compute_transform(coarse="teaser")`: truthy iff the maximum clique has MORE
    members than min_inliers (the reference's test, icp_utils.py:136).  Besides the ICP figures of `Success` it carries
    `clique_size`, `certified`, `status`, `matches` (the mutual matches the fit started from) and `coarse`, the 4 x 4 of
    the robust fit before the refinement."""

    def __init__(self, ok, result, fit):
        Success.__init__(self, ok, result)
        self.clique_size = fit.clique_size
        self.certified = fit.certified
        self.status = fit.status
        self.matches = fit.correspondences
        self.clique = fit.clique
        self.nodes = fit.nodes
        self.coarse = fit.transformation

    def __repr__(self):
        return "TeaserSuccess(%s, clique_size=%d of %d matches, certified=%s, fitness=%.4f, inlier_rmse=%.4f)" % (
            self.ok, self.clique_size, self.matches, self.certified, self.fitness, self.inlier_rmse)


def solve_teaser_pairs(pairs, voxel_size, min_inliers, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0):
    """The reference's `solve_teaser` (icp_utils.py:103-139) for a list of (src, dst) pairs in ONE batched chain on the
    device: one upload, FPFH of all 2n clouds, mutual matches, the robust fit with noise_bound = voxel_size, and
    `registration_icp(voxel_size, 100 iterations)` from the fit's transforms.  Returns per pair (valid, translation,
    rotation) with dst ~ rotation . src + translation; `valid` is a `TeaserSuccess`: clique size > min_inliers.  A pair
    that is not valid returns the unrefined fit, as the reference does."""
    c, budget = _noise(voxel_size), _budget(node_budget)
    pairs = list(pairs)
    srcs = [_points(s) for s, _ in pairs]
    dsts = [_points(d) for _, d in pairs]
    if any(len(x) == 0 for x in srcs + dsts):
        raise ValueError("every cloud needs at least one point with finite coordinates")
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    n = len(pairs)
    if n == 0:
        return []
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_in, off, head = _upload_clouds(srcs + dsts, dev)               # the sources, then the targets
        lists = _knn_enqueue(lib, t_in, off, head, 5.0 * c, 100)
        t_n = _normals_enqueue(lib, t_in, off, head, lists, 2.0 * c, 30, (0.0, 0.0, 0.0))
        t_f = _fpfh_enqueue(lib, t_in, off, head, t_n, lists, False)
        a_off = off[:n + 1].copy()
        b_off = (off[n:] - off[n]).copy()
        na, nb = int(a_off[-1]), int(b_off[-1])
        t_bo = torch.from_numpy(b_off).to(dev)
        p_src, p_so = t_in.data_ptr() + head, t_in.data_ptr()
        p_dst, p_do = p_src + 24 * na, t_bo.data_ptr()
        t_m = torch.empty(3 * na + nb + n, dtype=torch.int32, device=dev)     # nn01 | nn10 | rows | counts
        p_rows, p_cnt = t_m.data_ptr() + 4 * (na + nb), t_m.data_ptr() + 4 * (3 * na + nb)
        _lib.check(lib.cslam_feature_match_dev(t_f.data_ptr(), p_so, t_f.data_ptr() + 8 * FPFH_BINS * na, p_do, n, FPFH_BINS, t_m.data_ptr(),
                                               t_m.data_ptr() + 4 * na, p_rows, p_cnt, _host(a_off), _host(b_off), _stream()))
        t_T, t_info, t_clique = _fit_enqueue(lib, p_src, p_so, p_dst, p_do, p_rows, p_so, p_cnt, n, c, budget, a_off, None, dev)
        t_ref = torch.empty((n, 16), dtype=torch.float64, device=dev)
        t_stats = torch.empty((n, 4), dtype=torch.float64, device=dev)
        dists, iters = np.array([c]), np.array([100], dtype=np.int32)
        _lib.check(lib.cslam_icp_register_dev(p_src, p_so, p_dst, p_do, n, t_T.data_ptr(), _host(dists), _host(iters), 1, 1e-6, 1e-6,
                                              t_ref.data_ptr(), t_stats.data_ptr(), _stream()))
        out = torch.cat((t_T, t_ref, t_stats, t_info.to(torch.float64)), dim=1).cpu().numpy()     # one copy of the results
        clique = t_clique.cpu().numpy()
    fits = _fits(out[:, :16], out[:, 36:42].astype(np.int64), clique, a_off)
    results = []
    for p, fit in enumerate(fits):
        valid = fit.status == 0 and fit.clique_size > min_inliers
        T = out[p, 16:32].reshape(4, 4).copy() if valid else fit.transformation
        icp = RegistrationResult(T, float(out[p, 32]), float(out[p, 33]), int(out[p, 34]), int(out[p, 35]))
        results.append((TeaserSuccess(valid, icp, fit), T[:3, 3].copy(), T[:3, :3].copy()))
    return results


def solve_teaser(src, dst, voxel_size, min_inliers, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0):
    """Counterpart of the reference's solve_teaser (icp_utils.py:103-139), same name and argument order: (valid,
    translation, rotation)."""
    return solve_teaser_pairs([(src, dst)], voxel_size, min_inliers, node_budget, device)[0]


def _register(pairs, inits, max_dists, max_iters, relative_fitness, relative_rmse, want_correspondences, device):
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    srcs = [_points(s) for s, _ in pairs]
    dsts = [_points(d) for _, d in pairs]
    n = len(pairs)
    if n == 0:
        return []
    s_off = np.zeros(n + 1, dtype=np.int64)
    d_off = np.zeros(n + 1, dtype=np.int64)
    s_off[1:] = np.cumsum([len(c) for c in srcs])
    d_off[1:] = np.cumsum([len(c) for c in dsts])
    init = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float64).reshape(4, 4) for T in inits]).reshape(n, 16))
    dists = np.ascontiguousarray(max_dists, dtype=np.float64)
    iters = np.ascontiguousarray(max_iters, dtype=np.int32)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_src = torch.from_numpy(np.concatenate(srcs, axis=0)).to(dev)
        t_dst = torch.from_numpy(np.concatenate(dsts, axis=0)).to(dev)
        t_so = torch.from_numpy(s_off).to(dev)
        t_do = torch.from_numpy(d_off).to(dev)
        t_init = torch.from_numpy(init).to(dev)
        t_T = torch.empty((n, 16), dtype=torch.float64, device=dev)
        t_stats = torch.empty((n, 4), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.cslam_icp_register_dev(
            t_src.data_ptr(), t_so.data_ptr(), t_dst.data_ptr(), t_do.data_ptr(), n, t_init.data_ptr(),
            dists.ctypes.data_as(C.c_void_p), iters.ctypes.data_as(C.c_void_p), len(dists), float(relative_fitness),
            float(relative_rmse), t_T.data_ptr(), t_stats.data_ptr(), st))
        t_idx = None
        if want_correspondences:
            t_idx = torch.empty(int(s_off[-1]), dtype=torch.int32, device=dev)
            t_d2 = torch.empty(int(s_off[-1]), dtype=torch.float64, device=dev)
            _lib.check(lib.cslam_icp_correspondences_dev(
                t_src.data_ptr(), t_so.data_ptr(), t_dst.data_ptr(), t_do.data_ptr(), n, t_T.data_ptr(),
                float(dists[-1]), t_idx.data_ptr(), t_d2.data_ptr(), st))
        out = torch.cat((t_T, t_stats), dim=1).cpu().numpy()          # the one device -> host copy of the results
        idx = t_idx.cpu().numpy() if t_idx is not None else None
    results = []
    for p in range(n):
        corr = None
        if idx is not None:
            mine = idx[s_off[p]:s_off[p + 1]]
            rows = np.nonzero(mine >= 0)[0]
            corr = np.stack([rows, mine[rows].astype(np.int64)], axis=1)
        results.append(RegistrationResult(out[p, :16].reshape(4, 4).copy(), float(out[p, 16]), float(out[p, 17]),
                                          int(out[p, 18]), int(out[p, 19]), corr))
    return results


def nearest_correspondences(pairs, max_correspondence_distance, transformations=None, device=0):
    """One evaluation for a list of (src, dst) pairs (`cslam_icp_correspondences_dev`): per pair (idx, dist2), where
    idx[i] is the target row nearest to T . src[i] (ties -> the lower row), -1 when it is farther than the radius, and
    dist2[i] its squared distance either way.  `transformations`: one 4 x 4 per pair, None = identity."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    pairs = [(_points(s), _points(d)) for s, d in pairs]
    n = len(pairs)
    if n == 0:
        return []
    s_off = np.zeros(n + 1, dtype=np.int64)
    d_off = np.zeros(n + 1, dtype=np.int64)
    s_off[1:] = np.cumsum([len(s) for s, _ in pairs])
    d_off[1:] = np.cumsum([len(d) for _, d in pairs])
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        t_src = torch.from_numpy(np.concatenate([s for s, _ in pairs], axis=0)).to(dev)
        t_dst = torch.from_numpy(np.concatenate([d for _, d in pairs], axis=0)).to(dev)
        t_so = torch.from_numpy(s_off).to(dev)
        t_do = torch.from_numpy(d_off).to(dev)
        t_T = None
        if transformations is not None:
            t_T = torch.from_numpy(np.ascontiguousarray(
                np.stack([np.asarray(T, dtype=np.float64).reshape(16) for T in transformations]))).to(dev)
            assert t_T.shape == (n, 16)
        t_idx = torch.empty(int(s_off[-1]), dtype=torch.int32, device=dev)
        t_d2 = torch.empty(int(s_off[-1]), dtype=torch.float64, device=dev)
        _lib.check(lib.cslam_icp_correspondences_dev(
            t_src.data_ptr(), t_so.data_ptr(), t_dst.data_ptr(), t_do.data_ptr(), n,
            t_T.data_ptr() if t_T is not None else None, float(max_correspondence_distance), t_idx.data_ptr(),
            t_d2.data_ptr(), torch.cuda.current_stream().cuda_stream))
        idx, d2 = t_idx.cpu().numpy(), t_d2.cpu().numpy()
    return [(idx[s_off[p]:s_off[p + 1]], d2[s_off[p]:s_off[p + 1]]) for p in range(n)]


def registration_icp(src, dst, max_correspondence_distance, init=np.eye(4), max_iteration=100, relative_fitness=1e-6,
                     relative_rmse=1e-6, device=0):
    """open3d.pipelines.registration.registration_icp with TransformationEstimationPointToPoint: one stage.
    `transformation` maps source to target; `correspondence_set` is [n, 2] (source row, target row) at the result."""
    return _register([(src, dst)], [init], [max_correspondence_distance], [max_iteration], relative_fitness,
                     relative_rmse, True, device)[0]


def registration_icp_pairs(pairs, max_correspondence_distance, inits=None, max_iteration=100, relative_fitness=1e-6,
                           relative_rmse=1e-6, device=0):
    """`registration_icp` for a list of (src, dst) pairs in ONE batched call: one radius and one iteration cap for all,
    `inits` one 4 x 4 per pair (None = the identity for all).  A pair's result is the same bits as alone."""
    pairs = list(pairs)
    inits = [np.eye(4)] * len(pairs) if inits is None else list(inits)
    if len(inits) != len(pairs):
        raise ValueError("inits has %d entries for %d pairs" % (len(inits), len(pairs)))
    return _register(pairs, inits, [max_correspondence_distance], [max_iteration], relative_fitness, relative_rmse, True,
                     device)


def register_pairs(pairs, voxel_size, init_yaw_deg=None, stages=DEFAULT_STAGES, correspondence_sets=False, device=0):
    """Register a list of (src, dst) pairs in ONE batched call.  `init_yaw_deg`: None, one ScanContext yaw shift for
    all pairs, or one per pair (entries may be None).  Stage s runs open3d's loop with the radius
    stages[s][0] * voxel_size and at most stages[s][1] iterations from the previous stage's transform.  Returns one
    `RegistrationResult` per pair (fitness, rmse, correspondences, iterations of the last stage)."""
    pairs = list(pairs)
    if init_yaw_deg is None or np.isscalar(init_yaw_deg):
        yaws = [init_yaw_deg] * len(pairs)
    else:
        yaws = list(init_yaw_deg)
        if len(yaws) != len(pairs):
            raise ValueError("init_yaw_deg has %d entries for %d pairs" % (len(yaws), len(pairs)))
    return _register(pairs, [yaw_seed(y) for y in yaws], [float(m) * voxel_size for m, _ in stages],
                     [int(i) for _, i in stages], 1e-6, 1e-6, correspondence_sets, device)


def _accept(result, min_inliers, min_fitness):
    return result.correspondences > min_inliers and result.fitness >= min_fitness


def _coarse(coarse):
    if coarse not in ("yaw", "teaser"):
        raise ValueError("coarse is 'yaw' or 'teaser', got %r" % (coarse,))
    return coarse


def solve_icp(src, dst, voxel_size, min_inliers, init_yaw_deg=None, min_fitness=0.0, coarse="yaw"):
    """Counterpart of the reference's solve_teaser (icp_utils.py:103-139): (valid, translation, rotation) with
    dst ~ rotation . src + translation.  coarse="teaser": `solve_teaser` itself (`init_yaw_deg` and `min_fitness` are
    not used)."""
    if _coarse(coarse) == "teaser":
        return solve_teaser(src, dst, voxel_size, min_inliers)
    r = register_pairs([(src, dst)], voxel_size, init_yaw_deg)[0]
    return _accept(r, min_inliers, min_fitness), r.transformation[:3, 3].copy(), r.transformation[:3, :3].copy()


def compute_transform(src, dst, voxel_size, min_inliers, init_yaw_deg=None, min_fitness=0.0, coarse="yaw"):
    """Computes a 3D transform between 2 point clouds (reference icp_utils.py:178-196), dst ~ R . src + t, as
    registration_icp(source=src, target=dst) gives it.

    Args:
        src, dst: point clouds ([n, >=3] arrays or objects with `.points`) as `downsample(cloud, voxel_size)` returns them
        voxel_size: correspondence radius of the final stage (the coarse stages use 4x and 2x)
        min_inliers (int): the registration succeeds with MORE correspondences than this in the final stage ...
        init_yaw_deg: `ScanContextMatching.last_yaw_diff_deg` of the match (None: start from the identity)
        min_fitness: ... and a final fitness (correspondences / source points) of at least this
        coarse: "yaw" (the default: the staged ICP from the ScanContext yaw, as described above) or "teaser": the
            reference's own path, `solve_teaser` -- FPFH, mutual matches, the robust fit, one ICP stage; `init_yaw_deg`
            and `min_fitness` are not used, and the success flag is the reference's: clique size > min_inliers

    Returns:
        (Transform, Success): the transform message and a success flag that is truthy / falsy like the reference's bool
        and carries `fitness`, `inlier_rmse`, `correspondences`, `iterations` and the 4 x 4 `transformation`.

    A correspondence count is a MUCH weaker test than the size of TEASER++'s maximum clique, which the reference
    compares with min_inliers: the clique certifies mutually consistent matches, a count only says how many source points
    have some target point within voxel_size.  A wrong alignment of two clouds that share a ground plane still has a
    fitness of about 0.6 (thousands of "inliers"), a right one is above 0.9 on the same clouds.  Set `min_fitness`, or
    use coarse="teaser", whose test is the clique itself.
    """
    if _coarse(coarse) == "teaser":
        valid, t, R = solve_teaser(src, dst, voxel_size, min_inliers)
        return to_transform_msg(t, R), valid
    r = register_pairs([(src, dst)], voxel_size, init_yaw_deg)[0]
    transform = to_transform_msg(r.transformation[:3, 3], r.transformation[:3, :3])
    return transform, Success(_accept(r, min_inliers, min_fitness), r)


def _quaternion(Rm):
    """(x, y, z, w) of a rotation matrix: the largest of the four squared components first, the rest from the
    off-diagonal sums (Shepperd's method)."""
    m = np.asarray(Rm, dtype=np.float64)
    d = [m[0, 0], m[1, 1], m[2, 2]]
    four = [1 + d[0] - d[1] - d[2], 1 - d[0] + d[1] - d[2], 1 - d[0] - d[1] + d[2], 1 + d[0] + d[1] + d[2]]
    k = int(np.argmax(four))
    q = np.empty(4)
    q[k] = 0.5 * np.sqrt(four[k])
    f = 0.25 / q[k]
    if k == 3:
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * f, (m[0, 2] - m[2, 0]) * f, (m[1, 0] - m[0, 1]) * f
    else:
        i, j = (k + 1) % 3, (k + 2) % 3
        q[i] = (m[i, k] + m[k, i]) * f
        q[j] = (m[j, k] + m[k, j]) * f
        q[3] = (m[j, i] - m[i, j]) * f
    return q


class _Vec:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Transform:
    """Stand-in with the attributes of geometry_msgs.msg.Transform, for hosts without ROS."""

    def __init__(self):
        self.translation = _Vec(x=0.0, y=0.0, z=0.0)
        self.rotation = _Vec(x=0.0, y=0.0, z=0.0, w=1.0)


def to_transform_msg(translation, rotation):
    """geometry_msgs.msg.Transform of (translation, rotation matrix) when ROS is importable (icp_utils.py:142-153),
    else an object with the same `.translation.{x,y,z}` / `.rotation.{x,y,z,w}` attributes."""
    try:
        from geometry_msgs.msg import Transform
    except ImportError:
        Transform = _Transform
    T = Transform()
    T.translation.x, T.translation.y, T.translation.z = (float(v) for v in translation)
    q = _quaternion(rotation)
    T.rotation.x, T.rotation.y, T.rotation.z, T.rotation.w = (float(v) for v in q)
    return T
