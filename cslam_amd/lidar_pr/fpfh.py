"""FPFH features and mutual matches of lidar clouds (csrc/fpfh.hip): the counterparts of the reference's `extract_fpfh`,
`find_knn_cpu` and `find_correspondences` (icp_utils.py:26-65), batched.  The `*_enqueue` functions take a `_batch.Packed`
(device pointers and host offsets) and leave their results on the device: `icp_utils.solve_teaser_pairs` chains them."""
import collections

import numpy as np

from .. import _lib
from ._batch import gpu, host, rows, split, stream, upload

KNN_BLOCK = 256       # threads per workgroup of the radius search (csrc/fpfh.hip): one wave per query point, four per workgroup
KNN_CHUNK = 1024      # cloud points per LDS chunk of the radius search; the tests size around it
KNN_CAND = 512        # candidate buffer of a query: more in-radius points than this are cut to the best max_nn - 1 on the way
KNN_MAX_NN = 256      # widest neighbour list
FM_BLOCK = 64         # query rows per workgroup of the feature matching kernel
FM_CHUNK = 32         # target rows per LDS chunk of the feature matching kernel
FM_MAX_LANES = 16     # chunk lanes of its grid: a target of more chunks than this is walked lane-strided
FM_MAX_DIM = 64       # widest feature
FPFH_BINS = 33


def knn_enqueue(lib, cl, radius, max_nn):
    """`cslam_knn_radius_dev` on uploaded clouds (at least one point in all): device (idx, d2, count)."""
    import torch
    total, dev = int(cl.off[-1]), cl.buf.device
    t_idx = torch.empty((total, max_nn), dtype=torch.int32, device=dev)
    t_d2 = torch.empty((total, max_nn), dtype=torch.float64, device=dev)
    t_cnt = torch.empty(total, dtype=torch.int32, device=dev)
    _lib.check(lib.cslam_knn_radius_dev(cl.rows, cl.d_off, len(cl.off) - 1, float(radius), int(max_nn), t_idx.data_ptr(),
                                        t_d2.data_ptr(), t_cnt.data_ptr(), host(cl.off), stream()))
    return t_idx, t_d2, t_cnt


def normals_enqueue(lib, cl, lists, radius, max_nn, viewpoint):
    import torch
    t_idx, t_d2, t_cnt = lists
    view = np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
    t_n = torch.empty((int(cl.off[-1]), 3), dtype=torch.float64, device=cl.buf.device)
    _lib.check(lib.cslam_normals_dev(cl.rows, cl.d_off, len(cl.off) - 1, t_idx.data_ptr(), t_d2.data_ptr(), t_cnt.data_ptr(),
                                     t_idx.shape[1], float(radius), int(max_nn), host(view), t_n.data_ptr(), host(cl.off), stream()))
    return t_n


def fpfh_enqueue(lib, cl, t_normals, lists, spfh):
    """Device [total, 33] FPFH, or [2, total, 33] (FPFH, SPFH) with `spfh`."""
    import torch
    t_idx, t_d2, t_cnt = lists
    t_f = torch.empty((2 if spfh else 1, int(cl.off[-1]), FPFH_BINS), dtype=torch.float64, device=cl.buf.device)
    _lib.check(lib.cslam_fpfh_dev(cl.rows, t_normals.data_ptr(), cl.d_off, len(cl.off) - 1, t_idx.data_ptr(), t_d2.data_ptr(),
                                  t_cnt.data_ptr(), t_idx.shape[1], t_f.data_ptr(), t_f[1].data_ptr() if spfh else None,
                                  host(cl.off), stream()))
    return t_f if spfh else t_f[0]


def extract_enqueue(lib, cl, voxel_size, viewpoint):
    """The reference's `extract_fpfh` on uploaded clouds: device [total, 33].  One neighbour search at (5 voxels, 100) serves
    both steps: the normals at (2 voxels, 30) use the prefix of each list, which is the list a search of their own returns."""
    return extract_with_normals_enqueue(lib, cl, voxel_size, viewpoint)[0]


def extract_with_normals_enqueue(lib, cl, voxel_size, viewpoint):
    """`extract_enqueue` and the normals it computes on the way: device ([total, 33], [total, 3])."""
    lists = knn_enqueue(lib, cl, 5.0 * voxel_size, 100)
    t_n = normals_enqueue(lib, cl, lists, 2.0 * voxel_size, 30, viewpoint)
    return fpfh_enqueue(lib, cl, t_n, lists, False), t_n


class Matches(collections.namedtuple("Matches", "buf nn10 rows counts")):
    """The one int32 device buffer of a matching call, nn01 | nn10 | rows | counts, and where its parts begin (in elements;
    nn01 at 0): per pair the nearest target row of every source row, the nearest source row of every target row, the mutual
    rows (source row, target row) from the pair's first source row on, and how many of them there are."""

    def ptr(self, part):
        return self.buf.data_ptr() + 4 * part


def match_enqueue(lib, fa, fb, dim):
    """`cslam_feature_match_dev` on device features ([n_k, dim] rows of the sources `fa` and of the targets `fb`): `Matches`."""
    import torch
    n, na, nb = len(fa.off) - 1, int(fa.off[-1]), int(fb.off[-1])
    m = Matches(torch.empty(3 * na + nb + n, dtype=torch.int32, device=fa.buf.device), na, na + nb, 3 * na + nb)
    _lib.check(lib.cslam_feature_match_dev(fa.rows, fa.d_off, fb.rows, fb.d_off, n, dim, m.ptr(0), m.ptr(m.nn10), m.ptr(m.rows),
                                           m.ptr(m.counts), host(fa.off), host(fb.off), stream()))
    return m


def radius_neighbors_clouds(clouds, radius, max_nn, device=0):
    """The neighbour lists the normals and the features are computed from (`cslam_knn_radius_dev`, the counterpart of
    open3d's KDTreeSearchParamHybrid(radius, max_nn)) for a list of clouds in one call: per cloud (idx [n, max_nn] int32,
    d2 [n, max_nn], count [n]).  The list of point i is i itself, then the other points within the radius in ascending
    (d2, index), `max_nn` entries at most; beyond the count idx is -1 and d2 is +inf."""
    with gpu(device) as (lib, dev):
        clouds = [rows(c, finite=True) for c in clouds]
        if sum(len(c) for c in clouds) == 0:
            if not (np.isfinite(radius) and radius > 0 and 1 <= max_nn <= KNN_MAX_NN):
                raise _lib.CslamHipError("invalid argument: radius must be positive and finite, max_nn in [1, %d]" % KNN_MAX_NN)
            return [(np.zeros((0, max_nn), np.int32), np.zeros((0, max_nn)), np.zeros(0, np.int32)) for _ in clouds]
        cl = upload(clouds, dev)
        idx, d2, cnt = (t.cpu().numpy() for t in knn_enqueue(lib, cl, radius, max_nn))
    return list(zip(split(idx, cl.off), split(d2, cl.off), split(cnt, cl.off)))


def radius_neighbors(cloud, radius, max_nn, device=0):
    return radius_neighbors_clouds([cloud], radius, max_nn, device)[0]


def estimate_normals_clouds(clouds, radius, max_nn=30, viewpoint=(0.0, 0.0, 0.0), device=0):
    """open3d's `estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))` for a list of clouds in one call: per cloud
    the [n, 3] unit normals.  The eigenvector of the smallest eigenvalue of the neighbours' covariance; (0, 0, 1) with
    fewer than 3 neighbours (the point included).  The sign is fixed, which open3d leaves to its eigen-solver: every
    normal points to the side of `viewpoint` (default: the sensor at the origin of a keyframe cloud)."""
    with gpu(device) as (lib, dev):
        clouds = [rows(c, finite=True) for c in clouds]
        if sum(len(c) for c in clouds) == 0:
            return [np.zeros((0, 3)) for _ in clouds]
        cl = upload(clouds, dev)
        lists = knn_enqueue(lib, cl, radius, max_nn)
        normals = normals_enqueue(lib, cl, lists, radius, max_nn, viewpoint).cpu().numpy()
    return split(normals, cl.off)


def estimate_normals(cloud, radius, max_nn=30, viewpoint=(0.0, 0.0, 0.0), device=0):
    return estimate_normals_clouds([cloud], radius, max_nn, viewpoint, device)[0]


def compute_fpfh_feature(cloud, normals, radius, max_nn=100, return_spfh=False, device=0):
    """open3d's `compute_fpfh_feature(cloud, KDTreeSearchParamHybrid(radius, max_nn))` with the normals given: the
    [n, 33] features, one ROW per point (the reference transposes open3d's [33, n], icp_utils.py:37); with
    `return_spfh` the pair (FPFH, SPFH)."""
    with gpu(device) as (lib, dev):
        import torch
        pts = rows(cloud, finite=True)
        nrm = np.ascontiguousarray(normals, dtype=np.float64)
        if nrm.shape != pts.shape:
            raise ValueError("normals of shape %s for %d points with finite coordinates" % (nrm.shape, len(pts)))
        if len(pts) == 0:
            return (np.zeros((0, FPFH_BINS)),) * 2 if return_spfh else np.zeros((0, FPFH_BINS))
        cl = upload([pts], dev)
        lists = knn_enqueue(lib, cl, radius, max_nn)
        out = fpfh_enqueue(lib, cl, torch.from_numpy(nrm).to(dev), lists, return_spfh).cpu().numpy()
    return (out[0], out[1]) if return_spfh else out


def extract_fpfh_clouds(clouds, voxel_size, viewpoint=(0.0, 0.0, 0.0), device=0):
    """`extract_fpfh` for a list of clouds in ONE call (one upload, one download)."""
    with gpu(device) as (lib, dev):
        clouds = [rows(c, finite=True) for c in clouds]
        if sum(len(c) for c in clouds) == 0:
            return [np.zeros((0, FPFH_BINS)) for _ in clouds]
        cl = upload(clouds, dev)
        feats = extract_enqueue(lib, cl, voxel_size, viewpoint).cpu().numpy()
    return split(feats, cl.off)


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
    """`match_enqueue` on host features, in one upload and one download: per pair (nn01, nn10, mutual rows [m, 2]), int64."""
    with gpu(device) as (lib, dev):
        pairs = [(_features(a), _features(b)) for a, b in pairs]
        n = len(pairs)
        if n == 0:
            return []
        dim = pairs[0][0].shape[1]
        if any(a.shape[1] != dim or b.shape[1] != dim for a, b in pairs):
            raise ValueError("all feature arrays of a call need the same dimension")
        fa, fb = upload([a for a, _ in pairs], dev), upload([b for _, b in pairs], dev)
        m = match_enqueue(lib, fa, fb, dim)
        out = m.buf.cpu().numpy().astype(np.int64)
    nn10, mutual, a_off, b_off = out[m.nn10:m.rows], out[m.rows:m.counts].reshape(-1, 2), fa.off, fb.off
    return [(out[a_off[p]:a_off[p + 1]], nn10[b_off[p]:b_off[p + 1]], mutual[a_off[p]:a_off[p] + out[m.counts + p]])
            for p in range(n)]


def find_knn(feat0, feat1, device=0):
    """For every row of feat0 the nearest row of feat1 in squared Euclidean distance, ties -> the lower row (the
    reference's `find_knn_cpu` with knn=1, icp_utils.py:40-46), brute force on the GPU."""
    return _match([(feat0, feat1)], device)[0][0]


def find_correspondences_pairs(pairs, mutual_filter=True, device=0):
    """`find_correspondences` for a list of (feats0, feats1) in ONE call: per pair (idx0, idx1)."""
    return [(mutual[:, 0].copy(), mutual[:, 1].copy()) if mutual_filter else (np.arange(len(nn01)), nn01)
            for nn01, _, mutual in _match(pairs, device)]


def find_correspondences(feats0, feats1, mutual_filter=True, device=0):
    """Counterpart of the reference's `find_correspondences` (icp_utils.py:49-65): rows (idx0[k], idx1[k]) are each
    other's nearest neighbour in feature space; without the filter every row of feats0 with its nearest in feats1."""
    return find_correspondences_pairs([(feats0, feats1)], mutual_filter, device)[0]
