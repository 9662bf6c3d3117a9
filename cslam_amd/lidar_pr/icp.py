"""Batched ICP (csrc/icp.hip): open3d's `registration_icp` with TransformationEstimationPointToPoint (the default) or
TransformationEstimationPointToPlane (`estimation="point_to_plane"`, csrc/plane.h) in float64, brute-force nearest
neighbours and a fixed summation order -- a pair's result is the same bits alone or in any batch.  Every call uploads its
clouds in one copy: the sources, then the targets; normals given by the caller follow in a copy of their own.

Point-to-plane needs about a third of the updates on street scenes (ground and walls slide under point-to-point) but has
the narrower basin: from a ScanContext yaw seed run it through `DEFAULT_STAGES`, not in one stage at the voxel radius.  A
singular system (all normals parallel, fewer than six correspondences, |det| < 1e-6) leaves the transform as it is;
parity of that rule with open3d is not pinned (include/cslam_hip.h)."""
import numpy as np

from .. import _lib
from . import fpfh
from ._batch import gpu, host, rows, stream, upload

# (multiple of voxel_size, max iterations) per stage; the last is the reference's refinement (icp_utils.py:126-131)
DEFAULT_STAGES = ((4.0, 30), (2.0, 30), (1.0, 100))
ICP_CHUNK = 1024      # target points per LDS chunk of the nearest-neighbour kernel (csrc/icp.hip); the tests size around it
ICP_MAX_LANES = 64    # chunk lanes of its grid: a target of more chunks than this is walked lane-strided
ESTIMATIONS = ("point_to_point", "point_to_plane")
NORMALS_RADIUS, NORMALS_MAX_NN = 2.0, 30      # target normals from voxel_size: the reference's extract_fpfh (icp_utils.py:28-30)


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


def plane(estimation):
    """True for "point_to_plane", False for "point_to_point"; anything else is a ValueError (raised before the GPU is touched)."""
    if estimation not in ESTIMATIONS:
        raise ValueError("estimation is 'point_to_point' or 'point_to_plane', got %r" % (estimation,))
    return estimation == "point_to_plane"


def register_enqueue(lib, a, b, p_init, max_dists, max_iters, relative_fitness, relative_rmse, p_normals=None):
    """`cslam_icp_register_dev` on uploaded sources `a` and targets `b` from the device transforms at `p_init`, one stage
    per entry of the host arrays `max_dists` (float64) and `max_iters` (int32): device (T [n, 16], stats [n, 4]).  With
    `p_normals`, the device pointer of the targets' normals (rows as `b`): `cslam_icp_register_plane_dev`."""
    import torch
    n, dev = len(a.off) - 1, a.buf.device
    t_T = torch.empty((n, 16), dtype=torch.float64, device=dev)
    t_stats = torch.empty((n, 4), dtype=torch.float64, device=dev)
    tail = (n, p_init, host(max_dists), host(max_iters), len(max_dists), float(relative_fitness), float(relative_rmse),
            t_T.data_ptr(), t_stats.data_ptr(), stream())
    if p_normals is None:
        _lib.check(lib.cslam_icp_register_dev(a.rows, a.d_off, b.rows, b.d_off, *tail))
    else:
        _lib.check(lib.cslam_icp_register_plane_dev(a.rows, a.d_off, b.rows, b.d_off, p_normals, *tail))
    return t_T, t_stats


def target_normals_enqueue(lib, b, voxel_size):
    """Normals of the uploaded targets `b` at the reference's `extract_fpfh` parameters (2 voxels, 30 neighbours, viewpoint
    at the origin): device [target rows, 3]."""
    radius = NORMALS_RADIUS * voxel_size
    return fpfh.normals_enqueue(lib, b, fpfh.knn_enqueue(lib, b, radius, NORMALS_MAX_NN), radius, NORMALS_MAX_NN, (0.0, 0.0, 0.0))


def correspondences_enqueue(lib, a, b, p_T, max_dist):
    """`cslam_icp_correspondences_dev` on uploaded sources `a` and targets `b` under the device transforms at `p_T` (None =
    identity): device (idx [source rows] int32, dist2 [source rows])."""
    import torch
    total, dev = int(a.off[-1]), a.buf.device
    t_idx = torch.empty(total, dtype=torch.int32, device=dev)
    t_d2 = torch.empty(total, dtype=torch.float64, device=dev)
    _lib.check(lib.cslam_icp_correspondences_dev(a.rows, a.d_off, b.rows, b.d_off, len(a.off) - 1, p_T, float(max_dist), t_idx.data_ptr(),
                                                 t_d2.data_ptr(), stream()))
    return t_idx, t_d2


def _upload(pairs, dev):
    """The finite rows of (src, dst) pairs in one copy, the sources, then the targets: `Packed` sources and targets.  A side
    without any point has NULL rows, which the library refuses by that name."""
    sides = upload([rows(s, finite=True) for s, _ in pairs] + [rows(d, finite=True) for _, d in pairs], dev, pairs=True)[1:]
    return [x if x.off[-1] else x._replace(rows=None) for x in sides]


def _given_normals(estimation, pairs, normals):
    """The argument errors of the two estimators, and for point-to-plane the caller's normals per pair, float64, through the
    finite-row filter of their target: a normal whose target row is dropped is dropped with it.  None for point-to-point."""
    if not plane(estimation):
        if normals is not None:
            raise ValueError("target_normals are used by estimation='point_to_plane' only")
        return None
    if normals is None:
        raise ValueError("estimation='point_to_plane' needs target_normals: one [n_dst, 3] array per target")
    if isinstance(normals, np.ndarray) and normals.ndim == 2:
        normals = [normals] * len(pairs)
    normals = list(normals)
    if len(normals) != len(pairs):
        raise ValueError("target_normals has %d entries for %d pairs" % (len(normals), len(pairs)))
    out = []
    for (_, d), nr in zip(pairs, normals):
        pts, nr = rows(d), np.asarray(nr)
        if nr.shape != (len(pts), 3):
            raise ValueError("target_normals of shape %s for a target of %d points" % (nr.shape, len(pts)))
        out.append(np.ascontiguousarray(nr, dtype=np.float64)[np.isfinite(pts).all(axis=1)])
    return out


def _register(pairs, inits, max_dists, max_iters, relative_fitness, relative_rmse, want_correspondences, device, normals=None,
              normals_voxel=None):
    """`normals`: per pair the host normals of the finite target rows; `normals_voxel`: estimate them on the device at this
    voxel size instead; neither: point-to-point."""
    with gpu(device) as (lib, dev):
        import torch
        n = len(pairs)
        if n == 0:
            return []
        a, b = _upload(pairs, dev)
        p_normals = None
        if normals is not None:
            t_n = upload(normals, dev)
            p_normals = t_n.rows
        elif normals_voxel is not None:
            t_n = target_normals_enqueue(lib, b, normals_voxel)
            p_normals = t_n.data_ptr()
        init = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float64).reshape(4, 4) for T in inits]).reshape(n, 16))
        dists, iters = np.ascontiguousarray(max_dists, dtype=np.float64), np.ascontiguousarray(max_iters, dtype=np.int32)
        t_init = torch.from_numpy(init).to(dev)
        t_T, t_stats = register_enqueue(lib, a, b, t_init.data_ptr(), dists, iters, relative_fitness, relative_rmse, p_normals)
        t_idx = correspondences_enqueue(lib, a, b, t_T.data_ptr(), dists[-1])[0] if want_correspondences else None
        out = torch.cat((t_T, t_stats), dim=1).cpu().numpy()          # the one device -> host copy of the results
        idx = t_idx.cpu().numpy() if t_idx is not None else None
    results = []
    for p in range(n):
        corr = None
        if idx is not None:
            mine = idx[a.off[p]:a.off[p + 1]]
            hit = np.nonzero(mine >= 0)[0]
            corr = np.stack([hit, mine[hit].astype(np.int64)], axis=1)
        results.append(RegistrationResult(out[p, :16].reshape(4, 4).copy(), float(out[p, 16]), float(out[p, 17]),
                                          int(out[p, 18]), int(out[p, 19]), corr))
    return results


def nearest_correspondences(pairs, max_correspondence_distance, transformations=None, device=0):
    """One evaluation for a list of (src, dst) pairs (`cslam_icp_correspondences_dev`): per pair (idx, dist2), where
    idx[i] is the target row nearest to T . src[i] (ties -> the lower row), -1 when it is farther than the radius, and
    dist2[i] its squared distance either way.  `transformations`: one 4 x 4 per pair, None = identity."""
    with gpu(device) as (lib, dev):
        import torch
        pairs = list(pairs)
        n = len(pairs)
        if n == 0:
            return []
        a, b = _upload(pairs, dev)
        t_T = None
        if transformations is not None:
            t_T = torch.from_numpy(np.ascontiguousarray(
                np.stack([np.asarray(T, dtype=np.float64).reshape(16) for T in transformations]))).to(dev)
            assert t_T.shape == (n, 16)
        p_T = t_T.data_ptr() if t_T is not None else None
        idx, d2 = (t.cpu().numpy() for t in correspondences_enqueue(lib, a, b, p_T, max_correspondence_distance))
    return [(idx[a.off[p]:a.off[p + 1]], d2[a.off[p]:a.off[p + 1]]) for p in range(n)]


def registration_icp(src, dst, max_correspondence_distance, init=np.eye(4), max_iteration=100, relative_fitness=1e-6,
                     relative_rmse=1e-6, device=0, estimation="point_to_point", target_normals=None):
    """open3d.pipelines.registration.registration_icp with TransformationEstimationPointToPoint: one stage.
    `transformation` maps source to target; `correspondence_set` is [n, 2] (source row, target row) at the result.
    estimation="point_to_plane": TransformationEstimationPointToPlane; `target_normals` [n_dst, 3] is then required, as
    open3d requires normals on the target (`estimate_normals(dst, 2 * voxel_size)` gives the reference's)."""
    normals = _given_normals(estimation, [(src, dst)], None if target_normals is None else [target_normals])
    return _register([(src, dst)], [init], [max_correspondence_distance], [max_iteration], relative_fitness,
                     relative_rmse, True, device, normals)[0]


def registration_icp_pairs(pairs, max_correspondence_distance, inits=None, max_iteration=100, relative_fitness=1e-6,
                           relative_rmse=1e-6, device=0, estimation="point_to_point", target_normals=None):
    """`registration_icp` for a list of (src, dst) pairs in ONE batched call: one radius and one iteration cap for all,
    `inits` one 4 x 4 per pair (None = the identity for all).  A pair's result is the same bits as alone.
    `target_normals` (point-to-plane): one [n_dst, 3] array for all pairs, or one per pair."""
    pairs = list(pairs)
    inits = [np.eye(4)] * len(pairs) if inits is None else list(inits)
    if len(inits) != len(pairs):
        raise ValueError("inits has %d entries for %d pairs" % (len(inits), len(pairs)))
    normals = _given_normals(estimation, pairs, target_normals)
    return _register(pairs, inits, [max_correspondence_distance], [max_iteration], relative_fitness, relative_rmse, True,
                     device, normals)


def register_pairs(pairs, voxel_size, init_yaw_deg=None, stages=DEFAULT_STAGES, correspondence_sets=False, device=0,
                   estimation="point_to_point"):
    """Register a list of (src, dst) pairs in ONE batched call.  `init_yaw_deg`: None, one ScanContext yaw shift for
    all pairs, or one per pair (entries may be None).  Stage s runs open3d's loop with the radius
    stages[s][0] * voxel_size and at most stages[s][1] iterations from the previous stage's transform.  Returns one
    `RegistrationResult` per pair (fitness, rmse, correspondences, iterations of the last stage).
    estimation="point_to_plane": the targets' normals are estimated on the device in the same chain, from the neighbours
    within 2 voxels (30 at most), oriented to the origin.  Keep the coarse stages with it: its basin is the narrower one."""
    use_plane = plane(estimation)
    pairs = list(pairs)
    if init_yaw_deg is None or np.isscalar(init_yaw_deg):
        yaws = [init_yaw_deg] * len(pairs)
    else:
        yaws = list(init_yaw_deg)
        if len(yaws) != len(pairs):
            raise ValueError("init_yaw_deg has %d entries for %d pairs" % (len(yaws), len(pairs)))
    return _register(pairs, [yaw_seed(y) for y in yaws], [float(m) * voxel_size for m, _ in stages],
                     [int(i) for _, i in stages], 1e-6, 1e-6, correspondence_sets, device,
                     normals_voxel=float(voxel_size) if use_plane else None)
