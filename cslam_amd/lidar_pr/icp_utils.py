#!/usr/bin/env python
"""Relative transform between two lidar keyframes on an MI355X: FPFH features, mutual matches, the robust coarse fit
and batched ICP (point-to-point by default, point-to-plane with `estimation="point_to_plane"`).

Counterpart of cslam/lidar_pr/icp_utils.py (`compute_transform`, called by lidar_handler_node.py:115,133 for every
accepted ScanContext match).  The reference runs FPFH + mutual nearest neighbours + TEASER++ for a coarse alignment and
then open3d's `registration_icp(src, dst, voxel_size, T, PointToPoint, max_iteration=100)` (icp_utils.py:126-134), and
accepts the match when TEASER's maximum clique has more than min_inliers members.  Both coarse alignments exist here:
  coarse="yaw" (the default of `compute_transform` / `solve_icp`): the yaw shift of the ScanContext match
      (`ScanContextMatching.last_yaw_diff_deg`), helped by two coarse ICP stages at a larger correspondence radius
      (`DEFAULT_STAGES`); accepted on a correspondence count and a fitness;
  coarse="teaser" (`solve_teaser`, `solve_teaser_pairs`): the reference's path.  `extract_fpfh` and `find_correspondences`
      (icp_utils.py:26-65; fpfh.py over csrc/fpfh.hip) give putative matches that do not come from the alignment under test,
      and the robust fit (robust.py over csrc/robust.hip: `robust_fit_pairs` and its stages) is TEASER++'s algorithm at the
      reference's parameters.  It needs no yaw, and its acceptance test is the reference's: the clique size.
The refinement (icp.py over csrc/icp.hip) keeps open3d's documented semantics exactly in both.  This module holds the
reference's own names; every public name and constant of voxel.py, fpfh.py, robust.py and icp.py is importable from here too.

There is no CPU path: without the library or a GPU every call raises `CslamHipError`.  Parity with open3d itself is not
pinned (no open3d is available to record golden vectors from); the tests hold the kernels to a float64 restatement of
open3d's documented algorithm.

Clouds are [n, >=3] arrays or anything with a `.points` attribute (an open3d cloud); they are widened to float64 and
rows with a non-finite coordinate are dropped, as the reference's `downsample` does.  The clouds the handler stores
and sends are down-sampled ones: `downsample` / `downsample_clouds` (voxel.py over csrc/cloud.hip and csrc/voxel.hip), and
`keyframes.ingest` does it on the upload the ScanContext descriptor uses.

Yaw seed: with `matcher.add_item(descriptor(dst))`, `matcher.search(descriptor(src))`, a source that is the target
scene turned by +a degrees about z (dst ~ Rz(a) . src) matches at `last_yaw_diff_deg` = 360 - a (rounded to the 6 degree
sector).  The seed is therefore the rotation about z by MINUS `init_yaw_deg`.
"""
import numpy as np

from . import fpfh, icp, robust
from ._batch import gpu, rows, upload
from .fpfh import (FM_BLOCK, FM_CHUNK, FM_MAX_DIM, FM_MAX_LANES, FPFH_BINS, KNN_BLOCK, KNN_CAND, KNN_CHUNK, KNN_MAX_NN,  # noqa: F401
                   compute_fpfh_feature, estimate_normals, estimate_normals_clouds, extract_fpfh, extract_fpfh_clouds,
                   find_correspondences, find_correspondences_pairs, find_knn, radius_neighbors, radius_neighbors_clouds)
from .icp import (DEFAULT_STAGES, ESTIMATIONS, ICP_CHUNK, ICP_MAX_LANES, NORMALS_MAX_NN, NORMALS_RADIUS,  # noqa: F401
                  RegistrationResult, Rt2T, nearest_correspondences, register_pairs, registration_icp, registration_icp_pairs,
                  yaw_seed)
from .robust import (ROBUST_DEFAULT_NODE_BUDGET, ROBUST_GRAPH_BLOCK, ROBUST_GRAPH_CHUNK, ROBUST_MAX_N, ROBUST_STACK_DEPTH,  # noqa: F401
                     RobustFit, consistency_graph, consistency_graph_pairs, max_clique, max_clique_graphs, robust_fit_pairs,
                     robust_rotation, robust_rotation_pairs, robust_translation, robust_translation_pairs)
from .voxel import VOXEL_SEG_BLOCK, VOXEL_TILE, VoxelSizeError, downsample, downsample_clouds  # noqa: F401


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


def solve_teaser_pairs(pairs, voxel_size, min_inliers, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0,
                       estimation="point_to_point"):
    """The reference's `solve_teaser` (icp_utils.py:103-139) for a list of (src, dst) pairs in ONE batched chain on the
    device: one upload, FPFH of all 2n clouds, mutual matches, the robust fit with noise_bound = voxel_size, and
    `registration_icp(voxel_size, 100 iterations)` from the fit's transforms.  Returns per pair (valid, translation,
    rotation) with dst ~ rotation . src + translation; `valid` is a `TeaserSuccess`: clique size > min_inliers.  A pair
    that is not valid returns the unrefined fit, as the reference does.  estimation="point_to_plane": the refinement uses
    the targets' normals that the FPFH step has computed anyway."""
    c, budget, use_plane = robust.noise(voxel_size), robust.budget_of(node_budget), icp.plane(estimation)
    pairs = list(pairs)
    srcs = [rows(s, finite=True) for s, _ in pairs]
    dsts = [rows(d, finite=True) for _, d in pairs]
    if any(len(x) == 0 for x in srcs + dsts):
        raise ValueError("every cloud needs at least one point with finite coordinates")
    with gpu(device) as (lib, dev):
        import torch
        if not pairs:
            return []
        both, a, b = upload(srcs + dsts, dev, pairs=True)                # the sources, then the targets
        t_f, t_n = fpfh.extract_with_normals_enqueue(lib, both, c, (0.0, 0.0, 0.0))
        m = fpfh.match_enqueue(lib, a._replace(buf=t_f, rows=t_f.data_ptr()),
                               b._replace(buf=t_f, rows=t_f[int(a.off[-1]):].data_ptr()), FPFH_BINS)
        t_T, t_info, t_clique = robust.fit_enqueue(lib, a, b, m.ptr(m.rows), a.d_off, m.ptr(m.counts), c, budget, a.off, None)
        t_ref, t_stats = icp.register_enqueue(lib, a, b, t_T.data_ptr(), np.array([c]), np.array([100], dtype=np.int32), 1e-6, 1e-6,
                                              t_n[int(a.off[-1]):].data_ptr() if use_plane else None)
        out = torch.cat((t_T, t_ref, t_stats, t_info.to(torch.float64)), dim=1).cpu().numpy()     # one copy of the results
        clique = t_clique.cpu().numpy()
    fits = robust.fits(out[:, :16], out[:, 36:42].astype(np.int64), clique, a.off)
    results = []
    for p, fit in enumerate(fits):
        valid = fit.status == 0 and fit.clique_size > min_inliers
        T = out[p, 16:32].reshape(4, 4).copy() if valid else fit.transformation
        refined = RegistrationResult(T, float(out[p, 32]), float(out[p, 33]), int(out[p, 34]), int(out[p, 35]))
        results.append((TeaserSuccess(valid, refined, fit), T[:3, 3].copy(), T[:3, :3].copy()))
    return results


def solve_teaser(src, dst, voxel_size, min_inliers, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0, estimation="point_to_point"):
    """Counterpart of the reference's solve_teaser (icp_utils.py:103-139), same name and argument order: (valid,
    translation, rotation)."""
    return solve_teaser_pairs([(src, dst)], voxel_size, min_inliers, node_budget, device, estimation)[0]


def _accept(result, min_inliers, min_fitness):
    return result.correspondences > min_inliers and result.fitness >= min_fitness


def _coarse(coarse):
    if coarse not in ("yaw", "teaser"):
        raise ValueError("coarse is 'yaw' or 'teaser', got %r" % (coarse,))
    return coarse


def solve_icp(src, dst, voxel_size, min_inliers, init_yaw_deg=None, min_fitness=0.0, coarse="yaw", estimation="point_to_point"):
    """Counterpart of the reference's solve_teaser (icp_utils.py:103-139): (valid, translation, rotation) with
    dst ~ rotation . src + translation.  coarse="teaser": `solve_teaser` itself (`init_yaw_deg` and `min_fitness` are
    not used).  `estimation`: as for `compute_transform`."""
    icp.plane(estimation)
    if _coarse(coarse) == "teaser":
        return solve_teaser(src, dst, voxel_size, min_inliers, estimation=estimation)
    r = register_pairs([(src, dst)], voxel_size, init_yaw_deg, estimation=estimation)[0]
    return _accept(r, min_inliers, min_fitness), r.transformation[:3, 3].copy(), r.transformation[:3, :3].copy()


def compute_transform(src, dst, voxel_size, min_inliers, init_yaw_deg=None, min_fitness=0.0, coarse="yaw",
                      estimation="point_to_point"):
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
        estimation: "point_to_point" (the default: the reference's estimator) or "point_to_plane": open3d's
            TransformationEstimationPointToPlane on the targets' normals, which are estimated on the device from the
            neighbours within 2 voxels (30 at most), as the reference's `extract_fpfh` does.  On street scenes (ground and
            walls, which slide under point-to-point) it needs about a third of the updates.  Its basin is narrower: a single
            stage at the voxel radius from a yaw seed 3 degrees off can diverge where point-to-point converges, so with
            coarse="yaw" it relies on the coarse stages, and it is not the default.  A singular system (fewer than six
            correspondences, all normals parallel, |det| < 1e-6) leaves the transform as it is.

    Returns:
        (Transform, Success): the transform message and a success flag that is truthy / falsy like the reference's bool
        and carries `fitness`, `inlier_rmse`, `correspondences`, `iterations` and the 4 x 4 `transformation`.

    A correspondence count is a MUCH weaker test than the size of TEASER++'s maximum clique, which the reference
    compares with min_inliers: the clique certifies mutually consistent matches, a count only says how many source points
    have some target point within voxel_size.  A wrong alignment of two clouds that share a ground plane still has a
    fitness of about 0.6 (thousands of "inliers"), a right one is above 0.9 on the same clouds.  Set `min_fitness`, or
    use coarse="teaser", whose test is the clique itself.
    """
    icp.plane(estimation)
    if _coarse(coarse) == "teaser":
        valid, t, R = solve_teaser(src, dst, voxel_size, min_inliers, estimation=estimation)
        return to_transform_msg(t, R), valid
    r = register_pairs([(src, dst)], voxel_size, init_yaw_deg, estimation=estimation)[0]
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
