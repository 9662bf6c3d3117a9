"""Geometric verification of a visual loop closure on the GPU (csrc/vis.hip, csrc/pnp.h): nearest-neighbour matching of
32-byte binary descriptors with a ratio test, then 3D -> 2D PnP inside RANSAC with refinement on the inliers.

Replaces the `registration_.computeTransformation(from, to, ...)` calls of the reference's src/front_end/rgbd_handler.cpp:433-469
(`receive_local_keyframe_match`, intra-robot) and :493-554 (`receive_local_image_descriptors`, inter-robot), whose keyframes
carry 2D keypoints, their 3D points and their descriptors (:471-491); `frontend.pnp_min_inliers` = 20
(map_manager_node.cpp:18).  Behind that call is rtabmap's visual registration, taken at its defaults (ratio 0.8, 300
iterations, 2 px).  rtabmap and OpenCV are third party and were not available to compare against, so parity with them is
unpinned: the algorithm is the one include/cslam_hip.h states and tests/vis_reference.py restates in float64.

Convention: `transformation` maps points of the "from" camera frame into the "to" camera frame.  The 3D points come from
"from"; the pixels and the camera (fx, fy, cx, cy: pinhole, rectified, no distortion) from "to".

The level-aware forms (`register_level_pairs`, `pnp_ransac_level_pairs`) are for keyframes of the scale pyramid
(visual_pyramid.py), whose keypoints of level l are located on an image 1.2^l times coarser: with sigma2[l] = 36^l / 25^l a
correspondence whose "to" keypoint has level l is an inlier iff its depth is positive and its squared pixel error is
<= reproj_error^2 sigma2[l], and its Gauss-Newton terms are multiplied by 1 / sigma2[l]; everything else is the rule above
(tests/vis_levels_reference.py restates it).  Parity with rtabmap's use of cv::KeyPoint::octave is unpinned too.

The adjusted forms (`register_pairs_ba`, `compute_transformation_ba`, `bundle_adjust_pairs`; csrc/vis_ba.hip, csrc/ba.h) follow
the PnP fit with a two-view bundle adjustment, as rtabmap's computeTransformation does at its defaults: the transform and one
point per inlier are refined against the keypoints and depths of BOTH keyframes (include/cslam_hip.h states the rule,
tests/vis_ba_reference.py restates it).  Parity with rtabmap's g2o adjustment is unpinned like the rest, and the default
baseline of 0.1 m that weighs a depth against a pixel is this library's own choice.

There is no CPU path: without the library or a GPU the functions raise CslamHipError.
"""
from collections import namedtuple

import numpy as np

from .. import _lib
from ..back_end.pose_graph import DEFAULT_NOISE_STD, PoseGraphEdge
from ..lidar_pr._batch import gpu, host, offsets, stream, to_dev

VIS_MATCH_BLOCK = 256          # "from" rows per workgroup of the matcher
VIS_MATCH_CHUNK = 256          # "to" rows per LDS chunk of the matcher; the tests size around both
VIS_MAX_CORR = 2048            # most usable correspondences of a pair the PnP kernel attempts; above it: status 3
VIS_DESC_BYTES = 32
VIS_MAX_LEVEL = 7              # levels of the level-aware PnP are 0 .. 7, the levels a scale pyramid can have

Keyframe = namedtuple("Keyframe", "keypoints points descriptors")
Keyframe.__doc__ = """What a keyframe carries on the wire: keypoints [n, 2] pixels, points [n, 3] in the camera frame (a row
that is not finite: no depth), descriptors [n, 32] uint8.  float32 arrays are widened to float64 on upload."""

LevelKeyframe = namedtuple("LevelKeyframe", "keypoints points descriptors levels")
LevelKeyframe.__doc__ = """A `Keyframe` of the scale pyramid: also levels [n] uint8, the pyramid level of every keypoint (on the wire
one byte per keypoint, the counterpart of cv::KeyPoint::octave).  `register_pairs` takes it as it is and ignores the levels."""


class VisualRegistration:
    """The verification of one pair: `transformation` (4 x 4, "from" camera frame -> "to" camera frame), `success`
    (status 0), `status` (0 accepted; 1 rejected: too few inliers, the best fit found; 2 fewer usable correspondences than
    max(4, min_inliers): not attempted, the identity; 3 more than VIS_MAX_CORR: not attempted, the identity), `matches`
    [K, 2] (from row, to row), `inliers` [K] bool, `dropped_no_depth`, `best_hypothesis` (-1: not attempted)."""

    def __init__(self, transformation, success, status, matches, inliers, dropped_no_depth, best_hypothesis):
        self.transformation = transformation
        self.success = success
        self.status = status
        self.matches = matches
        self.inliers = inliers
        self.dropped_no_depth = dropped_no_depth
        self.best_hypothesis = best_hypothesis

    def __repr__(self):
        return "VisualRegistration(status=%d, inliers=%d of %d matches, dropped_no_depth=%d, best_hypothesis=%d)" % (
            self.status, int(np.count_nonzero(self.inliers)), len(self.matches), self.dropped_no_depth, self.best_hypothesis)

    def to_edge(self, key_from, key_to, noise_std=DEFAULT_NOISE_STD):
        """The closure as a `PoseGraphEdge` for back_end.pose_graph.optimize.  The between factor measures
        pose(key_from)^-1 pose(key_to), the pose of the "to" camera in the "from" camera frame: the inverse of
        `transformation`.  Raises for a registration that did not succeed."""
        if not self.success:
            raise ValueError("a registration with status %d is no loop closure" % self.status)
        return PoseGraphEdge(tuple(key_from), tuple(key_to), np.linalg.inv(self.transformation), np.asarray(noise_std, dtype=np.float64))


# ---- argument checks: everything that can be wrong raises here, before any launch ------------------------------------
def _descriptors(d):
    d = np.asarray(d)
    if d.ndim != 2 or d.shape[1] != VIS_DESC_BYTES:
        raise ValueError("descriptors are [n, %d] uint8 (ORB / BRIEF-32), got shape %s" % (VIS_DESC_BYTES, d.shape))
    if d.dtype != np.uint8:
        raise ValueError("descriptors are uint8, got %s" % d.dtype)
    return np.ascontiguousarray(d)


def _rows(a, width, what):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError("%s are an [n, %d] array, got shape %s" % (what, width, a.shape))
    return np.ascontiguousarray(a, dtype=np.float64)


def _keyframe(kf):
    kp, pts, desc = _rows(kf.keypoints, 2, "keypoints"), _rows(kf.points, 3, "points"), _descriptors(kf.descriptors)
    if not (len(kp) == len(pts) == len(desc)):
        raise ValueError("a keyframe has one point and one descriptor per keypoint: %d, %d, %d" % (len(kp), len(pts), len(desc)))
    return kp, pts, desc


def _levels(levels, n):
    lv = np.asarray(levels)
    if lv.ndim != 1 or len(lv) != n:
        raise ValueError("levels are an [n] array, one per keypoint: got shape %s for %d keypoints" % (lv.shape, n))
    if lv.dtype.kind not in "iu":
        raise ValueError("levels are whole numbers, got %s" % lv.dtype)
    if len(lv) and not (0 <= int(lv.min()) and int(lv.max()) <= VIS_MAX_LEVEL):
        raise ValueError("levels must be in [0, %d]" % VIS_MAX_LEVEL)
    return np.ascontiguousarray(lv, dtype=np.int32)


def _level_keyframe(kf):
    if not hasattr(kf, "levels"):
        raise ValueError("the level-aware registration takes LevelKeyframes (keypoints, points, descriptors, levels)")
    kp, pts, desc = _keyframe(kf)
    return kp, pts, desc, _levels(kf.levels, len(kp))


def _cameras(cameras, n):
    cam = np.asarray(cameras, dtype=np.float64)
    if cam.shape == (4,):
        cam = np.repeat(cam[None], n, axis=0)
    if cam.shape != (n, 4):
        raise ValueError("cameras are (fx, fy, cx, cy), one for all pairs or one per pair: got shape %s for %d pairs" % (cam.shape, n))
    if not (np.all(np.isfinite(cam)) and np.all(cam[:, :2] > 0.0)):
        raise ValueError("intrinsics must be finite and fx, fy positive")
    return np.ascontiguousarray(cam)


def _nndr(nndr):
    r = float(nndr)
    if not 0.0 <= r <= 1.0:
        raise ValueError("nndr must be in [0, 1]")
    return r


def _ransac(iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed):
    it, e, mi, ri, rr, sd = int(iterations), float(reproj_error), int(min_inliers), int(refine_iterations), int(refine_rounds), int(seed)
    if it < 1:
        raise ValueError("iterations must be at least 1")
    if not (np.isfinite(e) and e > 0.0):
        raise ValueError("reproj_error must be positive and finite")
    if mi < 1:
        raise ValueError("min_inliers must be at least 1")
    if ri < 0 or rr < 0:
        raise ValueError("refine_iterations and refine_rounds must not be negative")
    if not 0 <= sd < 2 ** 64:
        raise ValueError("seed must fit 64 unsigned bits")
    return it, e, mi, ri, rr, sd


def _cat(arrays, width, dtype):
    return np.concatenate(arrays, axis=0) if arrays else np.zeros((0, width), dtype=dtype)


# ---- the launches, each written once ------------------------------------------------------------------------------
def _outputs(n, total, dev):
    import torch
    return (torch.zeros((n, 16), dtype=torch.float64, device=dev), torch.zeros((n, 8), dtype=torch.int32, device=dev),
            torch.zeros(max(total, 1), dtype=torch.int32, device=dev))


def _registrations(T, info, flags, rows, off):
    out = []
    for p in range(len(T)):
        k = int(info[p, 1])
        out.append(VisualRegistration(T[p].reshape(4, 4).copy(), int(info[p, 0]) == 0, int(info[p, 0]),
                                      rows[off[p]:off[p] + k].astype(np.int64), flags[off[p]:off[p] + k].astype(bool),
                                      int(info[p, 3]), int(info[p, 5])))
    return out


def match_descriptors_pairs(pairs, nndr=0.8, device=0):
    """Matches of a list of (descriptors_from [n, 32] uint8, descriptors_to [m, 32] uint8) in ONE call
    (`cslam_vis_match_dev`): per pair rows [K, 2] int64 (from row, to row), ascending in the from row.  A "from" row matches
    its nearest "to" row (Hamming, lowest index on ties) iff m >= 2 and d1 <= nndr d2; of several "from" rows on one "to" row
    the smallest distance keeps it, then the lowest "from" row."""
    r = _nndr(nndr)
    da, db = [_descriptors(a) for a, _ in pairs], [_descriptors(b) for _, b in pairs]
    with gpu(device) as (lib, dev):
        import torch
        if not pairs:
            return []
        n = len(pairs)
        a_off, b_off = offsets([len(a) for a in da]), offsets([len(b) for b in db])
        t_a, t_b, t_ao, t_bo = to_dev(_cat(da, 32, np.uint8), dev), to_dev(_cat(db, 32, np.uint8), dev), to_dev(a_off, dev), to_dev(b_off, dev)
        t_rows = torch.zeros((max(int(a_off[-1]), 1), 2), dtype=torch.int32, device=dev)
        t_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_vis_match_dev(t_a.data_ptr(), t_ao.data_ptr(), t_b.data_ptr(), t_bo.data_ptr(), n, VIS_DESC_BYTES, r,
                                           t_rows.data_ptr(), t_cnt.data_ptr(), host(a_off), host(b_off), stream()))
        rows, cnt = t_rows.cpu().numpy(), t_cnt.cpu().numpy()
    return [rows[a_off[p]:a_off[p] + cnt[p]].astype(np.int64) for p in range(n)]


def match_descriptors(descriptors_from, descriptors_to, nndr=0.8, device=0):
    return match_descriptors_pairs([(descriptors_from, descriptors_to)], nndr, device)[0]


def _point_pairs(pairs):
    pts, pix = [], []
    for a, b in pairs:
        a, b = _rows(a, 3, "points3d"), _rows(b, 2, "pixels")
        if len(a) != len(b):
            raise ValueError("a pair is (points3d [M, 3], pixels [M, 2]): %d points, %d pixels" % (len(a), len(b)))
        pts.append(a)
        pix.append(b)
    return pts, pix


def _pnp_pairs(pairs, levels_to, cameras, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed, device):
    """`pnp_ransac_pairs` (levels_to None) and `pnp_ransac_level_pairs`."""
    it, e, mi, ri, rr, sd = _ransac(iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed)
    pts, pix = _point_pairs(pairs)
    cam = _cameras(cameras, len(pairs))
    if levels_to is not None:
        if len(levels_to) != len(pairs):
            raise ValueError("one array of levels per pair")
        lvl = [_levels(l, len(x)) for l, x in zip(levels_to, pix)]
    with gpu(device) as (lib, dev):
        if not pairs:
            return []
        n = len(pairs)
        off = offsets([len(a) for a in pts])
        rows = np.repeat(np.concatenate([np.arange(len(a), dtype=np.int32) for a in pts])[:, None], 2, axis=1)
        t_pts, t_pix, t_off, t_rows, t_cam = (to_dev(x, dev) for x in (_cat(pts, 3, np.float64), _cat(pix, 2, np.float64), off, rows, cam))
        t_T, t_info, t_flags = _outputs(n, int(off[-1]), dev)
        if levels_to is None:
            _lib.check(lib.cslam_vis_pnp_dev(t_pts.data_ptr(), t_off.data_ptr(), t_pix.data_ptr(), t_off.data_ptr(), t_rows.data_ptr(),
                                             t_off.data_ptr(), None, t_cam.data_ptr(), n, it, e, mi, ri, rr, sd, t_T.data_ptr(),
                                             t_info.data_ptr(), t_flags.data_ptr(), stream()))
        else:
            h_lvl = np.concatenate(lvl) if int(off[-1]) else np.zeros(1, dtype=np.int32)
            t_lvl = to_dev(h_lvl, dev)
            _lib.check(lib.cslam_vis_pnp_levels_dev(t_pts.data_ptr(), t_off.data_ptr(), t_pix.data_ptr(), t_off.data_ptr(), t_lvl.data_ptr(),
                                                    t_rows.data_ptr(), t_off.data_ptr(), None, t_cam.data_ptr(), n, it, e, mi, ri, rr, sd,
                                                    t_T.data_ptr(), t_info.data_ptr(), t_flags.data_ptr(), host(off), host(h_lvl), stream()))
        T, info, flags = t_T.cpu().numpy(), t_info.cpu().numpy(), t_flags.cpu().numpy()
    return _registrations(T, info, flags, rows, off)


def pnp_ransac_pairs(pairs, cameras, iterations=300, reproj_error=2.0, min_inliers=20, refine_iterations=10, refine_rounds=2, seed=0,
                     device=0):
    """PnP RANSAC of a list of (points3d [M, 3] in the "from" camera frame, pixels [M, 2] in the "to" image), row for row, in
    ONE call (`cslam_vis_pnp_dev`).  `cameras`: (fx, fy, cx, cy) of the "to" cameras, one for all or one per pair.  Returns a
    `VisualRegistration` per pair whose `matches` are (k, k)."""
    return _pnp_pairs(pairs, None, cameras, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed, device)


def pnp_ransac_level_pairs(pairs, levels_to, cameras, iterations=300, reproj_error=2.0, min_inliers=20, refine_iterations=10,
                           refine_rounds=2, seed=0, device=0):
    """The level-aware `pnp_ransac_pairs` in ONE call (`cslam_vis_pnp_levels_dev`): `levels_to` holds per pair the levels [M]
    (whole numbers in 0 .. 7) of the "to" keypoints behind its pixels."""
    return _pnp_pairs(pairs, levels_to, cameras, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed, device)


Hypotheses = namedtuple("Hypotheses", "R t valid inliers best_hypothesis best_inliers")


def hypotheses(pair, camera, iterations=300, reproj_error=2.0, seed=0, device=0):
    """The staged entry (`cslam_vis_hypotheses_dev`): every hypothesis of one (points3d, pixels) pair.  Returns
    `Hypotheses`: R [iterations, 3, 3], t [iterations, 3], valid [iterations] bool, inliers [iterations] counts, the best
    hypothesis and its inlier flags [M]."""
    it, e, _, _, _, sd = _ransac(iterations, reproj_error, 1, 0, 0, seed)
    pts, pix = _point_pairs([pair])
    cam = _cameras(camera, 1)
    with gpu(device) as (lib, dev):
        import torch
        off = offsets([len(pts[0])])
        t_pts, t_pix, t_off, t_cam = (to_dev(x, dev) for x in (pts[0], pix[0], off, cam))
        t_T, t_info, t_flags = _outputs(1, int(off[-1]), dev)
        t_pose = torch.zeros((it, 12), dtype=torch.float64, device=dev)
        t_hi = torch.zeros((it, 2), dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_vis_hypotheses_dev(t_pts.data_ptr(), t_pix.data_ptr(), t_off.data_ptr(), t_cam.data_ptr(), 1, it, e, sd,
                                                t_pose.data_ptr(), t_hi.data_ptr(), t_T.data_ptr(), t_info.data_ptr(),
                                                t_flags.data_ptr(), host(off), stream()))
        pose, hi, info, flags = t_pose.cpu().numpy(), t_hi.cpu().numpy(), t_info.cpu().numpy(), t_flags.cpu().numpy()
    return Hypotheses(pose[:, :9].reshape(it, 3, 3).copy(), pose[:, 9:].copy(), hi[:, 0].astype(bool), hi[:, 1].astype(np.int64),
                      int(info[0, 5]), flags[:int(off[-1])].astype(bool))


def _register(pairs_of_keyframes, with_levels, cameras, nndr, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed,
              device):
    """`register_pairs` and, `with_levels`, `register_level_pairs`."""
    r = _nndr(nndr)
    it, e, mi, ri, rr, sd = _ransac(iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed)
    check = _level_keyframe if with_levels else _keyframe
    kfs = [(check(a), check(b)) for a, b in pairs_of_keyframes]
    cam = _cameras(cameras, len(kfs))
    with gpu(device) as (lib, dev):
        import torch
        if not kfs:
            return []
        n = len(kfs)
        a_off, b_off = offsets([len(a[0]) for a, _ in kfs]), offsets([len(b[0]) for _, b in kfs])
        t_da = to_dev(_cat([a[2] for a, _ in kfs], 32, np.uint8), dev)
        t_db = to_dev(_cat([b[2] for _, b in kfs], 32, np.uint8), dev)
        t_pts = to_dev(_cat([a[1] for a, _ in kfs], 3, np.float64), dev)
        t_pix = to_dev(_cat([b[0] for _, b in kfs], 2, np.float64), dev)
        t_ao, t_bo, t_cam = to_dev(a_off, dev), to_dev(b_off, dev), to_dev(cam, dev)
        t_rows = torch.zeros((max(int(a_off[-1]), 1), 2), dtype=torch.int32, device=dev)
        t_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        t_T, t_info, t_flags = _outputs(n, int(a_off[-1]), dev)
        if not with_levels:
            _lib.check(lib.cslam_vis_register_dev(t_da.data_ptr(), t_pts.data_ptr(), t_ao.data_ptr(), t_db.data_ptr(), t_pix.data_ptr(),
                                                  t_bo.data_ptr(), t_cam.data_ptr(), n, VIS_DESC_BYTES, r, it, e, mi, ri, rr, sd,
                                                  t_rows.data_ptr(), t_cnt.data_ptr(), t_T.data_ptr(), t_info.data_ptr(), t_flags.data_ptr(),
                                                  host(a_off), host(b_off), stream()))
        else:
            h_lvl = np.concatenate([b[3] for _, b in kfs]) if int(b_off[-1]) else np.zeros(1, dtype=np.int32)
            t_lvl = to_dev(h_lvl, dev)
            _lib.check(lib.cslam_vis_register_levels_dev(t_da.data_ptr(), t_pts.data_ptr(), t_ao.data_ptr(), t_db.data_ptr(), t_pix.data_ptr(),
                                                         t_bo.data_ptr(), t_lvl.data_ptr(), t_cam.data_ptr(), n, VIS_DESC_BYTES, r, it, e, mi, ri,
                                                         rr, sd, t_rows.data_ptr(), t_cnt.data_ptr(), t_T.data_ptr(), t_info.data_ptr(),
                                                         t_flags.data_ptr(), host(a_off), host(b_off), host(h_lvl), stream()))
        T, info, flags, rows = t_T.cpu().numpy(), t_info.cpu().numpy(), t_flags.cpu().numpy(), t_rows.cpu().numpy()
    return _registrations(T, info, flags, rows, a_off)


def register_pairs(pairs_of_keyframes, cameras, nndr=0.8, iterations=300, reproj_error=2.0, min_inliers=20, refine_iterations=10,
                   refine_rounds=2, seed=0, device=0):
    """Matching and PnP RANSAC of a list of (keyframe_from, keyframe_to) in ONE call (`cslam_vis_register_dev`), chained on
    the device with no host wait between them: the matches select 3D points of "from" and pixels of "to".  Returns a
    `VisualRegistration` per pair."""
    return _register(pairs_of_keyframes, False, cameras, nndr, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed,
                     device)


def register_level_pairs(pairs_of_level_keyframes, cameras, nndr=0.8, iterations=300, reproj_error=2.0, min_inliers=20,
                         refine_iterations=10, refine_rounds=2, seed=0, device=0):
    """`register_pairs` on `LevelKeyframe`s with the level-aware PnP in ONE call (`cslam_vis_register_levels_dev`): the match
    is unchanged; the levels of the "to" keyframe scale the threshold and weight the refinement.  A plain `Keyframe` raises."""
    return _register(pairs_of_level_keyframes, True, cameras, nndr, iterations, reproj_error, min_inliers, refine_iterations, refine_rounds,
                     seed, device)


def compute_transformation(kf_from, kf_to, camera, **kwargs):
    """The one-pair form of `register_pairs`: what `registration_.computeTransformation(from, to, ...)` answers."""
    return register_pairs([(kf_from, kf_to)], camera, **kwargs)[0]


def compute_level_transformation(kf_from, kf_to, camera, **kwargs):
    """The one-pair form of `register_level_pairs`."""
    return register_level_pairs([(kf_from, kf_to)], camera, **kwargs)[0]


# ---- two-view bundle adjustment after PnP (csrc/vis_ba.hip, csrc/ba.h) ------------------------------------------------
class RefinedRegistration(VisualRegistration):
    """A `VisualRegistration` after the two-view bundle adjustment (`to_edge` works as before): `transformation`, `status`
    and `inliers` are the adjustment's (a PnP status other than 0 passes through untouched); also `pnp` (the registration
    before), `points` [K, 3] (the refined point of every final inlier in the "from" camera frame, NaN elsewhere),
    `cost_before`, `cost_after` (the weighted cost at the PnP fit and the one the last round ended with; NaN where nothing
    was adjusted), `set_in`, `ba_steps`, `rounds_discarded`, `points_held`."""

    def __init__(self, pnp, transformation, status, inliers, points, cost_before, cost_after, set_in, ba_steps, rounds_discarded, points_held):
        super().__init__(transformation, status == 0, status, pnp.matches, inliers, pnp.dropped_no_depth, pnp.best_hypothesis)
        self.pnp = pnp
        self.points = points
        self.cost_before, self.cost_after = cost_before, cost_after
        self.set_in, self.ba_steps, self.rounds_discarded, self.points_held = set_in, ba_steps, rounds_discarded, points_held

    def __repr__(self):
        return "RefinedRegistration(status=%d, inliers=%d of %d adjusted, steps=%d, cost %.6g -> %.6g; before: %r)" % (
            self.status, int(np.count_nonzero(self.inliers)), self.set_in, self.ba_steps, self.cost_before, self.cost_after, self.pnp)


def _baselines(baselines, n):
    b = np.asarray(baselines, dtype=np.float64)
    if b.ndim == 0:
        b = np.full((n, 2), float(b))
    elif b.shape == (2,):
        b = np.repeat(b[None], n, axis=0)
    if b.shape != (n, 2):
        raise ValueError("baselines are one number, (from, to), or one (from, to) per pair: got shape %s for %d pairs" % (b.shape, n))
    if not (np.all(np.isfinite(b)) and np.all(b > 0.0)):
        raise ValueError("baselines must be positive and finite")
    return np.ascontiguousarray(b)


def _ba_settings(ba_iterations, ba_rounds):
    bi, br = int(ba_iterations), int(ba_rounds)
    if bi < 0 or br < 0:
        raise ValueError("ba_iterations and ba_rounds must not be negative")
    return bi, br


def _ba_keyframes(pairs_of_keyframes):
    """Per pair ((kp, pts, desc, levels or None) of "from", the same of "to"); levels are kept only where both carry them."""
    out = []
    for a, b in pairs_of_keyframes:
        both = hasattr(a, "levels") and hasattr(b, "levels")
        ka, kb = (_level_keyframe(a), _level_keyframe(b)) if both else (_keyframe(a) + (None,), _keyframe(b) + (None,))
        out.append((ka, kb))
    return out


def _by_form(kfs):
    """The indices of the pairs with levels and of those without: each group is one call, so that a pair's bytes do not depend
    on what else the batch holds."""
    with_levels = [p for p, (a, _) in enumerate(kfs) if a[3] is not None]
    return [g for g in (with_levels, [p for p in range(len(kfs)) if kfs[p][0][3] is None]) if g]


def _ba_uploads(kfs, cam_a, cam_b, base, dev):
    a_off, b_off = offsets([len(a[0]) for a, _ in kfs]), offsets([len(b[0]) for _, b in kfs])
    t = dict(kp_a=to_dev(_cat([a[0] for a, _ in kfs], 2, np.float64), dev), pts_a=to_dev(_cat([a[1] for a, _ in kfs], 3, np.float64), dev),
             kp_b=to_dev(_cat([b[0] for _, b in kfs], 2, np.float64), dev), pts_b=to_dev(_cat([b[1] for _, b in kfs], 3, np.float64), dev),
             a_off=to_dev(a_off, dev), b_off=to_dev(b_off, dev), cam_a=to_dev(cam_a, dev), cam_b=to_dev(cam_b, dev), base=to_dev(base, dev))
    h_la = h_lb = None
    if kfs[0][0][3] is not None:
        h_la = np.concatenate([a[3] for a, _ in kfs]) if int(a_off[-1]) else np.zeros(1, dtype=np.int32)
        h_lb = np.concatenate([b[3] for _, b in kfs]) if int(b_off[-1]) else np.zeros(1, dtype=np.int32)
        t["la"], t["lb"] = to_dev(h_la, dev), to_dev(h_lb, dev)
    return t, a_off, b_off, h_la, h_lb


def _ba_outputs(n, total, dev):
    import torch
    return (_outputs(n, total, dev) + (torch.zeros((max(total, 1), 3), dtype=torch.float64, device=dev),
                                       torch.zeros((n, 2), dtype=torch.float64, device=dev)))


def _refined(pnp, T, info, flags, points, cost, off):
    out = []
    for p, reg in enumerate(pnp):
        k = len(reg.matches)
        out.append(RefinedRegistration(reg, T[p].reshape(4, 4).copy(), int(info[p, 0]), flags[off[p]:off[p] + k].astype(bool),
                                       points[off[p]:off[p] + k].copy(), float(cost[p, 0]), float(cost[p, 1]), int(info[p, 1]),
                                       int(info[p, 3]), int(info[p, 4]), int(info[p, 5])))
    return out


def _ptr(t, key):
    return t[key].data_ptr() if key in t else None


def _adjust_group(kfs, regs, cam_a, cam_b, base, e, mi, bi, br, lib, dev):
    n = len(kfs)
    t, a_off, b_off, h_la, h_lb = _ba_uploads(kfs, cam_a, cam_b, base, dev)
    rows = [np.ascontiguousarray(r.matches, dtype=np.int32).reshape(-1, 2) for r in regs]
    r_off = offsets([len(r) for r in rows])
    total = int(r_off[-1])
    h_rows = _cat(rows, 2, np.int32) if total else np.zeros((1, 2), dtype=np.int32)
    h_flags = np.concatenate([np.asarray(r.inliers).astype(np.int32) for r in regs]) if total else np.zeros(1, dtype=np.int32)
    h_T0 = np.stack([np.asarray(r.transformation, dtype=np.float64).reshape(16) for r in regs])
    h_info0 = np.zeros((n, 8), dtype=np.int32)
    for p, r in enumerate(regs):
        h_info0[p] = (r.status, len(r.matches), len(r.matches) - r.dropped_no_depth, r.dropped_no_depth, int(np.count_nonzero(r.inliers)),
                      r.best_hypothesis, 0, 0)
    t_rows, t_roff, t_f0, t_T0, t_i0 = (to_dev(x, dev) for x in (h_rows, r_off, h_flags, h_T0, h_info0))
    t_T, t_info, t_flags, t_pts, t_cost = _ba_outputs(n, total, dev)
    _lib.check(lib.cslam_vis_ba_dev(t["kp_a"].data_ptr(), t["pts_a"].data_ptr(), t["a_off"].data_ptr(), t["kp_b"].data_ptr(),
                                    t["pts_b"].data_ptr(), t["b_off"].data_ptr(), _ptr(t, "la"), _ptr(t, "lb"), t["cam_a"].data_ptr(),
                                    t["cam_b"].data_ptr(), t["base"].data_ptr(), t_rows.data_ptr(), t_roff.data_ptr(), None,
                                    t_T0.data_ptr(), t_i0.data_ptr(), t_f0.data_ptr(), n, e, mi, bi, br, t_T.data_ptr(), t_info.data_ptr(),
                                    t_flags.data_ptr(), t_pts.data_ptr(), t_cost.data_ptr(), host(a_off), host(b_off), host(r_off),
                                    None if h_la is None else host(h_la), None if h_lb is None else host(h_lb), host(base), stream()))
    return _refined(regs, t_T.cpu().numpy(), t_info.cpu().numpy(), t_flags.cpu().numpy(), t_pts.cpu().numpy(), t_cost.cpu().numpy(), r_off)


def bundle_adjust_pairs(pairs_of_keyframes, registrations, cameras_from, cameras_to=None, baselines=0.1, reproj_error=2.0, min_inliers=20,
                        ba_iterations=10, ba_rounds=2, device=0):
    """The staged form (`cslam_vis_ba_dev`): the two-view bundle adjustment of include/cslam_hip.h on a list of
    (keyframe_from, keyframe_to) and the `VisualRegistration` PnP gave for each (its `matches`, `inliers`, `transformation`
    and `status`).  `Keyframe` or `LevelKeyframe`; the levels weigh the residuals where both keyframes of a pair carry them.
    `cameras_from` / `cameras_to` (None: the same): (fx, fy, cx, cy), one for all or one per pair.  `baselines`: metres, one
    number, (from, to), or one (from, to) per pair; the depth weight of a view is fx * baseline: the real baseline of a
    stereo camera, a virtual one for RGB-D.  The default 0.1 m is this library's own choice; parity with rtabmap's value is
    unpinned.  Returns a `RefinedRegistration` per pair."""
    e, mi = float(reproj_error), int(min_inliers)
    if not (np.isfinite(e) and e > 0.0):
        raise ValueError("reproj_error must be positive and finite")
    if mi < 1:
        raise ValueError("min_inliers must be at least 1")
    bi, br = _ba_settings(ba_iterations, ba_rounds)
    kfs = _ba_keyframes(pairs_of_keyframes)
    regs = list(registrations)
    if len(regs) != len(kfs):
        raise ValueError("one registration per pair of keyframes: %d and %d" % (len(regs), len(kfs)))
    for r in regs:
        m = np.asarray(r.matches)
        if m.ndim != 2 or m.shape[1] != 2 or len(r.inliers) != len(m) or np.asarray(r.transformation).shape != (4, 4):
            raise ValueError("a registration carries matches [K, 2], inliers [K] and a 4 x 4 transformation")
    cam_a = _cameras(cameras_from, len(kfs))
    cam_b = cam_a if cameras_to is None else _cameras(cameras_to, len(kfs))
    base = _baselines(baselines, len(kfs))
    out = [None] * len(kfs)
    with gpu(device) as (lib, dev):
        for g in _by_form(kfs):
            res = _adjust_group([kfs[p] for p in g], [regs[p] for p in g], cam_a[g], cam_b[g], base[g], e, mi, bi, br, lib, dev)
            for p, r in zip(g, res):
                out[p] = r
    return out


def _register_ba_group(kfs, cam_a, cam_b, base, r, it, e, mi, ri, rr, sd, bi, br, lib, dev):
    import torch
    n = len(kfs)
    t, a_off, b_off, h_la, h_lb = _ba_uploads(kfs, cam_a, cam_b, base, dev)
    t_da = to_dev(_cat([a[2] for a, _ in kfs], 32, np.uint8), dev)
    t_db = to_dev(_cat([b[2] for _, b in kfs], 32, np.uint8), dev)
    total = int(a_off[-1])
    t_rows = torch.zeros((max(total, 1), 2), dtype=torch.int32, device=dev)
    t_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    t_T0, t_i0, t_f0 = _outputs(n, total, dev)
    t_T, t_info, t_flags, t_pts, t_cost = _ba_outputs(n, total, dev)
    _lib.check(lib.cslam_vis_register_ba_dev(t_da.data_ptr(), t["kp_a"].data_ptr(), t["pts_a"].data_ptr(), t["a_off"].data_ptr(),
                                             t_db.data_ptr(), t["kp_b"].data_ptr(), t["pts_b"].data_ptr(), t["b_off"].data_ptr(),
                                             _ptr(t, "la"), _ptr(t, "lb"), t["cam_a"].data_ptr(), t["cam_b"].data_ptr(), t["base"].data_ptr(),
                                             n, VIS_DESC_BYTES, r, it, e, mi, ri, rr, sd, bi, br, t_rows.data_ptr(), t_cnt.data_ptr(),
                                             t_T0.data_ptr(), t_i0.data_ptr(), t_f0.data_ptr(), t_T.data_ptr(), t_info.data_ptr(),
                                             t_flags.data_ptr(), t_pts.data_ptr(), t_cost.data_ptr(), host(a_off), host(b_off),
                                             None if h_la is None else host(h_la), None if h_lb is None else host(h_lb), host(base), stream()))
    pnp = _registrations(t_T0.cpu().numpy(), t_i0.cpu().numpy(), t_f0.cpu().numpy(), t_rows.cpu().numpy(), a_off)
    return _refined(pnp, t_T.cpu().numpy(), t_info.cpu().numpy(), t_flags.cpu().numpy(), t_pts.cpu().numpy(), t_cost.cpu().numpy(), a_off)


def register_pairs_ba(pairs_of_keyframes, cameras_from, cameras_to=None, baselines=0.1, ba_iterations=10, ba_rounds=2, nndr=0.8,
                      iterations=300, reproj_error=2.0, min_inliers=20, refine_iterations=10, refine_rounds=2, seed=0, device=0):
    """Matching, PnP RANSAC and the two-view bundle adjustment of a list of (keyframe_from, keyframe_to) in ONE call per form
    (`cslam_vis_register_ba_dev`), chained on the device with no host wait.  `Keyframe` or `LevelKeyframe`: a pair whose
    keyframes both carry levels gets the level-aware PnP (`register_level_pairs`) and level weights in the adjustment, any
    other pair the uniform PnP (`register_pairs`) and level 0; the two forms of a mixed batch are two calls.  PnP uses
    `cameras_to` (None: `cameras_from`).  `baselines` as for `bundle_adjust_pairs`: the default 0.1 m is this library's own
    choice and parity with rtabmap's value is unpinned.  Returns a `RefinedRegistration` per pair; its `pnp` equals what
    `register_pairs` / `register_level_pairs` return for the pair."""
    r = _nndr(nndr)
    it, e, mi, ri, rr, sd = _ransac(iterations, reproj_error, min_inliers, refine_iterations, refine_rounds, seed)
    bi, br = _ba_settings(ba_iterations, ba_rounds)
    kfs = _ba_keyframes(pairs_of_keyframes)
    cam_a = _cameras(cameras_from, len(kfs))
    cam_b = cam_a if cameras_to is None else _cameras(cameras_to, len(kfs))
    base = _baselines(baselines, len(kfs))
    out = [None] * len(kfs)
    with gpu(device) as (lib, dev):
        for g in _by_form(kfs):
            res = _register_ba_group([kfs[p] for p in g], cam_a[g], cam_b[g], base[g], r, it, e, mi, ri, rr, sd, bi, br, lib, dev)
            for p, x in zip(g, res):
                out[p] = x
    return out


def compute_transformation_ba(kf_from, kf_to, camera, **kwargs):
    """The one-pair form of `register_pairs_ba`: what `registration_.computeTransformation(from, to, ...)` answers with its
    bundle adjustment on."""
    return register_pairs_ba([(kf_from, kf_to)], camera, **kwargs)[0]
