"""Stereo keyframes on the GPU: the sparse disparity of the keypoints and the 3D points triangulated from it
(feat_stereo_kernel in csrc/feat.hip, the rules in csrc/stereo.h).

`StereoHandler` of the reference inherits `RGBDHandler::compute_local_descriptors` (rgbd_handler.cpp:266-312) unchanged;
a stereo frame differs only in where `generateKeypoints3D` (:309) gets depth: from a left and a right rectified image and
a stereo camera model (stereo_handler.cpp:148-227).  There is no depth image and so no depth mask; a keypoint without a
correspondence keeps a NaN point, which the matcher of `visual_registration` drops.  rtabmap was not available to compare
against: parity with its `Stereo::computeCorrespondences` is unpinned; the rule is the one include/cslam_hip.h states and
tests/stereo_reference.py restates, and the two agree bit for bit.

Images are uint8, the two sides of a frame of the same H x W; a camera is (fx, fy, cx, cy, baseline), baseline in metres,
one for all frames or one per frame.  Status: 0 accepted, 1 outside, 2 no range, 3 edge, 4 not unique, 5 left-right.
Raw (distorted, unrectified) pairs enter through rectify.py's `extract_keyframes_stereo_raw`.

Out of scope: different principal points, a pyramid inside the correspondence search (the keypoints' scale pyramid is
visual_pyramid.py's), rtabmap's optical-flow variant, Vis/MinDepth and Vis/MaxDepth.

There is no CPU path: without the library or a GPU the functions raise CslamHipError.
"""
import numpy as np

from .. import _lib
from ..lidar_pr._batch import gpu, host, offsets, stream, to_dev
from .visual_features import FEAT_DESC_BYTES, _Batch, _image, _ragged_keypoints, _selection
from .visual_registration import Keyframe

STEREO_MAX_DISPARITY = 255
STATUS = ("accepted", "outside", "no range", "edge", "not unique", "left-right")


# ---- argument checks: everything that can be wrong raises here, before any launch ------------------------------------
def _whole(value, what):
    if isinstance(value, (bool, np.bool_)) or int(value) != value:
        raise ValueError("%s is a whole number, got %r" % (what, value))
    return int(value)


def _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance):
    lo, hi = _whole(min_disparity, "min_disparity"), _whole(max_disparity, "max_disparity")
    uq, lr = _whole(uniqueness, "uniqueness"), _whole(lr_tolerance, "lr_tolerance")
    if not 1 <= lo <= hi <= STEREO_MAX_DISPARITY:
        raise ValueError("1 <= min_disparity <= max_disparity <= %d is required" % STEREO_MAX_DISPARITY)
    if not 0 <= uq <= 100:
        raise ValueError("uniqueness must be in [0, 100] percent")
    if not -1 <= lr <= 255:
        raise ValueError("lr_tolerance must be in [-1, 255]")
    return lo, hi, uq, lr


def _stereo_cameras(cameras, n):
    cam = np.asarray(cameras, dtype=np.float64)
    if cam.shape == (5,):
        cam = np.repeat(cam[None], n, axis=0)
    if cam.shape != (n, 5):
        raise ValueError("stereo cameras are (fx, fy, cx, cy, baseline), one for all frames or one per frame: got shape %s for %d frames"
                         % (cam.shape, n))
    if not (np.all(np.isfinite(cam)) and np.all(cam[:, :2] > 0.0) and np.all(cam[:, 4] > 0.0)):
        raise ValueError("a stereo camera must be finite, and fx, fy and the baseline positive")
    return np.ascontiguousarray(cam)


def _pairs(lefts, rights, channels_ok):
    if len(lefts) != len(rights):
        raise ValueError("one right image per left image")
    ls, rs = [_image(i, channels_ok) for i in lefts], [_image(i, channels_ok) for i in rights]
    for a, b in zip(ls, rs):
        if a.shape[:2] != b.shape[:2]:
            raise ValueError("the two sides of a frame have the same H x W, got %s and %s" % (a.shape[:2], b.shape[:2]))
    return ls, rs


def _pixels(kp):
    a = np.asarray(kp)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("keypoints are an [n, 2] array of (x, y), got shape %s" % (a.shape,))
    if a.dtype.kind not in "iuf" or not np.all(np.isfinite(a)) or np.abs(a).max(initial=0) > 2 ** 30:
        raise ValueError("keypoints are whole pixels")
    k = a.astype(np.int32)
    if not np.array_equal(k, a):
        raise ValueError("keypoints are whole pixels")
    return np.ascontiguousarray(k)


# ---- the stereo rule at given keypoints ------------------------------------------------------------------------------
def stereo_match_batch(lefts, rights, keypoints, cameras, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, device=0):
    """The stereo rule for a list of (left grey, right grey, keypoints [k, 2]) in ONE call (`cslam_feat_stereo_dev`).  Per
    frame a dict: disparity float64 [k] (NaN unless accepted), status int32 [k], best int32 [k, 4] = (d*, C(d* - 1), C(d*),
    C(d* + 1)), points float64 [k, 3] (a NaN row unless accepted).  A keypoint may lie anywhere: outside the image or nearer
    to its edge than the window it has status 1."""
    ls, rs = _pairs(lefts, rights, (1,))
    if len(keypoints) != len(ls):
        raise ValueError("one keypoint array per frame")
    kps = [_pixels(k) for k in keypoints]
    lo, hi, uq, lr = _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance)
    cam = _stereo_cameras(cameras, len(ls))
    with gpu(device) as (lib, dev):
        import torch
        if not ls:
            return []
        b = _Batch([i.shape for i in ls], dev)
        t_left, t_right, t_cam = b.flat(ls, np.uint8, dev), b.flat(rs, np.uint8, dev), to_dev(cam, dev)
        k_off, t_kp, t_ko = _ragged_keypoints(kps, dev)
        rows = max(int(k_off[-1]), 1)
        t_disp = torch.zeros(rows, dtype=torch.float64, device=dev)
        t_status = torch.zeros(rows, dtype=torch.int32, device=dev)
        t_best = torch.zeros((rows, 4), dtype=torch.int32, device=dev)
        t_pts = torch.zeros((rows, 3), dtype=torch.float64, device=dev)
        _lib.check(lib.cslam_feat_stereo_dev(t_left.data_ptr(), t_right.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n, t_kp.data_ptr(),
                                             t_ko.data_ptr(), t_cam.data_ptr(), lo, hi, uq, lr, t_disp.data_ptr(), t_status.data_ptr(),
                                             t_best.data_ptr(), t_pts.data_ptr(), host(b.off), host(b.hw), host(k_off), host(cam), stream()))
        disp, status, best, pts = (t.cpu().numpy() for t in (t_disp, t_status, t_best, t_pts))
    return [dict(disparity=disp[k_off[c]:k_off[c + 1]].copy(), status=status[k_off[c]:k_off[c + 1]].copy(),
                 best=best[k_off[c]:k_off[c + 1]].copy(), points=pts[k_off[c]:k_off[c + 1]].copy()) for c in range(len(ls))]


def stereo_match(left, right, keypoints, camera, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, device=0):
    return stereo_match_batch([left], [right], [keypoints], camera, min_disparity, max_disparity, uniqueness, lr_tolerance, device)[0]


# ---- the whole stereo frame ------------------------------------------------------------------------------------------
def extract_features_stereo(lefts, rights, cameras, max_features=1000, quality_level=0.001, min_distance=7, border=19, min_disparity=1,
                            max_disparity=128, uniqueness=15, lr_tolerance=1, device=0):
    """The whole chain of a list of stereo frames in ONE call (`cslam_feat_extract_stereo_dev`), chained on the device with no
    host wait in between: grey of both sides, corners and descriptors on the left without a mask, the stereo rule.  Per
    frame a dict as `extract_features` gives, plus disparity float64 [k] and status int32 [k].  The two sides may differ in
    channels (1 or 3, B, G, R)."""
    ls, rs = _pairs(lefts, rights, (1, 3))
    mf, q, md, bd = _selection(max_features, quality_level, min_distance, border, [i.shape for i in ls])
    lo, hi, uq, lr = _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance)
    cam = _stereo_cameras(cameras, len(ls))
    with gpu(device) as (lib, dev):
        if not ls:
            return []
        b = _Batch([i.shape for i in ls], dev)
        l_off, r_off = offsets([i.size for i in ls]), offsets([i.size for i in rs])
        return _extract_stereo_on_device(lib, dev, b, b.flat(ls, np.uint8, dev), to_dev(l_off, dev), l_off, b.flat(rs, np.uint8, dev),
                                         to_dev(r_off, dev), r_off, cam, (mf, q, md, bd), (lo, hi, uq, lr))


def _extract_stereo_on_device(lib, dev, b, t_left, t_lo, l_off, t_right, t_ro, r_off, cam, selection, parameters):
    """`cslam_feat_extract_stereo_dev` on pairs that are on the device already (front_end/rectify.py chains into it), and the one
    download: the list `extract_features_stereo` returns."""
    import torch
    mf, q, md, bd = selection
    lo, hi, uq, lr = parameters
    t_cam = to_dev(cam, dev)
    t_cnt = torch.zeros(b.n, dtype=torch.int32, device=dev)
    t_kp = torch.zeros((b.n, mf, 2), dtype=torch.int32, device=dev)
    t_resp = torch.zeros((b.n, mf), dtype=torch.int32, device=dev)
    t_bins = torch.zeros((b.n, mf), dtype=torch.int32, device=dev)
    t_desc = torch.zeros((b.n, mf, FEAT_DESC_BYTES), dtype=torch.uint8, device=dev)
    t_pts = torch.zeros((b.n, mf, 3), dtype=torch.float64, device=dev)
    t_disp = torch.zeros((b.n, mf), dtype=torch.float64, device=dev)
    t_status = torch.zeros((b.n, mf), dtype=torch.int32, device=dev)
    _lib.check(lib.cslam_feat_extract_stereo_dev(t_left.data_ptr(), t_lo.data_ptr(), t_right.data_ptr(), t_ro.data_ptr(), b.t_off.data_ptr(),
                                                 b.t_hw.data_ptr(), t_cam.data_ptr(), b.n, q, md, bd, mf, lo, hi, uq, lr, t_cnt.data_ptr(),
                                                 t_kp.data_ptr(), t_resp.data_ptr(), t_bins.data_ptr(), t_desc.data_ptr(), t_pts.data_ptr(),
                                                 t_disp.data_ptr(), t_status.data_ptr(), host(l_off), host(r_off), host(b.off), host(b.hw),
                                                 host(cam), stream()))
    cnt = t_cnt.cpu().numpy()
    kp, resp, bins, desc, pts, disp, status = (t.cpu().numpy() for t in (t_kp, t_resp, t_bins, t_desc, t_pts, t_disp, t_status))
    return [dict(keypoints=kp[c, :cnt[c]].copy(), responses=resp[c, :cnt[c]].copy(), bins=bins[c, :cnt[c]].copy(),
                 descriptors=desc[c, :cnt[c]].copy(), points=pts[c, :cnt[c]].copy(), disparity=disp[c, :cnt[c]].copy(),
                 status=status[c, :cnt[c]].copy()) for c in range(b.n)]


def extract_keyframes_stereo(lefts, rights, cameras, max_features=1000, quality_level=0.001, min_distance=7, border=19, min_disparity=1,
                             max_disparity=128, uniqueness=15, lr_tolerance=1, device=0):
    """A `Keyframe` (keypoints float64 [k, 2], points float64 [k, 3], descriptors uint8 [k, 32]) per stereo frame, ready for
    `register_pairs` with the first four numbers of the camera.  Keypoints without a correspondence keep a NaN point."""
    return [Keyframe(f["keypoints"].astype(np.float64), f["points"], f["descriptors"])
            for f in extract_features_stereo(lefts, rights, cameras, max_features, quality_level, min_distance, border, min_disparity,
                                             max_disparity, uniqueness, lr_tolerance, device)]
