"""What a visual keyframe carries, from the image, on the GPU (csrc/feat.hip, csrc/feat.h): Shi-Tomasi corners with a
minimum distance, a 32-bin orientation, steered BRIEF-32 descriptors and the 3D points of the keypoints.

Replaces `RGBDHandler::compute_local_descriptors` of the reference's src/front_end/rgbd_handler.cpp:266-312 (grey
conversion, depth mask, rtabmap's `Feature2D::generateKeypoints`, `generateDescriptors`, `generateKeypoints3D`) and the
keyframe decision of `generate_new_keyframe` (:314-351).  rtabmap and OpenCV are third party and were not available to
compare against, and OpenCV's learned ORB / BRIEF sampling tables are not ours to restate, so parity with rtabmap's
features is unpinned and stays so: the algorithm is the one include/cslam_hip.h states and tests/feat_reference.py restates
in integer numpy, and the two agree bit for bit.  Matching only needs every robot to use the same rule.

Images are uint8 [H, W] or [H, W, 3] (B, G, R); depths float32 metres [H, W] (uint16 millimetres are converted on the
host as np.float32(d) * np.float32(0.001)); a depth is valid iff finite and > 0.  A keypoint is (x, y), x to the right.

Out of scope: depth images smaller than the colour image, sub-pixel refinement.  A stereo frame (depth from the disparity
at the keypoints) is visual_stereo.py's, the scale pyramid of either visual_pyramid.py's.

There is no CPU path: without the library or a GPU the functions raise CslamHipError.
"""
import numpy as np

from .. import _lib
from ..lidar_pr._batch import gpu, host, offsets, stream, to_dev
from .visual_registration import Keyframe, _cameras

FEAT_TILE = 16                 # side of the response kernel's output tile; the tests size around it
FEAT_MIN_BORDER = 18           # patch radius 15 plus blur radius 3
FEAT_MAX_DISTANCE = 1024
FEAT_DESC_BYTES = 32


# ---- argument checks: everything that can be wrong raises here, before any launch ------------------------------------
def _image(img, channels_ok=(1, 3)):
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError("an image is uint8, got %s" % a.dtype)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3 and 3 in channels_ok)):
        raise ValueError("an image is [H, W]%s, got shape %s" % (" or [H, W, 3] (B, G, R)" if 3 in channels_ok else "", a.shape))
    if a.shape[0] < 2 or a.shape[1] < 2:
        raise ValueError("an image is at least 2 x 2, got shape %s" % (a.shape,))
    return np.ascontiguousarray(a)


def _map(m, dtype, what, like=None):
    a = np.asarray(m)
    if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 2:
        raise ValueError("%s is [H, W] and at least 2 x 2, got shape %s" % (what, a.shape))
    if a.dtype != dtype:
        raise ValueError("%s is %s, got %s" % (what, np.dtype(dtype).name, a.dtype))
    if like is not None and a.shape != like:
        raise ValueError("%s has shape %s, its image %s" % (what, a.shape, like))
    return np.ascontiguousarray(a)


def depth_metres(depth):
    """float32 metres of a depth image: float32 is taken as it is, uint16 millimetres as np.float32(d) * np.float32(0.001)."""
    d = np.asarray(depth)
    if d.dtype == np.uint16:
        return d.astype(np.float32) * np.float32(0.001)
    if d.dtype != np.float32:
        raise ValueError("a depth image is float32 metres or uint16 millimetres, got %s" % d.dtype)
    return d


def _depth(depth, like):
    return _map(depth_metres(depth), np.float32, "a depth image", like)


def _selection(max_features, quality_level, min_distance, border, shapes):
    mf, q, md, b = int(max_features), float(quality_level), int(min_distance), int(border)
    if not 1 <= mf <= 65535:
        raise ValueError("max_features must be in [1, 65535]")
    if not 0.0 <= q <= 1.0:
        raise ValueError("quality_level must be in [0, 1]")
    if not 1 <= md <= FEAT_MAX_DISTANCE:
        raise ValueError("min_distance must be in [1, %d]" % FEAT_MAX_DISTANCE)
    if b < FEAT_MIN_BORDER:
        raise ValueError("border must be at least %d (patch radius 15 plus blur radius 3)" % FEAT_MIN_BORDER)
    for s in shapes:
        if s[0] < 2 * b + 1 or s[1] < 2 * b + 1:
            raise ValueError("an image must be at least 2 * border + 1 = %d on each side, got %s" % (2 * b + 1, tuple(s[:2])))
    return mf, q, md, b


def _keypoints(kp):
    a = np.asarray(kp)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("keypoints are an [n, 2] array of (x, y), got shape %s" % (a.shape,))
    k = a.astype(np.int32)
    if not np.array_equal(k, a):
        raise ValueError("keypoints are whole pixels")
    return np.ascontiguousarray(k)


def _inside(k, shape, margin, what):
    H, W = shape[:2]
    if len(k) and not (k[:, 0].min() >= margin and k[:, 0].max() <= W - 1 - margin and k[:, 1].min() >= margin and k[:, 1].max() <= H - 1 - margin):
        raise ValueError(what)


# ---- a batch on the device -------------------------------------------------------------------------------------------
class _Batch:
    """The pixel offsets and sizes of a list of [H, W(, 3)] arrays, on the host and on the device."""

    def __init__(self, shapes, dev):
        self.n = len(shapes)
        self.hw = np.ascontiguousarray([[s[0], s[1]] for s in shapes], dtype=np.int32).reshape(self.n, 2)
        self.off = offsets([int(s[0]) * int(s[1]) for s in shapes])
        self.total = int(self.off[-1])
        self.t_hw, self.t_off = to_dev(self.hw, dev), to_dev(self.off, dev)

    def flat(self, arrays, dtype, dev):
        return to_dev(np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays]), dev)

    def split(self, flat):
        return [flat[self.off[c]:self.off[c + 1]].reshape(self.hw[c]).copy() for c in range(self.n)]


def _ragged_keypoints(kps, dev):
    off = offsets([len(k) for k in kps])
    cat = np.concatenate(kps, axis=0) if kps else np.zeros((0, 2), dtype=np.int32)
    return off, to_dev(cat, dev), to_dev(off, dev)


def to_gray_batch(images, device=0):
    """Grey images uint8 [H, W] of a list of images in ONE call (`cslam_feat_gray_dev`)."""
    imgs = [_image(i) for i in images]
    with gpu(device) as (lib, dev):
        import torch
        if not imgs:
            return []
        b = _Batch([i.shape for i in imgs], dev)
        src_off = offsets([i.size for i in imgs])
        t_src, t_so = b.flat(imgs, np.uint8, dev), to_dev(src_off, dev)
        t_gray = torch.zeros(b.total, dtype=torch.uint8, device=dev)
        _lib.check(lib.cslam_feat_gray_dev(t_src.data_ptr(), t_so.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n, t_gray.data_ptr(),
                                           host(src_off), host(b.off), host(b.hw), stream()))
        return b.split(t_gray.cpu().numpy())


def to_gray(image, device=0):
    return to_gray_batch([image], device)[0]


def corner_response_batch(grays, device=0):
    """(R int32 [H, W], Rmax) per grey image, in ONE call (`cslam_feat_response_dev`)."""
    imgs = [_image(g, channels_ok=(1,)) for g in grays]
    with gpu(device) as (lib, dev):
        import torch
        if not imgs:
            return []
        b = _Batch([i.shape for i in imgs], dev)
        t_gray = b.flat(imgs, np.uint8, dev)
        t_R = torch.zeros(b.total, dtype=torch.int32, device=dev)
        t_max = torch.zeros(b.n, dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_feat_response_dev(t_gray.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n, t_R.data_ptr(), t_max.data_ptr(),
                                               host(b.off), host(b.hw), stream()))
        R, rmax = b.split(t_R.cpu().numpy()), t_max.cpu().numpy()
    return [(R[c], int(rmax[c])) for c in range(len(imgs))]


def corner_response(gray, device=0):
    return corner_response_batch([gray], device)[0]


def select_keypoints_batch(responses, valids=None, max_features=1000, quality_level=0.001, min_distance=7, border=19, device=0):
    """Keypoints of a list of response maps (int32 [H, W]; `valids`: None or per map None / [H, W] bool or uint8) in ONE call
    (`cslam_feat_select_dev`): per map (keypoints int32 [k, 2] = (x, y), responses int32 [k]), in the order of selection.
    Rmax is the maximum of the map."""
    maps = [_map(r, np.int32, "a response map") for r in responses]
    mf, q, md, bd = _selection(max_features, quality_level, min_distance, border, [m.shape for m in maps])
    if valids is None:
        valids = [None] * len(maps)
    if len(valids) != len(maps):
        raise ValueError("one validity mask (or None) per response map")
    masks = []
    for v, m in zip(valids, maps):
        v = np.ones(m.shape, dtype=np.uint8) if v is None else np.asarray(v)
        if v.dtype == np.bool_:
            v = v.astype(np.uint8)
        masks.append(_map(v, np.uint8, "a validity mask", m.shape))
    if any(m.min() < 0 for m in maps):
        raise ValueError("a response is not negative")
    with gpu(device) as (lib, dev):
        import torch
        if not maps:
            return []
        b = _Batch([m.shape for m in maps], dev)
        t_R, t_valid = b.flat(maps, np.int32, dev), b.flat(masks, np.uint8, dev)
        t_max = to_dev(np.array([m.max() for m in maps], dtype=np.int32), dev)
        t_cnt = torch.zeros(b.n, dtype=torch.int32, device=dev)
        t_kp = torch.zeros((b.n, mf, 2), dtype=torch.int32, device=dev)
        t_resp = torch.zeros((b.n, mf), dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_feat_select_dev(t_R.data_ptr(), t_max.data_ptr(), t_valid.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n,
                                             q, md, bd, mf, t_cnt.data_ptr(), t_kp.data_ptr(), t_resp.data_ptr(), host(b.off), host(b.hw),
                                             stream()))
        cnt, kp, resp = t_cnt.cpu().numpy(), t_kp.cpu().numpy(), t_resp.cpu().numpy()
    return [(kp[c, :cnt[c]].copy(), resp[c, :cnt[c]].copy()) for c in range(len(maps))]


def select_keypoints(response, valid=None, max_features=1000, quality_level=0.001, min_distance=7, border=19, device=0):
    return select_keypoints_batch([response], [valid], max_features, quality_level, min_distance, border, device)[0]


def describe_batch(grays, keypoints, device=0):
    """(bins int32 [k], descriptors uint8 [k, 32]) per (grey image, keypoints [k, 2]) in ONE call (`cslam_feat_describe_dev`).
    Keypoints must lie at least 18 pixels from the edges."""
    imgs = [_image(g, channels_ok=(1,)) for g in grays]
    if len(keypoints) != len(imgs):
        raise ValueError("one keypoint array per image")
    kps = [_keypoints(k) for k in keypoints]
    for k, i in zip(kps, imgs):
        _inside(k, i.shape, FEAT_MIN_BORDER, "keypoints to describe must lie at least %d pixels from the edges" % FEAT_MIN_BORDER)
    with gpu(device) as (lib, dev):
        import torch
        if not imgs:
            return []
        b = _Batch([i.shape for i in imgs], dev)
        t_gray = b.flat(imgs, np.uint8, dev)
        k_off, t_kp, t_ko = _ragged_keypoints(kps, dev)
        t_bins = torch.zeros(max(int(k_off[-1]), 1), dtype=torch.int32, device=dev)
        t_desc = torch.zeros((max(int(k_off[-1]), 1), FEAT_DESC_BYTES), dtype=torch.uint8, device=dev)
        _lib.check(lib.cslam_feat_describe_dev(t_gray.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n, t_kp.data_ptr(), t_ko.data_ptr(),
                                               t_bins.data_ptr(), t_desc.data_ptr(), host(b.off), host(b.hw), host(k_off), stream()))
        bins, desc = t_bins.cpu().numpy(), t_desc.cpu().numpy()
    return [(bins[k_off[c]:k_off[c + 1]].copy(), desc[k_off[c]:k_off[c + 1]].copy()) for c in range(len(imgs))]


def describe(image, keypoints, device=0):
    return describe_batch([image], [keypoints], device)[0]


def back_project_batch(depths, keypoints, cameras, device=0):
    """Points float64 [k, 3] per (depth image, keypoints [k, 2]) in ONE call (`cslam_feat_points_dev`).  `cameras`:
    (fx, fy, cx, cy), one for all or one per image.  A keypoint without valid depth gives a NaN row."""
    if len(keypoints) != len(depths):
        raise ValueError("one keypoint array per depth image")
    dps = [_map(depth_metres(d), np.float32, "a depth image") for d in depths]
    kps = [_keypoints(k) for k in keypoints]
    for k, d in zip(kps, dps):
        _inside(k, d.shape, 0, "keypoints must lie inside the depth image")
    cam = _cameras(cameras, len(dps))
    with gpu(device) as (lib, dev):
        import torch
        if not dps:
            return []
        b = _Batch([d.shape for d in dps], dev)
        t_depth, t_cam = b.flat(dps, np.float32, dev), to_dev(cam, dev)
        k_off, t_kp, t_ko = _ragged_keypoints(kps, dev)
        t_pts = torch.zeros((max(int(k_off[-1]), 1), 3), dtype=torch.float64, device=dev)
        _lib.check(lib.cslam_feat_points_dev(t_depth.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n, t_kp.data_ptr(), t_ko.data_ptr(),
                                             t_cam.data_ptr(), t_pts.data_ptr(), host(b.off), host(b.hw), host(k_off), stream()))
        pts = t_pts.cpu().numpy()
    return [pts[k_off[c]:k_off[c + 1]].copy() for c in range(len(dps))]


def back_project(depth, keypoints, camera, device=0):
    return back_project_batch([depth], [keypoints], camera, device)[0]


def extract_features(images, depths, cameras, max_features=1000, quality_level=0.001, min_distance=7, border=19, depth_as_mask=True, device=0):
    """The whole chain of a list of images in ONE call (`cslam_feat_extract_dev`), chained on the device with no host wait in
    between.  Per image a dict: keypoints int32 [k, 2], responses int32 [k], bins int32 [k], descriptors uint8 [k, 32],
    points float64 [k, 3]."""
    imgs = [_image(i) for i in images]
    if len(depths) != len(imgs):
        raise ValueError("one depth image per image")
    dps = [_depth(d, i.shape[:2]) for d, i in zip(depths, imgs)]
    mf, q, md, bd = _selection(max_features, quality_level, min_distance, border, [i.shape for i in imgs])
    cam = _cameras(cameras, len(imgs))
    with gpu(device) as (lib, dev):
        if not imgs:
            return []
        b = _Batch([i.shape for i in imgs], dev)
        src_off = offsets([i.size for i in imgs])
        return _extract_on_device(lib, dev, b, b.flat(imgs, np.uint8, dev), to_dev(src_off, dev), src_off, b.flat(dps, np.float32, dev), cam,
                                  (mf, q, md, bd), depth_as_mask)


def _extract_on_device(lib, dev, b, t_src, t_so, src_off, t_depth, cam, selection, depth_as_mask):
    """`cslam_feat_extract_dev` on images and depths that are on the device already (front_end/rectify.py chains into it), and
    the one download: the list `extract_features` returns."""
    import torch
    mf, q, md, bd = selection
    t_cam = to_dev(cam, dev)
    t_cnt = torch.zeros(b.n, dtype=torch.int32, device=dev)
    t_kp = torch.zeros((b.n, mf, 2), dtype=torch.int32, device=dev)
    t_resp = torch.zeros((b.n, mf), dtype=torch.int32, device=dev)
    t_bins = torch.zeros((b.n, mf), dtype=torch.int32, device=dev)
    t_desc = torch.zeros((b.n, mf, FEAT_DESC_BYTES), dtype=torch.uint8, device=dev)
    t_pts = torch.zeros((b.n, mf, 3), dtype=torch.float64, device=dev)
    _lib.check(lib.cslam_feat_extract_dev(t_src.data_ptr(), t_so.data_ptr(), t_depth.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(),
                                          t_cam.data_ptr(), b.n, q, md, bd, mf, 1 if depth_as_mask else 0, t_cnt.data_ptr(), t_kp.data_ptr(),
                                          t_resp.data_ptr(), t_bins.data_ptr(), t_desc.data_ptr(), t_pts.data_ptr(), host(src_off),
                                          host(b.off), host(b.hw), stream()))
    cnt = t_cnt.cpu().numpy()
    kp, resp, bins, desc, pts = (t.cpu().numpy() for t in (t_kp, t_resp, t_bins, t_desc, t_pts))
    return [dict(keypoints=kp[c, :cnt[c]].copy(), responses=resp[c, :cnt[c]].copy(), bins=bins[c, :cnt[c]].copy(),
                 descriptors=desc[c, :cnt[c]].copy(), points=pts[c, :cnt[c]].copy()) for c in range(b.n)]


def extract_keyframes(images, depths, cameras, max_features=1000, quality_level=0.001, min_distance=7, border=19, depth_as_mask=True, device=0):
    """A `Keyframe` (keypoints float64 [k, 2], points float64 [k, 3], descriptors uint8 [k, 32]) per image: what
    `compute_local_descriptors` leaves in the reference, ready for `register_pairs`."""
    return [Keyframe(f["keypoints"].astype(np.float64), f["points"], f["descriptors"])
            for f in extract_features(images, depths, cameras, max_features, quality_level, min_distance, border, depth_as_mask, device)]


def is_new_keyframe(registration, n_previous_keypoints, ratio_threshold):
    """The rule of `generate_new_keyframe` (rgbd_handler.cpp:314-351) on the registration of the new frame against the
    previous keyframe: False iff the registration succeeded and has more inliers than `ratio_threshold` times the previous
    keyframe's keypoints.  A threshold above 0.99 always gives True (every frame is a keyframe)."""
    if ratio_threshold > 0.99:
        return True
    inliers = int(np.count_nonzero(registration.inliers))
    return not (registration.success and inliers > ratio_threshold * n_previous_keypoints)
