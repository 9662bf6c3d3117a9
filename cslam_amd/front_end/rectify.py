"""Raw cameras: undistort and rectify images and depth on the GPU (csrc/rectify.hip, the rule csrc/rectify.h's), and the
visual chains fed with a camera driver's raw frames.

The reference sits behind `image_proc` / `stereo_image_proc` (stereo_handler.cpp:120 hard-codes `alreadyRectified = true`);
this replaces their rectify step, OpenCV's `initUndistortRectifyMap` + `remap`, for a user who holds a `CameraInfo` (K, D, R,
P) and a raw image.  The map of a camera is made once and kept on the device (`rectify_maps`); images go through it
bilinearly on a 1/32-pixel grid with a validity map, depth by the nearest source pixel, never interpolated
(`rectify_images`, `rectify_depths`).  The `*_raw` chains rectify on the device and call the existing `_dev` entry points on
the rectified device buffers: no host copy of a rectified image in between.

Pinned: tests/rectify_reference.py restates the map, the bilinear and the nearest rule in float64 / integer numpy, and the
GPU agrees bit for bit (tests/test_rectify_gpu.py); the identity camera reproduces the input bytes.  Unpinned: parity with
OpenCV / image_proc (its fixed-point interpolation tables and border modes), which were not available to compare against.

A raw camera is K = (fx, fy, cx, cy), D = (k1, k2, p1, p2, k3, k4, k5, k6) (plumb-bob with the rational terms; shorter D are
padded with zeros), R 3 x 3, P = (fx', fy', cx', cy'[, Tx fx']) and the destination size (H, W).  The source size is the
image's own.  Images are uint8 [H, W] or [H, W, 3]; depth is uint16 or float32 [H, W].

Out of scope: different principal points of the two sides of a stereo pair, computing R and P from an extrinsic stereo
calibration (Bouguet's method; `CameraInfo` already carries them), fisheye / equidistant models.

There is no CPU path: without the library or a GPU the functions raise CslamHipError.
"""
import numpy as np

from .. import _lib
from ..lidar_pr._batch import gpu, host, offsets, stream, to_dev
from ..lidar_pr.voxel import VoxelSizeError
from .keyframe_clouds import _leaf
from .stereo_depth import _by_left_channels, _clouds, _Pairs
from .visual_features import _Batch, _extract_on_device, _image, _map, _selection, depth_metres
from .visual_registration import Keyframe
from .visual_stereo import _extract_stereo_on_device, _parameters

RECTIFY_CAM = 26
RECTIFY_U16, RECTIFY_F32 = 0, 1
MAX_PIXELS = 1 << 30                       # csrc/feat_args.h


# ---- argument checks: everything that can be wrong raises here, before any launch ------------------------------------
def _numbers(x, counts, what):
    a = np.asarray(x, dtype=np.float64).reshape(-1)
    if a.size not in counts:
        raise ValueError("%s has %s numbers, got %d" % (what, " or ".join(str(c) for c in counts), a.size))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s must be finite" % what)
    return a


class RawCamera:
    """A raw camera and the rectified one its frames are resampled to.  `values` is the float64 [26] the library takes."""

    def __init__(self, K, D, R, P, size):
        K, D, R = _numbers(K, (4,), "K = (fx, fy, cx, cy)"), _numbers(D, (0, 4, 5, 8), "D"), _numbers(R, (9,), "R")
        P = _numbers(P, (4, 5), "P = (fx', fy', cx', cy'[, Tx fx'])")
        if not (K[0] > 0.0 and K[1] > 0.0 and P[0] > 0.0 and P[1] > 0.0):
            raise ValueError("the focal lengths of K and P must be positive")
        Rm = R.reshape(3, 3)
        if np.abs(Rm @ Rm.T - np.identity(3)).max() > 1e-9 or not np.linalg.det(Rm) > 0.0:
            raise ValueError("R must be orthonormal to 1e-9 with a positive determinant")
        if len(size) != 2 or int(size[0]) != size[0] or int(size[1]) != size[1]:
            raise ValueError("size is (H, W) in whole pixels, got %r" % (size,))
        self.height, self.width = int(size[0]), int(size[1])
        if self.height < 2 or self.width < 2 or self.height * self.width > MAX_PIXELS:
            raise ValueError("a rectified image is at least 2 x 2 and at most 2^30 pixels, got %r" % (size,))
        self.values = np.concatenate([K, D, np.zeros(8 - D.size), R, P, np.zeros(5 - P.size)])

    @classmethod
    def from_camera_info(cls, K, D, R, P, width, height):
        """From the ROS layouts: K 3 x 3, D of 5 (k1, k2, p1, p2, k3) or 8 coefficients, R 3 x 3, P 3 x 4, row-major."""
        K, P = _numbers(K, (9,), "CameraInfo.K"), _numbers(P, (12,), "CameraInfo.P")
        if K[1] != 0.0 or P[1] != 0.0:
            raise ValueError("a skewed camera is not supported")
        return cls((K[0], K[4], K[2], K[5]), _numbers(D, (0, 4, 5, 8), "CameraInfo.D"), R, (P[0], P[5], P[2], P[6], P[3]), (height, width))

    @property
    def projection(self):
        """(fx', fy', cx', cy'): the camera of the rectified image."""
        return tuple(float(v) for v in self.values[21:25])


def stereo_camera(left, right):
    """(fx', fy', cx', cy', baseline) of a rectified pair, the baseline -P_right[0][3] / P_right[0][0] in metres."""
    if not (isinstance(left, RawCamera) and isinstance(right, RawCamera)):
        raise ValueError("stereo_camera takes two RawCamera")
    if not np.array_equal(left.values[21:25], right.values[21:25]):
        raise ValueError("the two sides of a pair must share fx', fy', cx', cy' (different principal points are out of scope)")
    if (left.height, left.width) != (right.height, right.width):
        raise ValueError("the two sides of a pair are rectified to the same H x W")
    baseline = float(-right.values[25] / right.values[21])
    if not baseline > 0.0:
        raise ValueError("the right camera's P[0][3] = Tx fx' must be negative (a positive baseline), got %r" % float(right.values[25]))
    return left.projection + (baseline,)


def _camera_list(cameras):
    cams = [cameras] if isinstance(cameras, RawCamera) else list(cameras)
    if not all(isinstance(c, RawCamera) for c in cams):
        raise ValueError("cameras are RawCamera objects")
    return cams


def _indices(map_index, n_frames, n_maps):
    if map_index is None:
        if n_maps != 1 and n_maps != n_frames:
            raise ValueError("%d frames and %d maps: say which map each frame uses (map_index)" % (n_frames, n_maps))
        return np.zeros(n_frames, dtype=np.int32) if n_maps == 1 else np.arange(n_frames, dtype=np.int32)
    a = np.asarray(map_index)
    if a.shape != (n_frames,) or a.dtype.kind not in "iu":
        raise ValueError("map_index is one whole number per frame")
    if n_frames and (a.min() < 0 or a.max() >= n_maps):
        raise ValueError("map_index must name one of the %d maps" % n_maps)
    return np.ascontiguousarray(a, dtype=np.int32)


def _depth_image(d):
    a = np.asarray(d)
    if a.dtype != np.uint16 and a.dtype != np.float32:
        raise ValueError("a depth image is uint16 or float32, got %s" % a.dtype)
    return _map(a, a.dtype, "a depth image")


# ---- the device side: every launch is written once -------------------------------------------------------------------
class RectifyMaps:
    """The maps of a list of cameras on the device: int32 [pixels, 2] = (qx, qy) in 1/32 source pixel per destination pixel."""

    def __init__(self, hw, t_map, device, cameras=None):
        import torch
        self.n, self.device, self.cameras = len(hw), device, cameras
        self.hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(self.n, 2)
        self.off = offsets([int(h) * int(w) for h, w in self.hw])
        dev = torch.device("cuda", device)
        self.t_map, self.t_hw, self.t_off = t_map, to_dev(self.hw, dev), to_dev(self.off, dev)

    def numpy(self):
        """The maps on the host, int32 [H, W, 2] each."""
        m = self.t_map.cpu().numpy()
        return [m[self.off[c]:self.off[c + 1]].reshape(self.hw[c][0], self.hw[c][1], 2).copy() for c in range(self.n)]

    @classmethod
    def from_numpy(cls, maps, device=0):
        """Maps made elsewhere (int32 [H, W, 2] each), uploaded as they are."""
        ms = []
        for m in maps:
            a = np.asarray(m)
            if a.ndim != 3 or a.shape[2] != 2 or a.dtype != np.int32 or a.shape[0] < 2 or a.shape[1] < 2:
                raise ValueError("a map is int32 [H, W, 2] and at least 2 x 2")
            ms.append(np.ascontiguousarray(a))
        if not ms:
            raise ValueError("at least one map")
        with gpu(device) as (lib, dev):
            return cls([m.shape[:2] for m in ms], to_dev(np.concatenate([m.reshape(-1, 2) for m in ms]), dev), device)


def rectify_maps(cameras, device=0):
    """The maps of a list of `RawCamera` in ONE call (`cslam_rectify_map_dev`), left on the device: make them once per
    camera and pass them to every later call."""
    cams = _camera_list(cameras)
    if not cams:
        raise ValueError("at least one camera")
    with gpu(device) as (lib, dev):
        import torch
        hw = np.array([[c.height, c.width] for c in cams], dtype=np.int32)
        values = np.ascontiguousarray(np.stack([c.values for c in cams]))
        maps = RectifyMaps(hw, torch.zeros((int(hw.prod(axis=1).sum()), 2), dtype=torch.int32, device=dev), device, cams)
        t_cam = to_dev(values, dev)
        _lib.check(lib.cslam_rectify_map_dev(t_cam.data_ptr(), maps.t_off.data_ptr(), maps.t_hw.data_ptr(), maps.n, maps.t_map.data_ptr(),
                                             host(maps.off), host(maps.hw), host(values), stream()))
    return maps


class _Sources:
    """A list of raw arrays ([Hs, Ws] or [Hs, Ws, 3]) on the device, and the maps they go through."""

    def __init__(self, arrays, maps, idx, dev):
        self.maps, self.idx = maps, idx
        self.b = _Batch([tuple(maps.hw[m]) for m in idx], dev)                  # the destinations
        self.src_hw = np.ascontiguousarray([[a.shape[0], a.shape[1]] for a in arrays], dtype=np.int32).reshape(len(arrays), 2)
        self.src_off = offsets([a.size for a in arrays])
        self.channels = [a.shape[2] if a.ndim == 3 else 1 for a in arrays]
        self.t_src = to_dev(np.concatenate([a.reshape(-1) for a in arrays]), dev)
        self.t_so, self.t_shw, self.t_idx = to_dev(self.src_off, dev), to_dev(self.src_hw, dev), to_dev(idx, dev)
        self.dev = dev

    def map_args(self):
        return self.maps.t_map.data_ptr(), self.maps.t_off.data_ptr(), self.t_idx.data_ptr(), self.maps.n

    def host_args(self):
        return host(self.src_off), host(self.src_hw), host(self.maps.off), host(self.maps.hw), host(self.idx), host(self.b.off), host(self.b.hw)


def _remap(lib, s):
    """`cslam_rectify_remap_dev`: (rectified bytes, their byte offsets on the host and on the device, validity) on the device."""
    import torch
    b = s.b
    dst_off = offsets([int(b.off[c + 1] - b.off[c]) * s.channels[c] for c in range(b.n)])
    t_dst = torch.zeros(max(int(dst_off[-1]), 1), dtype=torch.uint8, device=s.dev)
    t_valid = torch.zeros(max(b.total, 1), dtype=torch.uint8, device=s.dev)
    t_do = to_dev(dst_off, s.dev)
    _lib.check(lib.cslam_rectify_remap_dev(s.t_src.data_ptr(), s.t_so.data_ptr(), s.t_shw.data_ptr(), *s.map_args(), b.t_off.data_ptr(),
                                           b.t_hw.data_ptr(), b.n, t_dst.data_ptr(), t_do.data_ptr(), t_valid.data_ptr(), *s.host_args(),
                                           host(dst_off), stream()))
    return t_dst, dst_off, t_do, t_valid


def _nearest(lib, s, src_type, t_mask=None):
    """`cslam_rectify_nearest_dev`: the rectified depth on the device, in the layout of the destinations."""
    import torch
    t_dst = torch.zeros(max(s.b.total, 1), dtype=torch.float32 if src_type == RECTIFY_F32 else torch.int16, device=s.dev)
    _lib.check(lib.cslam_rectify_nearest_dev(s.t_src.data_ptr(), src_type, s.t_so.data_ptr(), s.t_shw.data_ptr(), *s.map_args(),
                                             s.b.t_off.data_ptr(), s.b.t_hw.data_ptr(), s.b.n, None if t_mask is None else t_mask.data_ptr(),
                                             t_dst.data_ptr(), *s.host_args(), stream()))
    return t_dst


def _valid_fractions(b, t_valid):
    import torch
    return torch.stack([t_valid[int(b.off[c]):int(b.off[c + 1])].sum(dtype=torch.float64) / float(b.off[c + 1] - b.off[c])
                        for c in range(b.n)]).cpu().numpy()


def _maps_for(cameras, n):
    """(maps made before or None, index per frame, the cameras still to make maps of or None) of what a chain takes as cameras: one `RawCamera` for all frames, one per frame (the same
    object named twice makes one map), or `RectifyMaps` / (`RectifyMaps`, map_index) made before from cameras."""
    if isinstance(cameras, RectifyMaps):
        cameras = (cameras, None)
    if isinstance(cameras, tuple) and len(cameras) == 2 and isinstance(cameras[0], RectifyMaps):
        if cameras[0].cameras is None:
            raise ValueError("these maps were not made from cameras")
        return cameras[0], _indices(cameras[1], n, cameras[0].n), None
    cams = _camera_list(cameras)
    if len(cams) == 1:
        cams = cams * n
    if len(cams) != n:
        raise ValueError("one camera for all frames or one per frame: got %d for %d frames" % (len(cams), n))
    unique, idx = [], np.zeros(n, dtype=np.int32)
    for k, c in enumerate(cams):
        if not any(c is u for u in unique):
            unique.append(c)
        idx[k] = next(j for j, u in enumerate(unique) if c is u)
    return None, idx, unique


def _resolve(spec, device):
    maps, idx, unique = spec
    return (maps if maps is not None else rectify_maps(unique, device)), idx


def _cameras_of(spec):
    maps, idx, unique = spec
    cams = maps.cameras if maps is not None else unique
    return [cams[m] for m in idx]


# ---- public: the staged calls ----------------------------------------------------------------------------------------
def rectify_images(images, maps, map_index=None):
    """(rectified uint8 [H, W] or [H, W, 3], valid uint8 [H, W]) per raw image in ONE call (`cslam_rectify_remap_dev`).  Frame
    k goes through map `map_index[k]` of `maps` (default: the only map, or map k).  valid is 1 where every source pixel
    that contributes lies inside the raw image; an invalid pixel still holds what the inside taps give."""
    if not isinstance(maps, RectifyMaps):
        raise ValueError("maps is what rectify_maps returns")
    imgs = [_image(i) for i in images]
    idx = _indices(map_index, len(imgs), maps.n)
    with gpu(maps.device) as (lib, dev):
        if not imgs:
            return []
        s = _Sources(imgs, maps, idx, dev)
        t_dst, dst_off, _, t_valid = _remap(lib, s)
        dst, valid = t_dst.cpu().numpy(), s.b.split(t_valid.cpu().numpy())
    out = []
    for c, (h, w) in enumerate(s.b.hw):
        shape = (h, w, 3) if s.channels[c] == 3 else (h, w)
        out.append((dst[dst_off[c]:dst_off[c + 1]].reshape(shape).copy(), valid[c]))
    return out


def rectify_depths(depths, maps, map_index=None):
    """The rectified depth image per raw depth image (all uint16 or all float32) in ONE call (`cslam_rectify_nearest_dev`):
    the nearest source element with its bits preserved, 0 where there is none."""
    if not isinstance(maps, RectifyMaps):
        raise ValueError("maps is what rectify_maps returns")
    dps = [_depth_image(d) for d in depths]
    idx = _indices(map_index, len(dps), maps.n)
    if len({d.dtype for d in dps}) > 1:
        raise ValueError("the depth images of one call are all uint16 or all float32")
    with gpu(maps.device) as (lib, dev):
        if not dps:
            return []
        f32 = dps[0].dtype == np.float32
        s = _Sources([d if f32 else d.view(np.int16) for d in dps], maps, idx, dev)      # int16 carries the bits of uint16
        out = _nearest(lib, s, RECTIFY_F32 if f32 else RECTIFY_U16).cpu().numpy()
    return [x.view(dps[0].dtype) for x in s.b.split(out)]


# ---- public: raw frames into the visual chains -----------------------------------------------------------------------
def _stereo_sides(lefts, rights, left_cams, right_cams):
    if len(lefts) != len(rights):
        raise ValueError("one right image per left image")
    ls, rs = [_image(i) for i in lefts], [_image(i) for i in rights]
    lspec, rspec = _maps_for(left_cams, len(ls)), _maps_for(right_cams, len(rs))
    cam = np.array([stereo_camera(a, b) for a, b in zip(_cameras_of(lspec), _cameras_of(rspec))], dtype=np.float64).reshape(len(ls), 5)
    return ls, rs, lspec, rspec, cam


def extract_keyframes_stereo_raw(lefts, rights, left_cams, right_cams, max_features=1000, quality_level=0.001, min_distance=7, border=19,
                                 min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, device=0):
    """`extract_keyframes_stereo` of raw pairs: both sides through their maps (`cslam_rectify_remap_dev`), then
    `cslam_feat_extract_stereo_dev` on the rectified device buffers with the stereo camera of `stereo_camera`.  Cameras: one
    `RawCamera` per side, one per frame, or (`RectifyMaps`, map_index) made before.  Returns (keyframes, valid float64
    [n, 2]): the fraction of valid pixels of the left and the right rectified image."""
    ls, rs, lspec, rspec, cam = _stereo_sides(lefts, rights, left_cams, right_cams)
    shapes = [(c.height, c.width) for c in _cameras_of(lspec)]
    sel = _selection(max_features, quality_level, min_distance, border, shapes)
    params = _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance)
    with gpu(device) as (lib, dev):
        if not ls:
            return [], np.zeros((0, 2))
        sl, sr = _Sources(ls, *_resolve(lspec, device), dev), _Sources(rs, *_resolve(rspec, device), dev)
        t_left, l_off, t_lo, t_vl = _remap(lib, sl)
        t_right, r_off, t_ro, t_vr = _remap(lib, sr)
        feats = _extract_stereo_on_device(lib, dev, sl.b, t_left, t_lo, l_off, t_right, t_ro, r_off, cam, sel, params)
        valid = np.stack([_valid_fractions(sl.b, t_vl), _valid_fractions(sr.b, t_vr)], axis=1)
    return [Keyframe(f["keypoints"].astype(np.float64), f["points"], f["descriptors"]) for f in feats], valid


def keyframe_clouds_stereo_raw(lefts, rights, left_cams, right_cams, voxel_size=0.05, max_range=2.0, min_disparity=1, max_disparity=128,
                               uniqueness=15, lr_tolerance=1, device=0):
    """`keyframe_clouds_stereo` of raw pairs, rectified on the device in front of `cslam_cloud_keyframes_stereo_dev`; cameras
    as in `extract_keyframes_stereo_raw`.  Returns (clouds, valid float64 [n, 2])."""
    v, r = _leaf(voxel_size, max_range)
    ls, rs, lspec, rspec, cam = _stereo_sides(lefts, rights, left_cams, right_cams)
    params = _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance)
    out, valid = [None] * len(ls), np.zeros((len(ls), 2))
    with gpu(device) as (lib, dev):
        if not ls:
            return out, valid
        (lmaps, lidx), (rmaps, ridx) = _resolve(lspec, device), _resolve(rspec, device)
        for channels, pick in _by_left_channels(ls).items():
            sl = _Sources([ls[k] for k in pick], lmaps, lidx[pick], dev)
            sr = _Sources([rs[k] for k in pick], rmaps, ridx[pick], dev)
            t_left, l_off, _, t_vl = _remap(lib, sl)
            t_right, r_off, _, t_vr = _remap(lib, sr)
            p = _Pairs.on_device(sl.b, t_left, l_off, t_right, r_off, cam[pick], dev)
            for k, x in zip(pick, _clouds(lib, p, channels, params, v, r)):
                out[k] = x
            valid[pick, 0], valid[pick, 1] = _valid_fractions(sl.b, t_vl), _valid_fractions(sr.b, t_vr)
    failed = [k for k, x in enumerate(out) if x is None]
    if failed:
        raise VoxelSizeError(failed, out)
    return out, valid


def extract_keyframes_raw(images, depths, cams, max_features=1000, quality_level=0.001, min_distance=7, border=19, depth_as_mask=True,
                          device=0):
    """`extract_keyframes` of raw RGB-D frames: the image bilinearly and the depth (float32 metres, or uint16 millimetres
    converted as `depth_metres` does) by the nearest pixel through the SAME map, then `cslam_feat_extract_dev` on the
    rectified device buffers with the camera's P.  A pixel whose image is not valid gets depth 0, which the depth mask
    drops.  The depth image has the raw image's size."""
    imgs = [_image(i) for i in images]
    if len(depths) != len(imgs):
        raise ValueError("one depth image per image")
    dps = [_map(depth_metres(d), np.float32, "a depth image", i.shape[:2]) for d, i in zip(depths, imgs)]
    spec = _maps_for(cams, len(imgs))
    cameras = _cameras_of(spec)
    sel = _selection(max_features, quality_level, min_distance, border, [(c.height, c.width) for c in cameras])
    cam = np.array([c.projection for c in cameras], dtype=np.float64).reshape(len(imgs), 4)
    with gpu(device) as (lib, dev):
        if not imgs:
            return []
        maps, idx = _resolve(spec, device)
        si, sd = _Sources(imgs, maps, idx, dev), _Sources(dps, maps, idx, dev)
        t_img, img_off, t_io, t_valid = _remap(lib, si)
        t_depth = _nearest(lib, sd, RECTIFY_F32, t_valid)
        feats = _extract_on_device(lib, dev, si.b, t_img, t_io, img_off, t_depth, cam, sel, depth_as_mask)
    return [Keyframe(f["keypoints"].astype(np.float64), f["points"], f["descriptors"]) for f in feats]
