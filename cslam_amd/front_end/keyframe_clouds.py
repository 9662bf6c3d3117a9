"""The coloured cloud of an RGB-D keyframe, on the GPU (csrc/cloud.hip, rules in csrc/cloud.h): the back-projection of
the depth image, a voxel grid filter and a clip on z.

Replaces `RGBDHandler::send_visualization_pointcloud` of the reference's src/front_end/rgbd_handler.cpp:640-682:
`create_colored_pointcloud` (src/front_end/visualization_utils.cpp:8-137), then pcl::VoxelGrid with
`visualization.voxel_size` (default 0.05) and pcl::PassThrough on z with [0, `visualization.max_range`] (default 2.0).
PCL was not available to compare against, and its VoxelGrid orders points with an unstable std::sort, so its float sums
have no defined order: parity with PCL is unpinned and stays so.  The rule is the one include/cslam_hip.h states and
tests/cloud_reference.py restates in numpy, and the two agree bit for bit: float32 arithmetic throughout, a voxel's
points summed in pixel order one at a time, colours as exact integer sums with a truncating division.

Images are uint8 [H, W] or [H, W, 3] (B, G, R); depths uint16 millimetres or float32 metres of the same size (uint16
goes to the device as it is: the reference folds the unit into its constant, which gives other bits than metres first).
A uint16 depth of 0 and a non-finite float depth are invalid and give a NaN row; a float depth of 0 or below is valid
here, as in the reference, although visual_features.py treats it as invalid.  A depth image of another size than its
image raises ValueError (the reference warns and returns an empty cloud).

A cloud is a `KeyframeCloud`: points float32 [m, 3], colors uint8 [m, 3] (r, g, b), counts int64 [m] (points per voxel).

Stereo frames have no depth image and the reference sends no cloud for them: `stereo_depth.keyframe_clouds_stereo` makes one
from the rectified pair and hands it to the chain below.  Out of scope: depth images smaller than the colour image, the
`range_max` substitution for invalid depths (the reference never passes it), ROS message packing.

There is no CPU path: without the library or a GPU the functions raise CslamHipError.
"""
import collections

import numpy as np

from .. import _lib
from ..lidar_pr import _batch
from ..lidar_pr._batch import gpu, host, offsets, result_args, result_buffer, stream, to_dev
from ..lidar_pr.voxel import VoxelSizeError, raise_failed
from .visual_features import _Batch, _image
from .visual_registration import _cameras

KeyframeCloud = collections.namedtuple("KeyframeCloud", "points colors counts")

CLOUD_DEPTH_U16, CLOUD_DEPTH_F32 = 0, 1      # csrc/cloud.h
CLOUD_BOUNDS_BLOCK = 256                     # threads per workgroup of the projection and bounds kernels
DEPTH_TYPES = {np.dtype(np.uint16): CLOUD_DEPTH_U16, np.dtype(np.float32): CLOUD_DEPTH_F32}


# ---- argument checks: everything that can be wrong raises here, before any launch ------------------------------------
def _frames(images, depths, cameras):
    imgs = [_image(i) for i in images]
    if len(depths) != len(imgs):
        raise ValueError("one depth image per image")
    dps = []
    for d, i in zip(depths, imgs):
        d = np.asarray(d)
        if d.dtype not in DEPTH_TYPES:
            raise ValueError("a depth image is uint16 millimetres or float32 metres, got %s" % d.dtype)
        if d.shape != i.shape[:2]:
            raise ValueError("a depth image has shape %s, its image %s (the reference returns an empty cloud)" % (d.shape, i.shape[:2]))
        dps.append(np.ascontiguousarray(d))
    return imgs, dps, _cameras(cameras, len(imgs))


def _leaf(voxel_size, max_range):
    v, r = float(voxel_size), float(max_range)
    if not np.isfinite(v):
        raise ValueError("voxel_size must be finite")
    if not r >= 0.0:
        raise ValueError("max_range must not be negative or NaN")
    return v, r


def _cloud(points, colors):
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("a cloud is an [n, 3] array, got shape %s" % (p.shape,))
    p = np.ascontiguousarray(p, dtype=np.float32)
    if colors is None:
        return p, None
    c = np.asarray(colors)
    if c.dtype != np.uint8 or c.shape != p.shape:
        raise ValueError("colours are uint8 [n, 3] (r, g, b), one row per point")
    return p, np.ascontiguousarray(c)


def pack_colors(colors):
    """uint8 [n, 3] (r, g, b) as the kernels' uint32 r | g << 8 | b << 16."""
    w = np.zeros((len(colors), 4), dtype=np.uint8)
    w[:, :3] = colors
    return w.view(np.uint32).reshape(-1)


def unpack_colors(words):
    return np.ascontiguousarray(words.view(np.uint8).reshape(-1, 4)[:, :3])


def _groups(imgs, dps):
    """Frame numbers by (depth type, channels): one call takes one of each."""
    g = collections.OrderedDict()
    for k, (i, d) in enumerate(zip(imgs, dps)):
        g.setdefault((DEPTH_TYPES[d.dtype], 3 if i.ndim == 3 else 1), []).append(k)
    return g


# ---- the device side: every launch is written once -------------------------------------------------------------------
class _Frames:
    """One group of frames on the device: the arguments both frame entry points start with."""

    def __init__(self, imgs, dps, cam, key, dev):
        self.b = _Batch([d.shape for d in dps], dev)
        self.t_img = self.b.flat(imgs, np.uint8, dev)
        self.t_depth = to_dev(np.concatenate([d.reshape(-1) for d in dps]).view(np.uint8), dev)      # as bytes: uint16 or float32
        self.t_cam = to_dev(cam, dev)
        self.depth_type, self.channels = key

    @classmethod
    def on_device(cls, b, t_img, t_depth, t_cam, key):
        """The same of arrays that are on the device already: `b` their `_Batch`, `t_cam` [n, 4]."""
        f = cls.__new__(cls)
        f.b, f.t_img, f.t_depth, f.t_cam = b, t_img, t_depth, t_cam
        f.depth_type, f.channels = key
        return f

    def head(self):
        b = self.b
        return (self.t_img.data_ptr(), self.channels, self.t_depth.data_ptr(), self.depth_type, b.t_off.data_ptr(), b.t_hw.data_ptr(),
                self.t_cam.data_ptr(), b.n)


def unpack_result(host_bytes, lay, n, dtype, colors=True):
    """The downloaded result buffer (`result_buffer` of lidar_pr/_batch.py) as a KeyframeCloud per cloud, and the numbers
    of the clouds with status 1."""
    res, failed = _batch.unpack_result(host_bytes, lay, n, dtype, colors)
    return [KeyframeCloud(p, unpack_colors(w) if colors else None, k) for p, w, k in res], failed


def _project(lib, f):
    import torch
    t_pts = torch.zeros((max(f.b.total, 1), 3), dtype=torch.float32, device=f.t_img.device)
    t_rgb = torch.zeros(max(f.b.total, 1), dtype=torch.int32, device=f.t_img.device)
    _lib.check(lib.cslam_cloud_from_depth_dev(*f.head(), t_pts.data_ptr(), t_rgb.data_ptr(), host(f.b.off), host(f.b.hw), stream()))
    return t_pts, t_rgb


def _organised(f, t_pts, t_rgb):
    pts, rgb = t_pts.cpu().numpy(), unpack_colors(t_rgb.cpu().numpy().view(np.uint32))
    off = f.b.off
    return [KeyframeCloud(pts[off[c]:off[c + 1]].copy(), rgb[off[c]:off[c + 1]].copy(), np.ones(int(off[c + 1] - off[c]), dtype=np.int64))
            for c in range(f.b.n)]


def _per_group(imgs, dps, cam, dev, one):
    """`one(frames)` -> a list per group, put back in the callers' order."""
    out = [None] * len(imgs)
    for key, sel in _groups(imgs, dps).items():
        f = _Frames([imgs[k] for k in sel], [dps[k] for k in sel], cam[sel], key, dev)
        for k, r in zip(sel, one(f)):
            out[k] = r
    return out


# ---- public ----------------------------------------------------------------------------------------------------------
def create_colored_pointclouds(images, depths, cameras, device=0):
    """The organised cloud of every frame (`cslam_cloud_from_depth_dev`): a `KeyframeCloud` of H * W rows in row-major
    pixel order, NaN rows for invalid depths, counts all 1.  `cameras`: (fx, fy, cx, cy), one for all or one per frame.
    Frames of different sizes go in one call; frames of different depth or image types in one call per type."""
    imgs, dps, cam = _frames(images, depths, cameras)
    with gpu(device) as (lib, dev):
        return _per_group(imgs, dps, cam, dev, lambda f: _organised(f, *_project(lib, f)))


def create_colored_pointcloud(image, depth, camera, device=0):
    """Counterpart of the reference's `create_colored_pointcloud` (visualization_utils.cpp:8-137)."""
    return create_colored_pointclouds([image], [depth], camera, device)[0]


def voxel_subsample_batch(clouds, voxel_size=0.05, max_range=2.0, device=0):
    """`visualization_pointcloud_voxel_subsampling` (rgbd_handler.cpp:640-663) of a list of (points, colors) pairs or
    KeyframeClouds in ONE call (`cslam_cloud_voxel_dev`): one row per occupied voxel of side `voxel_size`, in ascending
    (iz, iy, ix); then the rows with 0 <= z <= max_range.  Rows with a non-finite coordinate are left out.  `colors` may
    be None.  `voxel_size <= 0` returns the clouds as they are, unclipped (rgbd_handler.cpp:675).
    Raises `VoxelSizeError` naming the clouds that need a voxel index of 2^21 or more on some axis; PCL prints a warning
    and returns such a cloud unfiltered."""
    v, r = _leaf(voxel_size, max_range)
    cl = [_cloud(c[0], c[1]) for c in clouds]
    if any((c[1] is None) != (cl[0][1] is None) for c in cl):
        raise ValueError("either every cloud of a batch has colours or none")
    with gpu(device) as (lib, dev):
        if v <= 0.0:
            return [KeyframeCloud(p, c, np.ones(len(p), dtype=np.int64)) for p, c in cl]
        if not cl:
            return []
        colors = cl[0][1] is not None
        off = offsets([len(p) for p, _ in cl])
        n, total = len(cl), int(off[-1])
        t_pts = to_dev(np.concatenate([p for p, _ in cl], axis=0), dev)
        t_rgb = to_dev(np.concatenate([pack_colors(c) for _, c in cl]).view(np.int32), dev) if colors else None
        t_off = to_dev(off, dev)
        t_out, lay = result_buffer(n, total, 4, dev)
        _lib.check(lib.cslam_cloud_voxel_dev(t_pts.data_ptr(), t_rgb.data_ptr() if colors else None, t_off.data_ptr(), n, v, r,
                                             *result_args(t_out, lay, colors), host(off), stream()))
        host_bytes = t_out.cpu().numpy()
    return raise_failed(*unpack_result(host_bytes, lay, n, np.float32, colors))


def voxel_subsample(points, colors, voxel_size=0.05, max_range=2.0, device=0):
    """`voxel_subsample_batch` of one cloud: points [n, 3], colors uint8 [n, 3] or None -> a `KeyframeCloud`."""
    return voxel_subsample_batch([(points, colors)], voxel_size, max_range, device)[0]


def keyframe_clouds(images, depths, cameras, voxel_size=0.05, max_range=2.0, device=0):
    """What `send_visualization_pointcloud` (rgbd_handler.cpp:665-682) publishes, per frame, chained on the device with one
    host wait (`cslam_cloud_keyframes_dev`): the same bytes as `create_colored_pointclouds`, then `voxel_subsample_batch`.
    Ragged batches go in one call; mixed depth or image types in one call per type.  `voxel_size <= 0` returns the
    organised clouds.  Raises `VoxelSizeError` as `voxel_subsample_batch` does, numbering the frames as given."""
    v, r = _leaf(voxel_size, max_range)
    imgs, dps, cam = _frames(images, depths, cameras)

    def chain(f):
        t_out, lay = result_buffer(f.b.n, f.b.total, 4, f.t_img.device)
        _lib.check(lib.cslam_cloud_keyframes_dev(*f.head(), v, r, *result_args(t_out, lay), host(f.b.off), host(f.b.hw), stream()))
        res, bad = unpack_result(t_out.cpu().numpy(), lay, f.b.n, np.float32)
        return [None if c in bad else x for c, x in enumerate(res)]

    with gpu(device) as (lib, dev):
        if v <= 0.0:
            return _per_group(imgs, dps, cam, dev, lambda f: _organised(f, *_project(lib, f)))
        res = _per_group(imgs, dps, cam, dev, chain)
    failed = [k for k, x in enumerate(res) if x is None]
    if failed:
        raise VoxelSizeError(failed, res)
    return res
