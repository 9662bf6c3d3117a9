"""The depth image of a stereo keyframe and its coloured cloud, on the GPU (csrc/stereo_dense.hip; the rule is
csrc/stereo.h's, the tile plan and the per-pixel bookkeeping csrc/stereo_dense.h's).

The reference sends no cloud for a stereo frame: `StereoHandler` has no depth image to hand to
`send_visualization_pointcloud` (rgbd_handler.cpp:665-682).  Here the stereo rule of `visual_stereo` runs at EVERY pixel
of the rectified pair, the accepted disparities become a float32 depth image in metres, and that goes through the cloud
chain of `keyframe_clouds` unchanged; the results go straight into `back_end.swarm_map.assemble_map`.

Pinned: a pixel's status, best and disparity are the bits `stereo_match` gives for a keypoint at that pixel
(tests/test_stereo_dense_gpu.py, every pixel of twelve scenes), and tests/stereo_dense_reference.py restates the dense form
in numpy and agrees bit for bit.  Unpinned: parity with rtabmap's or OpenCV's dense matchers.

Images are uint8 [H, W] or [H, W, 3] (B, G, R), the two sides of a frame of the same H x W (they may differ in channels);
a camera is (fx, fy, cx, cy, baseline), one for all frames or one per frame.  Status as in `visual_stereo.STATUS`.

Raw (distorted, unrectified) pairs enter through rectify.py's `keyframe_clouds_stereo_raw`.

Out of scope: different principal points, pyramids, speckle and median post-filters.

There is no CPU path: without the library or a GPU the functions raise CslamHipError.
"""
import collections

import numpy as np

from .. import _lib
from ..lidar_pr._batch import gpu, host, offsets, result_args, result_buffer, stream, to_dev
from ..lidar_pr.voxel import VoxelSizeError
from .keyframe_clouds import CLOUD_DEPTH_F32, _Frames, _leaf, _organised, _project, unpack_result
from .visual_features import _Batch
from .visual_stereo import _pairs, _parameters, _stereo_cameras


# ---- the device side: every launch is written once -------------------------------------------------------------------
class _Pairs:
    """A list of stereo frames on the device: both sides as given (1 or 3 channels each) and the cameras."""

    def __init__(self, ls, rs, cam, dev):
        self.place(_Batch([i.shape for i in ls], dev), offsets([i.size for i in ls]), offsets([i.size for i in rs]), cam, dev)
        self.t_left, self.t_right = self.b.flat(ls, np.uint8, dev), self.b.flat(rs, np.uint8, dev)

    def place(self, b, l_off, r_off, cam, dev):
        self.b, self.l_off, self.r_off, self.cam, self.dev = b, l_off, r_off, np.ascontiguousarray(cam), dev
        self.t_lo, self.t_ro, self.t_cam = to_dev(l_off, dev), to_dev(r_off, dev), to_dev(self.cam, dev)

    @classmethod
    def on_device(cls, b, t_left, l_off, t_right, r_off, cam, dev):
        """Pairs whose bytes are on the device already (front_end/rectify.py chains into the functions below)."""
        p = cls.__new__(cls)
        p.place(b, l_off, r_off, cam, dev)
        p.t_left, p.t_right = t_left, t_right
        return p


def _gray(lib, p, t_src, t_so, src_off):
    import torch
    t_gray = torch.zeros(max(p.b.total, 1), dtype=torch.uint8, device=p.dev)
    _lib.check(lib.cslam_feat_gray_dev(t_src.data_ptr(), t_so.data_ptr(), p.b.t_off.data_ptr(), p.b.t_hw.data_ptr(), p.b.n, t_gray.data_ptr(),
                                       host(src_off), host(p.b.off), host(p.b.hw), stream()))
    return t_gray


def _dense(lib, p, params, with_best):
    """Grey of both sides, then the dense rule: device tensors (disparity, status, depth, best or None)."""
    import torch
    t_gl, t_gr = _gray(lib, p, p.t_left, p.t_lo, p.l_off), _gray(lib, p, p.t_right, p.t_ro, p.r_off)
    rows = max(p.b.total, 1)
    t_disp = torch.zeros(rows, dtype=torch.float32, device=p.dev)
    t_status = torch.zeros(rows, dtype=torch.uint8, device=p.dev)
    t_depth = torch.zeros(rows, dtype=torch.float32, device=p.dev)
    t_best = torch.zeros((rows, 4), dtype=torch.int32, device=p.dev) if with_best else None
    _lib.check(lib.cslam_stereo_dense_dev(t_gl.data_ptr(), t_gr.data_ptr(), p.b.t_off.data_ptr(), p.b.t_hw.data_ptr(), p.b.n,
                                          p.t_cam.data_ptr(), *params, t_disp.data_ptr(), t_status.data_ptr(), t_depth.data_ptr(),
                                          t_best.data_ptr() if with_best else None, host(p.b.off), host(p.b.hw), host(p.cam), stream()))
    return t_disp, t_status, t_depth, t_best


def _by_left_channels(ls):
    """Frame numbers by the channels of the left image: the cloud kernels take one number per call."""
    g = collections.OrderedDict()
    for k, i in enumerate(ls):
        g.setdefault(3 if i.ndim == 3 else 1, []).append(k)
    return g


def _clouds(lib, p, channels, params, v, r):
    """The clouds of the pairs `p`, whose left images have `channels` channels: organised for v <= 0, else the chain
    (`cslam_cloud_keyframes_stereo_dev`), a cloud that overflowed its voxel grid as None."""
    if v <= 0.0:
        f = _Frames.on_device(p.b, p.t_left, _dense(lib, p, params, False)[2], to_dev(p.cam[:, :4], p.dev), (CLOUD_DEPTH_F32, channels))
        return _organised(f, *_project(lib, f))
    b = p.b
    t_out, lay = result_buffer(b.n, b.total, 4, p.dev)
    _lib.check(lib.cslam_cloud_keyframes_stereo_dev(p.t_left.data_ptr(), p.t_lo.data_ptr(), channels, p.t_right.data_ptr(),
                                                    p.t_ro.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), p.t_cam.data_ptr(), b.n,
                                                    *params, v, r, *result_args(t_out, lay), host(p.l_off), host(p.r_off), host(b.off),
                                                    host(b.hw), host(p.cam), stream()))
    res, bad = unpack_result(t_out.cpu().numpy(), lay, b.n, np.float32)
    return [None if c in bad else x for c, x in enumerate(res)]


# ---- public ----------------------------------------------------------------------------------------------------------
def dense_disparity_batch(lefts, rights, cameras, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, return_best=False,
                          device=0):
    """The stereo rule at every pixel of a list of rectified pairs in ONE call (`cslam_stereo_dense_dev` after
    `cslam_feat_gray_dev` of both sides).  Per frame a dict: disparity float32 [H, W] (NaN unless accepted), status uint8
    [H, W], depth float32 [H, W] in metres (NaN unless accepted), and with `return_best` best int32 [H, W, 4] = (d*,
    C(d* - 1), C(d*), C(d* + 1)).  Ragged sizes and mixed channels go in one call; a frame's result does not depend on the
    batch it is in."""
    ls, rs = _pairs(lefts, rights, (1, 3))
    params = _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance)
    cam = _stereo_cameras(cameras, len(ls))
    with gpu(device) as (lib, dev):
        if not ls:
            return []
        p = _Pairs(ls, rs, cam, dev)
        t_disp, t_status, t_depth, t_best = _dense(lib, p, params, bool(return_best))
        disp, status, depth = p.b.split(t_disp.cpu().numpy()), p.b.split(t_status.cpu().numpy()), p.b.split(t_depth.cpu().numpy())
        res = [dict(disparity=d, status=s, depth=z) for d, s, z in zip(disp, status, depth)]
        if return_best:
            best = t_best.cpu().numpy()
            for c, r in enumerate(res):
                r["best"] = best[p.b.off[c]:p.b.off[c + 1]].reshape(p.b.hw[c][0], p.b.hw[c][1], 4).copy()
    return res


def dense_disparity(left, right, camera, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, return_best=False, device=0):
    return dense_disparity_batch([left], [right], camera, min_disparity, max_disparity, uniqueness, lr_tolerance, return_best, device)[0]


def keyframe_clouds_stereo(lefts, rights, cameras, voxel_size=0.05, max_range=2.0, min_disparity=1, max_disparity=128, uniqueness=15,
                           lr_tolerance=1, device=0):
    """The `KeyframeCloud` of every stereo frame, chained on the device with one host wait
    (`cslam_cloud_keyframes_stereo_dev`): the same bytes as `keyframe_clouds` of the left images and the depth of
    `dense_disparity_batch`, with the conventions of `keyframe_clouds`: `voxel_size <= 0` returns the organised clouds
    (H * W rows, a NaN row wherever the status is not 0), and `VoxelSizeError` numbers the frames as given.  Mixed left
    channels go in one call per number of channels."""
    v, r = _leaf(voxel_size, max_range)
    ls, rs = _pairs(lefts, rights, (1, 3))
    params = _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance)
    cam = _stereo_cameras(cameras, len(ls))

    out = [None] * len(ls)
    with gpu(device) as (lib, dev):
        for channels, sel in _by_left_channels(ls).items():
            p = _Pairs([ls[k] for k in sel], [rs[k] for k in sel], cam[sel], dev)
            for k, x in zip(sel, _clouds(lib, p, channels, params, v, r)):
                out[k] = x
    failed = [k for k, x in enumerate(out) if x is None]
    if failed:
        raise VoxelSizeError(failed, out)
    return out
