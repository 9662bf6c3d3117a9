"""Batched voxel down-sampling of keyframe clouds (`cslam_voxel_downsample_dev`: the filter chain of csrc/cloud.hip with
open3d's rule of csrc/cloud.h, on the engine of csrc/voxel.hip): the counterpart of
the reference's `downsample` (icp_utils.py:93-100, open3d's `voxel_down_sample`).  `enqueue` and `unpack` are the two
halves `keyframes.ingest` shares with `downsample_clouds`."""
import numpy as np

from .. import _lib
from ._batch import gpu, host, result_args, result_buffer, rows, stream, unpack_result, upload

VOXEL_TILE = 2048        # keys per workgroup per radix pass of the voxel sort (csrc/voxel_plan.h); the tests size around it
VOXEL_SEG_BLOCK = 256    # threads per workgroup of the kernel that sums a voxel's points (one wave per voxel)


def enqueue(lib, cl, voxel_size, counts, extra_bytes=0):
    """`cslam_voxel_downsample_dev` on uploaded clouds.  Every result lies in the one result buffer of `_batch`, with
    `extra_bytes` of the caller's own behind it at layout["end"]: returns (buffer, layout)."""
    n, total = len(cl.off) - 1, int(cl.off[-1])
    t_out, lay = result_buffer(n, total, 8, cl.buf.device, colors=False, counts=counts, extra_bytes=extra_bytes)
    p_rows, _, p_counts, p_out_off, p_status = result_args(t_out, lay, colors=False, counts=counts)
    _lib.check(lib.cslam_voxel_downsample_dev(cl.rows if total else None, cl.d_off, n, float(voxel_size), p_rows, p_out_off, p_counts,
                                              p_status, host(cl.off), stream()))
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


def raise_failed(res, failed):
    """`res` as it is, or VoxelSizeError with None in the places of the `failed` clouds."""
    if failed:
        raise VoxelSizeError(failed, [None if c in failed else r for c, r in enumerate(res)])
    return res


def unpack(host_bytes, lay, n, counts):
    """Split the downloaded result buffer into per-cloud arrays; raises VoxelSizeError for a status of 1."""
    res, failed = unpack_result(host_bytes, lay, n, np.float64, colors=False, counts=counts)
    return raise_failed([(pts, cnt) if counts else pts for pts, _, cnt in res], failed)


def downsample_clouds(clouds, voxel_size, counts=False, device=0):
    """Voxel down-sampling of a list of clouds in ONE call (one upload, one download): per cloud the [m, 3] float64
    means of the occupied voxels, in ascending lexicographic voxel index; with `counts` a pair (means, points per
    voxel).  The rule is open3d's `voxel_down_sample` after the reference's filter of non-finite rows
    (icp_utils.py:93-100); the filter too runs on the GPU.  A cloud without a finite row gives [0, 3].
    Raises `VoxelSizeError` (a ValueError) naming the clouds whose index range is beyond 2^21 per axis."""
    with gpu(device) as (lib, dev):
        clouds = [rows(c) for c in clouds]
        if not clouds:
            return []
        cl = upload(clouds, dev)
        t_out, lay = enqueue(lib, cl, voxel_size, counts)
        host_bytes = t_out.cpu().numpy()
    return unpack(host_bytes, lay, len(clouds), counts)


def downsample(points, voxel_size, device=0):
    """Counterpart of the reference's `downsample` (icp_utils.py:93-100): the down-sampled cloud as an [m, 3] float64
    array (every function of this package takes arrays or `.points`)."""
    return downsample_clouds([points], voxel_size, device=device)[0]
