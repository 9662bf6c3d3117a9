"""Batched voxel down-sampling of keyframe clouds (csrc/voxel.hip behind `cslam_voxel_downsample_dev`): the counterpart of
the reference's `downsample` (icp_utils.py:93-100, open3d's `voxel_down_sample`).  `enqueue` and `unpack` are the two
halves `keyframes.ingest` shares with `downsample_clouds`."""
import numpy as np

from .. import _lib
from ._batch import gpu, host, offsets, round256, rows, stream, upload

VOXEL_TILE = 2048        # keys per workgroup per radix pass of the voxel sort (csrc/voxel_plan.h); the tests size around it
VOXEL_SEG_BLOCK = 256    # threads per workgroup of the kernel that sums a voxel's points (one wave per voxel)


def enqueue(lib, cl, voxel_size, counts, extra_bytes=0):
    """`cslam_voxel_downsample_dev` on uploaded clouds.  Every result lies in ONE device byte buffer, so that it comes
    back in one copy: returns (buffer, layout) with layout = byte offsets of out_offsets, status, rows, counts, extra."""
    import torch
    n, total = len(cl.off) - 1, int(cl.off[-1])
    sizes = [round256(b) for b in (8 * (n + 1), 4 * n, 24 * total, 4 * total if counts else 0)]
    lay = dict(zip(("out_off", "status", "rows", "counts", "extra"), (int(o) for o in offsets(sizes))))
    t_out = torch.zeros(lay["extra"] + extra_bytes, dtype=torch.uint8, device=cl.buf.device)
    base = t_out.data_ptr()
    _lib.check(lib.cslam_voxel_downsample_dev(
        cl.rows if total else None, cl.d_off, n, float(voxel_size),
        base + lay["rows"] if total else None, base + lay["out_off"], base + lay["counts"] if counts and total else None,
        base + lay["status"], host(cl.off), stream()))
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


def unpack(host_bytes, lay, n, counts):
    """Split the downloaded result buffer into per-cloud arrays; raises VoxelSizeError for a status of 1."""
    out_off = host_bytes[lay["out_off"]:lay["out_off"] + 8 * (n + 1)].view(np.int64)
    status = host_bytes[lay["status"]:lay["status"] + 4 * n].view(np.int32)
    m = int(out_off[-1])
    means = host_bytes[lay["rows"]:lay["rows"] + 24 * m].view(np.float64).reshape(m, 3)
    cnt = host_bytes[lay["counts"]:lay["counts"] + 4 * m].view(np.int32) if counts else None
    res = []
    for c in range(n):
        a, b = int(out_off[c]), int(out_off[c + 1])
        pts = means[a:b].copy()
        res.append((pts, cnt[a:b].astype(np.int64)) if counts else pts)
    failed = [c for c in range(n) if status[c] != 0]
    if failed:
        raise VoxelSizeError(failed, [None if c in failed else r for c, r in enumerate(res)])
    return res


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
