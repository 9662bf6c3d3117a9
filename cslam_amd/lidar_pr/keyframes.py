#!/usr/bin/env python
"""Lidar keyframes on an MI355X: one upload per keyframe for both things the handler keeps of it.

The reference's handler computes the ScanContext descriptor of a keyframe's cloud (lidar_pr/scancontext.py:14-16) and
stores the voxel down-sampled cloud for the registration (lidar_handler_node.py:180,
`icp_utils.downsample_ros_pointcloud(cloud, frontend.voxel_size)`).  `ingest` uploads a batch of raw clouds once and
runs both on that device buffer: `cslam_scancontext_from_cloud_dev` and `cslam_voxel_downsample_dev`; the results come
back in one copy.  There is no CPU path: without the library or a GPU `CslamHipError` is raised.
"""
import numpy as np

from .. import _lib
from . import icp_utils
from .scancontext import theta_360_error

RINGS, SECTORS, MAX_LENGTH = 20, 60, 80       # as ScanContext (the ScanContext paper's shape)


def ingest(clouds, voxel_size, device=0):
    """(descriptors, downsampled) of a list of raw clouds ([n, >=3] arrays or objects with `.points`).

    descriptors: [len(clouds), RINGS * SECTORS] float64, the rows `ScanContext.compute_embeddings` gives for the same
    clouds; a point at exactly 360 degrees raises the same IndexError.
    downsampled: the list `icp_utils.downsample_clouds(clouds, voxel_size)` gives (`VoxelSizeError` likewise)."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    clouds = [icp_utils._rows(c) for c in clouds]
    n = len(clouds)
    if n == 0:
        return np.zeros((0, RINGS * SECTORS)), []
    dev = torch.device("cuda", device)
    desc_bytes = 8 * n * RINGS * SECTORS
    with torch.cuda.device(dev):
        t_in, off, head = icp_utils._upload_clouds(clouds, dev)
        t_out, lay = icp_utils._voxel_enqueue(lib, t_in, off, head, voxel_size, False, extra_bytes=desc_bytes + 256)
        base = t_out.data_ptr() + lay["extra"]
        _lib.check(lib.cslam_scancontext_from_cloud_dev(
            t_in.data_ptr() + head, t_in.data_ptr(), n, RINGS, SECTORS, float(MAX_LENGTH), base, base + desc_bytes,
            torch.cuda.current_stream().cuda_stream))
        host = t_out.cpu().numpy()
    at = lay["extra"]
    if int(host[at + desc_bytes:at + desc_bytes + 4].view(np.int32)[0]) != 0:
        raise theta_360_error(SECTORS)
    desc = host[at:at + desc_bytes].view(np.float64).reshape(n, RINGS * SECTORS).copy()
    return desc, icp_utils._voxel_unpack(host, lay, n, False)
