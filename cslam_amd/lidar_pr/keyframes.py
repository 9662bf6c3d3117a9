#!/usr/bin/env python
"""Lidar keyframes on an MI355X: one upload per keyframe for both things the handler keeps of it.

The reference's handler computes the ScanContext descriptor of a keyframe's cloud (lidar_pr/scancontext.py:14-16) and
stores the voxel down-sampled cloud for the registration (lidar_handler_node.py:180,
`icp_utils.downsample_ros_pointcloud(cloud, frontend.voxel_size)`).  `ingest` uploads a batch of raw clouds once and
runs both on that device buffer: `cslam_scancontext_from_cloud_dev` and `cslam_voxel_downsample_dev`; the results come
back in one copy.  There is no CPU path: without the library or a GPU `CslamHipError` is raised.
"""
import numpy as np

from . import scancontext, voxel
from ._batch import gpu, rows, upload

RINGS, SECTORS, MAX_LENGTH = 20, 60, 80       # as ScanContext (the ScanContext paper's shape)


def ingest(clouds, voxel_size, device=0):
    """(descriptors, downsampled) of a list of raw clouds ([n, >=3] arrays or objects with `.points`).

    descriptors: [len(clouds), RINGS * SECTORS] float64, the rows `ScanContext.compute_embeddings` gives for the same
    clouds; a point at exactly 360 degrees raises the same IndexError, an infinite x or y the same ValueError.
    downsampled: the list `icp_utils.downsample_clouds(clouds, voxel_size)` gives (`VoxelSizeError` likewise)."""
    with gpu(device) as (lib, dev):
        clouds = [rows(c) for c in clouds]
        n = len(clouds)
        if n == 0:
            return np.zeros((0, RINGS * SECTORS)), []
        desc_bytes = 8 * n * RINGS * SECTORS
        cl = upload(clouds, dev)
        t_out, lay = voxel.enqueue(lib, cl, voxel_size, False, extra_bytes=desc_bytes + 256)
        base = t_out.data_ptr() + lay["end"]
        scancontext.enqueue(lib, cl.rows, cl.d_off, n, RINGS, SECTORS, MAX_LENGTH, base, base + desc_bytes)
        host = t_out.cpu().numpy()
    at = lay["end"]
    err = scancontext.status_error(int(host[at + desc_bytes:at + desc_bytes + 4].view(np.int32)[0]), SECTORS)
    if err is not None:
        raise err
    desc = host[at:at + desc_bytes].view(np.float64).reshape(n, RINGS * SECTORS).copy()
    return desc, voxel.unpack(host, lay, n, False)
