"""The merged map of a swarm, on the GPU (csrc/cloud.hip behind `cslam_map_assemble_dev`): every keyframe cloud placed at
its optimised pose and the whole merged in one voxel grid.

The reference has no such function: its visualiser shows every cloud of `send_visualization_pointcloud`
(src/front_end/rgbd_handler.cpp:665-682) at the pose `optimized_estimates_callback` last gave its keyframe.  Every
optimisation moves all poses, so the map is rebuilt from all keyframes each time.  There is nothing of PCL's to be equal
to here, and the keyframe filter's parity with PCL is unpinned (front_end/keyframe_clouds.py); the rule is the one
include/cslam_hip.h states and tests/cloud_reference.py restates, bit for bit, all in float64:

    pw[r] = ((T[r,0] * x + T[r,1] * y) + T[r,2] * z) + T[r,3]          with T = pose @ sensor_to_body
    cell  = floor(pw / voxel_size), a grid anchored at the world origin: a map does not shift when a keyframe is added
            (this is not the origin rule of lidar_pr.voxel)
    rows in ascending (iz, iy, ix); a row = the sum of its points in input order (keys sorted, then row order), divided
    once by their number; colours = integer sums per channel, truncating division

There is no CPU path: without the library or a GPU `assemble_map` raises CslamHipError.  `write_ply` is host only.
"""
import collections

import numpy as np

from .. import _lib
from ..front_end.keyframe_clouds import pack_colors, unpack_result
from ..lidar_pr._batch import gpu, host, offsets, result_args, result_buffer, stream, to_dev
from ..lidar_pr.voxel import VoxelSizeError
from .pose_graph import as_pose

SwarmMap = collections.namedtuple("SwarmMap", "points colors counts")


def _rows(cloud):
    """(xyz float32 or float64 [n, 3], colors uint8 [n, 3] or None) of a KeyframeCloud or an [n, 3] array."""
    colors = getattr(cloud, "colors", None)
    p = np.asarray(cloud.points if hasattr(cloud, "points") else cloud)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("a cloud is an [n, 3] array or a KeyframeCloud, got shape %s" % (p.shape,))
    if p.dtype != np.float32:
        p = p.astype(np.float64)
    if colors is not None:
        colors = np.asarray(colors)
        if colors.dtype != np.uint8 or colors.shape != p.shape:
            raise ValueError("colours are uint8 [n, 3] (r, g, b), one row per point")
    return np.ascontiguousarray(p), colors


def assemble_map(clouds, poses, voxel_size, sensor_to_body=None, device=0):
    """`SwarmMap(points float64 [m, 3], colors uint8 [m, 3] or None, counts int64 [m])` of `clouds` = {key: KeyframeCloud or
    [n, 3] array} at `poses` = {key: pose} (4 x 4 or 7 numbers, as `PoseGraphResult.poses` gives them), in ONE call.

    Keys are taken in sorted order.  A cloud without a pose raises KeyError, a non-finite pose ValueError.
    `sensor_to_body`: one optional 4 x 4 transform of the sensor in the body frame, composed on the host as
    pose @ sensor_to_body.  Colours are kept only when every cloud has them (lidar keyframes have none: `colors` is None).
    If any cloud is float64 all are taken as float64.  Rows with a non-finite coordinate do not exist for the map.
    `counts` are numbers of INPUT ROWS per map voxel: the keyframe clouds' own counts are not used as weights, so a
    keyframe voxel that averaged 16 pixels weighs as much as one that held a single pixel.
    Raises `VoxelSizeError` when the map spans 2^21 voxels or more on some axis."""
    v = float(voxel_size)
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError("voxel_size must be positive and finite")
    ext = None if sensor_to_body is None else as_pose(sensor_to_body)
    keys = sorted(clouds)
    rows, Ts = [], []
    for k in keys:
        T = as_pose(poses[k])                              # KeyError: a cloud without a pose
        T = T if ext is None else T @ ext
        if not np.all(np.isfinite(T)):
            raise ValueError("the pose of keyframe %s is not finite" % (k,))
        rows.append(_rows(clouds[k]))
        Ts.append(T)
    colors = bool(rows) and all(c is not None for _, c in rows)
    dtype = np.float32 if rows and all(p.dtype == np.float32 for p, _ in rows) else np.float64
    with gpu(device) as (lib, dev):
        if not rows:
            return SwarmMap(np.zeros((0, 3)), None, np.zeros(0, dtype=np.int64))
        off = offsets([len(p) for p, _ in rows])
        n, total = len(rows), int(off[-1])
        t_pts = to_dev(np.concatenate([p.astype(dtype, copy=False) for p, _ in rows], axis=0), dev)
        t_rgb = to_dev(np.concatenate([pack_colors(c) for _, c in rows]).view(np.int32), dev) if colors else None
        t_off, t_T = to_dev(off, dev), to_dev(np.stack(Ts).reshape(n, 16), dev)
        t_out, lay = result_buffer(1, total, 8, dev)
        _lib.check(lib.cslam_map_assemble_dev(t_pts.data_ptr(), _lib.F32 if dtype == np.float32 else _lib.F64,
                                              t_rgb.data_ptr() if colors else None, t_off.data_ptr(), t_T.data_ptr(), n, v,
                                              *result_args(t_out, lay, colors), host(off), stream()))
        host_bytes = t_out.cpu().numpy()
    res, failed = unpack_result(host_bytes, lay, 1, np.float64, colors)
    if failed:
        raise VoxelSizeError(failed, [None])
    return SwarmMap(*res[0])


def write_ply(path, swarm_map):
    """Binary little-endian PLY of a `SwarmMap` (or a KeyframeCloud): x y z as float64 or float32, then red green blue as
    uchar when the map has colours.  Host only."""
    pts = np.asarray(swarm_map.points)
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float64)
    name = "double" if pts.dtype == np.float64 else "float"
    fields = [("x", "<" + pts.dtype.str[1:]), ("y", "<" + pts.dtype.str[1:]), ("z", "<" + pts.dtype.str[1:])]
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(pts)] + ["property %s %s" % (name, a) for a in "xyz"]
    if swarm_map.colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar %s" % c for c in ("red", "green", "blue")]
    rec = np.zeros(len(pts), dtype=fields)
    for a, name_a in enumerate("xyz"):
        rec[name_a] = pts[:, a]
    if swarm_map.colors is not None:
        for a, name_a in enumerate(("red", "green", "blue")):
            rec[name_a] = np.asarray(swarm_map.colors)[:, a]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())
