"""How a list of arrays becomes device memory with offsets, and how a lidar call reaches the GPU: shared by voxel.py, fpfh.py,
robust.py, icp.py, icp_utils.py and keyframes.py.  Nothing else in lidar_pr builds offsets or packs an upload.  Also the one
result buffer of the voxel filters, which front_end/keyframe_clouds.py, front_end/stereo_depth.py and back_end/swarm_map.py
use as voxel.py does."""
import collections
import contextlib
import ctypes as C

import numpy as np

from .. import _lib


@contextlib.contextmanager
def gpu(device):
    """Require a GPU, load the library and enter the device: `with gpu(device) as (lib, dev):`.  Without a GPU or the library
    this raises `CslamHipError`; a public function checks its Python arguments before it and returns for an empty list
    inside it."""
    _lib.require_gpu()
    lib = _lib.load()
    import torch
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        yield lib, dev


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def host(arr):
    return arr.ctypes.data_as(C.c_void_p)


def rows(cloud, finite=False):
    """[n, 3] float64 rows of a cloud ([n, >=3] array or anything with `.points`).  With `finite` the rows with a non-finite
    coordinate are dropped, as the reference's `downsample` does; the voxel kernels leave them out themselves."""
    pts = np.asarray(cloud.points if hasattr(cloud, "points") else cloud)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("a cloud is an [n, >=3] array, got shape %s" % (pts.shape,))
    pts = np.ascontiguousarray(pts[:, :3], dtype=np.float64)
    return pts[np.isfinite(pts).all(axis=1)] if finite else pts


def offsets(lengths):
    """int64 [n + 1]: where each of n arrays of these lengths starts in their concatenation, and its end."""
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    return off


def split(rows, off):
    return [rows[int(off[c]):int(off[c + 1])].copy() for c in range(len(off) - 1)]


def round256(n):
    return (n + 255) // 256 * 256


def to_dev(arr, dev):
    """Upload one array; an empty one as a single zero, so that its device pointer is never NULL."""
    import torch
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(dev)


# ---- what a voxel filter call returns (lidar down-sampling, keyframe clouds, the swarm map): ONE device byte buffer, so that
# everything comes back in one copy -------------------------------------------------------------------------------------
def result_buffer(n, total, xyz_bytes, dev, colors=True, counts=True, extra_bytes=0):
    """The buffer for `n` clouds of `total` input rows in all, with coordinates of `xyz_bytes` each: (tensor, layout), the
    layout being the byte offsets of out_off, status, rows, rgb, counts and end.  A piece that is not wanted takes no room;
    `extra_bytes` more follow at `end` for the caller's own use."""
    import torch
    sizes = [round256(s) for s in (8 * (n + 1), 4 * n, xyz_bytes * 3 * total, 4 * total if colors else 0, 4 * total if counts else 0)]
    lay = dict(zip(("out_off", "status", "rows", "rgb", "counts", "end"), (int(o) for o in offsets(sizes))))
    return torch.zeros(max(lay["end"] + extra_bytes, 256), dtype=torch.uint8, device=dev), lay


def result_args(t_out, lay, colors=True, counts=True):
    """Device pointers into the buffer, in the order the entry points take them: rows, rgb, counts, out_offsets, status."""
    p = t_out.data_ptr()
    return p + lay["rows"], p + lay["rgb"] if colors else None, p + lay["counts"] if counts else None, p + lay["out_off"], p + lay["status"]


def unpack_result(host_bytes, lay, n, dtype, colors=True, counts=True):
    """The downloaded buffer as (rows [m, 3] of `dtype`, packed colours uint32 [m] or None, counts int64 [m] or None) per
    cloud, and the numbers of the clouds with status 1."""
    out_off = host_bytes[lay["out_off"]:lay["out_off"] + 8 * (n + 1)].view(np.int64)
    status = host_bytes[lay["status"]:lay["status"] + 4 * n].view(np.int32)
    m, w = int(out_off[-1]), np.dtype(dtype).itemsize
    xyz = host_bytes[lay["rows"]:lay["rows"] + 3 * w * m].view(dtype).reshape(m, 3)
    rgb = host_bytes[lay["rgb"]:lay["rgb"] + 4 * m].view(np.uint32) if colors else None
    cnt = host_bytes[lay["counts"]:lay["counts"] + 4 * m].view(np.int32) if counts else None
    res = []
    for c in range(n):
        a, b = int(out_off[c]), int(out_off[c + 1])
        res.append((xyz[a:b].copy(), rgb[a:b].copy() if colors else None, cnt[a:b].astype(np.int64) if counts else None))
    return res, [c for c in range(n) if status[c] != 0]


# What an enqueue function takes of a batch: `rows` and `d_off` are device pointers (the float64 rows of all arrays, their
# int64 offsets), `off` the same offsets on the host, `buf` the tensor that owns the memory.
Packed = collections.namedtuple("Packed", "buf rows d_off off")


def upload(arrays, dev, pairs=False):
    """One host buffer, one copy: the int64 offsets, rounded up to 256 bytes, then the float64 rows of all arrays ([n_k, w]
    each, w = 3 for clouds).  Returns a `Packed`.  With `pairs` the arrays are n sources, then n targets, and the head also
    holds the targets' offsets re-based to 0: returns (all 2n, sources, targets), three views of the one buffer."""
    import torch
    off = offsets([len(a) for a in arrays])
    n = len(arrays) // 2
    ints = np.concatenate([off, off[n:] - off[n]]) if pairs else off
    total, head, width = int(off[-1]), round256(8 * len(ints)), arrays[0].shape[1] if arrays else 3
    buf = np.zeros(head + 8 * width * total, dtype=np.uint8)
    buf[:8 * len(ints)].view(np.int64)[:] = ints
    if total:
        np.concatenate(arrays, axis=0, out=buf[head:].view(np.float64).reshape(total, width))
    t = torch.from_numpy(buf).to(dev)
    both = Packed(t, t.data_ptr() + head, t.data_ptr(), off)
    if not pairs:
        return both
    return (both, Packed(t, both.rows, both.d_off, off[:n + 1]),
            Packed(t, both.rows + 8 * width * int(off[n]), both.d_off + 8 * len(off), ints[len(off):]))
