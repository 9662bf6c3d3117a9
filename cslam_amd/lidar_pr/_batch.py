"""How a list of arrays becomes device memory with offsets, and how a lidar call reaches the GPU: shared by voxel.py, fpfh.py,
robust.py, icp.py, icp_utils.py and keyframes.py.  Nothing else in lidar_pr builds offsets or packs an upload."""
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
