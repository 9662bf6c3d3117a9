"""Float64 restatement of the Winograd transforms of csrc/winograd.hip, csrc/wino_gemm.hip and csrc/wino_chain.hip (numpy, no GPU,
nothing imported from cslam_amd): the matrices written out, the input and output transforms with the magnitudes |B^T| |d| |B| and
|A^T| |M| |A| their rounding-error bars are stated in, the column fold of the Z form, the power-of-two scale rule of csrc/pairs.h and
the fp16 pair layouts.  tests/test_wino_reference_cpu.py checks this file against a float64 convolution before
tests/test_wino_transforms_gpu.py checks the kernels against it."""
import numpy as np

# F(4x4, 3x3): wino4_bt, wino4_at and the G of the weight packer
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], dtype=np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
G4 = np.array([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=np.float64) / 24.0
# F(2x2, 3x3): wino_input_kernel, wino_output_kernel
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
G2 = np.array([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], dtype=np.float64) / 2.0

U32 = 2.0 ** -24          # unit roundoff of float32


def matrices(tile):
    """(B^T [n, n], A^T [tile, n], G [n, 3]) of F(tile x tile, 3x3), n = tile + 2."""
    return (BT2, AT2, G2) if tile == 2 else (BT4, AT4, G4)


def tiles_of(H, W, tile):
    return -(-H // tile), -(-W // tile)


def input_transform(x_nhwc, tile):
    """x [B, H, W, C] -> (V, mag), both [n*n, T, C] float64: V[n i + j] = (B^T d B)[i][j] of the (tile+2)^2 window d of every tile
    (tile order (b, ti, tj), one pixel of padding, zero outside the map) and mag = |B^T| |d| |B|."""
    x = np.asarray(x_nhwc, dtype=np.float64)
    Bt = matrices(tile)[0]
    n = tile + 2
    B, H, W, C = x.shape
    TH, TW = tiles_of(H, W, tile)
    xp = np.zeros((B, TH * tile + 2, TW * tile + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.empty((B, TH, TW, n, n, C))
    for i in range(n):
        for j in range(n):
            d[:, :, :, i, j] = xp[:, i:i + TH * tile:tile, j:j + TW * tile:tile]
    V = np.einsum("pi,btuijc,qj->pqbtuc", Bt, d, Bt)
    mag = np.einsum("pi,btuijc,qj->pqbtuc", np.abs(Bt), np.abs(d), np.abs(Bt))
    return V.reshape(n * n, B * TH * TW, C), mag.reshape(n * n, B * TH * TW, C)


def z_fold(M):
    """M [36, T, C] -> Z [24, T, C], Z[4 i + q] = sum_j A^T[q][j] M[6 i + j]: the column half of the F(4x4) output transform."""
    M = np.asarray(M, dtype=np.float64)
    _, T, C = M.shape
    return np.einsum("qj,ijtc->iqtc", AT4, M.reshape(6, 6, T, C)).reshape(24, T, C)


def _pool(a):
    B, H, W, C = a.shape
    return a[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def output_transform(M, bias, res, B, H, W, tile, inv, relu, pool, folded=False):
    """M [n*n, T, C] (folded: the Z of `z_fold`, [24, T, C], tile 4) -> (y, mag, ymax):
    y = A^T M A inv + bias (+ res) (ReLU) (MaxPool2d(2, 2), flooring) in NHWC, cropped to the map;
    mag = |A^T| |M| |A| inv + |bias| + |res|, of a pooled output the largest of its window (max is 1-Lipschitz);
    ymax = the largest |y| inside the map before pooling."""
    M = np.asarray(M, dtype=np.float64)
    At = matrices(tile)[1]
    n = tile + 2
    _, T, C = M.shape
    TH, TW = tiles_of(H, W, tile)
    assert T == B * TH * TW
    if folded:
        m = M.reshape(n, tile, B, TH, TW, C)
        y = np.einsum("pi,iqbtuc->btpuqc", At, m)
        mag = np.einsum("pi,iqbtuc->btpuqc", np.abs(At), np.abs(m))
    else:
        m = M.reshape(n, n, B, TH, TW, C)
        y = np.einsum("pi,ijbtuc,qj->btpuqc", At, m, At)
        mag = np.einsum("pi,ijbtuc,qj->btpuqc", np.abs(At), np.abs(m), np.abs(At))
    y = y.reshape(B, TH * tile, TW * tile, C)[:, :H, :W] * inv
    mag = mag.reshape(B, TH * tile, TW * tile, C)[:, :H, :W] * inv
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))
    if res is not None:
        y = y + np.asarray(res, dtype=np.float64)
        mag = mag + np.abs(np.asarray(res, dtype=np.float64))
    if relu:
        y = np.maximum(y, 0.0)
    ymax = float(np.abs(y).max())
    if pool:
        y, mag = _pool(y), _pool(mag)
    return y, mag, ymax


def scale_le_327_68(amax):
    """csrc/pairs.h::scale_le_327_68 in float32 arithmetic: 2^floor(log2(327.68f / a)), a = amax clamped to [1e-30, 1e30]."""
    a = np.minimum(np.maximum(np.float32(amax), np.float32(1e-30)), np.float32(1e30))
    r = np.float32(327.68) / a
    assert r.dtype == np.float32
    _, e = np.frexp(r)                       # r = m 2^e, m in [0.5, 1)
    return float(np.ldexp(1.0, int(e) - 1))


def pair_layout(V2_halves, T, C):
    """fp16 [36][T][C/32][2][32] (any shape with that element order) -> (hi, lo), both [36, T, C] float64."""
    v = np.asarray(V2_halves).reshape(36, T, C // 32, 2, 32).astype(np.float64)
    return v[:, :, :, 0].reshape(36, T, C), v[:, :, :, 1].reshape(36, T, C)


def h3_layout(V3_halves, T, C):
    """fp16 [36][T][3 C] = hi | lo | hi -> (hi, lo, hi again), each [36, T, C] float16 (the caller compares the two hi blocks' bits)."""
    v = np.asarray(V3_halves).reshape(36, T, 3, C)
    return v[:, :, 0], v[:, :, 1], v[:, :, 2]


def ulp_fp16(h):
    """Spacing of fp16 at |h| (2^-24 in the subnormal range and at zero)."""
    a = np.abs(np.asarray(h, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)
