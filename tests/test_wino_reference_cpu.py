"""The float64 Winograd reference of tests/wino_reference.py, checked before any kernel is checked against it
(tests/test_wino_transforms_gpu.py): input transform, products with G g G^T and output transform give a float64 convolution; the
reference's G is the weight packer's; the Z fold composes to the full output transform; the scale rule steps where csrc/pairs.h's does."""
import numpy as np
import pytest

import wino_reference as wr

MAPS = [(5, 7), (1, 1), (4, 4), (9, 2)]


def _conv_case(H, W, seed):
    rng = np.random.default_rng(seed)
    B, cin, cout = 2, 3 + (H + W) % 2, 3 + H % 2
    x = rng.standard_normal((B, H, W, cin))
    w = rng.standard_normal((cout, cin, 3, 3))
    bias = rng.standard_normal(cout)
    return B, x, w, bias


@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("H,W", MAPS)
def test_transforms_around_the_products_give_the_float64_convolution(tile, H, W):
    """A^T [(G g G^T) . (B^T d B)] A + bias == conv2d(x, g, padding 1) + bias to 1e-12 of the largest output, ragged maps included."""
    import torch
    B, x, w, bias = _conv_case(H, W, 10 * H + W + tile)
    _, _, G = wr.matrices(tile)
    n = tile + 2
    V, mag = wr.input_transform(x, tile)
    U = np.einsum("ik,ockl,jl->ijco", G, w, G).reshape(n * n, w.shape[1], w.shape[0])
    M = np.einsum("ftc,fco->fto", V, U)
    y, ymag, ymax = wr.output_transform(M, bias, None, B, H, W, tile, 1.0, False, False)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w), torch.from_numpy(bias), padding=1)
    ref = ref.permute(0, 2, 3, 1).numpy()
    assert y.shape == ref.shape == (B, H, W, w.shape[0])
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()
    assert ymax == np.abs(y).max()
    assert (np.abs(V) <= mag).all() and (np.abs(y) <= ymag + 1e-12).all()
    TH, TW = wr.tiles_of(H, W, tile)
    assert V.shape == (n * n, B * TH * TW, x.shape[3])


@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("H,W", MAPS)
def test_output_epilogue_is_bias_residual_relu_then_a_flooring_pool(tile, H, W):
    """The epilogue against torch in float64: + bias + residual, ReLU, MaxPool2d(2, 2) (odd sides floor; a 1 x 1 map pools to nothing),
    the descale `inv`, and the un-pooled maximum."""
    import torch
    rng = np.random.default_rng(H + 7 * W + tile)
    B, C = 2, 3
    TH, TW = wr.tiles_of(H, W, tile)
    n = tile + 2
    M = rng.standard_normal((n * n, B * TH * TW, C))
    bias, res = rng.standard_normal(C), rng.standard_normal((B, H, W, C))
    y0, mag0, _ = wr.output_transform(M, None, None, B, H, W, tile, 1.0, False, False)
    y, mag, ymax = wr.output_transform(M, bias, res, B, H, W, tile, 0.125, True, False)
    want = np.maximum(y0 * 0.125 + bias + res, 0.0)
    assert np.array_equal(y, want) and ymax == want.max()
    assert np.allclose(mag, mag0 * 0.125 + np.abs(bias) + np.abs(res), rtol=1e-15, atol=0)
    yp, magp, ymaxp = wr.output_transform(M, bias, None, B, H, W, tile, 0.125, True, True)
    full = np.maximum(y0 * 0.125 + bias, 0.0)
    pooled = torch.nn.functional.max_pool2d(torch.from_numpy(full).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy() if min(H, W) >= 2 \
        else np.zeros((B, H // 2, W // 2, C))
    assert yp.shape == (B, H // 2, W // 2, C) == magp.shape
    assert np.array_equal(yp, pooled) and ymaxp == full.max()


@pytest.mark.parametrize("tile", [2, 4])
def test_reference_g_is_the_weight_packers(tile):
    """wino_weights(w, tile) (float32, computed in float64) equals the reference's G g G^T to 2^-24 relative."""
    import torch
    from cslam_amd.vpr.pair_weights import wino_weights
    rng = np.random.default_rng(tile)
    w = rng.standard_normal((5, 4, 3, 3))
    G = wr.matrices(tile)[2]
    n = tile + 2
    want = np.einsum("ik,ockl,jl->ijco", G, w, G).reshape(n * n, 4, 5)
    got = wino_weights(torch.from_numpy(w), tile).numpy().astype(np.float64)
    assert got.shape == want.shape
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want)).all()


@pytest.mark.parametrize("H,W", MAPS)
def test_z_fold_then_the_row_half_is_the_full_output_transform(H, W):
    rng = np.random.default_rng(H * W)
    B, C = 2, 4
    TH, TW = wr.tiles_of(H, W, 4)
    M = rng.standard_normal((36, B * TH * TW, C))
    bias = rng.standard_normal(C)
    Z = wr.z_fold(M)
    assert Z.shape == (24, B * TH * TW, C)
    for pool in (False, True):
        y, mag, ymax = wr.output_transform(M, bias, None, B, H, W, 4, 0.5, True, pool)
        yz, magz, ymaxz = wr.output_transform(Z, bias, None, B, H, W, 4, 0.5, True, pool, folded=True)
        scale = max(np.abs(y).max(), 1.0) if y.size else 1.0
        assert y.shape == yz.shape and (y.size == 0 or np.abs(y - yz).max() <= 1e-13 * scale)
        assert abs(ymax - ymaxz) <= 1e-13 * max(ymax, 1.0)
        assert (magz <= mag * (1 + 1e-13)).all()          # |A^T| |Z| <= |A^T| |M| |A|


def test_scale_rule_steps_exactly_at_327_68_over_a_power_of_two():
    c = np.float32(327.68)
    for k in (-6, -1, 0, 3, 10, 40):
        a = np.float32(np.ldexp(c, -k))                              # exact: a power-of-two multiple of a float32
        assert wr.scale_le_327_68(a) == 2.0 ** k and float(a) * wr.scale_le_327_68(a) == float(c)
        above = np.nextafter(a, np.float32(np.inf), dtype=np.float32)
        assert wr.scale_le_327_68(above) == 2.0 ** (k - 1)
        below = np.nextafter(a, np.float32(0), dtype=np.float32)
        assert wr.scale_le_327_68(below) == 2.0 ** k
    for a in (0.0, 1e-30, 1e30, 3e38):
        s = wr.scale_le_327_68(a)
        assert np.isfinite(s) and s > 0 and np.float32(s) == s
    assert wr.scale_le_327_68(0.0) == wr.scale_le_327_68(1e-30) and wr.scale_le_327_68(3e38) == wr.scale_le_327_68(1e30)


def test_pair_layouts_put_every_half_where_the_kernels_do():
    T, C = 3, 64
    idx = np.arange(36 * T * C).reshape(36, T, C)
    v2 = np.empty((36, T, C // 32, 2, 32), dtype=np.float16)
    hi_src, lo_src = (idx % 1024).astype(np.float16), (-(idx % 512)).astype(np.float16)
    v2[:, :, :, 0] = hi_src.reshape(36, T, C // 32, 32)
    v2[:, :, :, 1] = lo_src.reshape(36, T, C // 32, 32)
    hi, lo = wr.pair_layout(v2.ravel(), T, C)
    assert np.array_equal(hi, hi_src.astype(np.float64)) and np.array_equal(lo, lo_src.astype(np.float64))
    v3 = np.concatenate((hi_src, lo_src, hi_src), axis=2)
    h, l, h2 = wr.h3_layout(v3.ravel(), T, C)
    assert np.array_equal(h, hi_src) and np.array_equal(l, lo_src) and np.array_equal(h2, hi_src)
    assert np.array_equal(wr.ulp_fp16(np.array([0.0, 2.0 ** -20, 1.0, 1.5, 2.0, 1000.0])),
                          np.array([2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5]))
