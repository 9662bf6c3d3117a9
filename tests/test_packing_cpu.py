"""CPU suite: the host-side operand packers of the HIP kernels (pure tensor arithmetic, no GPU): the exact fp16 hi / lo pair
split and the memory orders the kernels read -- checked by re-assembling the original float32 values from the packed form."""
import numpy as np
import torch

from cslam_amd.vpr import heads
from cslam_amd.vpr import winograd as wg


def _halves(dwords):
    """int32 tensor of packed dwords -> (low half, high half) as float16 tensors"""
    u = dwords.to(torch.int64) & 0xFFFFFFFF
    lo = torch.from_numpy((u.numpy() & 0xFFFF).astype(np.uint16).view(np.float16))
    hi = torch.from_numpy(((u.numpy() >> 16) & 0xFFFF).astype(np.uint16).view(np.float16))
    return lo, hi


def test_pca_pair_weights_reassemble_to_22_bits_in_the_gemm_row_order():
    torch.manual_seed(0)
    w = torch.randn(256, 2048) / 45.0
    pairs, inv_sw = heads.pca_pair_weights(w, splits=4)
    assert pairs.shape == (4, 256, 16, 2, 32) and pairs.dtype == torch.float16
    rec = (pairs[:, :, :, 0, :].double() + pairs[:, :, :, 1, :].double()) * inv_sw          # [S, Dout, kb, 32]
    rec = rec.permute(1, 0, 2, 3).reshape(256, 2048)
    assert float((rec - w.double()).abs().max()) <= 2.0 ** -21 * float(w.abs().max())
    assert float(pairs.abs().max()) < 2.0 ** 15 and float(pairs[:, :, :, 0, :].abs().max()) >= 2.0 ** 13
    assert heads.pca_pair_weights(torch.randn(100, 2048)) is None and heads.pca_pair_weights(torch.randn(128, 1000)) is None


def test_stem_pair_weights_slots_taps_and_bound():
    torch.manual_seed(1)
    w = torch.randn(64, 3, 3, 3) / 5.0
    W1, inv_sw, sumw = wg.stem_pair_weights(w)
    assert W1.shape == (4, 2, 64, 4) and W1.dtype == torch.int32 and sumw.shape == (64,)
    sw = 1.0 / inv_sw
    for hl in (0, 1):
        lo16, hi16 = _halves(W1[:, hl].reshape(-1))
        vals = torch.stack((lo16, hi16), dim=1).reshape(4, 64, 4, 2).reshape(4, 64, 8)       # [kq][16 g + n][slot j]
        if hl == 0:
            hi_part = vals.double()
        else:
            lo_part = vals.double()
    rec = (hi_part + lo_part) * inv_sw
    for kq in range(4):
        for g in range(4):
            for n in range(16):
                co = 16 * kq + n
                for j in range(8):
                    if g < 3:
                        want = float(w[co, j % 3, g, j // 3])          # tap (ky = g, kx = j // 3, ci = j % 3)
                    elif j < 3:
                        want = float(w[co, 2, j, 2])                   # the ninth tap (kx = 2, ci = 2) of row ky = j
                    else:
                        want = 0.0
                    assert abs(float(rec[kq, 16 * g + n, j]) - want) <= 2.0 ** -21 * float(w.abs().max())
    assert torch.all(sumw.double() >= w.double().abs().sum(dim=(1, 2, 3)))                    # rounded UP: a rigorous bound
    assert float(sw) == 2.0 ** round(np.log2(sw))


def test_register_resident_weight_fragments_are_in_mfma_lane_order():
    """`stem_direct_pair_weights` / `direct_r_pair_weights` (csrc/conv_stem_direct_h.hip, conv_direct_r.hip): every (wave, tap, K step
    [, channel tile], half) is one v_mfma_f32_16x16x32_f16 A fragment -- lane l holds output channel l % 16 of the tile, input channels
    8 (l // 16) .. + 7 of the K step --, hi + lo reproduce the power-of-two-scaled weight to 22 bits."""
    torch.manual_seed(5)
    w = torch.randn(64, 64, 3, 3) / 24.0
    W, inv = wg.stem_direct_pair_weights(w)
    assert W.shape == (4, 9, 2, 2, 64, 8) and W.dtype == torch.float16 and float(1.0 / inv) == 2.0 ** round(np.log2(1.0 / inv))
    rec = (W[:, :, :, 0].double() + W[:, :, :, 1].double()) * inv                              # [q][tap][ks][lane][e]
    want = w.double().reshape(4, 16, 2, 4, 8, 9).permute(0, 5, 2, 3, 1, 4).reshape(4, 9, 2, 64, 8)   # [q][i][ks][kg][e][tap] -> lane = 16 kg + i
    assert float((rec - want).abs().max()) <= 2.0 ** -21 * float(w.abs().max())
    assert float(W.abs().max()) < 2.0 ** 15 and float(W[:, :, :, 0].abs().max()) >= 2.0 ** 13
    w2 = torch.randn(128, 64, 3, 3) / 24.0
    W2, inv2 = wg.direct_r_pair_weights(w2)
    assert W2.shape == (4, 9, 2, 2, 2, 64, 8) and W2.dtype == torch.float16
    rec2 = (W2[:, :, :, :, 0].double() + W2[:, :, :, :, 1].double()) * inv2                    # [q][tap][ks][mt][lane][e]
    want2 = w2.double().reshape(4, 2, 16, 2, 4, 8, 9).permute(0, 6, 3, 1, 4, 2, 5).reshape(4, 9, 2, 2, 64, 8)
    assert float((rec2 - want2).abs().max()) <= 2.0 ** -21 * float(w2.abs().max())


def test_split16_pair_weights_layout():
    torch.manual_seed(2)
    U4 = torch.randn(36, 64, 128) / 8.0
    U2, inv_su = wg.split16_pair_weights(U4)
    assert U2.shape == (36, 128, 2, 2, 32)
    rec = (U2[:, :, :, 0, :].double() + U2[:, :, :, 1, :].double()) * inv_su                # [36, Cout, kb, 32]
    rec = rec.reshape(36, 128, 64).transpose(1, 2)
    assert float((rec - U4.double()).abs().max()) <= 2.0 ** -21 * float(U4.abs().max())


def test_normalised_image_bound_covers_every_8_bit_value():
    b = heads.normalised_image_bound()
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    worst = max(float(np.abs((v - np.float32(m)) / np.float32(s)).max()) for m, s in zip(heads.IMAGENET_DEFAULT_MEAN,
                                                                                         heads.IMAGENET_DEFAULT_STD))
    assert worst <= b <= worst * 1.001


def test_pair_split_scale_bracket_and_error():
    """`heads.pair_split`, the one host split behind every weight packer: s a power of two with s max|w| in [2^14, 2^15),
    |hi + lo - s w| <= 2^-21 s max|w|, s = 1 for an all-zero weight."""
    torch.manual_seed(6)
    for w in (torch.randn(64, 3, 3, 3, dtype=torch.float64) / 5.0, torch.randn(256, 2048) / 45.0,
              torch.randn(36, 64, 128, dtype=torch.float64) * 300.0, torch.full((4, 32), 2.0 ** -20)):
        hi, lo, inv_s = heads.pair_split(w)
        s = 1.0 / inv_s
        assert hi.dtype == torch.float16 and lo.dtype == torch.float16 and hi.shape == w.shape and lo.shape == w.shape
        assert s == 2.0 ** round(np.log2(s))
        sw = w.double() * s
        smax = float(sw.abs().max())
        assert 2.0 ** 14 <= smax < 2.0 ** 15
        assert float((hi.double() + lo.double() - sw).abs().max()) <= 2.0 ** -21 * smax
    hi, lo, inv_s = heads.pair_split(torch.zeros(8, 32, dtype=torch.float64))
    assert inv_s == 1.0 and not hi.any() and not lo.any()


def test_igemm_pair_weights_reassemble_in_k_block_order():
    """`igemm_pair_weights` (csrc/conv_igemm.hip): W2[co][kb][hi | lo][j].  Cin = 3 (the 7x7 stem): block kb = kernel row kh, slot
    j = kw * 3 + c, slots 3 KW .. 31 zero; Cin % 32 == 0: blocks in (kh, kw, Cin / 32) order, j = the channel inside the block."""
    torch.manual_seed(7)
    w = torch.randn(64, 3, 7, 7) / 12.0
    W2, inv = wg.igemm_pair_weights(w)
    assert W2.shape == (64, 7, 2, 32) and W2.dtype == torch.float16
    rec = (W2[:, :, 0].double() + W2[:, :, 1].double()) * inv                                  # [co][kh][j]
    want = torch.zeros(64, 7, 32, dtype=torch.float64)
    for kh in range(7):
        for kw in range(7):
            for c in range(3):
                want[:, kh, kw * 3 + c] = w[:, c, kh, kw].double()
    assert float((rec - want).abs().max()) <= 2.0 ** -21 * float(w.abs().max())
    assert not W2[:, :, :, 21:].any()
    w = torch.randn(128, 64, 3, 3) / 24.0
    W2, inv = wg.igemm_pair_weights(w)
    assert W2.shape == (128, 18, 2, 32) and W2.dtype == torch.float16
    rec = (W2[:, :, 0].double() + W2[:, :, 1].double()) * inv                                  # [co][kb][j]
    want = torch.zeros(128, 18, 32, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            for cb in range(2):
                want[:, (kh * 3 + kw) * 2 + cb, :] = w[:, 32 * cb:32 * cb + 32, kh, kw].double()
    assert float((rec - want).abs().max()) <= 2.0 ** -21 * float(w.abs().max())


def test_direct_pair_weights_reassemble_in_tap_row_order():
    """`direct_pair_weights` (csrc/conv_direct_h.hip): W2[ky * 3 + kx][co][kb][hi | lo][j] = the pair halves of w[co][32 kb + j][ky][kx]."""
    torch.manual_seed(8)
    w = torch.randn(128, 128, 3, 3) / 34.0
    W2, inv = wg.direct_pair_weights(w)
    assert W2.shape == (9, 128, 4, 2, 32) and W2.dtype == torch.float16
    rec = (W2[:, :, :, 0].double() + W2[:, :, :, 1].double()) * inv                           # [tap][co][kb][j]
    want = torch.stack([w[:, :, t // 3, t % 3].double() for t in range(9)]).reshape(9, 128, 4, 32)
    assert float((rec - want).abs().max()) <= 2.0 ** -21 * float(w.abs().max())


def test_direct_r2_pair_weights_are_in_mfma_lane_order():
    """`direct_r2_pair_weights` (csrc/conv_direct_r.hip, conv3x3_direct_r2_kernel): W2r2[half][q][tap][ks][slab][hi | lo][lane][e] =
    the pair halves of w[64 half + 16 q + lane % 16][64 slab + 32 ks + 8 (lane // 16) + e][tap // 3][tap % 3]."""
    torch.manual_seed(9)
    w = torch.randn(128, 128, 3, 3) / 34.0
    W, inv = wg.direct_r2_pair_weights(w)
    assert W.shape == (2, 4, 9, 2, 2, 2, 64, 8) and W.dtype == torch.float16
    rec = (W[:, :, :, :, :, 0].double() + W[:, :, :, :, :, 1].double()) * inv                 # [half][q][tap][ks][slab][lane][e]
    half, q, tap, ks, slab, lane, e = torch.meshgrid(*(torch.arange(n) for n in (2, 4, 9, 2, 2, 64, 8)), indexing="ij")
    want = w.double()[64 * half + 16 * q + lane % 16, 64 * slab + 32 * ks + 8 * (lane // 16) + e, tap // 3, tap % 3]
    assert float((rec - want).abs().max()) <= 2.0 ** -21 * float(w.abs().max())


def test_fused64_pair_weights_pack_hi_lo_dwords_in_fused64_lane_order():
    """`fused64_pair_weights` (csrc/wino_fused_h.hip): Uh[kq][xi][w][g][c][s] = [uh | ul << 16] of U[xi][16 kq + 4 g + s][16 w + c]."""
    torch.manual_seed(10)
    for cout in (64, 128):
        U4 = wg.wino_weights(torch.randn(cout, 64, 3, 3) / 24.0, 4)
        Uh, inv = wg.fused64_pair_weights(U4)
        assert Uh.shape == (4, 36, cout // 16, 4, 16, 4) and Uh.dtype == torch.int32
        lo16, hi16 = _halves(Uh.reshape(-1))                                               # low half: uh, high half: ul
        rec = ((lo16.double() + hi16.double()) * inv).reshape(Uh.shape)
        kq, xi, w_, g, c, s = torch.meshgrid(*(torch.arange(n) for n in Uh.shape), indexing="ij")
        want = U4.double()[xi, 16 * kq + 4 * g + s, 16 * w_ + c]
        assert float((rec - want).abs().max()) <= 2.0 ** -21 * float(U4.abs().max())


def test_split16_weights_stack_hi_hi_lo():
    """`split16_weights` (csrc/winograd.hip, the split-fp16 GEMM): U3[xi] = [uh ; uh ; ul] along K, uh + ul = sU U to 22 bits."""
    torch.manual_seed(11)
    U4 = torch.randn(36, 64, 128) / 8.0
    U3, inv_su = wg.split16_weights(U4)
    assert U3.shape == (36, 192, 128) and U3.dtype == torch.float16
    assert torch.equal(U3[:, :64], U3[:, 64:128])
    rec = (U3[:, :64].double() + U3[:, 128:].double()) * inv_su
    assert float((rec - U4.double()).abs().max()) <= 2.0 ** -21 * float(U4.abs().max())


def test_winograd_namespace_keeps_every_name_bench_tests_and_tools_take_from_it():
    """The packers live in vpr/pair_weights.py and the kernel wrappers in vpr/conv_kernels.py; bench.py, tests/ and tools/ reach all of
    them, and the switches, through `cslam_amd.vpr.winograd` (`wg.X`, `wgm.X`, `winograd.X`, `from cslam_amd.vpr.winograd import X`):
    every such name stays an attribute of that module."""
    names = ("CHAIN_TILE_COLS", "DIRECT_P", "FP32_GEMM_FORMS", "PairAct", "TRUNK_FORMS", "VGG_PAIRS", "WinogradResNet", "WinogradTrunk",
             "Z_FORM_MAX", "_Workspace", "conv3x3_direct_h", "conv3x3_direct_hp", "conv3x3_direct_p", "conv3x3_direct_r",
             "conv3x3_direct_r2", "conv3x3_direct_r_pairs", "conv_igemm", "conv_igemm_p", "conv_stem_direct_h", "direct_p_fits",
             "direct_pair_weights", "direct_r2_pair_weights", "direct_r_pair_weights", "fused64_pair_weights", "fused64_weights",
             "igemm_pair_weights", "pairs_to_float", "split16_pair_weights", "split16_weights", "stem_direct_pair_weights",
             "stem_pair_weights", "stem_pool_fits", "use_tuned_gemms", "wino_conv3x3", "wino_fused64", "wino_fused64_h", "wino_stem64_h",
             "wino_weights")
    # the switches the runners read at call time, which callers therefore set on this module, and the rest of its public surface
    names += ("PAIR_ACTS", "IGEMM_CONVS", "fold_bn", "out_bound")
    missing = [n for n in names if not hasattr(wg, n)]
    assert not missing, missing
    from cslam_amd.vpr import conv_kernels, pair_weights
    for n in ("VGG_PAIRS", "Z_FORM_MAX", "PAIR_ACTS", "DIRECT_P", "IGEMM_CONVS", "TRUNK_FORMS", "CHAIN_TILE_COLS", "FP32_GEMM_FORMS"):
        assert not hasattr(conv_kernels, n) and not hasattr(pair_weights, n), n     # one copy of every switch: the one callers set
