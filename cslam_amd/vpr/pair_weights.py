"""Host-side weight packers of the convolution kernels (pure torch, no device library): the Winograd transforms of a 3x3 weight and
the exact fp16 hi / lo pair layouts (`heads.pair_split`) every pair kernel of csrc/ reads, one packer per operand layout; `out_bound`
for the output bound the pair-format epilogues scale by.  `vpr/conv_kernels.py` holds the kernels' wrappers, `vpr/winograd.py` the
trunk runners."""
import torch

from .heads import pair_split

_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
_G4 = torch.tensor([[1 / 4, 0.0, 0.0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
                    [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0.0, 0.0, 1.0]], dtype=torch.float64)


def wino_weights(weight, tile=2):
    """[Cout, Cin, 3, 3] -> U [n*n, Cin, Cout] float32, U[n*i+j] = (G g G^T)[i][j] (computed in float64);
    n = 4 for F(2x2,3x3) (tile=2), 6 for F(4x4,3x3) (tile=4)."""
    G = _G if tile == 2 else _G4
    g = weight.detach().to(torch.float64).cpu()
    u = torch.einsum("ik,ockl,jl->ijco", G, g, G)              # [n,n,Cin,Cout]
    return u.reshape(G.shape[0] ** 2, g.shape[1], g.shape[0]).to(torch.float32).contiguous()


def split16_weights(U4):
    """U4 [36, Cin, Cout] float32 -> (U3 [36, 3 Cin, Cout] float16 = [uh ; uh ; ul], inv_su): the weight operand of the
    split-fp16 GEMM (csrc/winograd.hip, `wino4_input_h3_kernel`): sU U = uh + ul exactly to 22 bits, sU the power of two
    that brings max |U| into [2^14, 2^15); inv_su = 1 / sU."""
    u = U4.detach().to(torch.float64)
    uh, ul, inv_su = pair_split(u)
    return torch.cat((uh, uh, ul), dim=1).contiguous(), inv_su


def split16_pair_weights(U4):
    """U4 [36, Cin, Cout] float32 -> (U2 [36, Cout, Cin/32, 2, 32] float16, inv_su): the weight operand of this library's
    split-fp16 GEMM (csrc/wino_gemm.hip): rows are OUTPUT channels, every 32-channel block of a row holds its hi halves
    then its lo halves; sU U = uh + ul exactly to 22 bits, sU the power of two that brings max |U| into [2^14, 2^15)."""
    n, cin, cout = U4.shape
    assert cin % 32 == 0
    u = U4.detach().to(torch.float64)
    uh, ul, inv_su = pair_split(u)
    pair = torch.stack((uh, ul), dim=0)                              # [2, 36, Cin, Cout]
    pair = pair.view(2, n, cin // 32, 32, cout).permute(1, 4, 2, 0, 3)   # [36, Cout, Cin/32, 2, 32]
    return pair.contiguous(), inv_su


def direct_pair_weights(weight):
    """conv weight [Cout, Cin, 3, 3] float32 -> (W2 [9, Cout, Cin/32, 2, 32] float16, inv_sw): the weight operand of the direct
    one-kernel convolution (csrc/conv_direct_h.hip): tap ky * 3 + kx major, rows = output channels, every 32-channel block of a row
    its hi halves then its lo halves (`split16_pair_weights` with the 9 taps in the place of the 36 Winograd frequencies)."""
    cout, cin = weight.shape[:2]
    return split16_pair_weights(weight.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(9, cin, cout))


def igemm_pair_weights(weight):
    """conv weight [Cout, Cin, KH, KW] float32 -> (W2 [Cout, nk, 2, 32] float16, inv_sw): the weight operand of the implicit-GEMM
    convolution on fp16 pairs (csrc/conv_igemm.hip).  Rows = output channels; every K block of 32 holds its hi halves then its lo
    halves; sw w = wh + wl exactly to 22 bits, sw the power of two that brings max |w| into [2^14, 2^15).  K blocks: Cin a multiple
    of 32: (kh, kw, Cin / 32) order; Cin = 3 (the 7x7 stem): one block per kernel row kh, slot kw * 3 + c, the other slots zero."""
    cout, cin, kh, kw = weight.shape
    w = weight.detach().to(torch.float64).permute(0, 2, 3, 1)          # [Cout, KH, KW, Cin]
    if cin == 3:
        assert 3 * kw <= 32
        k = torch.zeros((cout, kh, 32), dtype=torch.float64, device=weight.device)
        k[:, :, :3 * kw] = w.reshape(cout, kh, 3 * kw)
        k = k.reshape(cout, kh * 32)
    else:
        assert cin % 32 == 0
        k = w.reshape(cout, kh * kw * cin)
    wh, wl, inv_sw = pair_split(k)
    nk = k.shape[1] // 32
    pair = torch.stack((wh.view(cout, nk, 32), wl.view(cout, nk, 32)), dim=2)     # [Cout, nk, 2, 32]
    return pair.contiguous(), inv_sw


def direct_r_pair_weights(weight):
    """conv weight [128, 64, 3, 3] float32 -> (W2r float16 [4, 9, 2, 2, 2, 64, 8], inv_sw): the register-resident operand of
    `cslam_conv3x3_direct_r_dev` (csrc/conv_direct_r.hip).  sW w split into exact fp16 pairs;
    W2r[q][tap][ks][mt][hi | lo][lane][e] = the pair half of w[32 q + 16 mt + lane % 16][32 ks + 8 (lane // 16) + e][tap // 3][tap % 3]:
    one v_mfma_f32_16x16x32_f16 A fragment per (q, tap, ks, mt, half), wave q of a workgroup holding [q] for the whole kernel."""
    assert tuple(weight.shape) == (128, 64, 3, 3)
    w = weight.detach().to(torch.float64)
    wh, wl, inv_sw = pair_split(w)
    pair = torch.stack((wh, wl), dim=0).reshape(2, 4, 2, 16, 2, 4, 8, 9)    # [hl][q][mt][i][ks][kg][e][tap]
    W2r = pair.permute(1, 7, 4, 2, 0, 5, 3, 6).reshape(4, 9, 2, 2, 2, 64, 8)  # [q][tap][ks][mt][hl][lane = 16 kg + i][e]
    return W2r.contiguous(), inv_sw


def direct_r2_pair_weights(weight):
    """conv weight [128, 128, 3, 3] float32 -> (W2r2 float16 [2, 4, 9, 2, 2, 2, 64, 8], inv_sw): the register-resident operand of
    `cslam_conv3x3_direct_r2_dev` (csrc/conv_direct_r.hip).  sW w split into exact fp16 pairs;
    W2r2[half][q][tap][ks][slab][hi | lo][lane][e] = the pair half of
    w[64 half + 16 q + lane % 16][64 slab + 32 ks + 8 (lane // 16) + e][tap // 3][tap % 3]: one v_mfma_f32_16x16x32_f16 A fragment per
    (tap, ks, slab, pair half), wave q of the workgroup that owns output-channel half `half` holding [half][q] for the whole kernel."""
    assert tuple(weight.shape) == (128, 128, 3, 3)
    w = weight.detach().to(torch.float64)
    wh, wl, inv_sw = pair_split(w)
    pair = torch.stack((wh, wl), dim=0).reshape(2, 2, 4, 16, 2, 2, 4, 8, 9)      # [hl][half][q][i][slab][ks][kg][e][tap]
    W2 = pair.permute(1, 2, 8, 5, 4, 0, 6, 3, 7).reshape(2, 4, 9, 2, 2, 2, 64, 8)  # [half][q][tap][ks][slab][hl][lane = 16 kg + i][e]
    return W2.contiguous(), inv_sw


def fused64_weights(U):
    """U [16 | 36, 64, Cout] (`wino_weights(w, 2 | 4)`; Cout 64 or 128) -> the operand order of
    `cslam_wino2_fused_c64_dev` / `cslam_wino4_fused_c64_dev`: Up[kq][xi][w][g][c][s] = U[xi][16 kq + 4 g + s][16 w + c]
    (one float4 per MFMA lane and frequency)."""
    assert U.shape[0] in (16, 36) and U.shape[1] == 64 and U.shape[2] in (64, 128)
    return U.view(U.shape[0], 4, 4, 4, U.shape[2] // 16, 16).permute(1, 0, 4, 2, 5, 3).contiguous()


def fused64_pair_weights(U4):
    """U4 [36, 64, Cout] float32 (`wino_weights(w, 4)`; Cout 64 or 128) -> (Uh int32 [4, 36, Cout/16, 4, 16, 4], inv_su):
    the weight operand of `cslam_wino4_fused_c64_h_dev` (csrc/wino_fused_h.hip): sU U split into exact fp16 pairs and
    packed one dword per value, [uh | ul << 16], in the lane order of `fused64_weights`."""
    assert U4.shape[0] == 36 and U4.shape[1] == 64 and U4.shape[2] in (64, 128)
    u = U4.detach().to(torch.float64)
    uh, ul, inv_su = pair_split(u)
    packed = (uh.view(torch.int16).to(torch.int32) & 0xFFFF) | (ul.view(torch.int16).to(torch.int32) << 16)
    cout = U4.shape[2]
    return packed.view(36, 4, 4, 4, cout // 16, 16).permute(1, 0, 4, 2, 5, 3).contiguous(), inv_su


def stem_pair_weights(weight):
    """First-layer weights [64, 3, 3, 3] float32 -> (W1 int32 [4, 2, 64, 4], inv_sw, sumw float32 [64]): the operand of the
    3 -> 64 channel convolution folded into `cslam_wino4_stem_c64_h_dev` (csrc/wino_fused_h.hip).  sW w is split into exact
    fp16 pairs (sW the power of two that brings max |w| into [2^14, 2^15)); K slot (lane group g, slot j) of the 16x16x32
    MFMA holds tap (ky = g, kx = j // 3, ci = j % 3) for g < 3 and the ninth tap (ky = j, kx = 2, ci = 2) of every row for
    g = 3, j < 3 (zeros elsewhere); W1[kq][0 | 1][16 g + n][d] = halves 2d, 2d + 1 of the hi | lo parts for output channel
    16 kq + n.  sumw[co] = sum |w[co]| (float64, rounded up to float32): the kernel bounds max |first-layer output| with it."""
    assert tuple(weight.shape) == (64, 3, 3, 3)
    w = weight.detach().to(torch.float64).cpu()
    wh, wl, inv_sw = pair_split(w)
    slots = torch.zeros((2, 64, 4, 8), dtype=torch.float16)              # [hi | lo][co][g][j]
    for g in range(3):
        for j in range(8):
            slots[0, :, g, j] = wh[:, j % 3, g, j // 3]
            slots[1, :, g, j] = wl[:, j % 3, g, j // 3]
    for j in range(3):
        slots[0, :, 3, j] = wh[:, 2, j, 2]
        slots[1, :, 3, j] = wl[:, 2, j, 2]
    bits = slots.view(torch.int16).to(torch.int32) & 0xFFFF
    packed = bits[..., 0::2] | (bits[..., 1::2] << 16)                   # [2][64][4 g][4 d]
    W1 = packed.view(2, 4, 16, 4, 4).permute(1, 0, 3, 2, 4).reshape(4, 2, 64, 4).contiguous()   # [kq][hl][16 g + n][d]
    sumw = torch.nextafter(w.abs().sum(dim=(1, 2, 3)).to(torch.float32), torch.tensor(float("inf")))
    return W1.to(weight.device), inv_sw, sumw.to(weight.device).contiguous()


def stem_direct_pair_weights(weight):
    """Second-layer weights [64, 64, 3, 3] float32 -> (W2r float16 [4, 9, 2, 2, 64, 8], inv_sw): the register-resident operand of
    `cslam_conv_stem_direct_h_dev` (csrc/conv_stem_direct_h.hip).  sW w (sW the power of two that brings max |w| into
    [2^14, 2^15)) is split into exact fp16 pairs; W2r[q][tap][ks][hi | lo][lane][e] = the pair half of
    w[16 q + lane % 16][32 ks + 8 (lane // 16) + e][tap // 3][tap % 3]: one v_mfma_f32_16x16x32_f16 A fragment per (q, tap, ks, half),
    wave q of a workgroup -- the owner of output channels 16 q .. 16 q + 15 -- holding [q] for the whole kernel."""
    assert tuple(weight.shape) == (64, 64, 3, 3)
    w = weight.detach().to(torch.float64)
    wh, wl, inv_sw = pair_split(w)
    pair = torch.stack((wh, wl), dim=0).reshape(2, 4, 16, 2, 4, 8, 9)       # [hl][q][i][ks][kg][e][tap]
    W2r = pair.permute(1, 6, 3, 0, 4, 2, 5).reshape(4, 9, 2, 2, 64, 8)      # [q][tap][ks][hl][lane = 16 kg + i][e]
    return W2r.contiguous(), inv_sw


def out_bound(weight, bias):
    """(wl1, bmax) of the bound |conv(x) + bias| <= max |x| wl1 + bmax the pair-format outputs are scaled by: the largest L1 norm of
    one output channel's weights [Cout, Cin, KH, KW] and max |bias| (0 without one)."""
    return float(weight.detach().abs().sum(dim=(1, 2, 3)).max()), 0.0 if bias is None else float(bias.detach().abs().max())
