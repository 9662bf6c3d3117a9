"""One wrapper per convolution entry point of libcslam_hip.so (C ABI: include/cslam_hip.h): tensors in, tensors out, the output
allocated here, the kernel on the current stream.  The weight operands come from `vpr/pair_weights.py`; the trunk runners that pick
between these kernels are in `vpr/winograd.py`."""
import torch

from .. import _lib
from .heads import _p, _stream


def _po(t):
    """Pointer of an optional tensor (None = NULL)."""
    return _p(t) if t is not None else None


def _out(B, C, H, W, pool, device):
    """The channels_last float32 output map of a stride-1 layer on H x W maps, halved by a fused MaxPool2d(2, 2)."""
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    return torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=device, memory_format=torch.channels_last)


def _amax_slot(x, slot, have=False):
    """The 4-byte device slot with the bits of max |x|: as it is when its producer filled it (`have`), else after one pass over x."""
    if not have and x.numel() % 4 == 0:
        _lib.check(_lib.load().cslam_absmax_dev(_p(x), x.numel(), _p(slot), _stream(x)))
    elif not have:                                                    # the kernel reads 16 bytes per lane: odd sizes through torch
        slot.copy_(x.abs().max().reshape(1))
    return slot


def stem_pool_fits(Ho, Wo):
    """Whether the stem's output map splits into the 8 x 16-pixel tiles of the fused MaxPool2d(3, 2, 1) (csrc/conv_igemm.hip)."""
    return Ho % 8 == 0 and Wo % 16 == 0


def conv_igemm(ws, x, Wg, bias, kernel, stride, pad, relu, residual=None, amax_in=None, amax_out=None, pool=False):
    """y = act(conv(x) + bias (+ residual)) through `cslam_conv_igemm_h2_dev` (csrc/conv_igemm.hip): x [B,Cin,H,W] channels_last
    float32, Wg = `igemm_pair_weights(weight)`, kernel = (KH, KW).  amax_in: 4-byte device slot with (a bound of) max |x| (None:
    one pass over x measures it); amax_out: zeroed slot that receives max |y|.  pool (3-channel stem with ReLU, output map of
    8 x 16-pixel tiles: `stem_pool_fits`): MaxPool2d(3, 2, 1) fused, y is the pooled map (`cslam_conv_stem_pool_igemm_h2_dev`)."""
    lib = _lib.load()
    x = x.contiguous(memory_format=torch.channels_last)
    B, Cin, H, W = x.shape
    W2, inv_sw = Wg
    Cout = W2.shape[0]
    KH, KW = kernel
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    s = _stream(x)
    slot = amax_in if amax_in is not None else _amax_slot(x, ws._buf("amax", 1, x.device))
    if pool:
        assert Cin == 3 and relu and residual is None and stem_pool_fits(Ho, Wo)
        y = _out(B, Cout, Ho, Wo, True, x.device)
        _lib.check(lib.cslam_conv_stem_pool_igemm_h2_dev(_p(x), _p(W2), _po(bias), B, H, W, Cout, KH, KW, stride, pad, _p(slot),
                                                         float(inv_sw), _po(amax_out), _p(y), s))
        return y
    y = _out(B, Cout, Ho, Wo, False, x.device)
    residual = _residual_like(residual, y)
    _lib.check(lib.cslam_conv_igemm_h2_dev(_p(x), _p(W2), _po(bias), _po(residual), B, H, W, Cin, Cout, KH, KW, stride, pad,
                                           int(relu), _p(slot), float(inv_sw), _po(amax_out), _p(y), s))
    return y


class PairAct(object):
    """An activation between the implicit-GEMM layers of a ResNet trunk.  pairs = False: t is the [B,C,H,W] channels_last float32 map;
    pairs = True: t is the PAIR-FORMAT tensor [B,H,W,C/32,2,32] float16 (csrc/conv_igemm.hip: hi and lo halves of s x, s the power of
    two that brings `bound` into [2^13, 2^14)).  amax: 4-byte device slot with the measured max |x| (or a bound of it); bound: the slot
    the pairs were scaled by (float32 maps: the same slot as amax)."""
    __slots__ = ("t", "pairs", "shape", "amax", "bound")

    def __init__(self, t, pairs, shape, amax, bound):
        self.t, self.pairs, self.shape, self.amax, self.bound = t, pairs, tuple(shape), amax, bound


def pairs_to_float(act):
    """PairAct (pair format) -> [B,C,H,W] channels_last float32 (torch; tests and debugging: the trunk never converts)."""
    B, C, H, W = act.shape
    e = torch.frexp(act.bound.view(torch.float32).clamp(1e-30, 1e30))[1].item()
    s = 2.0 ** (14 - e)
    v = (act.t[:, :, :, :, 0, :].float() + act.t[:, :, :, :, 1, :].float()) / s           # [B,H,W,C/32,32]
    return v.reshape(B, H, W, C).permute(0, 3, 1, 2)


def _pair_out(B, Cout, Ho, Wo, out_pairs, device):
    """The output of a kernel between PairActs: the pair-format tensor, or the channels_last float32 map."""
    if out_pairs:
        return torch.empty((B, Ho, Wo, Cout // 32, 2, 32), dtype=torch.float16, device=device)
    return _out(B, Cout, Ho, Wo, False, device)


def _res_args(res, shape):
    """(pointer, pairs flag, bound pointer) of the optional shortcut of a kernel between PairActs."""
    if res is None:
        return None, 0, None
    assert res.shape == shape and (res.pairs or res.t.is_contiguous(memory_format=torch.channels_last))
    return _p(res.t), int(res.pairs), _p(res.bound)


def conv_igemm_p(ws, act, Wg, bias, kernel, stride, pad, relu, res, wl1, bmax, amax_out, bound_out, out_pairs):
    """`cslam_conv_igemm_h2p_dev`: the implicit-GEMM convolution between PairActs.  act / res (or None) in either format; the result is
    a PairAct in pair format (out_pairs) or float32, with amax_out (zeroed slot: measured max |y|) and bound_out as its slots."""
    B, Cin, H, W = act.shape
    W2, inv_sw = Wg
    Cout = W2.shape[0]
    KH, KW = kernel
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    y = _pair_out(B, Cout, Ho, Wo, out_pairs, act.t.device)
    rt, rpairs, rbound = _res_args(res, (B, Cout, Ho, Wo))
    assert act.pairs or act.t.is_contiguous(memory_format=torch.channels_last)
    _lib.check(_lib.load().cslam_conv_igemm_h2p_dev(
        _p(act.t), int(act.pairs), _p(act.bound), _p(W2), _po(bias), rt, rpairs, rbound, B, H, W, Cin, Cout, KH, KW, stride, pad,
        int(relu), _p(act.amax), float(inv_sw), float(wl1), float(bmax), _p(amax_out), int(out_pairs),
        _p(bound_out) if out_pairs else None, _p(y), _stream(act.t)))
    return PairAct(y, bool(out_pairs), (B, Cout, Ho, Wo), amax_out, bound_out if out_pairs else amax_out)


def conv3x3_direct_p(act, Wp, bias, relu, res, wl1, bmax, amax_out, bound_out, out_pairs):
    """`cslam_conv3x3_direct_p_dev` (csrc/conv_direct_p.hip): the 3x3 / stride 1 / pad 1 convolution 64 -> 64 between PairActs with the
    weights register-resident and the patch by LDS-DMA.  act: pair format, or (no shortcut) a float32 map split while it is staged;
    res (or None): either format; Wp = `stem_direct_pair_weights(weight)`; the other arguments and the result as `conv_igemm_p`."""
    B, Cin, H, W = act.shape
    assert Cin == 64 and (act.pairs or (res is None and act.t.is_contiguous(memory_format=torch.channels_last)))
    y = _pair_out(B, 64, H, W, out_pairs, act.t.device)
    rt, rpairs, rbound = _res_args(res, (B, 64, H, W))
    _lib.check(_lib.load().cslam_conv3x3_direct_p_dev(
        _p(act.t), int(act.pairs), _p(act.bound), _p(Wp[0]), _po(bias), rt, rpairs, rbound, B, H, W, 64, 64, int(relu),
        _p(act.amax), float(Wp[1]), float(wl1), float(bmax), _p(amax_out), int(out_pairs), _p(bound_out) if out_pairs else None,
        _p(y), _stream(act.t)))
    return PairAct(y, bool(out_pairs), (B, 64, H, W), amax_out, bound_out if out_pairs else amax_out)


def direct_p_fits(conv_shape, kernel, stride, pad, H, W):
    """Whether a convolution takes the register-resident pair-format kernel: 64 -> 64 channels, 3x3 / stride 1 / pad 1, two images' maps
    within 32-bit buffer offsets."""
    return (tuple(conv_shape[:2]) == (64, 64) and tuple(kernel) == (3, 3) and stride == 1 and pad == 1
            and H * W * 512 + 11 * W * 256 < 2 ** 31 - 16)


def conv3x3_direct_h(x, Wd, bias, relu, pool, amax_in, amax_out=None):
    """y = [pool](relu(conv3x3(x) + bias)) through `cslam_conv3x3_direct_h_dev` (csrc/conv_direct_h.hip): x [B,Cin,H,W]
    channels_last float32 (Cin a multiple of 32), 128 output channels; Wd = `direct_pair_weights(weight)`; amax_in = 4-byte device
    slot with (a bound of) max |x|; amax_out (optional): zeroed slot that receives max |y|."""
    x = x.contiguous(memory_format=torch.channels_last)
    B, Cin, H, W = x.shape
    W2, inv_sw = Wd
    Cout = W2.shape[1]
    y = _out(B, Cout, H, W, pool, x.device)
    _lib.check(_lib.load().cslam_conv3x3_direct_h_dev(_p(x), _p(W2), _po(bias), B, H, W, Cin, Cout, int(relu), int(pool), _p(amax_in),
                                                      float(inv_sw), _po(amax_out), _p(y), _stream(x)))
    return y


def _direct_r(fn, x, Wr, bias, relu, pool, amax_in, amax_out):
    """The two register-resident kernels of csrc/conv_direct_r.hip share one argument list."""
    x = x.contiguous(memory_format=torch.channels_last)
    B, Cin, H, W = x.shape
    y = _out(B, 128, H, W, pool, x.device)
    _lib.check(fn(_p(x), _p(Wr[0]), _po(bias), B, H, W, Cin, 128, int(relu), int(pool), _p(amax_in), float(Wr[1]), _po(amax_out),
                  _p(y), _stream(x)))
    return y


def conv3x3_direct_r(x, Wr, bias, relu, pool, amax_in, amax_out=None):
    """y = [pool](relu(conv3x3(x) + bias)) through `cslam_conv3x3_direct_r_dev` (csrc/conv_direct_r.hip): x [B,64,H,W] channels_last
    float32, 128 output channels; Wr = `direct_r_pair_weights(weight)`; amax_in / amax_out as `conv3x3_direct_h`."""
    return _direct_r(_lib.load().cslam_conv3x3_direct_r_dev, x, Wr, bias, relu, pool, amax_in, amax_out)


def conv3x3_direct_r2(x, Wr2, bias, relu, pool, amax_in, amax_out=None):
    """y = [pool](relu(conv3x3(x) + bias)) through `cslam_conv3x3_direct_r2_dev` (csrc/conv_direct_r.hip): x [B,128,H,W] channels_last
    float32, 128 output channels; Wr2 = `direct_r2_pair_weights(weight)`; amax_in / amax_out as `conv3x3_direct_h`."""
    return _direct_r(_lib.load().cslam_conv3x3_direct_r2_dev, x, Wr2, bias, relu, pool, amax_in, amax_out)


def conv3x3_direct_r_pairs(x, Wr, bias, wl1, bmax, amax_in, bound_out, amax_out=None):
    """relu(conv3x3(x) + bias), 64 -> 128 channels, written in PAIR FORMAT (`cslam_conv3x3_direct_r_pairs_dev`): returns the
    [B,H,W,4,2,32] float16 tensor scaled for the bound max|x| wl1 + bmax, which goes to the 4-byte slot bound_out."""
    x = x.contiguous(memory_format=torch.channels_last)
    B, Cin, H, W = x.shape
    y = torch.empty((B, H, W, 4, 2, 32), dtype=torch.float16, device=x.device)
    _lib.check(_lib.load().cslam_conv3x3_direct_r_pairs_dev(_p(x), _p(Wr[0]), _po(bias), B, H, W, Cin, 128, _p(amax_in), float(Wr[1]),
                                                            float(wl1), float(bmax), _po(amax_out), _p(bound_out), _p(y), _stream(x)))
    return y


def conv3x3_direct_hp(xp, shape, bound, Wd, bias, relu, pool, amax_out=None):
    """`conv3x3_direct_h` reading a PAIR-FORMAT map xp [B,H,W,Cin/32,2,32] float16 (shape = its (B,Cin,H,W), bound = its 4-byte bound
    slot) through `cslam_conv3x3_direct_hp_dev`: the patch is staged without conversion."""
    B, Cin, H, W = shape
    W2, inv_sw = Wd
    Cout = W2.shape[1]
    y = _out(B, Cout, H, W, pool, xp.device)
    _lib.check(_lib.load().cslam_conv3x3_direct_hp_dev(_p(xp), _p(bound), _p(W2), _po(bias), B, H, W, Cin, Cout, int(relu), int(pool),
                                                       float(inv_sw), _po(amax_out), _p(y), _stream(xp)))
    return y


def conv_stem_direct_h(x0, stem, bias1, Wr, bias, pool, amax_x0, amax_out=None):
    """VGG-16's first two convolutions as ONE direct kernel (`cslam_conv_stem_direct_h_dev`): x0 planar [B,3,H,W] float32,
    stem = `stem_pair_weights(conv1_1.weight)`, Wr = `stem_direct_pair_weights(conv1_2.weight)`; amax_x0 = 4-byte device slot with
    the bits of max |x0|.  Returns ReLU(conv(ReLU(conv(x0) + bias1)) + bias) (+ MaxPool2d), channels_last."""
    B, C3, H, W = x0.shape
    assert C3 == 3 and x0.is_contiguous()
    y = _out(B, 64, H, W, pool, x0.device)
    _lib.check(_lib.load().cslam_conv_stem_direct_h_dev(
        _p(x0), _p(stem[0]), _po(bias1), _p(stem[2]), float(stem[1]), _p(Wr[0]), _po(bias), float(Wr[1]), B, H, W, int(pool),
        _p(amax_x0), _po(amax_out), _p(y), _stream(x0)))
    return y


def wino_stem64_h(x0, stem, bias1, Uh, bias, pool, amax_x0, amax_out=None):
    """VGG-16's first two convolutions as ONE kernel (`cslam_wino4_stem_c64_h_dev`): x0 planar [B,3,H,W] float32,
    stem = `stem_pair_weights(conv1_1.weight)`, Uh = `fused64_pair_weights` of the 64 -> 64 layer; amax_x0 = 4-byte device
    slot with the bits of max |x0|.  Returns ReLU(conv(ReLU(conv(x0) + bias1)) + bias) (+ MaxPool2d), channels_last."""
    B, C3, H, W = x0.shape
    assert C3 == 3 and x0.is_contiguous() and Uh[0].shape[2] == 4
    y = _out(B, 64, H, W, pool, x0.device)
    _lib.check(_lib.load().cslam_wino4_stem_c64_h_dev(
        _p(x0), _p(stem[0]), _po(bias1), _p(stem[2]), float(stem[1]), _p(Uh[0]), _po(bias), B, H, W, int(pool), _p(amax_x0),
        float(Uh[1]), _po(amax_out), _p(y), _stream(x0)))
    return y


def _residual_like(residual, y):
    """The optional shortcut in channels_last storage, shaped like the output it is added to."""
    if residual is not None:
        residual = residual.contiguous(memory_format=torch.channels_last)
        assert residual.shape == y.shape
    return residual


def wino_fused64_h(x, Uh, bias, relu, pool, amax_in, amax_out=None, residual=None):
    """The fp16-pair form of `wino_fused64` (csrc/wino_fused_h.hip): Uh = `fused64_pair_weights(U4)`; amax_in = 4-byte
    device slot holding the bits of (a bound of) max |x|; amax_out (zeroed slot or None) receives those of max |y|."""
    B, _, H, W = x.shape
    Cout = Uh[0].shape[2] * 16
    y = _out(B, Cout, H, W, pool, x.device)
    residual = _residual_like(residual, y)
    _lib.check(_lib.load().cslam_wino4_fused_c64_h_dev(
        _p(x), _p(Uh[0]), _po(bias), _po(residual), B, H, W, Cout, int(relu), int(pool), _p(amax_in), float(Uh[1]), _po(amax_out),
        _p(y), _stream(x)))
    return y


def wino_fused64(x, Up, bias, relu, pool, residual=None):
    """64 -> 64 / 128 channel 3x3 convolution of x [B,64,H,W] (channels_last storage) as one kernel
    (csrc/wino_fused.hip); Up from `fused64_weights` (16 frequencies: the F(2x2) kernel, 36: the F(4x4) one)."""
    lib = _lib.load()
    B, _, H, W = x.shape
    Cout = Up.shape[2] * 16
    y = _out(B, Cout, H, W, pool, x.device)
    residual = _residual_like(residual, y)
    fn = lib.cslam_wino4_fused_c64_dev if Up.shape[1] == 36 else lib.cslam_wino2_fused_c64_dev
    _lib.check(fn(_p(x), _p(Up), _po(bias), _po(residual), B, H, W, Cout, int(relu), int(pool), _p(y), _stream(x)))
    return y
