"""Winograd F(2x2, 3x3) execution of the wide 3x3 convolutions of the extractor backbone.

The backbone stays a PyTorch module (same layer list, same parameter names, checkpoints load unchanged:
vpr/backbones.py); `WinogradTrunk` only changes HOW its 3x3 / stride 1 / pad 1 convolutions with many
input channels are executed: hand-written HIP input / output transforms (csrc/winograd.hip through
`cslam_wino_input_dev` / `cslam_wino_output_dev`, bias + ReLU + the following MaxPool fused into the
output transform) around 16 plain fp32 GEMMs (`torch.bmm` = rocBLAS).  2.25x fewer multiplications than
the direct convolution MIOpen runs for the same layer (4x with the F(4x4, 3x3) tiles used where the map
sides are multiples of 4); fp32 throughout, as close to a float64 evaluation as the direct fp32 form is
(1.3e-6 / 3.7e-6 of the largest activation for F(2x2) / F(4x4) against 1.4e-6, tests/test_heads_gpu.py).
The first convolution (3 input channels) stays on torch's direct form, with bias + ReLU (+ MaxPool) applied
in one HIP pass (`cslam_bias_act_pool_dev`).

Here: the Winograd pipeline (`wino_conv3x3`), the two trunk runners and every switch and table they read at call time.  The weight
packers are in vpr/pair_weights.py and the one-kernel wrappers in vpr/conv_kernels.py; both are re-exported below, so that
`cslam_amd.vpr.winograd` stays the one namespace callers import from and set switches on.
"""
import os

import torch
from torch import nn

from .. import _lib
from .conv_kernels import (PairAct, _amax_slot, _out, _po, _residual_like, conv3x3_direct_h, conv3x3_direct_hp,   # noqa: F401
                           conv3x3_direct_p, conv3x3_direct_r, conv3x3_direct_r2, conv3x3_direct_r_pairs, conv_igemm, conv_igemm_p,
                           conv_stem_direct_h, direct_p_fits, pairs_to_float, stem_pool_fits, wino_fused64, wino_fused64_h,
                           wino_stem64_h)
from .heads import _p, _stream
from .pair_weights import (direct_pair_weights, direct_r2_pair_weights, direct_r_pair_weights, fused64_pair_weights,    # noqa: F401
                           fused64_weights, igemm_pair_weights, out_bound, split16_pair_weights, split16_weights,
                           stem_direct_pair_weights, stem_pair_weights, wino_weights)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


_TUNED = {"done": False}


def use_tuned_gemms():
    """Pick the fastest library solution for the strided-batched fp32 GEMM shapes of the VGG-16 trunk at the
    256-frame chunk bench.py and the batched callers use: torch's TunableOp replays the selections recorded on an
    MI355X in `tunableop_gfx950.csv` (tuning itself stays off, unknown shapes keep the library default, and a
    library / architecture mismatch makes torch ignore the file).  +8 % frames/s over the default heuristic.
    Regenerate with `PYTORCH_TUNABLEOP_ENABLED=1 python tools/extract_leg.py`.  CSLAM_TUNED_GEMM=0 disables."""
    if _TUNED["done"] or os.environ.get("CSLAM_TUNED_GEMM", "1") == "0" or not torch.cuda.is_available():
        return
    _TUNED["done"] = True
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950.csv")
    try:
        import torch.cuda.tunable as tunable
        if tunable.is_enabled() or not os.path.exists(path):
            return                                   # the user drives TunableOp themselves
        tunable.enable(True)
        tunable.tuning_enable(False)
        tunable.read_file(path)
    except Exception as e:                            # never fatal: the default solutions are still correct
        import warnings
        warnings.warn("cslam_amd: tuned GEMM table not loaded (%s)" % e)


def _z_form(cin, cout):
    """Z form of the pair products (GEMM + column half of the output transform, 24 planes instead of 36) where it pays:
    measured per layer at the 256-frame chunk (profiles/r03_v4_perf_zform.log) the output kernel gains ~30 % everywhere, but
    the GEMM's 128 x 128 tiles (all the 128 Z registers per lane leave room for) lose more than that wherever the product is
    not purely HBM-bound -- only conv2_2 (128 -> 128 channels at 112 x 112: 2.08 -> 1.78 ms) comes out ahead.
    Z_FORM_MAX = largest Cin * Cout that takes it (128 * 128; 0 = off, 262144 = every layer: tests/test_wino_gemm_gpu.py runs both)."""
    return cin * cout <= Z_FORM_MAX


Z_FORM_MAX = 128 * 128
PAIR_ACTS = True              # ResNet trunks: pair-format maps between the implicit-GEMM layers (False: float32 maps, the A/B partner)
VGG_PAIRS = False             # VGG trunk: the map between conv2_1 and conv2_2 in pair format.  Built, tested and measured in round 6: conv2_2 staging pairs
                              # without the split 2.11 against 2.135 ms, conv2_1 writing them 1.15 against 1.04 -- the split was already hidden under
                              # the MFMAs, the two 8-byte stores per row are not (profiles/r06_j_vgg_pairs_ab.log): off by default
DIRECT_P = True               # ResNet trunks: the 64 -> 64 3x3 layers between pair-format maps through csrc/conv_direct_p.hip (False: the implicit GEMM)
IGEMM_CONVS = True            # ResNet trunks: strided / 1x1 / 7x7 layers through csrc/conv_igemm.hip (False: torch, the A/B partner)


def _f4_fits(B, H, W):
    """F(4x4) needs enough tiles to keep its 36 GEMMs efficient (single frames stay on F(2x2)) and maps whose sides waste at most
    ~1/3 of the padded tile area (14 -> 16, 7 -> 8); tiles may hang over the map."""
    t4h, t4w = -(-H // 4), -(-W // 4)
    return B * t4h * t4w >= 512 and 16 * t4h * t4w <= 1.35 * H * W


def _pair_pipeline(ws, x, layers, slots, relu, pool, residual, amax_out):
    """F(4x4) with the 36 products in this library's GEMM on exact fp16 pairs (csrc/wino_gemm.hip), V stored once at its fp32 size, M in
    fp32: the input transform of x, per layer the products and -- between two layers -- the chained transform (csrc/wino_chain.hip:
    ReLU, no pool), which writes the next layer's V over the one the products have just read; the scaled output transform (relu, pool,
    residual: the last layer's) ends it.  layers = [(U2, bias, wl1, bmax)] -- one entry: a single convolution, wl1 / bmax (`out_bound`,
    the scale of the next V) unread; slots[j] = 4-byte slot with max |input of layer j|, slots[0] filled by the caller and the others by
    the chained transforms; amax_out: zeroed slot that receives max |y|."""
    lib = _lib.load()
    B, Cin, H, W = x.shape
    T = B * -(-H // 4) * -(-W // 4)
    s = _stream(x)
    V2 = ws._buf("V", 36 * T * Cin, x.device)                      # 36 x T x 2 Cin halfs
    _lib.check(lib.cslam_wino4_input_h2_dev(_p(x), B, H, W, Cin, _p(slots[0:1]), _p(V2), s))
    vscale = slots[0:1]                                            # the slot the current V was scaled by
    for j, (U2, bias, wl1, bmax) in enumerate(layers):
        Cout = U2[0].shape[1]
        M = ws._buf("M", 36 * T * Cout, x.device)
        _lib.check(lib.cslam_wino_gemm_h2_dev(_p(V2), _p(U2[0]), T, Cin, Cout, _p(M), s))
        if j + 1 < len(layers):
            bound = ws._buf("chain_bounds", len(layers), x.device)[j + 1:j + 2]
            V2 = ws._buf("V", 36 * T * Cout, x.device)
            _lib.check(lib.cslam_wino4_chain_h2_dev(_p(M), _po(bias), B, H, W, Cout, _p(vscale), float(U2[1]), _p(slots[j:j + 1]),
                                                    wl1, bmax, _p(slots[j + 1:j + 2]), _p(bound), _p(V2), s))
            vscale, Cin = bound, Cout
    y = _out(B, Cout, H, W, pool, x.device)
    _lib.check(lib.cslam_wino4_output_scaled_dev(_p(M), _po(bias), _po(_residual_like(residual, y)), B, H, W, Cout, int(relu),
                                                 int(pool), _p(vscale), float(U2[1]), _po(amax_out), _p(y), s))
    return y


def wino_conv3x3(ws, x, U, U4, bias, relu, pool=False, residual=None, U3=None, amax_in=None, amax_out=None, U2=None):
    """3x3 / stride 1 / pad 1 convolution of x [B,Cin,H,W] (channels_last storage, any H and W) through the
    Winograd pipeline; U / U4 from `wino_weights` (U4 None = F(2x2,3x3) only).  bias [Cout] or None, residual
    (channels_last, shaped like the output) is added before the ReLU.  `ws` owns the V / M workspaces.
    U2 = `split16_pair_weights(U4)` (the default for wide layers): the 36 F(4x4) products run in this library's GEMM
    (csrc/wino_gemm.hip) over the exact fp16 hi / lo pairs of both operands, three of the four partial products in fp32
    accumulators: fp32-grade, at the fp16 MFMA rate, V and M at their fp32 sizes.
    U3 = `split16_weights(U4)` (round 1's form, split16_h3=True): the same arithmetic as ONE library fp16 GEMM over
    K' = 3 Cin, operands [vh | vl | vh] x [uh ; uh ; ul].
    amax_in: 4-byte device slot already holding the bits of (a bound of) max |x| -- saves the pass over x; amax_out: zeroed
    slot that receives the same for y from the F(4x4) output transform.  Returns y; `ws.amax_written` says whether amax_out
    was filled (only the F(4x4) output kernels do it)."""
    lib = _lib.load()
    B, Cin, H, W = x.shape
    Cout = U.shape[2]
    assert residual is None or not pool
    four = U4 is not None and _f4_fits(B, H, W)
    ws.amax_written = four and amax_out is not None
    T = B * -(-H // 4) * -(-W // 4) if four else B * -(-H // 2) * -(-W // 2)
    s = _stream(x)
    slot = None
    if four and (U2 is not None or U3 is not None):                   # the fp16-pair forms scale V by (a bound of) max |x|
        slot = amax_in if amax_in is not None else _amax_slot(x, ws._buf("amax", 1, x.device))
    z = four and U2 is not None and residual is None and _z_form(Cin, Cout)
    if four and U2 is not None and not z:
        return _pair_pipeline(ws, x, [(U2, bias, None, None)], slot, relu, pool, residual, amax_out)
    inv_su = 1.0
    if z:
        # the purely HBM-bound product (conv2_2): the column half of the output transform is folded into the GEMM, which then
        # writes -- and the output kernel reads -- 24 instead of 36 planes (csrc/wino_gemm.hip `wino_zgemm_h2_kernel`)
        V2 = ws._buf("V", 36 * T * Cin, x.device)
        M = ws._buf("M", 36 * T * Cout, x.device)
        _lib.check(lib.cslam_wino4_input_h2_dev(_p(x), B, H, W, Cin, _p(slot), _p(V2), s))
        _lib.check(lib.cslam_wino_zgemm_h2_dev(_p(V2), _p(U2[0]), T, Cin, Cout, _p(M), s))
        inv_su = U2[1]
    elif slot is not None:
        V3 = ws._buf("V", (36 * T * 3 * Cin + 1) // 2, x.device).view(torch.float16)[:36 * T * 3 * Cin].view(36, T, 3 * Cin)
        _lib.check(lib.cslam_wino4_input_h3_dev(_p(x), B, H, W, Cin, _p(slot), _p(V3), s))
        # torch 2.10's TunableOp does not cover `bmm` with out_dtype; hipBLASLt's default solution is used.  Routing it to
        # rocBLAS instead is 3-13 % faster on the isolated GEMMs and not measurable on the trunk (profiles/r01_exp_split16.log)
        M = torch.bmm(V3, U3[0], out_dtype=torch.float32)
        inv_su = U3[1]
    else:
        n2, Uu, fin = (36, U4, lib.cslam_wino4_input_dev) if four else (16, U, lib.cslam_wino_input_dev)
        V = ws._buf("V", n2 * T * Cin, x.device).view(n2, T, Cin)
        M = ws._buf("M", n2 * T * Cout, x.device).view(n2, T, Cout)
        _lib.check(fin(_p(x), B, H, W, Cin, _p(V), s))                       # x's storage is NHWC
        torch.bmm(V, Uu, out=M)
    y = _out(B, Cout, H, W, pool, x.device)
    residual = _residual_like(residual, y)
    if z:
        _lib.check(lib.cslam_wino4_output_z_dev(_p(M), _po(bias), B, H, W, Cout, int(relu), int(pool), _p(slot), float(inv_su),
                                                _po(amax_out), _p(y), s))
    elif slot is not None or ws.amax_written:
        _lib.check(lib.cslam_wino4_output_scaled_dev(_p(M), _po(bias), _po(residual), B, H, W, Cout, int(relu), int(pool),
                                                     _po(slot), float(inv_su), _po(amax_out), _p(y), s))
    else:
        fout = lib.cslam_wino4_output_dev if four else lib.cslam_wino_output_dev
        _lib.check(fout(_p(M), _po(bias), _po(residual), B, H, W, Cout, int(relu), int(pool), _p(y), s))
    return y


class _Workspace(object):
    def __init__(self):
        self._ws = {}
        self.amax_written = False

    def _buf(self, name, numel, device):
        b = self._ws.get(name)
        if b is None or b.numel() < numel or b.device != device:
            b = torch.empty(numel, dtype=torch.float32, device=device)
            self._ws[name] = b
        return b[:numel]


def fold_bn(conv, bn):
    """Eval-mode BatchNorm folded into the preceding convolution: (weight * s[co], beta - mean * s (+ bias * s)),
    s = gamma / sqrt(var + eps).  Exact in real arithmetic; computed in float64."""
    s = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps))
    w = (conv.weight.double() * s[:, None, None, None]).float().contiguous(memory_format=torch.channels_last)
    b = bn.bias.double() - bn.running_mean.double() * s
    if conv.bias is not None:
        b = b + conv.bias.double() * s
    return w, b.float().contiguous()


class _FoldedConv(object):
    """conv + eval BatchNorm as one convolution; 3x3 / stride 1 / pad 1 ones also carry Winograd weights."""

    def __init__(self, conv, bn, tile, min_in_channels, direct=False):
        self.weight, self.bias = fold_bn(conv, bn)
        self.stride, self.padding = conv.stride, conv.padding
        self.U = self.U4 = self.Wg = self.Wp = None
        self.kernel = tuple(conv.kernel_size)
        # the bound of the output the pair-format chain scales by: |y| <= max |x| wl1 + bmax (+ max |shortcut|)
        self.wl1, self.bmax = out_bound(self.weight, self.bias)
        self.in_channels = conv.in_channels
        igemm_ok = (IGEMM_CONVS and conv.dilation == (1, 1) and conv.groups == 1 and conv.stride[0] == conv.stride[1]
                    and conv.padding[0] == conv.padding[1] and conv.out_channels % 64 == 0 and conv.weight.is_cuda
                    and (conv.in_channels % 32 == 0 or (conv.in_channels == 3 and 3 * conv.kernel_size[1] <= 32)))
        if direct and igemm_ok:
            # every convolution of the trunk as this library's implicit GEMM on fp16 pairs (csrc/conv_igemm.hip): per layer faster than
            # the fp32 Winograd pipeline on ResNet-18's maps (profiles/r05_v23_igemm_layers.log), no library product anywhere
            self.Wg = igemm_pair_weights(self.weight)
            self.Wg = (self.Wg[0].to(self.weight.device), self.Wg[1])
            if (DIRECT_P and tuple(self.weight.shape) == (64, 64, 3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)):
                # layer1's 64 -> 64 convolutions between pair-format maps: the register-resident direct kernel (csrc/conv_direct_p.hip)
                self.Wp = stem_direct_pair_weights(self.weight)
                self.Wp = (self.Wp[0].to(self.weight.device), self.Wp[1])
        elif (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
                and conv.groups == 1 and conv.in_channels >= min_in_channels and conv.in_channels % 4 == 0
                and conv.out_channels % 4 == 0 and conv.weight.is_cuda):
            self.U = wino_weights(self.weight).to(self.weight.device)
            self.U4 = wino_weights(self.weight, 4).to(self.weight.device) if tile == 4 else None
        elif igemm_ok:
            # the 7x7 stem, the strided 3x3 and the 1x1 shortcut layers: this library's implicit GEMM on fp16 pairs
            # (csrc/conv_igemm.hip) instead of torch / MIOpen
            self.Wg = igemm_pair_weights(self.weight)
            self.Wg = (self.Wg[0].to(self.weight.device), self.Wg[1])
        # (layer1 of ResNet-18/34 through the one-kernel F(4x4) forms -- csrc/wino_fused.hip, round 1: 30.9k vs 31.8k frames/s; csrc/
        # wino_fused_h.hip on fp16 pairs with the shortcut fused, round 5 against the implicit GEMM: extract 45.9k vs 51.3k frames/s,
        # three alternating runs on one box -- is slower on 56 x 56 maps.  Not wired in.)

    def __call__(self, ws, x, relu, residual=None, amax_in=None, amax_out=None, pool=False):
        """amax_in: 4-byte device slot with (a bound of) max |x|, or None; amax_out: zeroed slot for max |y|.  `ws.amax_written` says
        whether amax_out was filled (the implicit-GEMM kernel always does)."""
        ws.amax_written = False
        if self.U is not None:
            return wino_conv3x3(ws, x.contiguous(memory_format=torch.channels_last), self.U, self.U4, self.bias, relu,
                                False, residual)
        if self.Wg is not None and x.shape[2] + 2 * self.padding[0] >= self.kernel[0] and x.shape[3] + 2 * self.padding[0] >= self.kernel[1]:
            # (a map smaller than the kernel: torch below, as for every geometry the implicit GEMM does not take)
            y = conv_igemm(ws, x, self.Wg, self.bias, self.kernel, self.stride[0], self.padding[0], relu, residual, amax_in, amax_out, pool)
            ws.amax_written = amax_out is not None
            return y
        y = torch.nn.functional.conv2d(x, self.weight, self.bias, self.stride, self.padding)
        if residual is not None:
            y += residual
        return torch.relu_(y) if relu else y


class WinogradResNet(_Workspace):
    """Runs the ResNet trunks of vpr/backbones.py (`resnet_trunk`: conv1, bn1, relu, maxpool, layer1..4 of
    BasicBlock / Bottleneck) like `trunk(x)` in eval mode, with every BatchNorm folded into its convolution.  Since round 5 EVERY
    convolution is a kernel of this library on fp16 pairs (`direct`, the default): the implicit GEMM (csrc/conv_igemm.hip), the
    register-resident direct kernel for layer1's 64 -> 64 layers (csrc/conv_direct_p.hip, round 6), pair-format maps between them --
    `frontend.backbone_conv` 'winograd' and 'winograd2' therefore run the SAME path for ResNets (the name is the VGG trunk's; `tile`
    only matters with direct=False: the 3x3 / stride-1 layers through the fp32 Winograd pipeline with library products, rounds 1-4's
    A/B partner; `IGEMM_CONVS = False` additionally sends the stem, strided and 1x1 layers to torch)."""

    def __init__(self, trunk, min_in_channels=64, tile=4, direct=None):
        """direct (default: IGEMM_CONVS): EVERY eligible convolution through the implicit GEMM on fp16 pairs; False: the 3x3 / stride 1
        layers through the fp32 Winograd pipeline with library products (rounds 1-4; the A/B partner)."""
        super().__init__()
        self.trunk, self.min_in_channels, self.tile = trunk, int(min_in_channels), int(tile)
        self.direct = IGEMM_CONVS if direct is None else bool(direct)
        use_tuned_gemms()
        self.refresh()

    def refresh(self):
        mods = list(self.trunk)
        mk = lambda c, b: _FoldedConv(c, b, self.tile, self.min_in_channels, self.direct)      # noqa: E731
        self.stem = mk(mods[0], mods[1])
        self.stem_pool = mods[3]
        self.blocks = []
        for layer in mods[4:]:
            for blk in layer:
                d = {"down": None if blk.downsample is None else mk(blk.downsample[0], blk.downsample[1]),
                     "c1": mk(blk.conv1, blk.bn1), "c2": mk(blk.conv2, blk.bn2),
                     "c3": mk(blk.conv3, blk.bn3) if hasattr(blk, "conv3") else None}
                self.blocks.append(d)
        return self

    @torch.no_grad()
    def __call__(self, x, x_bound=None):
        """x_bound: a known bound of max |x| (a normalised 8-bit image: heads.normalised_image_bound()) spares the pass that measures it."""
        x = x.contiguous(memory_format=torch.channels_last)
        # max |activation| travels from the epilogue that produced a map to the kernels that read it (4-byte device slots, the power-of-two
        # scale of the fp16 pairs): no pass over an activation just to measure it.  `ax` = slot of the current x, or None (unknown)
        slots = self._buf("amax_slots", 4 * len(self.blocks) + 6, x.device)
        slots.zero_()
        free = iter(slots.split(1))

        def run(conv, inp, relu, res, a_in):
            out_slot = next(free)
            y = conv(self, inp, relu, res, a_in, out_slot)
            return y, (out_slot if self.amax_written else None)
        a0 = None
        if x_bound is not None:
            a0 = next(free)
            a0.fill_(float(x_bound))
        sp = self.stem_pool
        ho = (x.shape[2] + 2 * self.stem.padding[0] - self.stem.kernel[0]) // self.stem.stride[0] + 1
        wo = (x.shape[3] + 2 * self.stem.padding[1] - self.stem.kernel[1]) // self.stem.stride[1] + 1
        if (self.stem.Wg is not None and x.shape[1] == 3 and stem_pool_fits(ho, wo) and isinstance(sp, torch.nn.MaxPool2d)
                and _pair(sp.kernel_size) == (3, 3) and _pair(sp.stride) == (2, 2) and _pair(sp.padding) == (1, 1)
                and _pair(sp.dilation) == (1, 1) and not sp.ceil_mode):
            ax = next(free)                               # conv1 + bn1 + relu + maxpool as one kernel: the 112 x 112 map never exists
            x = self.stem(self, x, True, None, a0, ax, pool=True)
        else:
            y, ax = run(self.stem, x, True, None, a0)
            x = sp(y)                                     # max |pool(y)| <= max |y|: the slot stays a bound
        convs = [c for b in self.blocks for c in (b["down"], b["c1"], b["c2"], b["c3"]) if c is not None]
        if PAIR_ACTS and ax is not None and all(c.Wg is not None and c.in_channels % 32 == 0 for c in convs):
            # every layer is the implicit GEMM: the maps between them travel in PAIR FORMAT (written once by the producing epilogue, read
            # by LDS-DMA: no split per tap and output tile); the pooled stem output goes in as float32, the last map comes out as float32
            pslots = self._buf("pair_slots", 2 * len(convs) + 2, x.device)
            pslots.zero_()
            pfree = iter(pslots.split(1))                 # per layer: the slot of max |y|, then the slot of the bound its pairs are scaled by
            last = convs[-1]

            def runp(conv, a, relu, res):
                amax_out, bound_out = next(pfree), next(pfree)
                if (conv.Wp is not None and (a.pairs or res is None) and conv is not last
                        and direct_p_fits(conv.weight.shape, conv.kernel, conv.stride[0], conv.padding[0], a.shape[2], a.shape[3])):
                    return conv3x3_direct_p(a, conv.Wp, conv.bias, relu, res, conv.wl1, conv.bmax, amax_out, bound_out, True)
                return conv_igemm_p(self, a, conv.Wg, conv.bias, conv.kernel, conv.stride[0], conv.padding[0], relu, res, conv.wl1,
                                    conv.bmax, amax_out, bound_out, conv is not last)
            cur = PairAct(x, False, x.shape, ax, ax)
            for b in self.blocks:
                idt = cur if b["down"] is None else runp(b["down"], cur, False, None)
                o = runp(b["c1"], cur, True, None)
                if b["c3"] is None:                   # BasicBlock
                    cur = runp(b["c2"], o, True, idt)
                else:                                 # Bottleneck
                    o = runp(b["c2"], o, True, None)
                    cur = runp(b["c3"], o, True, idt)
            return cur.t
        for b in self.blocks:
            idt = x if b["down"] is None else run(b["down"], x, False, None, ax)[0]
            o, ao = run(b["c1"], x, True, None, ax)
            if b["c3"] is None:                       # BasicBlock
                x, ax = run(b["c2"], o, True, idt, ao)
            else:                                     # Bottleneck
                o, ao = run(b["c2"], o, True, None, ao)
                x, ax = run(b["c3"], o, True, idt, ao)
        return x


class _Step(object):
    __slots__ = ("kind", "module", "conv", "relu", "pool", "U", "U4", "U3", "U2", "Up", "Uph", "bias", "stem", "Wd", "Wr", "Wdr", "Wdr2", "wl1", "bmax")

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)
        self.kind, self.relu, self.pool = "torch", False, False


def _wants(st):
    """Whether a step of the VGG trunk scales its input by max |x| (the fp16-pair forms): the step before it then measures it."""
    return st.U3 is not None or st.U2 is not None or st.Uph is not None or st.Wd is not None


# Which form every layer of a VGG-style trunk takes (the defaults are the measured best; the others are the A/B partners the tests and
# tools/ select through WinogradTrunk(forms={...}) -- no environment variables):
#   conv_direct      1: conv2_1 and conv2_2 as the direct one-kernel convolution on fp16 pairs; 2: conv2_2 only; 0: round 3's F(4x4) forms
#   conv_direct_r    conv2_1 through the register-resident direct kernel (csrc/conv_direct_r.hip); False: the streaming one
#   conv_direct_r2   conv2_2 through the register-resident kernel on output-channel halves (csrc/conv_direct_r.hip, round 6); False: the
#                    kernel with the weights through an LDS ring (csrc/conv_direct_h.hip)
#   stem_direct      conv1_1 + conv1_2 as ONE direct kernel (csrc/conv_stem_direct_h.hip); False: the one-kernel F(4x4) stem
#   wino_stem        conv1_1 folded into conv1_2's kernel at all; False: conv1_1 as its own fp32 kernel
#   fused_h          the one-kernel F(4x4) convolutions on fp16 pairs (csrc/wino_fused_h.hip); False: the f32-input MFMA kernels
#   split16_min_cin  F(4x4) layers from that many input channels on run their 36 products on fp16 pairs (None: 128, or 256 with
#                    split16_h3); 0: plain fp32 library GEMMs everywhere (bench.py's `value_fp32_gemms`)
#   wino_chain       between two pair-product F(4x4) layers on the same map (ReLU, no pool), layer L's output transform and layer L + 1's
#                    input transform as ONE kernel, y_L kept in LDS (csrc/wino_chain.hip); False: the two separate transforms
TRUNK_FORMS = {"conv_direct": 1, "conv_direct_r": True, "conv_direct_r2": True, "stem_direct": True, "wino_stem": True, "fused_h": True, "split16_min_cin": None,
               "wino_chain": True}
# tile columns (ceil(W / 4)) of the maps whose boundaries take the chained transform: the classes measured faster than the output + input
# pair at the 256-frame chunk
CHAIN_TILE_COLS = (5, 16)
FP32_GEMM_FORMS = {"split16_min_cin": 0, "fused_h": False, "wino_stem": False}      # the trunk on plain fp32 library GEMMs


def _pool2_at(mods, i):
    """Whether mods[i] exists and is the MaxPool2d(2, 2) the output transforms and epilogues fuse."""
    p = mods[i] if i < len(mods) else None
    return (isinstance(p, nn.MaxPool2d) and p.kernel_size in (2, (2, 2)) and p.stride in (2, (2, 2))
            and p.padding in (0, (0, 0)) and not p.ceil_mode)


class WinogradTrunk(_Workspace):
    """Runs an nn.Sequential of Conv2d / ReLU / MaxPool2d like `encoder(x)`, with the eligible
    convolutions (+ their ReLU, + their MaxPool2d(2,2)) replaced by the Winograd pipeline or, where one is faster, by a one-kernel
    form of this library (`TRUNK_FORMS`)."""

    def __init__(self, encoder, min_in_channels=256, tile=2, fused64=None, split16_h3=False, forms=None):
        """min_in_channels: 3x3 / stride 1 / pad 1 layers from that many input channels on leave torch.  tile = 2: F(2x2,3x3)
        everywhere; tile = 4: F(4x4,3x3) wherever the batch has enough tiles and the map sides waste little of them (`_f4_fits`;
        F(2x2,3x3) elsewhere), and the one-kernel forms of `TRUNK_FORMS` for the 64- and 128-channel layers.  fused64 (default on): the
        64 -> 64 / 128 channel layers (VGG-16 conv1_2, conv2_1) as ONE kernel instead of transform / GEMM / transform.  split16_h3:
        the F(4x4) products on fp16 pairs as one library GEMM over [vh | vl | vh] (round 1's form, a test partner) instead of this
        library's pair GEMM.  forms: overrides of `TRUNK_FORMS`."""
        super().__init__()
        self.encoder = encoder
        self.min_in_channels = int(min_in_channels)
        self.tile = int(tile)
        self.fused64 = True if fused64 is None else bool(fused64)
        self.fused_min_blocks = 256                  # fewer tile blocks than this (single frames): the three-kernel form
        self.fused_couts = (64, 128)
        # a known bound of max |input| (e.g. a normalised 8-bit image: heads.normalised_image_bound()) spares the stem kernel
        # its pass over the input; None = measured per call
        self.input_bound = None
        self.forms = dict(TRUNK_FORMS)
        self.forms.update(forms or {})
        assert set(self.forms) == set(TRUNK_FORMS), "unknown trunk form"
        # forms['conv_direct'] = 0: conv2_1 / conv2_2 through the F(4x4) forms of round 3 (the A/B partner)
        self.direct128 = int(self.forms["conv_direct"]) != 0
        # input widths that take the direct kernel (conv_direct = 2: conv2_2 only, conv2_1 on the one-kernel F(4x4) form)
        self.direct_cins = (128,) if int(self.forms["conv_direct"]) == 2 else (64, 128)
        self.split16_h3 = bool(split16_h3)
        # split-fp16 GEMMs on the F(4x4) layers from this many input channels on (0 = off: plain fp32 library GEMMs).
        # Default: this library's pair GEMM (`split16_pair_weights`, csrc/wino_gemm.hip) from 128 channels on -- V is no
        # larger than its fp32 form, so every layer the three-kernel form runs gains; with split16_h3 256, the measured optimum
        # of the library GEMM over [vh | vl | vh] (profiles/r01_exp_split16.log)
        self.split16_min_cin = (256 if self.split16_h3 else 128) if self.forms["split16_min_cin"] is None else int(self.forms["split16_min_cin"])
        use_tuned_gemms()
        self.refresh()

    def refresh(self):
        """(Re)build the plan and the transformed weights from the encoder's current parameters."""
        mods = list(self.encoder)
        self.steps = []
        i = 0
        while i < len(mods):
            m = mods[i]
            st = _Step()
            ok = (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1)
                  and m.dilation == (1, 1) and m.groups == 1 and m.in_channels >= self.min_in_channels
                  and m.in_channels % 4 == 0 and m.out_channels % 4 == 0 and m.weight.is_cuda)
            if ok:
                st.kind, st.conv, st.relu, st.pool = "wino", m, False, False
                st.U = wino_weights(m.weight).to(m.weight.device)
                st.U4 = wino_weights(m.weight, 4).to(m.weight.device) if self.tile == 4 else None
                if st.U4 is not None and 0 < self.split16_min_cin <= m.in_channels:
                    if not self.split16_h3 and m.in_channels % 32 == 0 and m.out_channels % 128 == 0:
                        st.U2 = split16_pair_weights(st.U4)
                    else:
                        st.U3 = split16_weights(st.U4)
                if self.fused64 and m.in_channels == 64 and m.out_channels in self.fused_couts:
                    # F(4x4) one-kernel form on the F(4x4) trunk, the F(2x2) one on an F(2x2) trunk
                    t4 = self.tile == 4
                    st.Up = fused64_weights(st.U4 if t4 else st.U)
                    # the fp16-pair form of the one-kernel convolution (csrc/wino_fused_h.hip); forms['fused_h'] = False keeps
                    # the f32-MFMA kernel
                    if t4 and self.forms["fused_h"]:
                        st.Uph = fused64_pair_weights(st.U4)
                if (self.direct128 and self.tile == 4 and m.out_channels == 128 and m.in_channels in self.direct_cins):
                    # VGG-16 conv2_2 (128 -> 128 on 112 x 112 maps, + MaxPool2d): the direct one-kernel form on fp16 pairs
                    # (csrc/conv_direct_h.hip) -- HBM sees the activation in and out, nothing else; the F(4x4) pipeline moved 10 x
                    # the activation there (17 of the pass's 63 GB) and was bound by it: 2.6-2.7 ms against 2.8, -14 GB.  conv2_1
                    # (64 -> 128) stays on the one-kernel F(4x4) form: 1.47 ms against the direct kernel's 1.62 (a quarter of the
                    # multiplications; measured, profiles/r04_v9_direct_conv.log)
                    st.Wd = direct_pair_weights(m.weight)
                    # 64 -> 128 (conv2_1): the register-resident form (csrc/conv_direct_r.hip); forms['conv_direct_r'] = False keeps the one above
                    if m.in_channels == 64 and self.forms["conv_direct_r"]:
                        st.Wdr = direct_r_pair_weights(m.weight)
                    # 128 -> 128 (conv2_2): the register-resident form on output-channel halves
                    if m.in_channels == 128 and self.forms["conv_direct_r2"]:
                        st.Wdr2 = direct_r2_pair_weights(m.weight)
                st.bias = None if m.bias is None else m.bias.detach().to(torch.float32).contiguous()
                # bound of the output, max|x| wl1 + bmax: the scale of a pair-format output (conv2_1 under VGG_PAIRS) and of the next
                # layer's V when the chained transform writes it
                st.wl1, st.bmax = out_bound(m.weight, m.bias)
                i += 1
                if i < len(mods) and isinstance(mods[i], nn.ReLU):
                    st.relu = True
                    i += 1
                    if _pool2_at(mods, i):
                        st.pool = True
                        i += 1
            elif (isinstance(m, nn.Conv2d) and m.in_channels == 3 and m.kernel_size == (3, 3) and m.stride == (1, 1)
                  and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1 and m.out_channels % 16 == 0
                  and m.out_channels <= 512 and m.weight.is_cuda and not (i + 2 < len(mods) and isinstance(
                      mods[i + 1], nn.ReLU) and isinstance(mods[i + 2], nn.MaxPool2d))):
                # first layer: hand-written direct convolution, bias + ReLU fused, planar input -> NHWC
                st.kind, st.conv = "c3", m
                st.U = m.weight.detach().to(torch.float32).permute(1, 2, 3, 0).reshape(27, m.out_channels).contiguous()
                st.bias = None if m.bias is None else m.bias.detach().to(torch.float32).contiguous()
                i += 1
                if i < len(mods) and isinstance(mods[i], nn.ReLU):
                    st.relu = True
                    i += 1
            elif (isinstance(m, nn.Conv2d) and m.groups == 1 and m.out_channels % 4 == 0 and m.bias is not None
                  and m.weight.is_cuda and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)):
                # direct convolution without its bias, then bias + ReLU (+ MaxPool) in one HIP pass
                st.kind, st.conv, st.relu = "direct", m, True
                st.bias = m.bias.detach().to(torch.float32).contiguous()
                i += 2
                if _pool2_at(mods, i):
                    st.pool = True
                    i += 1
            else:
                st.kind, st.module = "torch", m
                i += 1
            self.steps.append(st)
        # first layer (3 -> 64, ReLU) followed by a one-kernel fp16-pair layer (64 -> 64, ReLU): both in ONE kernel, the
        # 64-channel map between them never reaches HBM (csrc/wino_fused_h.hip, STEM; forms['wino_stem'] = False keeps them apart)
        if self.forms["wino_stem"]:
            for a, b in zip(self.steps, self.steps[1:]):
                if (a.kind == "c3" and a.relu and a.conv.out_channels == 64 and b.kind == "wino" and b.Uph is not None
                        and b.relu and b.conv.out_channels == 64):
                    a.stem = stem_pair_weights(a.conv.weight)
                    # the direct one-kernel form of the pair (csrc/conv_stem_direct_h.hip); forms['stem_direct'] = False keeps the F(4x4) one
                    if self.forms["stem_direct"]:
                        a.Wr = stem_direct_pair_weights(b.conv.weight)
        return self

    def _chain_len(self, k, B, H, W):
        """How many steps from step k on run as one chain (1: step k alone): consecutive layers that all take the pair-product branch
        of `wino_conv3x3` on the same map, every one but the last with ReLU and neither pool nor Z form."""
        if not (self.forms["wino_chain"] and _f4_fits(B, H, W) and CHAIN_TILE_COLS[0] <= -(-W // 4) <= CHAIN_TILE_COLS[1]):
            return 1
        pair = lambda st_: (st_.kind == "wino" and st_.U2 is not None and st_.Wd is None and st_.Up is None       # noqa: E731
                            and not _z_form(st_.conv.in_channels, st_.conv.out_channels))
        n = 1
        while (k + n < len(self.steps) and pair(self.steps[k + n - 1]) and pair(self.steps[k + n])
               and self.steps[k + n - 1].relu and not self.steps[k + n - 1].pool):
            n += 1
        return n

    def _want(self, slots, j):
        """The slot step j reads max |its input| from, for the step before it to fill (None: no step j, or it scales nothing by it)."""
        return slots[j:j + 1] if j < len(self.steps) and _wants(self.steps[j]) else None

    # One method per case of `__call__`, tried in the order below.  Each takes the step index k, x, whether slots[k] already holds max |x|
    # (`have`) and the slots, and returns None (the case does not take this step at this shape) or (y, whether the slot of the next step
    # to run was filled, how many following steps ran with this one).

    def _stem_pair(self, k, x, slots):
        """conv1_1 + conv1_2 (+ MaxPool2d) as ONE kernel: the direct form or the F(4x4) one."""
        st, (B, _, H, W) = self.steps[k], x.shape
        nxt = self.steps[k + 1] if st.stem is not None else None            # a stem pair has its second layer
        if nxt is None or not (B * -(-H // 16) * -(-W // 16) >= self.fused_min_blocks and not (nxt.pool and (H % 2 or W % 2))
                               and B * H * W * 64 < 2 ** 31):
            return None
        slot = slots[k:k + 1]
        if self.input_bound is not None:
            slot.fill_(float(self.input_bound))
        else:
            _amax_slot(x, slot)
        want = self._want(slots, k + 2)
        if st.Wr is not None:
            y = conv_stem_direct_h(x, st.stem, st.bias, st.Wr, nxt.bias, nxt.pool, slot, want)
        else:
            y = wino_stem64_h(x, st.stem, st.bias, nxt.Uph, nxt.bias, nxt.pool, slot, want)
        return y, want is not None, 1

    def _first_layer(self, k, x, slots):
        """The 3-channel first layer alone: hand-written direct convolution, planar input -> NHWC."""
        st, (B, _, H, W) = self.steps[k], x.shape
        Cout = st.conv.out_channels
        y = _out(B, Cout, H, W, False, x.device)
        want = self._want(slots, k + 1) if Cout == 64 else None
        _lib.check(_lib.load().cslam_conv3x3_c3_amax_dev(_p(x), _p(st.U), _po(st.bias), B, H, W, Cout, int(st.relu), _p(y), _po(want),
                                                         _stream(x)))
        return y, want is not None, 0

    def _torch_direct(self, k, x):
        """torch's convolution without its bias, then bias + ReLU (+ MaxPool2d) in one HIP pass."""
        st = self.steps[k]
        c = st.conv
        x = torch.nn.functional.conv2d(x, c.weight, None, c.stride, c.padding, c.dilation)
        x = x.contiguous(memory_format=torch.channels_last)
        B, Cout, H, W = x.shape
        pool = st.pool and H % 2 == 0 and W % 2 == 0
        y = _out(B, Cout, H, W, True, x.device) if pool else x
        _lib.check(_lib.load().cslam_bias_act_pool_dev(_p(x), _p(st.bias), B, H, W, Cout, 1, int(pool), _p(y), _stream(x)))
        return (torch.nn.functional.max_pool2d(y, 2, 2) if st.pool and not pool else y), None, 0

    def _direct128(self, k, x, have, slots):
        """The direct one-kernel forms with 128 output channels (conv2_1, conv2_2), with the VGG_PAIRS hand-off between the two."""
        st, (B, _, H, W) = self.steps[k], x.shape
        if not (st.Wd is not None and not (st.pool and (H % 2 or W % 2))
                and B * -(-H // 16) * -(-W // 16) >= self.fused_min_blocks and x.numel() % 4 == 0):
            return None
        slot = _amax_slot(x, slots[k:k + 1], have)
        nxt = self.steps[k + 1] if k + 1 < len(self.steps) else None
        if (VGG_PAIRS and st.Wdr is not None and st.relu and not st.pool and nxt is not None and nxt.Wd is not None
                and nxt.Wdr is None and nxt.conv.in_channels == 128 and H * W * 512 < 2 ** 31 - 16
                and not (nxt.pool and (H % 2 or W % 2))):
            # conv2_1 writes pairs, conv2_2 stages them without conversion: both steps here
            bslot = self._buf("vgg_pair_bound", 1, x.device)
            xp = conv3x3_direct_r_pairs(x, st.Wdr, st.bias, st.wl1, st.bmax, slot, bslot)
            want = self._want(slots, k + 2)
            return conv3x3_direct_hp(xp, (B, 128, H, W), bslot, nxt.Wd, nxt.bias, nxt.relu, nxt.pool, want), want is not None, 1
        want = self._want(slots, k + 1)
        if st.Wdr is not None and H * W * 512 < 2 ** 31 - 16:
            y = conv3x3_direct_r(x, st.Wdr, st.bias, st.relu, st.pool, slot, want)
        elif st.Wdr2 is not None and H * W * 512 < 2 ** 31 - 16:
            y = conv3x3_direct_r2(x, st.Wdr2, st.bias, st.relu, st.pool, slot, want)
        else:
            y = conv3x3_direct_h(x, st.Wd, st.bias, st.relu, st.pool, slot, want)
        return y, want is not None, 0

    def _fused64(self, k, x, have, slots):
        """The one-kernel Winograd forms of the 64-channel layers: on fp16 pairs, or the f32-input MFMA kernels."""
        st, (B, _, H, W) = self.steps[k], x.shape
        if st.Up is None or (st.pool and (H % 2 or W % 2)):
            return None
        # one persistent workgroup per compute unit: worth it from one tile block per CU on (a single 224 x 224
        # frame has 196: VGG-16 at B = 1 502 us through it, 459 us through the three-kernel form)
        bh, bw = (16, 16) if st.Up.shape[1] == 36 else (8, 16)
        if B * -(-H // bh) * -(-W // bw) * st.Up.shape[2] // 4 < self.fused_min_blocks:
            return None
        if st.Uph is None or x.numel() >= 2 ** 31:
            return wino_fused64(x, st.Up, st.bias, st.relu, st.pool), None, 0
        slot = _amax_slot(x, slots[k:k + 1], have)
        want = self._want(slots, k + 1)
        return wino_fused64_h(x, st.Uph, st.bias, st.relu, st.pool, slot, want), want is not None, 0

    def _winograd(self, k, x, have, slots):
        """The Winograd pipeline: a chain of n pair-product layers with the chained transform between them (`_chain_len`), or the step
        alone through `wino_conv3x3`."""
        st = self.steps[k]
        n = self._chain_len(k, x.shape[0], x.shape[2], x.shape[3])
        if n == 1:
            want = self._want(slots, k + 1)
            y = wino_conv3x3(self, x, st.U, st.U4, st.bias, st.relu, st.pool, U3=st.U3, U2=st.U2,
                             amax_in=slots[k:k + 1] if have else None, amax_out=want)
            return y, want is not None and self.amax_written, 0
        _amax_slot(x, slots[k:k + 1], have)
        want = self._want(slots, k + n)
        chain = self.steps[k:k + n]
        y = _pair_pipeline(self, x, [(t.U2, t.bias, t.wl1, t.bmax) for t in chain], slots[k:k + n], chain[-1].relu, chain[-1].pool,
                           None, want)
        return y, want is not None, n - 1

    @torch.no_grad()
    def __call__(self, x):
        """x [B,C,H,W] float32 (any memory format) -> [B,C',H',W'] float32, channels_last memory."""
        # one 4-byte slot per step for max |activation| between consecutive split-fp16 layers: slot k holds max |input of
        # step k|, written by the step before it when that step can (first-layer kernel, fused fp16 kernel, F(4x4) output
        # transform); otherwise the consumer makes its own pass over x
        slots = have = None
        if any(_wants(st) for st in self.steps):
            slots = self._buf("amax_slots", len(self.steps) + 1, x.device)
            slots.zero_()
        k = 0
        while k < len(self.steps):
            st = self.steps[k]
            if st.kind == "c3":
                x = x.contiguous()                                   # planar [B,3,H,W]
                x, have, ran = self._stem_pair(k, x, slots) or self._first_layer(k, x, slots)
            else:
                x = x.contiguous(memory_format=torch.channels_last)
                if st.kind == "torch":
                    x, have, ran = st.module(x), None, 0
                elif st.kind == "direct":
                    x, have, ran = self._torch_direct(k, x)
                else:
                    x, have, ran = (self._direct128(k, x, have, slots) or self._fused64(k, x, have, slots)
                                    or self._winograd(k, x, have, slots))
            k += 1 + ran
        return x
