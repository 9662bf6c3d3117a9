"""Plain float64 restatement of the convolution kernels (csrc/conv_direct_*.hip, conv_stem_direct_h.hip, conv_igemm.hip, the F(2x2)
one-kernel form of wino_fused.hip) and the integer input classes on which those kernels must be EXACT.  numpy / torch on the CPU,
no device, no library of this project except `heads.pair_split` (pure torch).

Why exact.  Every activation and weight scale of the pair kernels is a power of two (csrc/pairs.h rules A, B, C; `pair_split`), a
scaled value v is split into hi = fp16(v), lo = fp16(v - hi) (exact to 22 bits), products of fp16 halves are exact in the MFMA's fp32
accumulator, and the kernels sum xh wh + xl wh + xh wl, dropping xl wl only.  With inputs that are integers times a power of two, chosen
so that xl wl is zero everywhere and the sum of the ABSOLUTE values of all products, bias and shortcut stays below 2^24 units, every
product and every partial sum in any order is an integer below 2^24 units: float32 represents all of them, nothing rounds, and the
kernel's output equals the float64 convolution bit for bit.  `premise` computes those facts from the inputs alone;
tests/test_conv_reference_cpu.py proves the consequence by emulating the three-product sum in float32 in several orders."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from cslam_amd.vpr.heads import pair_split

CLASSES = ("ints", "x_lo", "w_lo")


# ---------------------------------------------------------------------------------------------------------------- the reference

def conv64(x, w, bias=None, stride=1, pad=0, relu=False, pool=0, res=None):
    """float64 y = pool(relu(conv(x, w) + bias + res)) -- the order every kernel documents: bias, shortcut, ReLU, pooling.
    x [B,Cin,H,W], w [Cout,Cin,KH,KW], bias [Cout] or None, res (y's un-pooled shape) or None; pool: 0 none, 2 MaxPool2d(2) (flooring),
    3 the ResNet stem's MaxPool2d(3, 2, 1).  Returns a contiguous float64 CPU tensor [B,Cout,Ho,Wo]."""
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()  # noqa: E731
    x, w = t(x), t(w)
    small = 2.0 * x.shape[0] * x.shape[2] * x.shape[3] * w.numel() / (stride * stride) < 2e8
    threads = torch.get_num_threads()
    if small and threads > 1:
        torch.set_num_threads(1)                           # most maps here are a few pixels: waking the thread pool costs more than the sums
    try:
        y = F.conv2d(x, w, t(bias), stride=stride, padding=pad)
    finally:
        if small and threads > 1:
            torch.set_num_threads(threads)
    if res is not None:
        y = y + t(res)
    if relu:
        y = y.relu()
    if pool == 2:
        y = F.max_pool2d(y, 2)
    elif pool == 3:
        y = F.max_pool2d(y, 3, 2, 1)
    else:
        assert pool == 0
    return y.contiguous()


# ---------------------------------------------------------------------------------------------------------------- input classes

def _pow2(rng):
    return 2.0 ** int(rng.integers(-9, 7))


def _lo_values(rng, shape, sh, bmax):
    """a 2^sh + b, a in {-1, 0, 1}, b in [-bmax, bmax]: with sh >= 11 the fp16 rounding of every |a| = 1 value whose b is not a multiple
    of 2^(sh - 10) leaves a remainder, whatever power of two scales the tensor."""
    a = rng.integers(-1, 2, size=shape)
    b = rng.integers(-bmax, bmax + 1, size=shape)
    v = a * (1 << sh) + b
    flat = v.reshape(-1)
    flat[0] = (1 << sh) + bmax                           # the class's maximum is always present: the scale is the same for every seed
    return v


@functools.lru_cache(maxsize=8)
def _shared_weights(wseed, wshape, lo, sh, wm):
    """(integer weights, their power of two) of a weight seed: drawn once for all the cases that share it"""
    rngw = np.random.default_rng(wseed)
    w = _lo_values(rngw, wshape, sh, 15) if lo else rngw.integers(-wm, wm + 1, size=wshape)
    w.setflags(write=False)
    return w, _pow2(rngw)


def make_case(cls, shape, seed, stride=1, pad=1, bias=True, res=False, bits=24, k_eff=None, w_mult=1, wseed=None, distinct=None):
    """One exact case.  shape = (B, Cin, H, W, Cout, KH, KW); returns a dict of float32 torch CPU tensors x [B,Cin,H,W], w
    [Cout,Cin,KH,KW], bias [Cout] | None, res [B,Cout,Ho,Wo] | None and the two powers of two px, pw the tensors were multiplied by.
    cls (the issue's table): `ints` x in [-15, 15], w in [-2, 2]; `x_lo` x = a 2^sh + b (sh = 11 for even seeds, 12 for odd ones), w in
    [-2, 2]; `w_lo` x in [-15, 15], w = a 2^sh + b.  The ranges shrink so that K max|x| max|w| + 200 < 2^bits (K = Cin KH KW, or k_eff
    where the kernel's intermediate sums are larger than the convolution's; bits = 22 for pair-format outputs): the worst case, so
    `premise` holds for every seed.  Where the 2^12 form does not fit even with the other operand in [-1, 1] -- K (2^12 + 19) >= 2^bits:
    K = 1152 with a pair-format output (the 128 -> 128 layers of conv_igemm_p) and the F(2x2) form -- odd seeds take sh = 11 as well; the
    exponent used comes back as `sh`.  distinct: the batch repeats its first `distinct` images (image b = image b mod distinct; the
    many-block launches: the reference of the distinct images serves all of them).  w_mult: the weights are multiplied by it (4 for the
    F(2x2) form: G g G^T then has no fractions).
    Every element is drawn on its own from a seeded generator -- no separable pattern that a transposed index would survive.  wseed (of
    the seed's parity): the weights and their power of two come from a generator of their own, so that cases which differ in the map
    only share one weight tensor (and a test its packed form)."""
    Bfull, Cin, H, W, Cout, KH, KW = shape
    B = Bfull if distinct is None else min(distinct, Bfull)
    rng = np.random.default_rng(seed)
    assert wseed is None or (wseed - seed) % 2 == 0
    wshape = (Cout, Cin, KH, KW)
    draw_w = lambda lo, sh, wm: (_lo_values(rng, wshape, sh, 15) if lo else rng.integers(-wm, wm + 1, size=wshape), None) \
        if wseed is None else _shared_weights(wseed, wshape, lo, sh, wm)    # noqa: E731
    K = k_eff if k_eff is not None else Cin * KH * KW
    budget = (1 << bits) - 200
    sh = 11 + (seed & 1)
    if cls == "ints":
        xm, wm = 15, 2
        while K * xm * wm * w_mult > budget:
            xm -= 1
        assert xm >= 1
        x = rng.integers(-xm, xm + 1, size=(B, Cin, H, W))
        w, pw = draw_w(False, 0, wm)
    elif cls == "x_lo":
        top = (1 << sh) + 15 + (1 << (sh - 10))          # |xh| + |xl| <= |x| + 2 |xl|
        wm = min(2, budget // (K * top * w_mult))
        if wm < 1:
            sh = 11
            top = (1 << sh) + 15 + 2
            wm = min(2, budget // (K * top * w_mult))
        assert wm >= 1, "x_lo does not fit: K = %d, %d bits" % (K, bits)
        x = _lo_values(rng, (B, Cin, H, W), sh, 15)
        w, pw = draw_w(False, 0, wm)
    elif cls == "w_lo":
        top = ((1 << sh) + 15 + (1 << (sh - 10))) * w_mult
        xm = min(15, budget // (K * top))
        if xm < 1:
            sh = 11
            top = ((1 << sh) + 15 + 2) * w_mult
            xm = min(15, budget // (K * top))
        assert xm >= 1, "w_lo does not fit: K = %d, %d bits" % (K, bits)
        x = rng.integers(-xm, xm + 1, size=(B, Cin, H, W))
        w, pw = draw_w(True, sh, 0)
    else:
        raise ValueError(cls)
    x.reshape(-1)[-1] = np.abs(x).max()                   # ... and so does max |x| sit in the last pixel of the last image (a ragged block)
    px = _pow2(rng)
    pw = _pow2(rng) if pw is None else pw
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    out = {"x": torch.from_numpy((x * px).astype(np.float32)), "w": torch.from_numpy((w * (w_mult * pw)).astype(np.float32)),
           "bias": None, "res": None, "px": px, "pw": pw, "stride": stride, "pad": pad, "sh": sh, "distinct": B}
    if bias:
        out["bias"] = torch.from_numpy((rng.integers(-100, 101, size=Cout) * (px * pw)).astype(np.float32))
    if res:
        out["res"] = torch.from_numpy((rng.integers(-100, 101, size=(B, Cout, Ho, Wo)) * (px * pw)).astype(np.float32))
    if B < Bfull:
        rep = torch.arange(Bfull) % B
        out["x"] = out["x"][rep]
        if res:
            out["res"] = out["res"][rep]
    return out


def make_stem_case(cls, B, H, W, seed, bias=True, wseed=None, distinct=None):
    """A case of the two-layer stem kernel (conv 3 -> 64 + ReLU, conv 64 -> 64 + ReLU): x0 [B,3,H,W], w1 [64,3,3,3], b1, w2 [64,64,3,3],
    b2.  The classes name the operands that carry a lo half; the others are small integers, chosen so that the first layer's ReLU output
    a1 -- which the kernel splits again -- keeps at most 22 significant bits and the second layer's absolute sums stay below 2^24 units
    (`premise` on both layers; the worst case of these ranges is larger than 2^24, the seeds of the table are checked one by one):
      ints  x0 in [-3, 3], w1 in [-1, 1], b1 in [-5, 5] (a1 <= 86: no lo half), w2 in [-2, 2];
      x_lo  x0 = a 2^11 + b, w1, w2 in [-1, 1]: the image's lo half and a1's (up to 16 bits);
      w_lo  even seeds: w2 = a 2^11 + b on the small a1 of `ints`; odd seeds: w1 = a 2^11 + b with x0, w2 in [-1, 1].
    distinct: as `make_case`."""
    Bfull, B = B, B if distinct is None else min(distinct, B)
    rng = np.random.default_rng(seed)
    rngw = rng if wseed is None else np.random.default_rng(wseed)          # as `make_case`
    assert wseed is None or (wseed - seed) % 2 == 0
    small = lambda m, s: rng.integers(-m, m + 1, size=s)    # noqa: E731
    smallw = lambda m, s: rngw.integers(-m, m + 1, size=s)  # noqa: E731
    if cls == "ints":
        x0, w1, w2 = small(3, (B, 3, H, W)), smallw(1, (64, 3, 3, 3)), smallw(2, (64, 64, 3, 3))
    elif cls == "x_lo":
        x0, w1, w2 = _lo_values(rng, (B, 3, H, W), 11, 15), smallw(1, (64, 3, 3, 3)), smallw(1, (64, 64, 3, 3))
    elif cls == "w_lo" and seed % 2 == 0:
        x0, w1, w2 = small(3, (B, 3, H, W)), smallw(1, (64, 3, 3, 3)), _lo_values(rngw, (64, 64, 3, 3), 11, 15)
    elif cls == "w_lo":
        x0, w1, w2 = small(1, (B, 3, H, W)), _lo_values(rngw, (64, 3, 3, 3), 11, 15), smallw(1, (64, 64, 3, 3))
    else:
        raise ValueError(cls)
    x0.reshape(-1)[-1] = np.abs(x0).max()
    px, p1, p2 = _pow2(rng), _pow2(rngw), _pow2(rngw)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).astype(np.float32))    # noqa: E731
    x0 = f(x0 * px)
    if B < Bfull:
        x0 = x0[torch.arange(Bfull) % B]
    return {"x0": x0, "distinct": B, "w1": f(w1 * p1), "w2": f(w2 * p2),
            "b1": f(small(5, 64) * (px * p1)) if bias else None, "b2": f(small(100, 64) * (px * p1 * p2)) if bias else None}


def ints(shape, seed, **kw):
    return make_case("ints", shape, seed, **kw)


def x_lo(shape, seed, **kw):
    return make_case("x_lo", shape, seed, **kw)


def w_lo(shape, seed, **kw):
    return make_case("w_lo", shape, seed, **kw)


# ---------------------------------------------------------------------------------------------------------------- the premise

def act_split(x):
    """The kernels' split of an activation, restated: s = the power of two of rule B (max|x| s <= 32752), v = float32(s x), hi =
    fp16(v), lo = fp16(v - hi).  Rules A and C and a bound in the slot give another power of two: the halves scale with it (fp16 keeps 11
    bits at every exponent these values reach), so hi / s and lo / s are the same.  Returns (hi / s, lo / s) in float64."""
    x = torch.as_tensor(x).double()
    amax = float(x.abs().max())
    s = 2.0 ** math.floor(math.log2(32752.0 / amax)) if amax > 0 else 1.0
    v = (x * s).float()
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double() / s, lo.double() / s


def unit_of(*tensors):
    """The largest power of two that divides every value of the tensors (float64)."""
    u = None
    for t in tensors:
        if t is None:
            continue
        a = torch.as_tensor(t).double().abs().reshape(-1)
        a = a[a > 0]
        if a.numel() == 0:
            continue
        m, e = torch.frexp(a)                              # a = m 2^e, m in [0.5, 1): 53 bits
        bits = (m * 2.0 ** 53).to(torch.int64)
        tz = torch.log2((bits & -bits).double()).to(torch.int64)          # trailing zeros of the 53-bit significand
        ue = int((e.to(torch.int64) - 53 + tz).min())
        u = ue if u is None else min(u, ue)
    return None if u is None else 2.0 ** u


def premise(x, w, bias=None, res=None, stride=1, pad=0):
    """The facts that make a case exact, from the inputs alone (float64): a dict with
    unit       the power of two all of x w, bias and res are multiples of,
    max_units  max over the outputs of (sum (|xh| + |xl|) (|wh| + |wl|) + |bias| + |res|) / unit: a bound of every partial sum of the
               three products in any order, and of the result,
    split      hi + lo == v exactly for the host split of w (`pair_split`) and the restated split of x,
    lolo_zero  xl wl == 0 for every pair of operands that meet in a product (here: one of the two lo tensors is all zero),
    ok         max_units < 2^24 and split and lolo_zero."""
    x64, w64 = torch.as_tensor(x).double(), torch.as_tensor(w).double()
    xh, xl = act_split(x64)
    wh, wl, inv_s = pair_split(w64)
    wh, wl = wh.double() * inv_s, wl.double() * inv_s
    split = bool(torch.equal(xh + xl, x64) and torch.equal(wh + wl, w64))
    lolo_zero = bool((xl == 0).all() or (wl == 0).all())
    unit = (unit_of(x64) or 1.0) * (unit_of(w64) or 1.0)
    ubr = unit_of(bias, res)
    aligned = ubr is None or ubr >= unit                   # bias and shortcut are multiples of the products' unit
    mag = F.conv2d(xh.abs() + xl.abs(), wh.abs() + wl.abs(), None if bias is None else torch.as_tensor(bias).double().abs(),
                   stride=stride, padding=pad)
    if res is not None:
        mag = mag + torch.as_tensor(res).double().abs()
    max_units = float(mag.max()) / unit
    return {"unit": unit, "max_units": max_units, "split": split, "lolo_zero": lolo_zero, "aligned": bool(aligned),
            "x_lo_nonzero": int((xl != 0).sum()), "w_lo_nonzero": int((wl != 0).sum()),
            "ok": bool(max_units < 2 ** 24 and split and lolo_zero and aligned)}


def wino2_premise(x, w, bias=None, res=None):
    """Exactness of the float32 F(2x2, 3x3) form (csrc/wino_fused.hip) on a case: B^T and A^T hold 0 and +-1, G halves -- with weights
    that are multiples of 4 units U = G g G^T is a multiple of the unit, and the form is exact when the absolute sums of its three stages
    stay below 2^24 units: |B^T| |d| |B|, sum_c |U_c| |V_c|, and |A^T| (sum_c |U_c| |V_c|) |A| + |bias| + |res|.  Returns the dict of
    `premise` (max_units over the three stages; `split` = U is a multiple of the unit)."""
    import wino_reference as wr
    x64, w64 = torch.as_tensor(x).double(), torch.as_tensor(w).double()
    BT, AT, G = wr.matrices(2)
    ux, uw = unit_of(x64) or 1.0, (unit_of(w64) or 4.0) / 4.0
    U = np.einsum("ik,ockl,jl->ijco", G, w64.numpy(), G).reshape(16, w64.shape[1], w64.shape[0])       # [16, Cin, Cout]
    split = bool(np.array_equal(np.round(U / uw), U / uw))
    V, mag = wr.input_transform(x64.permute(0, 2, 3, 1).numpy(), 2)                                     # [16, T, Cin]
    m = np.einsum("ftc,fco->fto", mag, np.abs(U))                                                       # sum_c |U| (|B^T| |d| |B|) >= sum_c |U| |V|
    A = np.abs(AT)
    n, T, Co = m.shape
    out = np.einsum("pi,ijto,qj->pqto", A, m.reshape(4, 4, T, Co), A)
    extra = 0.0
    if bias is not None:
        extra += float(torch.as_tensor(bias).double().abs().max())
    if res is not None:
        extra += float(torch.as_tensor(res).double().abs().max())
    unit = ux * uw
    max_units = max(float(mag.max()) / ux, float(m.max()) / unit, (float(out.max()) + extra) / unit)
    return {"unit": unit, "max_units": max_units, "split": split, "lolo_zero": True, "aligned": True,
            "ok": bool(split and max_units < 2 ** 24)}


# ---------------------------------------------------------------------------------------------------------------- the pair format

def scale_c(bound):
    """csrc/pairs.h rule C in float32: the power of two that brings `bound` (clamped to [1e-30, 1e30]) into [2^13, 2^14)."""
    a = np.minimum(np.maximum(np.float32(bound), np.float32(1e-30)), np.float32(1e30))
    _, e = np.frexp(a)
    return float(np.ldexp(np.float32(1.0), 14 - int(e)))


def pack_pairs(y, bound):
    """[B,C,H,W] float32 (C a multiple of 32) -> the pair-format tensor [B,H,W,C/32,2,32] float16: per pixel and 32-channel block the 32
    hi halves then the 32 lo halves of v = float32(s y), s = `scale_c(bound)`: hi = fp16(v), lo = fp16(v - hi)."""
    y = torch.as_tensor(y).float()
    B, C, H, W = y.shape
    assert C % 32 == 0
    v = (y.permute(0, 2, 3, 1) * scale_c(bound)).contiguous()                     # NHWC; a power of two: exact
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.stack((hi.view(B, H, W, C // 32, 32), lo.view(B, H, W, C // 32, 32)), dim=4).contiguous()


def unpack_pairs(t, bound):
    """The inverse: [B,H,W,C/32,2,32] float16 -> [B,C,H,W] float32 (hi + lo) / s (the sum in float64: exact, then rounded once)."""
    B, H, W, nb = t.shape[:4]
    v = (t[:, :, :, :, 0, :].double() + t[:, :, :, :, 1, :].double()) / scale_c(bound)
    return v.reshape(B, H, W, nb * 32).permute(0, 3, 1, 2).float()


def out_bound64(w, bias):
    """(wl1, bmax) of the pair-format bound, restated in float64: the largest L1 norm of one output channel's weights, max |bias|."""
    wl1 = float(torch.as_tensor(w).double().abs().sum(dim=(1, 2, 3)).max())
    return wl1, 0.0 if bias is None else float(torch.as_tensor(bias).double().abs().max())


def bound_formula(xmax, wl1, bmax, rmax=0.0):
    """The pair-format epilogues' bound (max|x| wl1 + bmax + max|res|) 1.001 in float32, as the kernels compute it: the product and the
    first sum as one fused multiply-add or as two roundings (the compiler may contract them) -- both values, as a set."""
    f = np.float32
    two = f(f(f(f(xmax) * f(wl1)) + f(bmax)) + f(rmax)) * f(1.001)
    fused = f(f(f(np.float64(f(xmax)) * np.float64(f(wl1)) + np.float64(f(bmax))) + f(rmax)) * f(1.001))
    return {float(two), float(fused)}


# ---------------------------------------------------------------------------------------------------------------- locating a mismatch

def locate(y, ref, block_h=None, block_w=None, tile=None):
    """None when y equals ref bit for bit (as float32 values), else a dict: `first` = the first differing (b, h, w, co) in NHWC order, the
    two values there, `count` of differing elements (and of pixels), `block` = (b, h // block_h, w // block_w) of the first one, or with
    `tile` its index in the flat [B][H][W] pixel order divided by the tile size; `channels` = the output channels that differ anywhere."""
    y, ref = torch.as_tensor(y).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    assert y.shape == ref.shape, (tuple(y.shape), tuple(ref.shape))
    yv, rv = y.permute(0, 2, 3, 1).contiguous().double(), ref.permute(0, 2, 3, 1).contiguous().double()
    bad = (yv != rv) | (torch.isnan(yv) != torch.isnan(rv))
    if not bool(bad.any()):
        return None
    idx = torch.nonzero(bad)
    b, h, w, co = (int(v) for v in idx[0])
    B, H, W, C = yv.shape
    out = {"first": (b, h, w, co), "got": float(yv[b, h, w, co]), "want": float(rv[b, h, w, co]), "count": int(idx.shape[0]),
           "of": int(bad.numel()), "pixels": int(bad.any(dim=3).sum()), "channels": sorted(set(int(c) for c in idx[:, 3].unique()))[:16]}
    if block_h and block_w:
        out["block"] = (b, h // block_h, w // block_w)
    if tile:
        out["tile"] = ((b * H + h) * W + w) // tile
    return out
