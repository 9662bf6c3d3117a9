"""Bit-exact GPU tests of the convolution kernels (-m gpu): the direct forms (csrc/conv_direct_h.hip, conv_direct_r.hip,
conv_direct_p.hip, conv_stem_direct_h.hip), the implicit GEMM and the pooled stem (conv_igemm.hip) and the float32 F(2x2) one-kernel form
(wino_fused.hip), one entry point at a time, against the float64 convolution of tests/conv_reference.py -- with no tolerance.

On the integer input classes of conv_reference (`ints`, `x_lo`, `w_lo`) every product and every partial sum of these kernels is an
integer below 2^24 units, so nothing rounds and the output must equal the float64 result at every element
(tests/test_conv_reference_cpu.py proves that from the reference alone, for every case of the table below).  A wrong tap, pad,
swizzled chunk, tile edge, dropped channel group or stale buffer therefore fails, and `locate` names the element and its block.

The table: per entry point the shared maps (B x H x W; with pooling even ones), then the maps at which that kernel's own edges exist
-- one block, one block plus a row / a column, halves that straddle rows and images, pixel tiles minus / plus one pixel and across
images -- and for every persistent kernel one launch of 16 x 16 maps with more blocks than twice its workgroup count (the count as the
launcher derives it from the compute units; N_CU_NOMINAL where no device is there to ask; its images repeat with period DISTINCT, so
one reference of 61 images serves it).  Bias (present / NULL) and ReLU follow a map's place in the entry's list, so that every entry and
every pooling mode of it has both; the x_lo / w_lo exponent (2^11 / 2^12) follows the map, except where 2^12 does not fit -- the 128 ->
128 conv_igemm_p entries with pair-format output and the F(2x2) entries take 2^11 throughout (conv_reference.make_case).  Entries that
take the same operands meet the same tensors (one reference); every launch is repeated and must repeat its bits.

The one-kernel F(4x4) forms (G holds 1/6: not exact) get a per-element bound instead, and the CosPlace head (gem_fc_kernel,
gem_fc_nhwc_kernel) a float64 comparison over its sizes: at the end of this file."""
import collections
import ctypes as C

import numpy as np
import pytest

import conv_reference as cr
import wino_reference as wr

pytestmark = pytest.mark.gpu

N_CU_NOMINAL = 256                       # MI355X; the GPU tests ask the device

NOPOOL = [(1, 1, 1), (2, 5, 7), (3, 9, 2), (1, 3, 61), (1, 17, 33)]
POOL = [(1, 2, 2), (2, 6, 10), (1, 16, 16), (1, 18, 34)]

Entry = collections.namedtuple("Entry", "name family cin cout k stride pad pools relus res bits block tile maps pmaps per_image opts")
Case = collections.namedtuple("Case", "entry kind cls shape stride pad bias res relu pool bits seed w_mult k_eff wseed distinct")


def _entry(name, family, cin, cout, k=3, stride=1, pad=1, pools=(0,), relus=(True, False), res=False, bits=24, block=None, tile=None,
           maps=(), pmaps=(), per_image=None, **opts):
    return Entry(name, family, cin, cout, k, stride, pad, pools, relus, res, bits, block, tile, list(maps), list(pmaps), per_image, opts)


B16 = [(1, 16, 16), (1, 17, 16), (1, 16, 17), (2, 16, 33)]                 # 16 x 16 blocks: one, + a row, + a column, three columns
B8 = [(1, 8, 16), (1, 9, 16), (1, 8, 17), (2, 8, 33)]                      # 8 x 16 blocks
B8P = [(1, 8, 16), (1, 10, 16), (1, 8, 18)]
HALVES = [(1, 8, 16), (1, 8, 8), (1, 8, 24), (1, 9, 16), (3, 8, 8), (2, 16, 56), (1, 8, 17)]   # two 8 x 8 halves a block: 1, 1/2, 1 1/2 blocks;
#                                                                            halves that pair across block rows (56 = 7 halves) and images
TILES = [(1, 8, 16), (1, 1, 127), (1, 3, 43), (5, 7, 7), (2, 5, 130), (65, 16, 16)]   # 128-pixel tiles: 1, - 1, + 1 pixel, across images,
#                                                                            a row longer than a tile, 16 640 pixels (past 16 384)
TILES_S2 = [(1, 16, 32), (1, 2, 254), (1, 6, 86), (5, 14, 14), (2, 9, 260), (17, 64, 64)]    # the same output maps at stride 2 (17: 17 408 px)
T256_S2 = [(1, 31, 31), (1, 5, 169), (1, 1, 513)]                          # 1x1 / 2: 256, 255 and 257 output pixels (the 256-pixel tiles)
STEM_POOL = [(1, 16, 32), (1, 32, 32), (2, 32, 64), (1, 48, 96), (3, 16, 64)]          # output maps of 8 x 16 tiles: 1, 2 x 1, 2 x 2, 3 x 3, 1 x 2

# F(2x2): the worst case of the form's absolute sums is 9 x 64 x 4 max|x| x 2.25 max|w| (K = 5184), which no x_lo / w_lo range fits; the
# ranges are shrunk for K = 1800 and `wino2_premise` checks the actual sums of every case of the table
WINO2_K = 1800

ENTRIES = []
for _c in (32, 64, 128):
    # (all the block-edge maps at 32 input channels; more channels are more passes of the same K loop: the shared maps and two ragged ones)
    _m, _pm = (B16, [(1, 18, 16), (2, 16, 34)]) if _c == 32 else ([(1, 17, 16), (2, 16, 33)], [(2, 16, 34)])
    for _f in ("direct_h", "direct_hp"):
        ENTRIES.append(_entry("%s_c%d" % (_f, _c), _f, _c, 128, pools=(0, 2), block=(16, 16), maps=_m, pmaps=_pm, per_image=1 if _c == 32 else None))
ENTRIES += [
    _entry("direct_r", "direct_r", 64, 128, pools=(0, 2), block=(8, 16), maps=B8, pmaps=B8P, per_image=2),
    _entry("direct_r2", "direct_r2", 128, 128, pools=(0, 2), block=(8, 16), maps=B8, pmaps=B8P, per_image=2),
    _entry("direct_r_pairs", "direct_r_pairs", 64, 128, relus=(True,), bits=22, block=(8, 16), maps=B8, per_image=2),
    _entry("stem_direct", "stem_direct", 3, 64, pools=(0, 2), relus=(True,), block=(8, 16), maps=B8, pmaps=B8P, per_image=2),
    _entry("stem_pool_patch", "stem_pool", 3, 64, k=7, stride=2, pad=3, pools=(3,), relus=(True,), block=(8, 16), pmaps=STEM_POOL, per_image=1),
    _entry("stem_pool_igemm", "stem_pool", 3, 128, k=3, stride=2, pad=1, pools=(3,), relus=(True,), block=(8, 16), pmaps=STEM_POOL),
    _entry("wino2_c64", "wino2", 64, 64, pools=(0, 2), block=(8, 16), maps=B8, pmaps=B8P, per_image=2, w_mult=4, k_eff=WINO2_K),
    _entry("wino2_c128", "wino2", 64, 128, pools=(0, 2), block=(8, 16), maps=B8[3:], pmaps=B8P[1:2], per_image=4, w_mult=4, k_eff=WINO2_K),
    _entry("wino2_c64_res", "wino2", 64, 64, res=True, block=(8, 16), maps=B8, w_mult=4, k_eff=WINO2_K),
    _entry("igemm_stem7", "igemm", 3, 64, k=7, stride=2, pad=3, tile=128, maps=TILES_S2[:5] + [(2, 37, 53)]),
    _entry("igemm_3x3s2", "igemm", 64, 128, k=3, stride=2, pad=1, tile=128, maps=TILES_S2[:5]),
    _entry("igemm_1x1s2", "igemm", 64, 128, k=1, stride=2, pad=0, tile=128, maps=TILES_S2[:5]),
    _entry("igemm_3x3s1_res", "igemm", 128, 128, res=True, tile=128, maps=TILES[:5]),
    _entry("igemm_3x3s1_c64", "igemm", 64, 64, res=True, tile=128, maps=TILES[:5]),
    _entry("igemm_3x3s2_c256", "igemm", 128, 256, k=3, stride=2, pad=1, tile=128, maps=TILES_S2[:5]),
]
# (name, cin, cout, k, stride, pad, x format, shortcut, output format); the launcher's forms: shared kernel rows (3x3 / 1, pair input or
# float32 input with pair output) on 128 x 128 and 128 x 64 tiles, 256 x 64 tiles (pair input, 64 channels, no shared rows), the rest
for _n, _ci, _co, _k, _s, _p, _xf, _rf, _of in [
        ("igemm_p_kws128", 128, 128, 3, 1, 1, "pairs", "pairs", "pairs"), ("igemm_p_kws64", 64, 64, 3, 1, 1, "pairs", "f32", "f32"),
        ("igemm_p_open", 64, 64, 3, 1, 1, "f32", None, "pairs"), ("igemm_p_tm256", 64, 64, 1, 2, 0, "pairs", None, "pairs"),
        ("igemm_p_s2", 64, 128, 3, 2, 1, "pairs", None, "f32"), ("igemm_p_1x1_c256", 128, 256, 1, 2, 0, "pairs", None, "pairs"),
        ("igemm_p_kws128_f32res", 128, 128, 3, 1, 1, "pairs", "f32", "pairs")]:
    _big = _n in ("igemm_p_kws128", "igemm_p_tm256")                                   # these two also take the 16 640 / 17 408-pixel launch
    ENTRIES.append(_entry(_n, "igemm_p", _ci, _co, k=_k, stride=_s, pad=_p, res=_rf is not None, bits=22 if _of == "pairs" else 24,
                          tile=256 if _n == "igemm_p_tm256" else 128,
                          maps=[] if _n == "igemm_p_kws128_f32res" else                               # (igemm_p_kws128's kernel: the shared maps)
                          (TILES if _s == 1 else TILES_S2)[:6 if _big else 5] + (T256_S2 if _n == "igemm_p_tm256" else []),
                          xf=_xf, rf=_rf, of=_of))
for _xf, _rf, _of in [("f32", None, "f32"), ("f32", None, "pairs"), ("pairs", None, "f32"), ("pairs", None, "pairs"), ("pairs", "pairs", "f32"),
                      ("pairs", "pairs", "pairs"), ("pairs", "f32", "f32"), ("pairs", "f32", "pairs")]:
    _full = (_xf, _rf, _of) in (("f32", None, "pairs"), ("pairs", None, "f32"), ("pairs", "pairs", "pairs"), ("pairs", "f32", "f32"))
    # (every input, shortcut and output format once on all the half-block maps; the other four combinations differ in the epilogue only)
    ENTRIES.append(_entry("direct_p_%s_%s_%s" % (_xf, _rf or "nores", _of), "direct_p", 64, 64, res=_rf is not None,
                          bits=22 if _of == "pairs" else 24, block=(8, 8), maps=HALVES if _full else [(1, 8, 24), (3, 8, 8)],
                          per_image=2 if (_xf, _rf, _of) in
                          (("f32", None, "pairs"), ("pairs", "pairs", "pairs")) else None, xf=_xf, rf=_rf, of=_of))
ENTRY = {e.name: e for e in ENTRIES}
PERSISTENT_CLASS = "w_lo"                # the class of the many-block launches (one case per persistent kernel)
DISTINCT = 61                            # ... whose images repeat with this period: a prime, so that no two blocks a workgroup meets in a row
#                                          (its stride is the workgroup count or an eighth of it) and no two neighbours hold the same image; the
#                                          reference of 61 images serves the launch, and the data do not depend on the device's CU count


def persistent_images(e, n_cu):
    """Images of 16 x 16 (the stem-pool form: of 32 x 32, a 16 x 16 output map) that give more blocks than twice the workgroup count of
    the launch: every launcher here starts min(blocks, n_cu) workgroups (conv_direct_r2: n_cu workgroups = n_cu / 2 block streams).
    per_image = the blocks of one image (the stem-pool patch form: two tiles an image, and a workgroup takes two tiles at a time: 1; the
    F(2x2) form with 128 output channels: two blocks of 8 x 16 pixels times two channel halves)."""
    return (2 * n_cu) // e.per_image + 1


def _sig(e):
    """What the inputs of an entry's cases depend on: entries with the same signature are run on the same tensors (one reference)."""
    return (e.family == "stem_direct", e.cin, e.cout, e.k, e.stride, e.pad, e.bits, e.res, e.opts.get("w_mult", 1), e.opts.get("k_eff"))


SIGS = sorted(set(_sig(e) for e in ENTRIES), key=repr)
CLS_SEED = {"ints": 0, "x_lo": 100003, "w_lo": 200003}


def cases(e, cls, n_cu=N_CU_NOMINAL):
    """The cases of entry e in class cls: every map of its table plus its persistent one.  ReLU, bias and the seed (so the x_lo / w_lo
    exponent) follow from the map, so that entries of one signature meet the same inputs; an entry's weights are two tensors per class
    (one per exponent)."""
    out = []
    base = 7919 * (SIGS.index(_sig(e)) + 1) + CLS_SEED[cls]
    kind = "stem" if e.family == "stem_direct" else "conv"

    def add(B, H, W, pool, relu, bias, m, distinct=None):
        seed = base + 31 * m
        out.append(Case(e.name, kind, cls, (B, e.cin, H, W, e.cout, e.k, e.k), e.stride, e.pad, bias, e.res, relu, pool, e.bits, seed,
                        e.opts.get("w_mult", 1), e.opts.get("k_eff"), 2 * base + 1000002 + (seed & 1), distinct))

    for pool in e.pools:
        own = e.pmaps if pool else e.maps
        shared = [] if e.family == "stem_pool" else (POOL if pool else NOPOOL)       # (the pooled stem: maps of whole 8 x 16 tiles only)
        for j, (B, H, W) in enumerate(shared + own):
            # by the map's place in the list, so that every entry and every pooling mode of it runs with and without a bias and, where
            # the entry point has the choice, with and without ReLU (a shared map has the same place, so the same inputs, in every entry)
            add(B, H, W, pool, e.relus[j % len(e.relus)], j % 3 != 1, 131 * B + 17 * H + W)
        mine = [c for c in out if c.pool == pool]
        assert {c.bias for c in mine} == {True, False} and {c.relu for c in mine} == set(e.relus), e.name
    if e.per_image and cls == PERSISTENT_CLASS:
        hw = 32 if e.family == "stem_pool" else 16
        add(persistent_images(e, n_cu), hw, hw, e.pools[-1], True, True, 977, DISTINCT)
    return out


_BUILT = {}


def build(case):
    """(inputs, float64 reference) of a case: the inputs of conv_reference, the reference of `conv64` (the stem: both layers).  Computed
    once for the entries that share them (kept for the class being run)."""
    key = case._replace(entry="")
    if key in _BUILT:
        return _BUILT[key]
    if _BUILT and next(iter(_BUILT)).cls != case.cls:
        _BUILT.clear()
    B, cin, H, W, cout, kh, kw = case.shape
    if case.kind == "stem":
        t = cr.make_stem_case(case.cls, B, H, W, case.seed, bias=case.bias, wseed=case.wseed, distinct=case.distinct)
        d = t["distinct"]
        a1 = cr.conv64(t["x0"][:d], t["w1"], t["b1"], 1, 1, relu=True)
        ref = cr.conv64(a1, t["w2"], t["b2"], 1, 1, relu=True, pool=case.pool)
    else:
        t = cr.make_case(case.cls, case.shape, case.seed, stride=case.stride, pad=case.pad, bias=case.bias, res=case.res, bits=case.bits,
                         k_eff=case.k_eff, w_mult=case.w_mult, wseed=case.wseed, distinct=case.distinct)
        d = t["distinct"]
        ref = cr.conv64(t["x"][:d], t["w"], t["bias"], case.stride, case.pad, relu=case.relu, pool=case.pool,
                        res=None if t["res"] is None else t["res"][:d])
    if d < B:                                               # image b = image b mod d, and so is its reference
        ref = ref[np.arange(B) % d].contiguous()
    _BUILT[key] = t, ref
    return _BUILT[key]


# ---------------------------------------------------------------------------------------------------------------- running a case

class _Env(object):
    def __init__(self):
        import torch
        from cslam_amd import _lib
        from cslam_amd.vpr import winograd as wg
        self.torch, self._lib, self.lib, self.wg = torch, _lib, _lib.load(), wg
        self.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        self.ws = wg._Workspace()
        self.packed = {}

    def weights(self, case, make):
        """make() on the device, once per weight tensor of the table (the cases of an entry share two per class)"""
        key = (case.entry, case.cls, case.wseed)
        if key not in self.packed:
            self.packed[key] = self.dev(make())
        return self.packed[key]

    def cl(self, t):
        """CPU [B,C,H,W] -> device, channels_last storage"""
        return None if t is None else t.cuda().contiguous(memory_format=self.torch.channels_last)

    def dev(self, t):
        if isinstance(t, tuple):
            return tuple(self.dev(v) for v in t)
        return t.cuda() if self.torch.is_tensor(t) else t

    def slot(self, v=0.0):
        return self.torch.full((1,), float(v), dtype=self.torch.float32, device="cuda")


@pytest.fixture(scope="module")
def E():
    return _Env()


def _same(got, ref64, what, e):
    """got [B,C,H,W] (any device / storage) equals the float64 reference bit for bit; the message names the first element and its block."""
    want = ref64.float()
    assert want.double().equal(ref64), what + ": the reference itself is no float32 number"
    got = got.detach().cpu()
    if got.shape == want.shape and bool((got == want).all()):
        return
    bad = cr.locate(got, want, *(e.block or (None, None)), tile=e.tile)
    assert bad is None, "%s: %d of %d elements differ (%d pixels; channels %s); first at (b, h, w, co) = %s: got %r, reference %r; %s" % (
        what, bad["count"], bad["of"], bad["pixels"], bad["channels"], bad["first"], bad["got"], bad["want"],
        "block %s" % (bad["block"],) if "block" in bad else "tile %s" % bad.get("tile"))


def _pairs_out(E, act, ref64, xmax, wl1, bmax, rmax, what, e):
    """A pair-format result: decodes to the reference exactly (through `unpack_pairs` and through `pairs_to_float`), its halves are the
    canonical split of the scaled reference, its bound slot holds the documented formula and is no smaller than max |ref|."""
    bound = float(act.bound.item())
    top = float(ref64.abs().max())
    assert bound in cr.bound_formula(xmax, wl1, bmax, rmax), (what, bound, cr.bound_formula(xmax, wl1, bmax, rmax))
    assert bound >= top, (what, bound, top)
    t = act.t.cpu()
    want = cr.pack_pairs(ref64.float(), bound)
    if t.numel() <= 1 << 17:                                # (the small maps; tests/test_conv_reference_cpu.py: unpack_pairs(pack_pairs(ref)) == ref)
        assert E.torch.equal(E.wg.pairs_to_float(act).cpu().contiguous(), cr.unpack_pairs(t, bound).contiguous()), what + ": pairs_to_float"
    if E.torch.equal(t.view(E.torch.int16), want.view(E.torch.int16)):
        return
    _same(cr.unpack_pairs(t, bound), ref64, what + " (pairs)", e)
    assert E.torch.equal(t.float(), want.float()), what + ": the halves are not hi = fp16(s y), lo = fp16(s y - hi)"


def _wl1(w, bias):
    """wl1 and bmax as a caller passes them, from the float64 restatement (not from the packers under test)"""
    return cr.out_bound64(w, bias)


def _run(E, case):
    """Launches the case's entry point twice; checks output, slots and repetition."""
    torch, wg = E.torch, E.wg
    e = ENTRY[case.entry]
    t, ref = build(case)
    B, cin, H, W, cout, kh, kw = case.shape
    what = "%s %s B=%d H=%d W=%d relu=%d pool=%d bias=%d seed=%d" % (case.entry, case.cls, B, H, W, case.relu, case.pool, case.bias, case.seed)
    fam = e.family
    relu, pool = case.relu, bool(case.pool)
    if fam == "stem_direct":
        x0 = t["x0"].cuda().contiguous()
        stem, Wr = E.weights(case, lambda: (wg.stem_pair_weights(t["w1"]), wg.stem_direct_pair_weights(t["w2"])))
        b1, b2 = E.dev(t["b1"]), E.dev(t["b2"])
        outs = []
        for _ in range(2):
            so = E.slot()
            outs.append((wg.conv_stem_direct_h(x0, stem, b1, Wr, b2, pool, E.slot(t["x0"].abs().max()), so), so))
        _same(outs[0][0], ref, what, e)
        assert outs[0][1].item() == float(ref.abs().max()), (what, outs[0][1].item(), float(ref.abs().max()))
        assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1].item() == outs[1][1].item(), what + ": the second launch differs"
        return
    x, w, bias, res = t["x"], t["w"], E.dev(t["bias"]), t["res"]
    xmax = float(x.abs().max())
    top = float(ref.abs().max())
    amax = E.slot(xmax)
    if fam in ("direct_h", "direct_hp", "direct_r", "direct_r2"):
        Wp = E.weights(case, lambda: {"direct_h": wg.direct_pair_weights, "direct_hp": wg.direct_pair_weights,
                                      "direct_r": wg.direct_r_pair_weights, "direct_r2": wg.direct_r2_pair_weights}[fam](w))
        xd = E.cl(x)
        bound = E.slot(xmax * (1.5 if case.seed % 2 else 1.0))                     # hp: the pairs may be scaled for a bound above the maximum
        xp = cr.pack_pairs(x, bound.item()).cuda() if fam == "direct_hp" else None
        outs = []
        for _ in range(2):
            so = E.slot()
            if fam == "direct_hp":
                y = wg.conv3x3_direct_hp(xp, (B, cin, H, W), bound, Wp, bias, relu, pool, so)
            else:
                fn = {"direct_h": wg.conv3x3_direct_h, "direct_r": wg.conv3x3_direct_r, "direct_r2": wg.conv3x3_direct_r2}[fam]
                y = fn(xd, Wp, bias, relu, pool, amax, so)
            outs.append((y, so))
        _same(outs[0][0], ref, what, e)
        assert outs[0][1].item() == top, (what, "max |y| slot", outs[0][1].item(), top)
        assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1].item() == outs[1][1].item(), what + ": the second launch differs"
    elif fam == "direct_r_pairs":
        Wr = E.weights(case, lambda: wg.direct_r_pair_weights(w))
        wl1, bmax = _wl1(w, t["bias"])
        xd = E.cl(x)
        outs = []
        for _ in range(2):
            so, sb = E.slot(), E.slot()
            yp = wg.conv3x3_direct_r_pairs(xd, Wr, bias, wl1, bmax, amax, sb, so)
            outs.append(wg.PairAct(yp, True, (B, cout, H, W), so, sb))
        _pairs_out(E, outs[0], ref, xmax, wl1, bmax, 0.0, what, e)
        assert outs[0].amax.item() == top, (what, "max |y| slot", outs[0].amax.item(), top)
        assert torch.equal(outs[0].t, outs[1].t) and outs[0].amax.item() == outs[1].amax.item(), what + ": the second launch differs"
    elif fam == "wino2":
        Up = E.weights(case, lambda: wg.fused64_weights(wg.wino_weights(w, 2)))
        xd, rd = E.cl(x), E.cl(res)
        ys = [wg.wino_fused64(xd, Up, bias, relu, pool, rd) for _ in range(2)]
        _same(ys[0], ref, what, e)
        assert torch.equal(ys[0], ys[1]), what + ": the second launch differs"
    elif fam == "igemm":
        Wg = E.weights(case, lambda: wg.igemm_pair_weights(w))
        xd, rd = E.cl(x), E.cl(res)
        so = E.slot()
        y = wg.conv_igemm(E.ws, xd, Wg, bias, (kh, kw), case.stride, case.pad, relu, rd, amax_out=so)          # max |x| measured by the wrapper
        _same(y, ref, what, e)
        assert so.item() == top, (what, "max |y| slot", so.item(), top)
        s2 = E.slot()
        y2 = wg.conv_igemm(E.ws, xd, Wg, bias, (kh, kw), case.stride, case.pad, relu, rd, amax_in=E.slot(np.float32(xmax) * np.float32(1.7)),
                           amax_out=s2)                                                                       # a bound in the slot: another scale
        _same(y2, ref, what + " (amax_in = 1.7 max)", e)
        assert s2.item() == top
    elif fam == "stem_pool":
        Wg = E.weights(case, lambda: wg.igemm_pair_weights(w))
        xd = E.cl(x)
        unpooled = float(cr.conv64(x, w, t["bias"], case.stride, case.pad, relu=True).abs().max())
        outs = []
        for _ in range(2):
            so = E.slot()
            outs.append((wg.conv_igemm(E.ws, xd, Wg, bias, (kh, kw), case.stride, case.pad, True, amax_in=amax, amax_out=so, pool=True), so))
        _same(outs[0][0], ref, what, e)
        assert outs[0][1].item() == unpooled, (what, "max of the un-pooled map", outs[0][1].item(), unpooled)
        assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1].item() == outs[1][1].item(), what + ": the second launch differs"
    elif fam in ("igemm_p", "direct_p"):
        xf, rf, of = e.opts["xf"], e.opts["rf"], e.opts["of"]
        wl1, bmax = _wl1(w, t["bias"])
        if xf == "pairs":
            xb = E.slot(xmax * (1.5 if case.seed % 2 else 1.0))
            act = wg.PairAct(cr.pack_pairs(x, xb.item()).cuda(), True, (B, cin, H, W), amax, xb)
        else:
            act = wg.PairAct(E.cl(x), False, (B, cin, H, W), amax, amax)
        rmax, ract = 0.0, None
        if rf is not None:
            rmax = float(res.abs().max())
            rb = E.slot(rmax)
            ract = wg.PairAct(cr.pack_pairs(res, rmax).cuda(), True, tuple(res.shape), rb, rb) if rf == "pairs" else \
                wg.PairAct(E.cl(res), False, tuple(res.shape), rb, rb)
        Wk = E.weights(case, lambda: wg.igemm_pair_weights(w) if fam == "igemm_p" else wg.stem_direct_pair_weights(w))
        outs = []
        for _ in range(2):
            so, sb = E.slot(), E.slot()
            if fam == "igemm_p":
                a = wg.conv_igemm_p(E.ws, act, Wk, bias, (kh, kw), case.stride, case.pad, relu, ract, wl1, bmax, so, sb, of == "pairs")
            else:
                a = wg.conv3x3_direct_p(act, Wk, bias, relu, ract, wl1, bmax, so, sb, of == "pairs")
            outs.append(a)
        if of == "pairs":
            _pairs_out(E, outs[0], ref, xmax, wl1, bmax, rmax, what, e)
        else:
            _same(outs[0].t, ref, what, e)
        assert outs[0].amax.item() == top, (what, "max |y| slot", outs[0].amax.item(), top)
        assert torch.equal(outs[0].t, outs[1].t) and outs[0].amax.item() == outs[1].amax.item(), what + ": the second launch differs"
    else:
        raise AssertionError(fam)


@pytest.mark.parametrize("cls", cr.CLASSES)
@pytest.mark.parametrize("name", [e.name for e in ENTRIES])
def test_convolution_entry_point_is_exact_on_integer_classes(E, name, cls):
    """Every case of the entry's table (`cases`) equals the float64 convolution bit for bit, with its max |y| slot equal to max |ref|, its
    bound slot equal to the documented (max|x| wl1 + bmax + max|res|) 1.001 and >= max |ref|, pair-format outputs equal to the canonical
    split of the reference, and a second launch that repeats the first's bits.  Nothing is narrowed per kernel except what
    conv_reference's generators document: ranges shrunk to K max|x| max|w| < 2^24 (2^22 for pair-format outputs) and the stem's
    two-layer classes (`make_stem_case`)."""
    E.packed.clear()
    for case in cases(ENTRY[name], cls, E.n_cu):
        if case.distinct and case.shape[0] < DISTINCT:
            # (a device with so few compute units that the many-block launch has fewer than DISTINCT images: other data than the CPU file proved)
            t, _ = build(case)
            assert case.kind == "stem" or (cr.wino2_premise if ENTRY[name].family == "wino2" else cr.premise)(
                t["x"], t["w"], t["bias"], t["res"], *(() if ENTRY[name].family == "wino2" else (case.stride, case.pad)))["ok"], case
        _run(E, case)


def test_pair_helpers_agree_with_pairs_to_float(E):
    """`pack_pairs` / `unpack_pairs` against `conv_kernels.pairs_to_float` on values with and without a lo half, for bounds at, above and
    far above the maximum (lo halves down to fp16's subnormal range)."""
    torch, wg = E.torch, E.wg
    rng = np.random.default_rng(5)
    y = torch.from_numpy((rng.integers(-(1 << 21), 1 << 21, size=(2, 64, 3, 5)) * 2.0 ** -7).astype(np.float32))
    for mul in (1.0, 1.001, 1.7, 64.0, 1024.0):
        bound = float(np.float32(float(y.abs().max()) * mul))
        t = cr.pack_pairs(y, bound)
        slot = E.slot(bound)
        got = wg.pairs_to_float(wg.PairAct(t.cuda(), True, tuple(y.shape), slot, slot)).cpu()
        assert torch.equal(got.contiguous(), cr.unpack_pairs(t, bound).contiguous()), mul
        if mul <= 64.0:                                         # 22 bits fit while the lo half stays a multiple of fp16's 2^-24
            assert torch.equal(got.contiguous(), y), mul


# ---------------------------------------------------------------------------------------------------------------- 4. the F(4x4) forms

W4_BAR = {"f32": 80.0, "h": 222.0}
W4_MAPS = NOPOOL + POOL


@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("form", ["f32", "h"])
def test_fused_winograd_f4_within_the_per_element_bound(E, form, cout):
    """`cslam_wino4_fused_c64_dev` (f32) and `cslam_wino4_fused_c64_h_dev` (fp16 pairs) cannot be exact (G holds 1/6): every element within
    W4_BAR u of the float64 convolution, relative to the magnitude the float64 Winograd evaluation of tests/wino_reference.py gives for
    that element (so an element that is small next to the map's maximum has a small bound), on the shared maps with channel magnitudes
    six binades apart; ReLU, pooling, bias and shortcut alternate.  The bars are derived from the operation counts, not tuned:

    The bar of |y - ref| <= BAR u mag, u = 2^-24, mag = |A^T| (sum_c |U_c| o (|B^T| |d_c| |B|)) |A| + |bias| + |res| per element, derived
    from the operation counts (first order: relative errors add; the second-order terms are below 0.1 at these counts):
      U = float32(G g G^T): one rounding of the float64 transform                                        1
      input transform: two 1-D passes of B^T, at most three roundings deep each
        (tests/test_wino_transforms_gpu.py, IN_BAR)                                                      6.5
      output transform: two passes of A^T, three roundings deep each, + bias + shortcut (OUT_BAR there)  8.5
      f32 form: 64 products, each added to an fp32 accumulator: a term passes through at most 64
        roundings of a partial sum that the absolute sum bounds                                          64
      pair form: V and U split into hi + lo, 2^-22 = 4 u of the value each                               4 + 4
                 the dropped lo lo product, 2^-11 2^-11 of |U| |V|                                       4
                 lo halves below fp16's subnormal spacing (2^-25 of a scaled value that is at least
                 2^7 when it matters to mag: the largest channels carry mag)                             1
                 fp16 products exact; 3 x 64 of them added in fp32, the absolute sum of the three
                 families (1 + 2^-10) sum |U| |V|                                                        192.2
    f32: 1 + 6.5 + 8.5 + 64 = 80; pair form: 1 + 6.5 + 8.5 + 8 + 4 + 1 + 192.2 = 221.2 -> 222.

    These are worst-case counts (every rounding at its limit and of one sign): random roundings stay about a hundred times below them,
    which is what the measured ratios show.  The strength of the check is mag: an element that is small next to its map's maximum gets a
    small bound.
    Measured worst error / bound on an MI355X (printed with -s): f32 0.0073 (64 channels) and 0.0085 (128), pair form 0.0019 and 0.0031."""
    torch, wg = E.torch, E.wg
    worst = 0.0
    for i, (B, H, W) in enumerate(W4_MAPS):
        rng = np.random.default_rng(4000 + 10 * i + cout)
        pool = i >= len(NOPOOL)
        relu, has_bias, has_res = i % 2 == 0, i % 3 != 1, (i % 2 == 1 and not pool)
        x = (rng.standard_normal((B, 64, H, W)) * 2.0 ** (np.arange(64) % 7 - 3)[None, :, None, None]).astype(np.float32)
        w = (rng.standard_normal((cout, 64, 3, 3)) / 24.0 * 2.0 ** (np.arange(cout) % 4 - 2)[:, None, None, None]).astype(np.float32)
        bias = rng.standard_normal(cout).astype(np.float32) if has_bias else None
        res = rng.standard_normal((B, cout, H, W)).astype(np.float32) if has_res else None
        tx, tw = torch.from_numpy(x), torch.from_numpy(w)
        U4 = wg.wino_weights(tw, 4)                                                         # [36, 64, cout] float32
        V, mag = wr.input_transform(x.transpose(0, 2, 3, 1), 4)                             # [36, T, 64]
        m = np.einsum("ftc,fco->fto", mag, np.abs(U4.double().numpy()))
        nhwc = lambda a: None if a is None else a.transpose(0, 2, 3, 1)                     # noqa: E731
        _, ymag, _ = wr.output_transform(m, None if bias is None else np.abs(bias), None if res is None else np.abs(nhwc(res)), B, H, W, 4, 1.0,
                                         False, pool)
        ref = cr.conv64(tx, tw, None if bias is None else torch.from_numpy(bias), 1, 1, relu=relu, pool=2 if pool else 0,
                        res=None if res is None else torch.from_numpy(res))
        xd, rd, bd = E.cl(tx), E.cl(None if res is None else torch.from_numpy(res)), None if bias is None else torch.from_numpy(bias).cuda()
        if form == "f32":
            y = wg.wino_fused64(xd, wg.fused64_weights(U4).cuda(), bd, relu, pool, rd)
        else:
            y = wg.wino_fused64_h(xd, E.dev(wg.fused64_pair_weights(U4)), bd, relu, pool, E.slot(np.abs(x).max()), None, rd)
        got = y.cpu().permute(0, 2, 3, 1).double().numpy()
        want = ref.permute(0, 2, 3, 1).numpy()
        bar = W4_BAR[form] * wr.U32 * np.asarray(ymag, dtype=np.float64)
        err = np.abs(got - want)
        bad = ~(err <= bar)
        if bad.any():
            k = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("wino4 %s cout=%d B=%d H=%d W=%d: %d of %d elements outside the bound; first at (b, h, w, co) = %s: got %r, "
                                 "reference %r, error %.3e, bound %.3e" % (form, cout, B, H, W, int(bad.sum()), bad.size, k, got[k], want[k], err[k], bar[k]))
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
    print("wino4 fused %s cout=%d: worst error / bound = %.4f (bar %.0f u)" % (form, cout, worst, W4_BAR[form]))


# ---------------------------------------------------------------------------------------------------------------- 5. the CosPlace head

def _head_ref(torch, x, p, eps, W, b, dtype):
    """L2Norm -> GeM -> Flatten -> Linear -> L2Norm as the reference's modules compute it (F.normalize, clamp(min=eps).pow(p), avg_pool2d,
    pow(1 / p), F.linear, F.normalize), in `dtype` on the CPU."""
    F = torch.nn.functional
    x, W = x.to(dtype), W.to(dtype)
    v = F.normalize(x, p=2.0, dim=1)
    v = F.avg_pool2d(v.clamp(min=eps).pow(p), (v.size(-2), v.size(-1))).pow(1.0 / p).flatten(1)
    v = F.linear(v, W, None if b is None else b.to(dtype))
    return F.normalize(v, p=2.0, dim=1)


@pytest.mark.parametrize("C_", [4, 64, 260, 2048])
def test_cosplace_head_both_layouts_against_float64(E, C_):
    """`gem_fc_kernel` (NCHW) and `gem_fc_nhwc_kernel` through their C entry points, B = 5, for every P in {1, 3, 49, 50}, Dout in {1, 5, 64,
    130}, p = 3 (the cube path) and 2.37, with and without bias, on signed input with values the eps clamp catches and one all-zero pixel:
    no further from the float64 restatement than 4 x the float32 torch modules on the same input + 2e-7, and the two layouts within that
    figure of each other.  Prints the largest measured errors (-s); on an MI355X the worst error / tolerance was 0.34 (NCHW), 0.30 (NHWC)
    and 0.38 between the layouts, torch's own float32 error up to 7.1e-7."""
    torch, lib, ck = E.torch, E.lib, E._lib.check
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())    # noqa: E731
    worst = [0.0, 0.0, 0.0, 0.0]
    for (h, w_) in [(1, 1), (1, 3), (7, 7), (5, 10)]:
        P = h * w_
        gen = torch.Generator().manual_seed(C_ * 131 + P)
        x = torch.randn((5, C_, h, w_), generator=gen)
        x[:, ::3] *= 1e-4                                              # after the pixel norm below eps = 1e-6 in wide maps, above it in narrow ones
        x[1, :, h - 1, w_ - 1] = 0.0                                   # an all-zero pixel: norm 0, clamped to eps
        x[2, 1::2] = x[2, 1::2].abs() * 1e-9
        for Dout in (1, 5, 64, 130):
            W = torch.randn((Dout, C_), generator=gen) / C_ ** 0.5
            b0 = torch.randn((Dout,), generator=gen) * 0.1
            for p in (3.0, 2.37):
                for b in (b0, None):
                    r64 = _head_ref(torch, x, p, 1e-6, W, b, torch.float64)
                    r32 = _head_ref(torch, x, p, 1e-6, W, b, torch.float32)
                    e32 = float((r32.double() - r64).abs().max())
                    tol = 4 * e32 + 2e-7
                    Wd, bd = W.cuda(), None if b is None else b.cuda()
                    outs = []
                    for fn, xd in ((lib.cslam_gem_fc_head_dev, x.cuda().contiguous()),
                                   (lib.cslam_gem_fc_head_nhwc_dev, x.permute(0, 2, 3, 1).contiguous().cuda())):
                        out = torch.full((5, Dout), float("nan"), device="cuda")
                        ck(fn(ptr(xd), p, 1e-6, ptr(Wd), ptr(bd), 5, C_, P, Dout, ptr(out), st))
                        outs.append(out.cpu().double())
                    en, ec, el = (float((outs[0] - r64).abs().max()), float((outs[1] - r64).abs().max()), float((outs[0] - outs[1]).abs().max()))
                    what = "C=%d P=%d Dout=%d p=%g bias=%d" % (C_, P, Dout, p, b is not None)
                    assert en <= tol and ec <= tol and el <= tol, (what, "nchw %.3e nhwc %.3e between %.3e" % (en, ec, el), "float32 torch %.3e" % e32, "tolerance %.3e" % tol)
                    for k, v in enumerate((en / tol, ec / tol, el / tol, e32)):
                        worst[k] = max(worst[k], v)
    print("gem_fc C=%d: worst error / tolerance nchw %.3f nhwc %.3f between the layouts %.3f; largest float32-torch error %.3e" % (C_, *worst))
