"""The premise of tests/test_conv_exact_gpu.py, proved from the reference alone (no device): for every class and every case of that
file's table `premise` holds, and the kernels' arithmetic -- the three products xh wh + xl wh + xh wl of the exact fp16 halves,
accumulated in float32 -- gives the float64 convolution bit for bit in whatever order it is summed.  A mismatch on the GPU can then
only be the kernel's.  Three orders are emulated with numpy in float32:
  a. the 3 K products one after the other, the K terms in a random order (hh, lh, hl of a term together);
  b. another random order of the K terms, all hh products first, then all lh, then all hl;
  c. the matrix pipe's: K in blocks of 32, a block's products summed first (a float32 matrix product), hh then lh then hl.
Orders a and b are run on a sample of 64 output pixels x 8 output channels per case, and there EVERY partial sum is compared with its
float64 value; order c on all outputs.  Launches of more than 4096 output pixels are emulated on their first two images and the last
one (`premise` sees all of them; the many-block launches repeat their first 61 images, whatever the device's workgroup count).  The F(2x2) form is emulated stage by stage in float32 likewise; the pair-format helpers are tested
at the end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_reference as cr
import test_conv_exact_gpu as G
import wino_reference as wr
from cslam_amd.vpr.heads import pair_split

f32 = np.float32
_DONE = set()                # inputs already proved for another entry (entries of one signature share them)


def _halves(x, w):
    xh, xl = cr.act_split(x)
    wh, wl, inv_s = pair_split(torch.as_tensor(w).double())
    return xh, xl, wh.double() * inv_s, wl.double() * inv_s


def _emulate(x, w, bias, res, stride, pad, rng, what):
    """The pre-activation output conv(x, w) + bias + res of the three-product arithmetic in float32, order c, [B,Cout,Ho,Wo] float32;
    orders a and b are checked on a sample inside."""
    B, Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    K = Cin * KH * KW
    xh, xl, wh, wl = _halves(x, w)
    ch = F.unfold(xh, (KH, KW), padding=pad, stride=stride).permute(0, 2, 1).reshape(-1, K).numpy()       # [N, K] float64, K = (c, kh, kw)
    cl = F.unfold(xl, (KH, KW), padding=pad, stride=stride).permute(0, 2, 1).reshape(-1, K).numpy()
    Wh, Wl = wh.reshape(Cout, K).numpy(), wl.reshape(Cout, K).numpy()
    N = ch.shape[0]
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    ref = cr.conv64(x, w, bias, stride, pad, res=res)                                                     # float64
    extra = np.zeros((N, Cout))
    if bias is not None:
        extra += bias.double().numpy()[None, :]
    if res is not None:
        extra += res.double().permute(0, 2, 3, 1).reshape(N, Cout).numpy()
    want = ref.permute(0, 2, 3, 1).reshape(N, Cout).numpy()
    # c: blocks of 32 (K padded with zeros), float32 matrix products
    Kp = -(-K // 32) * 32
    pad32 = lambda a: np.pad(a, ((0, 0), (0, Kp - K))).astype(f32)    # noqa: E731
    Ah, Al, Bh, Bl = pad32(ch), pad32(cl), pad32(Wh), pad32(Wl)
    assert np.array_equal(Ah.astype(np.float64)[:, :K], ch) and np.array_equal(Bl.astype(np.float64)[:, :K], Wl)
    acc = np.zeros((N, Cout), dtype=f32)
    for k0 in range(0, Kp, 32):
        for a, b in ((Ah, Bh), (Al, Bh), (Ah, Bl)):
            acc = acc + a[:, k0:k0 + 32] @ b[:, k0:k0 + 32].T
            assert acc.dtype == f32
    y = (acc + extra.astype(f32)).astype(f32)
    assert np.array_equal(y.astype(np.float64), want), "%s: order c differs from conv64 at %s" % (what, np.argwhere(y != want)[0].tolist())
    # a, b: sequential sums on a sample, every partial sum against float64
    pix = rng.choice(N, size=min(N, 64), replace=False)
    co = rng.choice(Cout, size=min(Cout, 8), replace=False)
    sh, sl, vh, vl = ch[pix][:, None, :], cl[pix][:, None, :], Wh[co][None, :, :], Wl[co][None, :, :]   # [n, 1, K], [1, c, K]
    for order in ("a", "b"):
        perm = rng.permutation(K)
        hh, lh, hl = (sh * vh)[..., perm], (sl * vh)[..., perm], (sh * vl)[..., perm]
        terms = np.stack((hh, lh, hl), axis=-1).reshape(len(pix), len(co), 3 * K) if order == "a" else np.concatenate((hh, lh, hl), axis=-1)
        t32 = terms.astype(f32)
        assert np.array_equal(t32.astype(np.float64), terms), what + ": a product of two halves is no float32 number"
        run32, run64 = np.cumsum(t32, axis=-1, dtype=f32), np.cumsum(terms, axis=-1)
        assert np.array_equal(run32.astype(np.float64), run64), "%s: order %s: a partial sum rounds" % (what, order)
        got = (run32[..., -1] + extra[np.ix_(pix, co)].astype(f32)).astype(f32)
        assert np.array_equal(got.astype(np.float64), want[np.ix_(pix, co)]), "%s: order %s differs from conv64" % (what, order)
    return torch.from_numpy(y.reshape(B, Ho, Wo, Cout)).permute(0, 3, 1, 2)


def _finish(y, relu, pool):
    """ReLU and pooling in float32"""
    if relu:
        y = y.relu()
    if pool == 2:
        y = F.max_pool2d(y, 2)
    elif pool == 3:
        y = F.max_pool2d(y, 3, 2, 1)
    return y.contiguous()


def _subset(t, idx):
    return None if t is None else t[idx]


def _emulate_wino2(x, w, bias, res, rng, what):
    """F(2x2, 3x3) stage by stage in float32: V = B^T d B, M = sum_c U_c V_c as a float32 matrix product and, on 16 output channels, in a random order of c with every partial sum against float64,
    y = A^T M A + bias + res."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    BT, AT, Gm = wr.matrices(2)
    U = np.einsum("ik,ockl,jl->ijco", Gm, w.double().numpy(), Gm).reshape(16, Cin, Cout)
    assert np.array_equal(U.astype(f32).astype(np.float64), U)
    V, _ = wr.input_transform(x.double().permute(0, 2, 3, 1).numpy(), 2)                                # [16, T, Cin] float64
    # the input transform in float32, rows then columns
    xn = x.permute(0, 2, 3, 1).numpy().astype(f32)
    TH, TW = wr.tiles_of(H, W, 2)
    xp = np.zeros((B, TH * 2 + 2, TW * 2 + 2, Cin), dtype=f32)
    xp[:, 1:H + 1, 1:W + 1] = xn
    d = np.stack([np.stack([xp[:, i:i + TH * 2:2, j:j + TW * 2:2] for j in range(4)], axis=3) for i in range(4)], axis=3)   # [B,TH,TW,4,4,C]
    BT32 = BT.astype(f32)
    t1 = np.zeros_like(d)
    for p in range(4):
        for i in range(4):
            t1[:, :, :, p] = t1[:, :, :, p] + BT32[p, i] * d[:, :, :, i]
    V32 = np.zeros_like(d)
    for q in range(4):
        for j in range(4):
            V32[:, :, :, :, q] = V32[:, :, :, :, q] + BT32[q, j] * t1[:, :, :, :, j]
    V32 = V32.transpose(3, 4, 0, 1, 2, 5).reshape(16, B * TH * TW, Cin)
    assert V32.dtype == f32 and np.array_equal(V32.astype(np.float64), V), what + ": the input transform rounds"
    perm = rng.permutation(Cin)
    co = rng.choice(Cout, size=16, replace=False)                                                       # every partial sum, on 16 output channels
    terms = V[:, :, perm, None] * U[:, None, perm][..., co]                                             # [16, T, Cin, 16]
    run32, run64 = np.cumsum(terms.astype(f32), axis=2, dtype=f32), np.cumsum(terms, axis=2)
    assert np.array_equal(run32.astype(np.float64), run64), what + ": a partial sum over the channels rounds"
    M = np.matmul(V32, U.astype(f32))                                                                   # [16, T, Cout] float32, the library's order
    assert M.dtype == f32 and np.array_equal(M[..., co], run32[:, :, -1]), what + ": two orders of the channel sum differ"
    T = M.shape[1]
    m = M.reshape(4, 4, T, Cout)
    AT32 = AT.astype(f32)
    z = np.zeros((2, 4, T, Cout), dtype=f32)
    for p in range(2):
        for i in range(4):
            z[p] = z[p] + AT32[p, i] * m[i]
    y = np.zeros((2, 2, T, Cout), dtype=f32)
    for q in range(2):
        for j in range(4):
            y[:, q] = y[:, q] + AT32[q, j] * z[:, j]
    y = y.reshape(2, 2, B, TH, TW, Cout).transpose(2, 3, 0, 4, 1, 5).reshape(B, TH * 2, TW * 2, Cout)[:, :H, :W]
    if bias is not None:
        y = y + bias.numpy()[None, None, None, :]
    if res is not None:
        y = y + res.permute(0, 2, 3, 1).numpy()
    assert y.dtype == f32
    return torch.from_numpy(np.ascontiguousarray(y)).permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", [e.name for e in G.ENTRIES])
def test_premise_and_float32_emulation_of_every_case(name):
    e = G.ENTRY[name]
    n = 0
    for cls in cr.CLASSES:
        for case in G.cases(e, cls):
            n += 1
            if case._replace(entry="") in _DONE:
                continue
            rng = np.random.default_rng(case.seed)
            B, cin, H, W, cout, kh, kw = case.shape
            what = "%s %s B=%d H=%d W=%d seed=%d" % (name, cls, B, H, W, case.seed)
            Ho, Wo = (H + 2 * case.pad - kh) // case.stride + 1, (W + 2 * case.pad - kw) // case.stride + 1
            idx = list(range(B)) if B * Ho * Wo <= 4096 else [0, 1, B - 1]
            d = min(case.distinct or B, B)                  # the many-block launches repeat their first d images: the premise is theirs
            if e.family == "stem_direct":
                t = cr.make_stem_case(cls, B, H, W, case.seed, bias=case.bias, wseed=case.wseed, distinct=case.distinct)
                p1 = cr.premise(t["x0"][:d], t["w1"], t["b1"], None, 1, 1)
                assert torch.equal(t["x0"], t["x0"][torch.arange(B) % d])
                a1_64 = cr.conv64(t["x0"][:d], t["w1"], t["b1"], 1, 1, relu=True)
                p2 = cr.premise(a1_64.float(), t["w2"], t["b2"], None, 1, 1)
                assert p1["ok"] and p2["ok"], (what, p1, p2)
                assert a1_64.float().double().equal(a1_64) and float(a1_64.abs().max()) / p1["unit"] < 2 ** 22, what
                if cls == "x_lo":
                    assert p1["x_lo_nonzero"] > 0 and p2["x_lo_nonzero"] > 0, what
                if cls == "w_lo":
                    assert (p2["w_lo_nonzero"] if case.seed % 2 == 0 else p1["w_lo_nonzero"]) > 0, what
                a1 = _finish(_emulate(t["x0"][idx], t["w1"], t["b1"], None, 1, 1, rng, what + " layer 1"), True, 0)
                a1_64 = a1_64[torch.arange(B) % d]
                assert a1.double().equal(a1_64[idx]), what
                y = _finish(_emulate(a1, t["w2"], t["b2"], None, 1, 1, rng, what + " layer 2"), True, case.pool)
                ref = cr.conv64(a1_64[idx], t["w2"], t["b2"], 1, 1, relu=True, pool=case.pool)
            else:
                t = cr.make_case(cls, case.shape, case.seed, stride=case.stride, pad=case.pad, bias=case.bias, res=case.res, bits=case.bits,
                                 k_eff=case.k_eff, w_mult=case.w_mult, wseed=case.wseed, distinct=case.distinct)
                x, w, bias, res = t["x"], t["w"], t["bias"], t["res"]
                assert torch.equal(x, x[torch.arange(B) % d]) and (res is None or torch.equal(res, res[torch.arange(B) % d]))
                ref = cr.conv64(x[idx], w, bias, case.stride, case.pad, relu=case.relu, pool=case.pool, res=_subset(res, idx))
                if e.family == "wino2":
                    p = cr.wino2_premise(x[:d], w, bias, None if res is None else res[:d])
                    assert p["ok"], (what, p)
                    y = _finish(_emulate_wino2(x[idx], w, bias, _subset(res, idx), rng, what), case.relu, case.pool)
                else:
                    p = cr.premise(x[:d], w, bias, None if res is None else res[:d], case.stride, case.pad)
                    assert p["ok"], (what, p)
                    assert p["max_units"] < 2 ** case.bits, (what, p)
                    if cls == "x_lo":
                        assert p["x_lo_nonzero"] > 0 and p["w_lo_nonzero"] == 0, (what, p)
                    if cls == "w_lo":
                        assert p["w_lo_nonzero"] > 0 and p["x_lo_nonzero"] == 0, (what, p)
                    y = _finish(_emulate(x[idx], w, bias, _subset(res, idx), case.stride, case.pad, rng, what), case.relu, case.pool)
                    if case.bits == 22:                 # pair-format output: the canonical split of the result loses nothing
                        top = float(ref.abs().max()) * 1.001 + 1e-30
                        assert cr.unpack_pairs(cr.pack_pairs(ref.float(), top), top).double().equal(ref), what
            assert y.dtype == torch.float32 and y.double().equal(ref), "%s: %s" % (what, cr.locate(y, ref.float(), 8, 16))
            _DONE.add(case._replace(entry=""))
    assert n >= 3 * 5


def test_input_classes_are_what_the_table_says():
    shape = (2, 64, 5, 7, 64, 3, 3)
    for seed in (10, 11):
        a, b, c = cr.ints(shape, seed), cr.x_lo(shape, seed), cr.w_lo(shape, seed)
        for t in (a, b, c):
            assert t["x"].dtype == t["w"].dtype == t["bias"].dtype == torch.float32
        xi, wi = a["x"].double() / a["px"], a["w"].double() / a["pw"]
        assert xi.abs().max() == 15 and wi.abs().max() == 2 and xi.equal(xi.round()) and wi.equal(wi.round())
        assert len(set(xi.reshape(-1, 7).unique(dim=0).shape)) > 1 and xi.reshape(-1, 7).unique(dim=0).shape[0] > 600   # no repeated rows
        xb = b["x"].double() / b["px"]
        sh = 11 + seed % 2
        assert xb.abs().max() == 2 ** sh + 15 and ((xb.abs() - 2 ** sh).abs() <= 15).logical_or(xb.abs() <= 15).all()
        wc = c["w"].double() / c["pw"]
        assert wc.abs().max() == 2 ** sh + 15
        assert (a["bias"].double() / (a["px"] * a["pw"])).abs().max() <= 100
        assert -9 <= np.log2(a["px"]) <= 6 and -9 <= np.log2(a["pw"]) <= 6
    with pytest.raises(AssertionError):                      # a range that cannot be made to fit is refused, not silently narrowed
        cr.x_lo((1, 512, 4, 4, 64, 3, 3), 3, bits=22)


def test_premise_refuses_what_is_not_exact():
    rng = np.random.default_rng(1)
    t = cr.ints((1, 32, 4, 4, 64, 3, 3), 5)
    assert cr.premise(t["x"], t["w"], t["bias"], None, 1, 1)["ok"]
    both = cr.x_lo((1, 32, 4, 4, 64, 3, 3), 6)
    both["w"] = cr.w_lo((1, 32, 4, 4, 64, 3, 3), 6)["w"]
    p = cr.premise(both["x"], both["w"], None, None, 1, 1)
    assert not p["lolo_zero"] and not p["ok"]
    x = torch.from_numpy(rng.standard_normal((1, 32, 4, 4)).astype(np.float32))
    p = cr.premise(x, t["w"], None, None, 1, 1)
    assert not p["ok"] and (not p["split"] or p["max_units"] >= 2 ** 24)
    p = cr.premise(t["x"], t["w"], t["bias"] * 0.5 ** 12, None, 1, 1)                 # a bias below the products' unit
    assert not p["aligned"] and not p["ok"]


def test_locate_names_the_element_and_its_block():
    ref = torch.arange(2 * 4 * 20 * 20, dtype=torch.float32).reshape(2, 4, 20, 20)
    assert cr.locate(ref.clone(), ref, 8, 16) is None
    y = ref.clone()
    y[1, 2, 9, 17] += 1
    y[1, 3, 19, 0] += 1
    r = cr.locate(y, ref, 8, 16, tile=128)
    assert r["first"] == (1, 9, 17, 2) and r["count"] == 2 and r["pixels"] == 2 and r["block"] == (1, 1, 1) and r["channels"] == [2, 3]
    assert r["tile"] == (400 + 9 * 20 + 17) // 128 and r["got"] == r["want"] + 1


def test_pair_helpers_round_trip_and_subnormal_lo_halves():
    rng = np.random.default_rng(2)
    # 22-bit values: hi + lo is the value, whatever the bound's binade
    y = torch.from_numpy((rng.integers(-(1 << 22) + 1, 1 << 22, size=(2, 64, 3, 5)) * 2.0 ** -9).astype(np.float32))
    top = float(y.abs().max())
    for bound in (top, top * 1.001, top * 1.99, top * 3.0):
        t = cr.pack_pairs(y, bound)
        assert t.shape == (2, 3, 5, 2, 2, 32) and t.dtype == torch.float16
        s = cr.scale_c(bound)
        assert 2 ** 13 <= np.float32(bound) * s < 2 ** 14
        assert torch.equal(t[0, 1, 2, 1, 0], (y[0, 32:, 1, 2] * s).half())                     # [pixel][block][hi 32 | lo 32]
        assert torch.equal(cr.unpack_pairs(t, bound), y)
        hi, lo = t[..., 0, :].double(), t[..., 1, :].double()
        assert (lo.abs().numpy() <= wr.ulp_fp16(hi.numpy()) / 2).all()
    # lo halves in fp16's subnormal range (|lo| < 2^-14): multiples of 2^-24 survive, finer remainders are rounded to that spacing
    s = cr.scale_c(1.0)                                                                         # 2^13
    v = torch.tensor([1.0, 2.0 ** -13 * (1 + 2.0 ** -21), 2.0 ** -37, 2.0 ** -13 * (2.0 ** -3 + 2.0 ** -26)]).reshape(1, 4, 1, 1)
    y = torch.zeros((1, 32, 1, 1))
    y[:, :4] = v
    t = cr.pack_pairs(y, 1.0)
    lo = t[0, 0, 0, 0, 1, :4].double()
    assert lo[1] == 2.0 ** -21 and 0 < lo[1] < 2.0 ** -14                                       # subnormal and exact
    assert lo[2] == 0 and t[0, 0, 0, 0, 0, 2] == 2.0 ** -24                                     # s v = 2^-24: the smallest hi there is
    back = cr.unpack_pairs(t, 1.0)
    assert back[0, 1, 0, 0] == y[0, 1, 0, 0] and back[0, 0, 0, 0] == 1.0
    assert abs(float(back[0, 3, 0, 0]) - float(y[0, 3, 0, 0])) <= 2.0 ** -25 / s                # rounded to the subnormal spacing, no more
    assert cr.bound_formula(3.0, 5.0, 1.0, 2.0) == {float(np.float32(18.0) * np.float32(1.001))}
