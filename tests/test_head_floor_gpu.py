"""GPU tests of the NetVLAD head's fused forms (-m gpu): the VLAD kernel whose final store writes the projection's fp16 pair rows
(cslam_vlad_aggregate_nhwc_pairs_dev), the projection of such rows (cslam_pca_project_from_pairs_dev) and the pair epilogue that
keeps a row in registers.  References: float64 restatements of NetVLADLayer.forward and of pca.transform + normalize
(oracle/heads_oracle.py), and the unfused kernels as bit-for-bit partners.
"""
import numpy as np
import pytest

from oracle import heads_oracle as ho

pytestmark = pytest.mark.gpu

K, C = 64, 512


@pytest.fixture(scope="module")
def T():
    import torch
    from cslam_amd.vpr import heads
    return torch, heads


@pytest.fixture(scope="module")
def layer():
    """Centroids on the scale of the unit-norm local descriptors and an assignment tied to them (2 alpha centroids), a small bias."""
    rng = np.random.default_rng(12)
    cent = rng.standard_normal((K, C))
    cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True) * 0.5).astype(np.float32)
    w = (2.0 * 10.0 * cent).astype(np.float32)
    b = (0.1 * rng.standard_normal(K)).astype(np.float32)
    return w, b, cent


def frames(B, H, W, cent, seed):
    """Trunk-like maps (non-negative, a few dead channels); frame 0 all zeros (zero-norm rule); in the last frame (B > 1) every
    pixel lies along centroid 5, so that one cluster takes every pixel."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((B, C, H, W)), 0).astype(np.float32) * 3
    x[:, ::37] = 0
    x[0] = 0
    if B > 1:
        x[-1] = (40.0 * cent[5][:, None, None] + 0.5 * rng.random((C, H, W))).astype(np.float32)
    return x


def vlad_f64(x, w, b, cent):
    """NetVLADLayer.forward (netvlad.py:94-130) in float64"""
    B = x.shape[0]
    xf = x.astype(np.float64).reshape(B, x.shape[1], -1)
    xf = xf / np.maximum(np.linalg.norm(xf, axis=1, keepdims=True), 1e-12)
    sa = np.einsum("kc,ncp->nkp", w.astype(np.float64), xf)
    if b is not None:
        sa = sa + b.astype(np.float64)[None, :, None]
    a = np.exp(sa - sa.max(axis=1, keepdims=True))
    a /= a.sum(axis=1, keepdims=True)
    v = np.einsum("nkp,ncp->nkc", a, xf) - a.sum(axis=2)[:, :, None] * cent.astype(np.float64)[None]
    v = v / np.maximum(np.linalg.norm(v, axis=2, keepdims=True), 1e-12)
    v = v.reshape(B, -1)
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12), a


def pair_rows(torch, v, x_bound, splits):
    """pca_pairs_rows_kernel (gemm_nt.hip) restated: [B, Din] float32 -> A2 [S, B, Din / S / 32, hi 32 | lo 32] float16 of s v, s the
    power of two with x_bound s in [2^13, 2^14]."""
    sc = 2.0 ** (int(np.frexp(np.float32(16384.0) / np.float32(x_bound))[1]) - 1)
    B, din = v.shape
    sv = v * sc
    hi = sv.to(torch.float16)
    lo = (sv - hi.to(torch.float32)).to(torch.float16)
    kb = din // splits // 32
    a2 = torch.stack((hi.view(B, splits, kb, 32), lo.view(B, splits, kb, 32)), dim=3)          # [B, S, kb, 2, 32]
    return a2.permute(1, 0, 2, 3, 4).reshape(splits, B, kb, 64).contiguous()


def dev(T, a):
    return T[0].from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("bias", [False, True])
def test_vlad_pair_store_against_float64_and_the_row_kernel(T, layer, B, bias):
    """14 x 14 maps of 512 channels, 64 clusters: the float32 rows within 2e-7 of float64 (zero frame and one-cluster frame included),
    the pair rows byte-equal to the row kernel's arithmetic on those float32 rows, with and without the float32 rows asked for."""
    torch, heads = T
    w, b, cent = layer
    b = b if bias else None
    x = frames(B, 14, 14, cent, 100 + B)
    xl = dev(T, x).contiguous(memory_format=torch.channels_last)
    args = (dev(T, w), dev(T, b) if bias else None, dev(T, cent))
    a2, v = heads.vlad_aggregate_pairs(xl, *args, keep_v=True)
    ref, a = vlad_f64(x, w, b, cent)
    if B > 1:
        assert np.all(a[-1].argmax(axis=0) == 5) and a[-1, 5].min() > 0.9                  # one cluster takes every pixel
    err = float(np.max(np.abs(v.cpu().numpy() - ref)))
    print("B = %d bias = %s: max |v - float64| = %.3g" % (B, bias, err))
    assert np.all(np.isfinite(v.cpu().numpy())) and err < 2e-7
    assert np.max(np.abs(v.cpu().numpy() - ho.vlad_forward(x, w, b, cent))) < 1e-6
    want = pair_rows(torch, v.contiguous(), heads.VLAD_BOUND, heads.PCA_PAIR_SPLITS)
    assert a2.shape == want.shape and torch.equal(a2.view(torch.int16), want.view(torch.int16))
    a2_only, none = heads.vlad_aggregate_pairs(xl, *args)
    assert none is None and torch.equal(a2_only.view(torch.int16), a2.view(torch.int16))


def test_vlad_pair_store_equals_the_batch_kernel_and_its_projection(T, layer):
    """B = 33: the float32 rows byte-equal to cslam_vlad_aggregate_nhwc_dev (the same kernel without the pair store), and the
    projection of the pair rows byte-equal to cslam_pca_project_pairs_dev on those rows (its row kernel, product and epilogue)."""
    torch, heads = T
    w, b, cent = layer
    B, dout = 33, 256
    x = frames(B, 14, 14, cent, 7)
    xl = dev(T, x).contiguous(memory_format=torch.channels_last)
    args = (dev(T, w), dev(T, b), dev(T, cent))
    a2, v = heads.vlad_aggregate_pairs(xl, *args, keep_v=True)
    v0 = heads.vlad_aggregate(xl, *args)
    assert torch.equal(v, v0)
    gen = torch.Generator(device="cuda").manual_seed(5)
    comp = torch.randn((dout, K * C), generator=gen, device="cuda") / (K * C) ** 0.5
    mp = torch.randn(dout, generator=gen, device="cuda") * 0.1
    pairs = heads.pca_pair_weights(comp)
    assert heads.vlad_pairs_fit(xl, args[2], pairs)
    y = heads.pca_project_from_pairs(a2, comp, mp, None, pairs)
    y0 = heads.pca_project(v0, comp, mp, None, pairs, heads.VLAD_BOUND)
    assert torch.equal(y, y0)
    ref = v0.double() @ comp.double().T - mp.double()
    ref = ref / ref.norm(dim=1, keepdim=True)
    assert float((y.double() - ref).abs().max()) < 1e-5


def test_vlad_pair_store_refuses_maps_outside_the_matrix_form(T, layer):
    """15 x 20 = 300 pixels is beyond the matrix kernel's 200: an error, never another kernel behind the caller's back."""
    torch, heads = T
    w, b, cent = layer
    from cslam_amd import _lib
    xl = torch.zeros((3, C, 15, 20), device="cuda").contiguous(memory_format=torch.channels_last)
    assert not heads.vlad_pairs_fit(torch.zeros((40, C, 15, 20), device="cuda").contiguous(memory_format=torch.channels_last),
                                    dev(T, cent), (torch.empty((8, 128, 128, 2, 32)), 1.0))
    with pytest.raises(_lib.CslamHipError):
        heads.vlad_aggregate_pairs(xl, dev(T, w), None, dev(T, cent))


@pytest.fixture(scope="module")
def pca_case(T):
    """One 257-row input per (Din, Dout) shared by the PCA tests: rows two decades apart, row 40 all zeros, mean and whitening terms."""
    torch, heads = T
    cases = {}
    for din, dout in [(2048, 128), (4096, 384)]:
        gen = torch.Generator(device="cuda").manual_seed(din + dout)
        x = torch.randn((257, din), generator=gen, device="cuda")
        x[128:] *= 0.01
        x[40] = 0
        comp = torch.randn((dout, din), generator=gen, device="cuda") / din ** 0.5
        mp = torch.randn(dout, generator=gen, device="cuda") * 0.1
        inv = torch.rand(dout, generator=gen, device="cuda") + 0.5
        pairs = heads.pca_pair_weights(comp)
        assert pairs is not None and pairs[0].shape[0] == 8
        ref = (x.double() @ comp.double().T - mp.double()) * inv.double()
        ref = ref / ref.norm(dim=1, keepdim=True)
        cases[(din, dout)] = (x, comp, mp, inv, pairs, ref)
    return cases


@pytest.mark.parametrize("B", [32, 33, 255, 257])
@pytest.mark.parametrize("din,dout", [(2048, 128), (4096, 384)])
def test_pca_pairs_epilogue_against_float64(T, pca_case, B, din, dout):
    """S = 8 splits, the smallest pair batch and one row either side of the 256-row block: within 1e-5 of float64, unit rows; the
    projection of ready-made pair rows (scaled from a given bound) byte-equal to the projection that makes them itself."""
    torch, heads = T
    x, comp, mp, inv, pairs, ref = pca_case[(din, dout)]
    xb = x[:B]
    y = heads.pca_project(xb, comp, mp, inv, pairs)
    err = float((y.double() - ref[:B]).abs().max())
    print("B = %d, %d -> %d: max |y - float64| = %.3g" % (B, din, dout, err))
    assert err < 1e-5
    assert float((y.norm(dim=1) - 1.0).abs().max()) < 1e-5
    bound = float(xb.abs().max()) * 1.5
    yb = heads.pca_project(xb, comp, mp, inv, pairs, bound)
    yp = heads.pca_project_from_pairs(pair_rows(torch, xb.contiguous(), bound, 8), comp, mp, inv, pairs, bound)
    assert torch.equal(yp, yb)
    assert float((yb.double() - ref[:B]).abs().max()) < 1e-5


@pytest.mark.parametrize("din,dout", [(2048, 128), (4096, 384)])
def test_pca_pairs_row_does_not_depend_on_its_batch(T, pca_case, din, dout):
    """A 257-row call byte-equal to two calls on the row slices [0, 100) and [100, 257); a row of zeros stays zero (no mean term:
    sklearn's normalize leaves a zero row alone)."""
    torch, heads = T
    x, comp, mp, inv, pairs, _ = pca_case[(din, dout)]
    bound = float(x.abs().max())
    y = heads.pca_project(x, comp, mp, inv, pairs, bound)
    y01 = torch.cat((heads.pca_project(x[:100], comp, mp, inv, pairs, bound), heads.pca_project(x[100:], comp, mp, inv, pairs, bound)))
    assert torch.equal(y, y01)
    z = heads.pca_project(x, comp, None, inv, pairs, bound)
    assert torch.equal(z[40], torch.zeros_like(z[40])) and float((z.norm(dim=1) - 1.0).abs()[41:].max()) < 1e-5


def test_extraction_lanes_take_the_callers_stream_as_lane_zero(T):
    """heads.extract_over_lanes: `lanes` passes in flight use `lanes` streams, the caller's among them (four side lanes beside the
    caller's stream would put two lanes on one of a process's four hardware queues, one behind the other).  Seven chunks over three
    lanes, from the default stream and from a side stream: every chunk on its round-robin lane, the caller's stream last in a
    round, the rows in place."""
    torch, heads = T
    x = torch.arange(7 * 5 * 4, device="cuda", dtype=torch.float32).reshape(35, 4).to(torch.uint8)
    for caller in (torch.cuda.current_stream(), torch.cuda.Stream()):
        lanes, ran = [], []

        def run_chunk(fr, runner):
            ran.append((runner, torch.cuda.current_stream()))
            return fr.to(torch.float32) * 2.0 + 1.0

        caller.wait_stream(torch.cuda.current_stream())                 # x was made on the default stream
        with torch.cuda.stream(caller):
            out = heads.extract_over_lanes(lanes, x, 5, 3, lambda i: i, run_chunk)
            want = x.to(torch.float32) * 2.0 + 1.0
            assert torch.equal(out, want)
        assert [st for st, _ in lanes][0] is None and len({id(st) for st, _ in lanes}) == 3
        assert [r for r, _ in ran] == [1, 2, 0, 1, 2, 0, 1]
        streams = {r: s for r, s in ran}
        assert streams[0] == caller and len({s.cuda_stream for s in streams.values()}) == 3
        assert all(s == streams[r] for r, s in ran)
