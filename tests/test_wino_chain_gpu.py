"""GPU tests of the chained Winograd transform (csrc/wino_chain.hip; -m gpu): between two F(4x4,3x3) layers on the same map
(VGG-16 conv3_1 -> 3_2 -> 3_3, conv4_x, conv5_x: cslam/vpr/netvlad.py:163-171) the output transform of layer L and the input
transform of layer L + 1 run as ONE kernel and y_L stays in LDS.  Compared with the two separate kernels (bit for bit where the
scales agree) and, through the next layer's products, with a float64 evaluation of the two convolutions.  The kernel on its own meets a
float64 transform per element, at every dispatch corner, in tests/test_wino_transforms_gpu.py."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cmid, Cout): conv3 / conv4 / conv5 shapes (the 14 x 14 map's tiles hang over to 16 x 16), a map ragged in both
# directions on the 64-channel group, and one that is a single tile row high and the full 16 tile columns wide
SHAPES = [(3, 56, 56, 128, 256, 256), (4, 28, 28, 256, 512, 512), (9, 14, 14, 512, 512, 512), (2, 30, 22, 64, 128, 128),
          (2, 3, 61, 32, 128, 128)]


@pytest.fixture(scope="module")
def T():
    import torch
    from cslam_amd import _lib
    return torch, _lib


def _p(t):
    return C.c_void_p(t.data_ptr())


def _weights(torch, cout, cin, heavy, gen):
    """He-initialised weights and small biases, or the heavy-tailed ones of test_netvlad_batch_path_descriptors_with_heavy_tailed_weights:
    output channels rescaled log-normally (sigma 0.7), 0.5 % of the weights blown up 8 x, biases spread."""
    w = torch.randn((cout, cin, 3, 3), generator=gen) * (2.0 / (9 * cin)) ** 0.5
    b = 0.05 * torch.randn(cout, generator=gen)
    if heavy:
        scale = torch.exp(0.7 * torch.randn(cout, generator=gen))
        scale = scale / scale.pow(2).mean().sqrt()
        spikes = 1.0 + 7.0 * (torch.rand(w.shape, generator=gen) < 0.005).float()
        w = w * scale.reshape(-1, 1, 1, 1) * spikes
        b = 0.3 * torch.randn(cout, generator=gen) * w.abs().mean() * 27.0
    return w.cuda(), b.cuda()


class _Pair(object):
    """Two consecutive 3x3 convolutions (ReLU after both) through the library's entry points, the transforms between them separate or
    chained.  Every run leaves its intermediate buffers on the object."""

    def __init__(self, T, shape, amp, heavy, seed):
        torch, _lib = T
        from cslam_amd.vpr import winograd as wg
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.B, self.H, self.W, self.cin, self.cmid, self.cout = shape
        gen = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.relu(torch.randn((self.B, self.cin, self.H, self.W), generator=gen)) * amp
        self.x = x.cuda().contiguous(memory_format=torch.channels_last)
        self.w1, self.b1 = _weights(torch, self.cmid, self.cin, heavy, gen)
        self.w2, self.b2 = _weights(torch, self.cout, self.cmid, heavy, gen)
        self.U1 = wg.split16_pair_weights(wg.wino_weights(self.w1, 4).cuda())
        self.U2 = wg.split16_pair_weights(wg.wino_weights(self.w2, 4).cuda())
        self.wl1 = float(self.w1.abs().sum(dim=(1, 2, 3)).max())
        self.bmax = float(self.b1.abs().max())
        self.Tn = self.B * -(-self.H // 4) * -(-self.W // 4)
        self.st = torch.cuda.current_stream().cuda_stream

    def _new(self, *shape, dtype=None):
        return self.torch.empty(shape, dtype=dtype or self.torch.float32, device="cuda")

    def first_products(self, stream=None):
        """x -> V1 -> M1; returns (slot of max |x|, M1)."""
        torch, lib, ck = self.torch, self.lib, self._lib.check
        st = self.st if stream is None else stream
        ax = self.x.abs().max().reshape(1).clone()
        V1 = self._new(36 * self.Tn * self.cin)
        M1 = self._new(36 * self.Tn * self.cmid)
        ck(lib.cslam_wino4_input_h2_dev(_p(self.x), self.B, self.H, self.W, self.cin, _p(ax), _p(V1), st))
        ck(lib.cslam_wino_gemm_h2_dev(_p(V1), _p(self.U1[0]), self.Tn, self.cin, self.cmid, _p(M1), st))
        return ax, M1

    def separate(self, ax, M1):
        """output transform -> y -> input transform: returns (y, slot of max |y|, V2 as int16 bits)."""
        torch, lib, ck = self.torch, self.lib, self._lib.check
        y = torch.empty((self.B, self.cmid, self.H, self.W), device="cuda").contiguous(memory_format=torch.channels_last)
        ay = torch.zeros(1, device="cuda")
        V2 = self._new(36 * self.Tn * self.cmid)
        ck(lib.cslam_wino4_output_scaled_dev(_p(M1), _p(self.b1), None, self.B, self.H, self.W, self.cmid, 1, 0, _p(ax), float(self.U1[1]),
                                             _p(ay), _p(y), self.st))
        ck(lib.cslam_wino4_input_h2_dev(_p(y), self.B, self.H, self.W, self.cmid, _p(ay), _p(V2), self.st))
        return y, ay, V2

    def chained(self, ax, M1, wl1, bmax, stream=None):
        """the chained transform: returns (slot of max |y|, bound slot, V2)."""
        torch, lib, ck = self.torch, self.lib, self._lib.check
        ay, bound = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        V2 = self._new(36 * self.Tn * self.cmid)
        ck(lib.cslam_wino4_chain_h2_dev(_p(M1), _p(self.b1), self.B, self.H, self.W, self.cmid, _p(ax), float(self.U1[1]), _p(ax),
                                        float(wl1), float(bmax), _p(ay), _p(bound), _p(V2), self.st if stream is None else stream))
        return ay, bound, V2

    def second_layer(self, V2, vslot):
        """V2 -> M2 -> z = relu(conv(y) + b2), descaled by the slot V2 was scaled with."""
        torch, lib, ck = self.torch, self.lib, self._lib.check
        M2 = self._new(36 * self.Tn * self.cout)
        z = torch.empty((self.B, self.cout, self.H, self.W), device="cuda").contiguous(memory_format=torch.channels_last)
        ck(lib.cslam_wino_gemm_h2_dev(_p(V2), _p(self.U2[0]), self.Tn, self.cmid, self.cout, _p(M2), self.st))
        ck(lib.cslam_wino4_output_scaled_dev(_p(M2), _p(self.b2), None, self.B, self.H, self.W, self.cout, 1, 0, _p(vslot), float(self.U2[1]),
                                             None, _p(z), self.st))
        return z

    def float64(self):
        torch = self.torch
        Fn = torch.nn.functional
        y = torch.relu(Fn.conv2d(self.x.double(), self.w1.double(), self.b1.double(), padding=1))
        return torch.relu(Fn.conv2d(y, self.w2.double(), self.b2.double(), padding=1))


def _errors(z, ref):
    d = z.double() - ref
    return float(d.abs().max() / ref.abs().max()), float((d ** 2).sum().sqrt() / (ref ** 2).sum().sqrt())


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("amp", [1e-3, 1.0, 40.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_chained_pair_against_float64_and_the_three_kernel_form(T, shape, amp, heavy):
    """Two layers with the chained transform between them (V2 scaled by the a-priori bound max|x| wl1 + bmax) against a float64
    evaluation, next to the same two layers with output and input transform apart (V2 scaled by the measured max |y|).  The rule of
    test_split16_trunk_equals_fp32_gemm_trunk: the chained error is at most 1.5 x the three-kernel form's + 1e-7 in max norm (relative to
    the largest output) and + 1e-8 in relative 2-norm.  The bound really bounds: the slot holds at least the measured maximum."""
    torch, _ = T
    p = _Pair(T, shape, amp, heavy, seed=11)
    ax, M1 = p.first_products()
    y, ay, V2s = p.separate(ax, M1)
    zs = p.second_layer(V2s, ay)
    ayc, bound, V2c = p.chained(ax, M1, p.wl1, p.bmax)
    zc = p.second_layer(V2c, bound)
    torch.cuda.synchronize()
    ref = p.float64()
    (ms, rs), (mc, rc) = _errors(zs, ref), _errors(zc, ref)
    print("shape", shape, "amp", amp, "heavy", heavy, "three-kernel max %.3e rms %.3e  chained max %.3e rms %.3e  bound / max|y| = 2^%.2f"
          % (ms, rs, mc, rc, float(torch.log2(bound / ay))))
    assert ayc.item() == ay.item() == y.abs().max().item()
    assert bound.item() >= ay.item()
    assert mc <= 1.5 * ms + 1e-7 and rc <= 1.5 * rs + 1e-8, (mc, ms, rc, rs)
    assert ms <= 2e-5 and mc <= 2e-5, (ms, mc)              # the trunk tolerance of the F(4x4) forms


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("amp", [1e-3, 1.0, 40.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_chained_transform_with_the_measured_scale_is_bit_equal_to_the_separate_kernels(T, shape, amp, heavy):
    """wl1 = 0 and bmax = the measured max |y| make the bound that maximum: V2 then equals the separate kernels' bit for bit (same
    operation order on the same y, zeros where tiles hang over the map), and so does the measured max |y| slot."""
    torch, _ = T
    p = _Pair(T, shape, amp, heavy, seed=12)
    ax, M1 = p.first_products()
    y, ay, V2s = p.separate(ax, M1)
    torch.cuda.synchronize()
    ayc, bound, V2c = p.chained(ax, M1, 0.0, ay.item())
    torch.cuda.synchronize()
    assert bound.item() == ay.item() and ayc.item() == ay.item()
    assert torch.equal(V2c.view(torch.int32), V2s.view(torch.int32))


@pytest.mark.parametrize("shape", [(64, 56, 56, 128, 256, 256), (64, 28, 28, 256, 512, 512), (128, 14, 14, 512, 512, 512)])
def test_chained_transform_twice_and_beside_a_stream_that_thrashes_the_l2_is_bit_identical(T, shape):
    """The kernel prefetches the next tile row of M across its barrier and hands y from one half to the other through LDS: the same
    launch again, and beside a stream that keeps HBM and the L2 busy, gives the same V2, max |y| and bound bit for bit."""
    torch, _ = T
    p = _Pair(T, shape, 1.0, False, seed=13)
    ax, M1 = p.first_products()
    ref = p.chained(ax, M1, p.wl1, p.bmax)
    again = p.chained(ax, M1, p.wl1, p.bmax)
    torch.cuda.synchronize()
    for a, b in zip(ref, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.zeros(64 << 20, device="cuda")
    for _ in range(4):
        with torch.cuda.stream(s2):
            for _ in range(4):
                big.add_(1.0)
        with torch.cuda.stream(s1):
            got = [p.chained(ax, M1, p.wl1, p.bmax, stream=s1.cuda_stream) for _ in range(3)]
        torch.cuda.synchronize()
        for g in got:
            for a, b in zip(ref, g):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_trunk_runs_the_chained_form_and_matches_the_three_kernel_trunk(T):
    """VGG-16 at 32 frames (conv5_x reaches the 512-tile floor): by default the six boundaries without a pool between them run the
    chained transform; against forms wino_chain = False and a float64 evaluation, the rule of test_split16_trunk_equals_fp32_gemm_trunk."""
    torch, _ = T
    from cslam_amd.vpr.backbones import vgg16_features_trunk
    from cslam_amd.vpr import winograd as wg
    torch.manual_seed(41)
    enc = vgg16_features_trunk().cuda().eval()
    x = torch.randn((32, 3, 224, 224), device="cuda")
    tc, t3 = wg.WinogradTrunk(enc, 64, 4), wg.WinogradTrunk(enc, 64, 4, forms={"wino_chain": False})
    lo, hi = wg.CHAIN_TILE_COLS
    lens = {k: tc._chain_len(k, 32, hw, hw) for k, hw in ((4, 56), (7, 28), (10, 14))}      # conv3_1, conv4_1, conv5_1
    assert all(n == (3 if lo <= hw // 4 + (hw % 4 > 0) <= hi else 1) for (k, n), hw in zip(lens.items(), (56, 28, 14))), lens
    assert all(t3._chain_len(k, 32, hw, hw) == 1 for k, hw in ((4, 56), (7, 28), (10, 14)))
    yc, y3 = tc(x), t3(x)
    with torch.no_grad():
        ref = enc.double()(x.double())
    enc.float()
    (mc, rc), (m3, r3) = _errors(yc, ref), _errors(y3, ref)
    print("trunk: three-kernel max %.3e rms %.3e  chained max %.3e rms %.3e" % (m3, r3, mc, rc))
    assert mc <= 2e-5 and mc <= 1.5 * m3 + 1e-7 and rc <= 1.5 * r3 + 1e-8, (mc, m3, rc, r3)


def test_chain_entry_point_rejects_what_it_does_not_serve(T):
    torch, _lib = T
    lib = _lib.load()
    z = torch.zeros(64, device="cuda")
    pz = _p(z)
    with pytest.raises(_lib.CslamHipError, match="NULL"):
        _lib.check(lib.cslam_wino4_chain_h2_dev(pz, None, 1, 8, 8, 32, pz, 1.0, pz, 1.0, 0.0, None, pz, pz, None))
    with pytest.raises(_lib.CslamHipError, match="multiple of 32"):
        _lib.check(lib.cslam_wino4_chain_h2_dev(pz, None, 1, 8, 8, 48, pz, 1.0, pz, 1.0, 0.0, pz, pz, pz, None))
    with pytest.raises(_lib.CslamHipError, match="wider than 64"):
        _lib.check(lib.cslam_wino4_chain_h2_dev(pz, None, 1, 8, 68, 32, pz, 1.0, pz, 1.0, 0.0, pz, pz, pz, None))
