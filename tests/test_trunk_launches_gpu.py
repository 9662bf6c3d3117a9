"""GPU tests (-m gpu) that pin WHICH entry points of libcslam_hip.so the default paths of the two trunk runners call, and in what order
(DESIGN.md describes them; vpr/winograd.py picks them by shape).  `_lib.load` is replaced by a proxy that forwards every call to the
real library and records its name.  The expected lists were recorded before the runners were split into vpr/pair_weights.py,
vpr/conv_kernels.py and vpr/winograd.py: a change of this file is a change of behaviour."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture
def launches(monkeypatch):
    """List that receives the name (without `cslam_` and `_dev`) of every library entry point called from here on."""
    from cslam_amd import _lib
    real, names = _lib.load(), []

    class Recorder(object):
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name == "cslam_last_error":
                return fn

            def call(*args):
                names.append(name[len("cslam_"):-len("_dev")])
                return fn(*args)
            return call

    proxy = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    return names


PAIR_LAYER = ["wino4_input_h2", "wino_gemm_h2", "wino4_output_scaled"]
CHAIN_OF_3 = ["wino4_input_h2", "wino_gemm_h2", "wino4_chain_h2", "wino_gemm_h2", "wino4_chain_h2", "wino_gemm_h2", "wino4_output_scaled"]
# 256 frames: the input's max |x|, conv1_1 + conv1_2 + pool as one direct kernel, conv2_1 and conv2_2 (+ pool) on the register-resident
# direct kernels, conv3_x and conv4_x as chains of three pair-product layers, conv5_x (14 x 14 maps: 4 tile columns) layer by layer
VGG16_BATCH = ["absmax", "conv_stem_direct_h", "conv3x3_direct_r", "conv3x3_direct_r2"] + 2 * CHAIN_OF_3 + 3 * PAIR_LAYER
# one frame: the first layer alone (it measures max |y|), conv1_2 and conv2_1 as F(4x4) with fp32 library products, conv2_2 in the Z
# form of the pair products, every later layer (fewer than 512 F(4x4) tiles) as F(2x2) with fp32 library products
VGG16_SINGLE = (["conv3x3_c3_amax"] + 2 * ["wino4_input", "wino4_output_scaled"] + ["wino4_input_h2", "wino_zgemm_h2", "wino4_output_z"]
                + 9 * ["wino_input", "wino_output"])
# conv1 + bn1 + relu + maxpool as one kernel, layer1 on the register-resident pair kernel, everything else the implicit GEMM between
# pair-format maps (3 downsampling blocks of 3 + 2 convolutions)
RESNET18 = ["absmax", "conv_stem_pool_igemm_h2"] + 4 * ["conv3x3_direct_p"] + 15 * ["conv_igemm_h2p"]


@pytest.mark.parametrize("B,expected", [(256, VGG16_BATCH), (1, VGG16_SINGLE)])
def test_vgg16_trunk_default_launches(launches, B, expected):
    import torch
    from cslam_amd.vpr.backbones import vgg16_features_trunk
    from cslam_amd.vpr.winograd import WinogradTrunk
    torch.manual_seed(1)
    encoder = vgg16_features_trunk().cuda().eval()
    trunk = WinogradTrunk(encoder, 64, 4)
    x = torch.randn((B, 3, 224, 224), device="cuda")
    del launches[:]
    y = trunk(x)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, 512, 14, 14)
    assert launches == expected


def test_resnet18_trunk_default_launches(launches):
    import torch
    from cslam_amd.vpr.backbones import resnet_trunk
    from cslam_amd.vpr.winograd import WinogradResNet
    torch.manual_seed(17)
    run = WinogradResNet(resnet_trunk("resnet18").cuda().eval())
    x = torch.randn((8, 3, 224, 224), device="cuda")
    del launches[:]
    y = run(x)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (8, 512, 7, 7)
    assert launches == RESNET18
