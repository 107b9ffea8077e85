"""Depthwise Conv3d and the channel-separated trunk, the part that needs no device: what the layer accepts and refuses, the
``ir_csn_50`` surface, the head width of ``network.Model``, and the refusals of the zsv_dwconv3d_* entry points, which are all
decided on the host before anything is launched."""
import ctypes

import pytest
import torch

from csn_twin import TwinCSN
from helpers import make_opt
from zeroshotvideoclassification_amd import _lib, layers, network, resnet

FAKE = 0x10000          # a non-NULL address no refused call ever dereferences


def test_layer_accepts_depthwise_and_refuses_the_rest():
    conv = layers.Conv3d(8, 8, 3, padding=1, groups=8, bias=False)
    assert tuple(conv.weight.shape) == (8, 1, 3, 3, 3) and conv.groups == 8
    assert conv.pre_supported((2, 8, 4, 8, 8)) is False
    assert layers.Conv3d(8, 8, 3, padding=1).groups == 1
    with pytest.raises(NotImplementedError):
        layers.Conv3d(8, 8, 3, groups=2)
    with pytest.raises(NotImplementedError):
        layers.Conv3d(8, 16, 3, groups=8)
    with pytest.raises(NotImplementedError):
        layers.Conv3d(8, 8, 3, dilation=2)
    with pytest.raises(NotImplementedError):
        layers.Conv3d(8, 8, 3, groups=8, dilation=2)
    with pytest.raises(NotImplementedError):
        layers.Conv3d(8, 8, 3, padding=1, groups=8, padding_mode="replicate")
    with pytest.raises(AssertionError):
        resnet.Conv3DDepthwise(8, 16)
    assert resnet.Conv3DDepthwise.get_downsample_stride(2) == (2, 2, 2)


def test_ops_conv3d_refuses_true_grouped_convolutions():
    from zeroshotvideoclassification_amd import ops
    x, w = torch.zeros(1, 8, 2, 4, 4), torch.zeros(8, 4, 3, 3, 3)
    with pytest.raises(NotImplementedError):
        ops.conv3d(x, w, None, 1, 1, groups=2)


def test_ir_csn_50_surface():
    model = resnet.ir_csn_50()
    planes = {"layer1": 64, "layer2": 128, "layer3": 256, "layer4": 512}
    depth = {"layer1": 3, "layer2": 4, "layer3": 6, "layer4": 3}
    sd = model.state_dict()
    for name, n in depth.items():
        for i in range(n):
            assert tuple(sd[f"{name}.{i}.conv2.0.weight"].shape) == (planes[name], 1, 3, 3, 3)
            assert getattr(model, name)[i].conv2[0].groups == planes[name]
    twin = TwinCSN([3, 4, 6, 3]).state_dict()
    assert list(sd.keys()) == list(twin.keys())
    assert all(sd[k].shape == twin[k].shape for k in sd)
    assert model.fc.in_features == 2048
    assert "not key-compatible" in " ".join(resnet.ir_csn_50.__doc__.lower().split())


# every state_dict shape of the three networks get_network built before the channel-separated branch existed that depends on the
# head: the trunk and the head are 512 wide
def test_get_network_head_width():
    csn = network.get_network(make_opt("ir_csn_50"))
    assert isinstance(csn.model, resnet.VideoResNet) and csn.output2emb_proj.layers[0].in_features == 2048
    assert tuple(csn.output2emb_proj.layers[1].weight.shape) == (300, 512)
    for name, factory in (("r2plus1d_18", resnet.r2plus1d_18), ("r3d_18", resnet.r3d_18)):
        model = network.get_network(make_opt(name))
        assert model.output2emb_proj.layers[0].in_features == 512
        sd = model.state_dict()
        assert tuple(sd["output2emb_proj.layers.0.weight"].shape) == (512, 512)
        assert tuple(sd["output2emb_proj.layers.1.weight"].shape) == (300, 512)
        assert tuple(sd["feature2input_proj.weight"].shape) == (256, 512) and tuple(sd["t_pos_embeds.weight"].shape) == (1, 512)
        trunk = factory().state_dict()
        assert {k: v.shape for k, v in sd.items() if k.startswith("model.")} == {"model." + k: v.shape for k, v in trunk.items()}
    c3d = network.get_network(make_opt("c3d"))
    assert not hasattr(c3d, "output2emb_proj")
    with pytest.raises(Exception):
        network.get_network(make_opt("resnext"))


def _desc(shape, k=(3, 3, 3), s=(1, 1, 1), p=(1, 1, 1), cout=None):
    n, c, t, h, w = shape
    o = [(e + 2 * pp - kk) // ss + 1 for e, kk, ss, pp in zip((t, h, w), k, s, p)]
    return _lib.ConvDesc(n, c, t, h, w, c if cout is None else cout, *o, *k, *s, *p)


def _calls(lib, d, workspace_bytes=None):
    """status of the three launching entry points with every pointer present"""
    need = lib.zsv_dwconv3d_wgrad_workspace_bytes(ctypes.byref(d)) if workspace_bytes is None else workspace_bytes
    return (lib.zsv_dwconv3d_fwd(ctypes.byref(d), FAKE, FAKE, None, FAKE, 0, None),
            lib.zsv_dwconv3d_dgrad(ctypes.byref(d), FAKE, FAKE, FAKE, None),
            lib.zsv_dwconv3d_wgrad(ctypes.byref(d), FAKE, FAKE, FAKE, FAKE, need, None))


def test_c_abi_refusals_without_a_device():
    lib = _lib.load()
    good = _desc((2, 8, 4, 9, 9))
    assert lib.zsv_dwconv3d_supported(ctypes.byref(good)) == 1
    assert lib.zsv_dwconv3d_supported(None) == 0
    # NULL pointers -> ZSV_E_NULL, whichever one is missing
    g = ctypes.byref(good)
    assert lib.zsv_dwconv3d_fwd(None, FAKE, FAKE, None, FAKE, 0, None) == 2
    assert [lib.zsv_dwconv3d_fwd(g, *a, 0, None) for a in ((None, FAKE, None, FAKE), (FAKE, None, None, FAKE), (FAKE, FAKE, None, None))] == [2] * 3
    assert [lib.zsv_dwconv3d_dgrad(g, *a, None) for a in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None))] == [2] * 3
    assert [lib.zsv_dwconv3d_wgrad(g, *a, FAKE, 1 << 30, None) for a in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None))] == [2] * 3
    # Cin != Cout and extents that do not follow from the formula -> ZSV_E_BAD_SHAPE
    wrong_extent = _desc((2, 8, 4, 9, 9))
    wrong_extent.Ho += 1
    for d in (_desc((2, 8, 4, 9, 9), cout=16), wrong_extent):
        assert lib.zsv_dwconv3d_supported(ctypes.byref(d)) == 0
        assert _calls(lib, d, 1 << 30) == (1, 1, 1)
    # consistent, outside the supported set -> ZSV_E_UNSUPPORTED
    for d in (_desc((2, 8, 6, 9, 9), k=(5, 3, 3), p=(2, 1, 1)), _desc((2, 8, 6, 9, 9), k=(3, 3, 5), p=(1, 1, 2)),
              _desc((2, 8, 6, 9, 9), s=(3, 1, 1)), _desc((2, 8, 6, 9, 9), s=(1, 1, 3)), _desc((2, 8, 6, 9, 9), k=(1, 3, 3), p=(1, 1, 1)),
              _desc((2, 8, 6, 9, 9), k=(2, 3, 3), p=(0, 1, 1))):
        assert lib.zsv_dwconv3d_supported(ctypes.byref(d)) == 0
        assert _calls(lib, d, 1 << 30) == (6, 6, 6)
        assert lib.zsv_dwconv3d_wgrad_workspace_bytes(ctypes.byref(d)) == 0
    # a tensor of 2^31 elements -> ZSV_E_TOO_LARGE; one element fewer per clip is taken
    big = _desc((1 << 15, 64, 4, 16, 16))
    assert big.N * big.Cin * big.Ti * big.Hi * big.Wi == 1 << 31
    assert lib.zsv_dwconv3d_supported(ctypes.byref(big)) == 0
    assert _calls(lib, big, 1 << 40) == (4, 4, 4)
    assert lib.zsv_dwconv3d_supported(ctypes.byref(_desc(((1 << 15) - 1, 64, 4, 16, 16)))) == 1
    # the weight gradient's workspace: one byte short, NULL, or off its 16-byte alignment -> ZSV_E_WORKSPACE
    need = lib.zsv_dwconv3d_wgrad_workspace_bytes(g)
    assert need > 0 and need % 256 == 0
    assert lib.zsv_dwconv3d_wgrad(g, FAKE, FAKE, FAKE, FAKE, need - 1, None) == 3
    assert lib.zsv_dwconv3d_wgrad(g, FAKE, FAKE, FAKE, None, need, None) == 3
    assert lib.zsv_dwconv3d_wgrad(g, FAKE, FAKE, FAKE, FAKE + 4, need, None) == 3
    # the supported set: kernels 1 / 3, strides 1 / 2, padding < kernel
    for k, s, p in (((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((1, 3, 3), (1, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (1, 0, 0)),
                    ((3, 3, 3), (1, 1, 1), (0, 0, 0)), ((3, 3, 3), (1, 1, 1), (2, 2, 2)), ((1, 1, 1), (2, 2, 2), (0, 0, 0))):
        assert lib.zsv_dwconv3d_supported(ctypes.byref(_desc((2, 8, 6, 9, 9), k, s, p))) == 1, (k, s, p)
