"""The channel-separated residual unit (resnet.Bottleneck with resnet.Conv3DDepthwise: 1x1x1 -> 3x3x3 depthwise -> 1x1x1) and a
trunk built from it, on the device against plain ``torch.nn`` twins in fp64 with the same ``state_dict`` (tests/csn_twin.py); and
the refusals of the paths that do not take such a trunk."""
import pytest
import torch

from csn_twin import TwinBottleneck, TwinCSN, twin_downsample
from helpers import rel_err, rel_l2
from zeroshotvideoclassification_amd import _lib, amp, inference, network, optim, resnet, train

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT = 1e-4          # the project's bar for fp32 against fp64 (tests/test_model_gpu.py); an indexing error is of order 1


def _randomise(module, seed):
    """Non-trivial BatchNorm affines and running statistics (the initial 1 / 0 would hide a swapped channel)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))


def _block_and_twin(inplanes, planes, stride, seed):
    torch.manual_seed(seed)
    down = twin = None
    if stride != 1 or inplanes != planes * 4:
        s = resnet.Conv3DDepthwise.get_downsample_stride(stride)
        down = resnet._FusedSequential(resnet.Conv3d(inplanes, planes * 4, kernel_size=1, stride=s, bias=False), resnet.BatchNorm3d(planes * 4))
        twin = twin_downsample(inplanes, planes * 4, s)
    block = resnet.Bottleneck(inplanes, planes, resnet.Conv3DDepthwise, stride, down)
    _randomise(block, seed)
    ref = TwinBottleneck(inplanes, planes, stride, twin)
    assert list(ref.state_dict().keys()) == list(block.state_dict().keys())
    ref.load_state_dict(block.state_dict())
    return block.to(DEV).train(), ref.double().train()


@pytest.mark.parametrize("inplanes,planes,stride,shape", [(32, 8, 1, (2, 32, 4, 8, 8)), (16, 8, 2, (2, 16, 4, 9, 9))],
                         ids=["identity_shortcut", "stride2_downsample"])
def test_block_parity_in_training_mode(inplanes, planes, stride, shape):
    block, ref = _block_and_twin(inplanes, planes, stride, seed=11 + stride)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g)
    x64 = x.double().requires_grad_(True)
    y64 = ref(x64)
    dy = torch.randn(y64.shape, generator=g)
    y64.backward(dy.double())

    xd = x.to(DEV).requires_grad_(True)
    y = block(xd)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    errors = {"y": rel_err(y.detach().cpu(), y64.detach()), "dx": rel_l2(xd.grad.cpu(), x64.grad)}
    grads64 = dict(ref.named_parameters())
    for name, p in block.named_parameters():
        assert p.grad is not None, name
        errors[name] = rel_l2(p.grad.cpu(), grads64[name].grad)
    print(f"Bottleneck({inplanes}, {planes}, Conv3DDepthwise, stride={stride}) on {shape}: " +
          ", ".join(f"{k} {v:.2e}" for k, v in errors.items()))
    assert max(errors.values()) < TIGHT, errors
    # the running statistics moved like torch's
    for name, b in block.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            assert rel_err(b.cpu(), dict(ref.named_buffers())[name]) < TIGHT, name


def _small_trunk():
    return resnet.VideoResNet(resnet.Bottleneck, [resnet.Conv3DDepthwise] * 4, [1, 1, 1, 1], resnet.BasicStem)


def test_trunk_eval_forward():
    """Eval mode: layer 4 has 8 values per channel on this clip, batch statistics there are ill-conditioned in any precision."""
    torch.manual_seed(21)
    trunk = _small_trunk()
    _randomise(trunk, 22)
    ref = TwinCSN([1, 1, 1, 1])
    assert list(ref.state_dict().keys()) == list(trunk.state_dict().keys())
    ref.load_state_dict(trunk.state_dict())
    ref.double().eval()
    trunk.to(DEV).eval()
    clip = torch.randn(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(23))
    with torch.no_grad():
        pooled, feats = trunk(clip.to(DEV))
        want = ref(clip.double())
    assert tuple(pooled.shape) == (2, 2048) and tuple(feats.shape) == (2, 2048, 1, 2, 2)      # 4x32x32 -> stem 4x16x16 -> 2x8x8 -> 1x4x4 -> 1x2x2
    err = rel_err(pooled.cpu(), want)
    print(f"channel-separated trunk [1,1,1,1], eval forward: pooled features {err:.2e}")
    assert err < TIGHT


def _model():
    torch.manual_seed(31)
    model = network.Model(lambda pretrained=False: _small_trunk())
    assert model.output2emb_proj.layers[0].in_features == 2048
    return model.to(DEV)


def test_trunk_training_step_with_fused_adam():
    model = _model().train()
    opt = optim.FusedAdam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 1, 3, 4, 32, 32, generator=g).to(DEV)
    z = torch.nn.functional.normalize(torch.randn(2, 300, generator=g)).to(DEV)
    before = {n: p.detach().clone() for n, p in model.model.named_parameters()}
    y, loss = train.train_step(model, opt, torch.nn.MSELoss(), x, z)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2, 300) and bool(torch.isfinite(loss))
    for name, p in model.model.named_parameters():
        if name.startswith("fc."):            # built, never applied (as in every VideoResNet here)
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[name]), name


def _count(monkeypatch, names):
    lib = _lib.load()
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)

        def counted(*a, _n=n, _real=real):
            calls[_n] += 1
            return _real(*a)

        monkeypatch.setattr(lib, n, counted, raising=False)
    return calls


def test_bf16_paths_refuse_the_trunk(monkeypatch):
    """The inference engines and ``amp`` go on refusing Bottleneck / grouped trunks, before anything is packed or launched."""
    model = _model()
    calls = _count(monkeypatch, ["zsv_conv3d_bf16_pack", "zsv_conv3d_bf16_fwd", "zsv_conv3d_bf16_fwd_stats", "zsv_clip_to_bf16",
                                 "zsv_conv3d_fwd_full", "zsv_dwconv3d_fwd"])
    x = torch.randn(2, 1, 3, 4, 32, 32, generator=torch.Generator().manual_seed(33)).to(DEV)
    model.eval()
    with pytest.raises(RuntimeError):
        inference.engine_for(model, torch.bfloat16)
    model.train()
    with pytest.raises(RuntimeError):
        with amp.autocast():
            model(x)
    assert not amp.is_autocast_enabled()
    with pytest.raises(RuntimeError):
        inference.ConvGeometry(model.model.layer1[0].conv2[0])
    assert all(v == 0 for v in calls.values()), calls
